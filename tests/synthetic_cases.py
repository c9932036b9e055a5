"""Kernel cases of dpc_synthetic_input (csrc/synthetic.hip), shared by the simulator tier (tests/test_synthetic_input_emu.py) and the
GPU tier (tests/test_entry_graph_gpu.py).  The definition restated here is the one include/dpc_hip.h documents:

    e = flat index of the block [BN][3][T][H][W], q = e >> 2
    (w0, w1, w2, w3) = Philox4x32-10(counter (q, d, 2, 0), key (lo(seed), hi(seed)))     d = the draw counter on the device
    j in {0, 1}: u = ((w_2j >> 8) + 1) 2^-24, v = (w_2j+1 >> 8) 2^-24, r = sqrt(-2 log u), th = 2 pi v
                 x[4q + 2j] = r cos th, x[4q + 2j + 1] = r sin th
"""
import numpy as np
import torch

from dpc_amd import _lib as L
from kcases import K, philox4x32_10_np

STREAM_INPUT = 2


def words_np(n, seed, d, stream=STREAM_INPUT):
    """[ceil(n/4), 4] uint32 Philox words of the first n elements"""
    nb = (n + 3) // 4
    ctr = np.zeros((nb, 4), np.uint32)
    ctr[:, 0] = np.arange(nb, dtype=np.uint32)
    ctr[:, 1] = np.uint32(d & 0xFFFFFFFF)
    ctr[:, 2] = stream
    return philox4x32_10_np(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def normals_np(words, n):
    """f64 Box-Muller of the words (the kernel's formulas, 2 pi v with v exact)"""
    w = words.astype(np.uint64)
    out = np.empty((w.shape[0], 4), np.float64)
    for j in (0, 1):
        u = ((w[:, 2 * j] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        v = (w[:, 2 * j + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u))
        out[:, 2 * j] = r * np.cos(2 * np.pi * v)
        out[:, 2 * j + 1] = r * np.sin(2 * np.pi * v)
    return out.reshape(-1)[:n]


def draw(k: K, shape, seed, counter, dtype=torch.float32, block=True, s2d=True):
    """one dpc_synthetic_input call: (block f32 [BN][3][T][H][W] or None, s2d operand [BN][T][H/2][W/2][16] or None)"""
    BN, T, H, W = shape
    b = k.empty(BN, 3, T, H, W) if block else None
    o = torch.full((BN, T, H // 2, W // 2, 16), 7.0, dtype=dtype, device=k.dev) if s2d else None   # 7: pad channels must be written
    k.call("dpc_synthetic_input", b, o, L.dtype_code(dtype), BN, T, H, W, seed, counter)
    k.sync()
    return b, o


def case_normals(k: K, shape, seed=0x0123456789ABCDEF, d=5):
    """the normals are the definition's, computed in f64 from the numpy Philox words, within 1e-5; the same formulas on words of a
    neighbouring counter, another stream or the other half of a block miss by O(1): the words themselves are pinned"""
    ctr = torch.tensor([d], dtype=torch.int32, device=k.dev)
    b, _ = draw(k, shape, seed, ctr, s2d=False)
    got = b.cpu().double().reshape(-1).numpy()
    n = got.size
    ref = normals_np(words_np(n, seed, d), n)
    err = np.abs(got - ref).max()
    assert err < 1e-5, err
    for wrong in (words_np(n, seed, d + 1), words_np(n, seed, d, stream=1), words_np(n, seed ^ (1 << 40), d),
                  words_np(n, seed, d)[:, [2, 3, 0, 1]]):
        assert np.abs(got - normals_np(wrong, n)).max() > 0.5
    assert int(ctr.item()) == d   # the generator never writes the counter
    return got


def case_s2d(k: K, shape, dtype, seed=77, d=3):
    """the operand of a two-output call == dpc_pack_input_s2d of the block of the same call, bit for bit; an operand-only call writes
    the same bits; channels 12-15 are zero"""
    ctr = torch.tensor([d], dtype=torch.int32, device=k.dev)
    BN, T, H, W = shape
    b, o = draw(k, shape, seed, ctr, dtype)
    ref = torch.full_like(o, 5.0)
    k.call("dpc_pack_input_s2d", b, ref, L.dtype_code(dtype), BN, T, H, W)
    _, o2 = draw(k, shape, seed, ctr, dtype, block=False)
    k.sync()
    assert torch.equal(o.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       ref.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    assert torch.equal(o2.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       o.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    assert bool((o[..., 12:] == 0).all()) and bool((o[..., :12] != 0).any())


def case_counter(k: K, shape, seed=11):
    """same counter -> same draw; dpc_counter_advance -> a new draw; another seed -> another draw; the counter is only read"""
    ctr = torch.tensor([0], dtype=torch.int32, device=k.dev)
    a, _ = draw(k, shape, seed, ctr, s2d=False)
    a2, _ = draw(k, shape, seed, ctr, s2d=False)
    assert torch.equal(a, a2) and int(ctr.item()) == 0
    k.call("dpc_counter_advance", ctr)
    k.sync()
    assert int(ctr.item()) == 1
    b, _ = draw(k, shape, seed, ctr, s2d=False)
    c, _ = draw(k, shape, seed + 1, ctr, s2d=False)
    assert int(ctr.item()) == 1
    assert (a != b).float().mean().item() > 0.99 and (b != c).float().mean().item() > 0.99
