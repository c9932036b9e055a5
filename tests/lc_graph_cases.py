"""Cases of the on-device label draw (dpc_synthetic_labels, csrc/labels.hip) and of the labels that stay on the device
(LCEngine.set_labels / fill_synthetic), shared by the simulator tier (tests/test_lc_labels_emu.py) and the GPU tier
(tests/test_lc_graph_gpu.py).  The definition restated here is the one include/dpc_hip.h documents:

    (w0, w1, w2, w3) = Philox4x32-10(counter (b >> 2, d, 3, 0), key (lo(seed), hi(seed)))     d = the draw counter on the device
    label[b] = ((uint64) w_(b & 3) * num_class) >> 32
"""
import numpy as np
import pytest
import torch

from dpc_amd import _lib as L
from kcases import K
from synthetic_cases import words_np

STREAM_LABEL = 3
LABEL_CASES = [(1, 101), (5, 51), (7, 1), (4096, 400)]   # one label, a tail block, one class, more than one workgroup


def labels_np(B, num_class, seed, d):
    """the definition in numpy: int64 [B]"""
    w = words_np(B, seed, d, stream=STREAM_LABEL).reshape(-1)[:B].astype(np.uint64)
    return ((w * np.uint64(num_class)) >> np.uint64(32)).astype(np.int64)


def draw(k: K, B, num_class, seed, counter, pad=3):
    """one dpc_synthetic_labels call into the middle of a poisoned buffer: (labels [B], the buffer)"""
    buf = torch.full((B + 2 * pad,), -7, dtype=torch.int64, device=k.dev)
    k.call("dpc_synthetic_labels", buf[pad:], B, num_class, seed, counter)
    k.sync()
    return buf[pad:pad + B].cpu().numpy(), buf.cpu()


def case_definition(k: K, B, num_class, seed=0x0123456789ABCDEF, d=5, pad=3):
    ctr = torch.tensor([d], dtype=torch.int32, device=k.dev)
    got, buf = draw(k, B, num_class, seed, ctr, pad)
    assert np.array_equal(got, labels_np(B, num_class, seed, d))
    assert got.min() >= 0 and got.max() < num_class
    assert bool((buf[:pad] == -7).all()) and bool((buf[pad + B:] == -7).all())   # nothing outside [0, B) is written
    assert int(ctr.item()) == d                                                  # the counter is read, never written
    if num_class == 1:
        assert not got.any()
    return got


def case_counter_and_seed(k: K, B=4096, num_class=400, seed=11):
    ctr = torch.tensor([0], dtype=torch.int32, device=k.dev)
    a, _ = draw(k, B, num_class, seed, ctr)
    a2, _ = draw(k, B, num_class, seed, ctr)
    assert np.array_equal(a, a2) and int(ctr.item()) == 0
    k.call("dpc_counter_advance", ctr)
    k.sync()
    b, _ = draw(k, B, num_class, seed, ctr)
    c, _ = draw(k, B, num_class, seed + 1, ctr)
    hi, _ = draw(k, B, num_class, seed ^ (1 << 40), ctr)   # the high key word counts
    assert int(ctr.item()) == 1 and np.array_equal(b, labels_np(B, num_class, seed, 1))
    for x, y in ((a, b), (b, c), (b, hi)):
        assert (x != y).mean() > 0.99
    # not the words of the input stream (2) under the same key and counter
    w2 = words_np(B, seed, 1, stream=2).reshape(-1)[:B].astype(np.uint64)
    assert (b != ((w2 * np.uint64(num_class)) >> np.uint64(32)).astype(np.int64)).mean() > 0.99


def case_bad_arguments(k: K):
    ctr = torch.zeros(1, dtype=torch.int32, device=k.dev)
    t = torch.zeros(4, dtype=torch.int64, device=k.dev)
    for args in ((None, 4, 5, 1, ctr), (t, 4, 5, 1, None), (t, 0, 5, 1, ctr), (t, -1, 5, 1, ctr), (t, 4, 0, 1, ctr), (t, 4, -3, 1, ctr)):
        with pytest.raises(L.DpcError, match=r"code -1\b"):
            k.call("dpc_synthetic_labels", *args)
    k.sync()
    assert not t.any()


def chi_square(got, num_class):
    n = got.size
    cnt = np.bincount(got, minlength=num_class).astype(np.float64)
    e = n / num_class
    return float(((cnt - e) ** 2 / e).sum())


def case_uniform(k: K, seed, d, num_class, n=1 << 20):
    """chi-square of n labels of one launch over num_class bins against df + 5 sqrt(2 df) (df = num_class - 1: mean df, variance
    2 df under the null).  The definition itself gives 93.6 (bound 170.7) at (1000, 9, 101) and 44.5 (bound 100.0) at (1001, 1, 51)."""
    ctr = torch.tensor([d], dtype=torch.int32, device=k.dev)
    got, _ = draw(k, n, num_class, seed, ctr)
    assert np.array_equal(got, labels_np(n, num_class, seed, d))
    df = num_class - 1
    chi, bound = chi_square(got, num_class), df + 5 * (2 * df) ** 0.5
    print(f"chi-square over {num_class} bins, {n} labels: {chi:.1f} (bound {bound:.1f})")
    assert chi < bound, (chi, bound)


# ---- the engine: labels as they stand, fill_synthetic
def lc_engine(lib, dev, dtype, widths, B, size=64, N=2, SL=2, num_class=101, seed=666):
    """the engine as dpc_amd.lc_main builds it (tests/test_lc_frames_entry.py: make_engine)"""
    from dpc_amd.lc import LC, LCEngine
    from dpc_amd.plan import LAYER_WIDTH
    w = widths or LAYER_WIDTH
    eng = LCEngine("resnet18", size, N, SL, B, dev, dtype, w, lib=lib if lib is not None and lib.kind != "hip" else None, lr=1e-3, wd=1e-3,
                   dropout=0.5, num_class=num_class, seed=seed)
    init = LC(size, N, SL, "resnet18", 0.5, num_class, widths=w, seed=0)
    eng.load_params({k: v.detach() for k, v in init.state_dict().items()})
    return eng


def case_labels_as_they_stand(lib, dev, dtype, widths, B=2):
    """set_labels(y); forward(None, None) on a filled operand == forward(block, y) (logits, result), and train_step(None, None) ==
    train_step(block, y) (flat_p, flat_m), bit for bit; labels set once stay for the next step"""
    a, b = (lc_engine(lib, dev, dtype, widths, B) for _ in range(2))
    block = torch.empty(B, a.N, 3, a.SL, a.size, a.size, device=dev)
    y = torch.tensor([(17 * i + 3) % a.num_class for i in range(B)])
    # eval-mode forward
    a.fill_synthetic(1000, block)
    a.set_labels(y)
    assert torch.equal(a.target.cpu(), y)
    oa, _ = a.forward(None, None, train=False)
    ob, _ = b.forward(block, y, train=False)
    assert torch.equal(oa, ob) and torch.equal(a.result, b.result) and torch.isfinite(a.result).all()
    other = (y + 1) % a.num_class
    a.set_labels(other.to(dev))                                   # a device tensor works as well; the loss follows the labels
    a.forward(None, None, train=False)
    assert torch.equal(a.logits, b.logits) and not torch.equal(a.result, b.result)
    # train steps
    for step in range(2):
        a.fill_synthetic(1000, block)
        if step == 0:
            a.set_labels(y)                                       # fill_synthetic drew its own labels: put ours back
            ra = a.train_step(None, None).clone()
        else:
            ra = a.train_step(None, y).clone()                    # a target given: as before
        rb = b.train_step(block.clone(), y).clone()
        assert torch.equal(ra, rb)
    assert torch.equal(a.flat_p, b.flat_p) and torch.equal(a.flat_m, b.flat_m) and a.flat_m.abs().sum() > 0
    assert a.step_count == b.step_count == 2


def case_fill_synthetic_labels(lib, dev, dtype, widths, B=3, seed=1000):
    """LCEngine.fill_synthetic leaves in eng.target the definition's labels for dev_input's NEW value, beside the batch of that value"""
    eng = lc_engine(lib, dev, dtype, widths, B)
    seen = []
    for d in (1, 2, 3):
        eng.fill_synthetic(seed)
        assert int(eng.dev_input.item()) == d
        got = eng.target.cpu().numpy()
        assert np.array_equal(got, labels_np(B, eng.num_class, seed, d))
        seen.append(tuple(got))
    assert len(set(seen)) == 3
    x = eng.x_s2d.clone()
    eng.dev_input.sub_(1)
    from dpc_amd.engine import BackboneEngine
    BackboneEngine.fill_synthetic(eng, seed)                      # the batch is the base class's draw at the same counter
    assert torch.equal(eng.x_s2d, x) and int(eng.dev_input.item()) == 3
