"""CPU tier: the stem oracle of tests/test_stem_grads_gpu.py is itself tested before it judges the kernels.

``oracle.stem_backward_chunked`` -- the closed-form stem backward the full-batch GPU checks use, frame chunk by frame chunk -- is pinned
to torch autograd of ``oracle.stem_rounded`` / ``stem_unrounded`` at a small shape: several chunks with a ragged last one, and
constant input patches that make exact ties inside pooling windows (the tie rule: first maximum in scan order, pool.hip)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import dpc_oracle as O


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _case(seed, N=4, T=2, H=22, W=26, Co=16):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 3, T, H, W, generator=g)
    x[0, :, :, 2:14, 4:16] = 0.5      # constant patches: equal raw values inside windows -> exact ties
    x[3, :, 1, 6:20, 0:12] = -0.25
    p = {O.STEM_W: torch.randn(Co, 3, 1, 7, 7, generator=g) * 0.1,
         O.STEM_G: 1.0 + 0.2 * torch.randn(Co, generator=g), O.STEM_B: 0.2 * torch.randn(Co, generator=g)}
    return x, p, g


def frames(t):  # [N,C,T,h,w] -> [N*T,h,w,C] (the engine's channels-last, frame-major order)
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[3], t.shape[4], t.shape[1])


@pytest.mark.parametrize("rounded", [True, False])
def test_chunked_stem_backward_is_autograd_of_the_stem(rounded):
    x, p, g = _case(3)
    N, _, T, H, W = x.shape
    stored = torch.bfloat16 if rounded else torch.float32
    fwd = O.stem_rounded if rounded else O.stem_unrounded
    # the stored raw values and the oracle's routing come from a forward without gradients ...
    with torch.no_grad():
        pooled0, raw0 = fwd(x, p)
    raw_cl = frames(raw0).to(stored)                        # exact: raw0 is already bf16-valued in the rounded form
    dy = (0.05 * (pooled0 - pooled0.mean()) / pooled0.std() + 0.02 * torch.randn(pooled0.shape, generator=g)).to(stored).float()
    dzs, routes, nears, pooled_c = {}, {}, {}, {}

    def keep(f0, f1, d):
        dzs[f0], routes[f0], nears[f0], pooled_c[f0] = d["dz"], d["route"], d["near"], d["pooled"]

    xf = x.permute(0, 2, 1, 3, 4).reshape(N * T, 3, H, W)
    res = O.stem_backward_chunked(xf, raw_cl, p[O.STEM_G], p[O.STEM_B], frames(dy), p[O.STEM_W].shape, stored=stored,
                                  round_x=rounded, chunk=3, on_chunk=keep)
    assert sorted(dzs) == [0, 3, 6]                          # 8 frames: chunks of 3, 3 and a ragged 2
    cat = lambda d: torch.cat([d[k] for k in sorted(d)])      # [F,C,h,w]
    route, near = cat(routes), cat(nears)
    # ... and autograd runs the same stem with that routing
    Ho, Wo = route.shape[2:]
    route5 = route.view(N, T, -1, Ho, Wo).permute(0, 2, 1, 3, 4)
    leaves = {k: v.clone().requires_grad_() for k, v in p.items()}
    pooled, raw = fwd(x, leaves, route=route5)
    raw.retain_grad()
    pooled.backward(dy)
    # forward: the chunked pooling is max-pool of the rounded stem, and its routing is max-pool's argmax away from near-ties
    assert torch.equal(pooled, pooled0)
    assert rel(cat(pooled_c), pooled0.permute(0, 2, 1, 3, 4).reshape(N * T, -1, Ho, Wo)) < (3e-3 if rounded else 1e-6)
    with torch.no_grad():
        act = F.relu(O.bn_batch(raw0, p[O.STEM_G], p[O.STEM_B]))
        a2 = act.permute(0, 2, 1, 3, 4).reshape(N * T, -1, H // 2, W // 2)
        mp, idx = F.max_pool2d(a2, 3, 2, 1, return_indices=True)
    ih, iw = idx // (W // 2), idx % (W // 2)
    oh = torch.arange(Ho).view(1, 1, Ho, 1)
    ow = torch.arange(Wo).view(1, 1, 1, Wo)
    tap = ((ih - (2 * oh - 1)) * 3 + (iw - (2 * ow - 1)))
    torch_route = torch.where(mp > 0, tap, torch.full_like(tap, 9))
    win = F.unfold(F.pad(a2, (1, 1, 1, 1), value=-1.0), 3, stride=2).view(N * T, a2.shape[1], 9, Ho, Wo)
    exact_ties = ((win == win.amax(2, keepdim=True)).sum(2) > 1) & (mp > 0)
    assert exact_ties.sum().item() > 20              # the deliberate ties are there ...
    assert torch.equal(route[exact_ties].long(), torch_route[exact_ties])   # ... and resolve to the first maximum, as torch's
    assert torch.equal(route[~near].long(), torch_route[~near])
    assert 0 < res["near_frac"] < 0.2
    assert res["route_mismatch"] == 0
    # backward
    assert rel(res["dbeta"], leaves[O.STEM_B].grad) < 1e-5
    assert rel(res["dgamma"], leaves[O.STEM_G].grad) < 1e-5
    assert rel(res["dw"], leaves[O.STEM_W].grad) < 1e-4
    assert rel(cat(dzs), raw.grad.permute(0, 2, 1, 3, 4).reshape(N * T, -1, H // 2, W // 2)) < 1e-4
    # statistics of the stored values
    r64 = raw0.double()
    assert rel(res["mean"], r64.mean((0, 2, 3, 4))) < 1e-12
    assert rel(res["invstd"], 1 / torch.sqrt(r64.var((0, 2, 3, 4), unbiased=False) + O.BN_EPS)) < 1e-10


def test_chunked_stem_mutations_and_engine_routing_move_the_result():
    """the switches the GPU tests use: each moves the oracle, and a routing given for the near-tie windows only is followed there"""
    x, p, g = _case(5)
    N, _, T, H, W = x.shape
    with torch.no_grad():
        pooled0, raw0 = O.stem_rounded(x, p)
    dy = frames((0.05 * (pooled0 - pooled0.mean()) / pooled0.std() + 0.02 * torch.randn(pooled0.shape, generator=g)).to(torch.bfloat16))
    xf = x.permute(0, 2, 1, 3, 4).reshape(N * T, 3, H, W)
    args = (xf, frames(raw0).to(torch.bfloat16), p[O.STEM_G], p[O.STEM_B], dy, p[O.STEM_W].shape)
    routes = []
    base = O.stem_backward_chunked(*args, chunk=5, on_chunk=lambda f0, f1, d: routes.append((d["own_route"], d["near"])))
    same = O.stem_backward_chunked(*args, chunk=8)
    assert rel(same["dw"], base["dw"]) < 1e-6   # chunking does not change the sums
    assert rel(O.stem_backward_chunked(*args, drop_xhat_term=True)["dw"], base["dw"]) > 0.1
    first = O.stem_backward_chunked(*args, route_first=True)
    assert rel(first["dw"], base["dw"]) > 0.1 and rel(first["dgamma"], base["dgamma"]) > 0.1
    own = torch.cat([r for r, _ in routes]).permute(0, 2, 3, 1)
    near = torch.cat([m for _, m in routes]).permute(0, 2, 3, 1)
    flipped = torch.where(own < 9, (own + 1) % 9, own)           # a routing that differs from the oracle's wherever it routes
    eng = torch.where(near, flipped, own)
    follow = O.stem_backward_chunked(*args, engine_route=eng)
    assert follow["route_mismatch"] == 0 and rel(follow["dgamma"], base["dgamma"]) > 0   # followed on the near-ties ...
    wrong = O.stem_backward_chunked(*args, engine_route=flipped)
    assert wrong["route_mismatch"] == int(((flipped != own) & ~near).sum())              # ... and counted everywhere else
