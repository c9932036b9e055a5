"""Case bodies of the retrieval tests, shared by the simulator tier (tests/test_retrieval_emu.py) and the MI355X tier
(tests/test_retrieval_gpu.py): csrc/retrieval.hip through the C ABI and dpc_amd/retrieval.py, LCEngine.embed_video, and
`python -m dpc_amd.lc_main --retrieval`.

Expectations never come from the code under test: float64 numpy products sorted by (-similarity, index), a ten-line numpy
restatement of the recall counts, and by-hand forwards on a twin engine (the forward that tests/golden/lc.npz pins) followed by a
float64 mean and normalisation.  Bounds are derived: a D-term f32 sum in any order is within D * 2^-24 * sum |q_d||g_d| of the
float64 value."""
import os
import re

import numpy as np
import torch

from test_lc_frames_entry import CROP, DS, N, SIZE, SL, base_frames, long_video, make_engine, variants

U = 2.0 ** -24
SLABS = (1, 2, 3, 0)
EXACT_SHAPES = ((70, 333, 64, 10, False), (33, 130, 256, 64, False), (5, 7, 32, 10, False), (64, 64, 32, 1, True))
ROUNDING_SHAPES = ((70, 333, 64, 10), (40, 150, 256, 5), (45, 1100, 32, 20))
MAX_LEFT_OUT = 0.05


def _sync(dev):
    if str(dev) != "cpu":
        torch.cuda.synchronize()


def _topk_all_slabs(lib, dev, Q, G, K, skip):
    """knn_topk under every slab count of the issue; the results must be the same bits; returns (idx, sim) as numpy"""
    from dpc_amd import retrieval as R
    Qt, Gt = torch.from_numpy(Q).to(dev), torch.from_numpy(G).to(dev)
    sk = None if skip is None else torch.from_numpy(skip).to(dev)
    res = []
    for s in SLABS:
        idx, sim = R.knn_topk(lib, Qt, Gt, K, skip=sk, n_slabs=s)
        _sync(dev)
        res.append((idx.cpu().numpy(), sim.cpu().numpy()))
    for s, (idx, sim) in zip(SLABS[1:], res[1:]):
        assert np.array_equal(idx, res[0][0]), f"n_slabs {s}: other neighbours than n_slabs {SLABS[0]}"
        assert np.array_equal(sim.view(np.uint32), res[0][1].view(np.uint32)), f"n_slabs {s}: other similarity bits than n_slabs {SLABS[0]}"
    return res[0]


def reference_topk(sim64, K, skip=None):
    """the float64 similarities sorted by (-similarity, index); -1 / -inf where the gallery runs out"""
    nq, ng = sim64.shape
    idx = np.full((nq, K), -1, np.int32)
    val = np.full((nq, K), -np.inf)
    for i in range(nq):
        cand = [j for j in range(ng) if skip is None or j != skip[i]]
        cand.sort(key=lambda j: (-sim64[i, j], j))
        cand = cand[:K]
        idx[i, :len(cand)] = cand
        val[i, :len(cand)] = sim64[i, cand]
    return idx, val


# ---- top-k, exact data: every dot product is exact in f32 in any order, ties abound ------------------------------------------------
def topk_exact_case(lib, dev, nq, ng, D, K, loo):
    rng = np.random.Generator(np.random.PCG64(5))
    vals = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], np.float32)
    Q = vals[rng.integers(0, 5, (nq, D))]
    G = vals[rng.integers(0, 5, (ng, D))]
    skip = np.arange(nq, dtype=np.int32) if loo else None
    want_idx, want_sim = reference_topk(Q.astype(np.float64) @ G.astype(np.float64).T, K, skip)
    ties = sum(int((np.diff(row[np.isfinite(row)]) == 0).sum()) for row in want_sim)
    print(f"exact ({nq}, {ng}, {D}, {K}): {ties} ties inside the expected lists, {int((want_idx < 0).sum())} empty slots")
    idx, sim = _topk_all_slabs(lib, dev, Q, G, K, skip)
    assert idx.dtype == np.int32 and sim.dtype == np.float32
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(sim.astype(np.float64), want_sim)
    if loo:
        assert not (idx == skip[:, None]).any()
    if ng < K:
        assert (idx[:, ng:] == -1).all() and np.isneginf(sim[:, ng:]).all()


# ---- top-k, rounding data ----------------------------------------------------------------------------------------------------------
def rounding_data(nq, ng, D, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    Q = rng.standard_normal((nq, D), dtype=np.float32)
    G = rng.standard_normal((ng, D), dtype=np.float32)
    Q = (Q / np.linalg.norm(Q.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    G = (G / np.linalg.norm(G.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    return Q, G


def rounding_bound(Q, G):
    return Q.shape[1] * U * float((np.abs(Q).astype(np.float64) @ np.abs(G).astype(np.float64).T).max())


def check_topk_rounding(sim64, e, idx, sim, K, skip=None):
    """the three conditions of the rounding-data rule; returns (list of violations, share of queries left out of the third)"""
    bad, left_out = [], 0
    nq = sim64.shape[0]
    for i in range(nq):
        row = sim64[i].copy()
        if skip is not None:
            row[skip[i]] = -np.inf
        order = sorted(range(row.shape[0]), key=lambda j: (-row[j], j))
        best = row[order[:K + 1]]
        got = idx[i]
        if (got < 0).any() or len(set(got.tolist())) != K:
            bad.append((i, "slots"))
            continue
        if not (np.abs(sim[i].astype(np.float64) - row[got]) <= e).all():
            bad.append((i, "top_sim is further than e from the f64 similarity of its index"))
        if not (row[got] >= best[K - 1] - 2 * e).all():
            bad.append((i, "an index below the f64 K-th best - 2e"))
        if (-(np.diff(best)) > 2 * e).all():
            if not np.array_equal(got, np.array(order[:K], np.int32)):
                bad.append((i, "index list differs from the f64 list although every gap exceeds 2e"))
        else:
            left_out += 1
    return bad, left_out / nq


def topk_rounding_case(lib, dev, nq, ng, D, K):
    Q, G = rounding_data(nq, ng, D)
    sim64 = Q.astype(np.float64) @ G.astype(np.float64).T
    e = rounding_bound(Q, G)
    idx, sim = _topk_all_slabs(lib, dev, Q, G, K, None)
    worst = float(np.abs(sim.astype(np.float64) - np.take_along_axis(sim64, idx.astype(np.int64), 1)).max())
    bad, left_out = check_topk_rounding(sim64, e, idx, sim, K)
    print(f"rounding ({nq}, {ng}, {D}, {K}): e = {e:.3g}, worst |top_sim - f64| = {worst:.3g}, {left_out:.1%} of the queries left out of "
          f"the list comparison")
    assert left_out <= MAX_LEFT_OUT
    assert not bad, bad[:5]
    # the mutation: a reference that lost one gallery row (the first neighbour of query 0) must be rejected
    mutated = sim64.copy()
    mutated[:, int(idx[0, 0])] = -np.inf
    bad, _ = check_topk_rounding(mutated, e, idx, sim, K)
    assert bad, "a reference without one gallery row was accepted"


# ---- the recall kernel -------------------------------------------------------------------------------------------------------------
def recall_reference(top_idx, ql, gl, ks, num_class):
    first = np.full(len(ql), -1, np.int32)
    conf = np.zeros((num_class, num_class), np.int64)
    for i, row in enumerate(top_idx):
        hit = [k for k, j in enumerate(row) if j >= 0 and gl[j] == ql[i]]
        first[i] = hit[0] if hit else -1
        if row[0] >= 0:
            conf[gl[row[0]], ql[i]] += 1
    hits = np.array([((first >= 0) & (first < k)).sum() for k in ks], np.int64)
    return hits, first, conf


def recall_case(lib, dev):
    from dpc_amd import retrieval as R
    rng = np.random.Generator(np.random.PCG64(3))
    nq, ng, K, NC, ks = 300, 41, 6, 7, [1, 2, 5, 6]
    top = np.stack([rng.permutation(ng)[:K] for _ in range(nq)]).astype(np.int32)
    top[5, 2:] = -1                  # a short list
    top[6, :] = -1                   # no neighbour at all: no first hit, no confusion entry
    top[7, 0], top[7, 3] = -1, -1    # holes are ignored (the kernel never produces them; the ABI allows them)
    ql, gl = rng.integers(0, NC, nq), rng.integers(0, NC, ng)
    want = recall_reference(top, ql, gl, ks, NC)
    assert 0 < want[0][0] < want[0][-1] < nq and (want[1] == -1).any()
    t = lambda a: torch.from_numpy(a).to(dev)    # noqa: E731
    hits, first, conf = R.recall_at_k(lib, t(top), t(ql), t(gl), ks, NC)
    _sync(dev)
    assert hits.dtype == torch.int64 and first.dtype == torch.int32 and conf.dtype == torch.int64
    assert np.array_equal(hits.cpu().numpy(), want[0]) and np.array_equal(first.cpu().numpy(), want[1])
    assert np.array_equal(conf.cpu().numpy(), want[2]) and int(conf.sum()) == nq - 2
    hits2, first2, conf2 = R.recall_at_k(lib, t(top), t(ql), t(gl), ks, NC, out=(hits, conf))    # a second call accumulates
    _sync(dev)
    assert hits2 is hits and conf2 is conf
    assert np.array_equal(hits.cpu().numpy(), 2 * want[0]) and np.array_equal(conf.cpu().numpy(), 2 * want[2])
    assert np.array_equal(first2.cpu().numpy(), want[1])


# ---- the embedding kernels ---------------------------------------------------------------------------------------------------------
def embed_bound(ref64, n_rows, D):
    """|out - ref| allowed per component: n_rows additions, the division, D squares and additions, the square root and the last
    division, each within 2^-24 relative"""
    return (n_rows + D + 4) * U * np.abs(ref64) + 1e-12


def embed_reference(rows64):
    m = rows64.mean(0)
    return m / max(float(np.sqrt((m * m).sum())), 1e-12)


def embed_kernels_case(lib, dev, D):
    rng = np.random.Generator(np.random.PCG64(17))
    rows, ld, nv = 6, D + 4, 4
    f32, nan = torch.float32, float("nan")
    esum, count = torch.zeros(D, dtype=f32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((D,), 7.0, dtype=f32, device=dev)
    call = lambda name, *a: lib.call(name, *a, lib.stream())    # noqa: E731
    chunks = []
    for _ in range(2):
        ctx = np.full((rows, ld), nan, np.float32)
        ctx[:nv, :D] = rng.uniform(0.25, 1.0, (nv, D)).astype(np.float32) * np.where(np.arange(D) % 3 == 0, -1.0, 1.0).astype(np.float32)
        chunks.append(ctx)
        call("dpc_embed_accumulate", torch.from_numpy(ctx).to(dev), rows, nv, D, ld, esum, count)
    _sync(dev)
    assert int(count.cpu()) == 2 * nv and torch.isfinite(esum).all()
    call("dpc_embed_finish", esum, count, D, 1e-12, out)
    _sync(dev)
    ref = embed_reference(np.concatenate([c[:nv, :D] for c in chunks]).astype(np.float64))
    got = out.cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    print(f"embedding kernels D = {D}: worst error / bound {float((err / embed_bound(ref, 2 * nv, D)).max()):.3g}, |out| = {np.linalg.norm(got):.9f}")
    assert (err <= embed_bound(ref, 2 * nv, D)).all()
    assert int(count.cpu()) == 0 and not esum.cpu().numpy().any()                       # the state is cleared
    # count == 0 writes nothing
    out.fill_(7.0)
    call("dpc_embed_finish", esum, count, D, 1e-12, out)
    _sync(dev)
    assert (out.cpu() == 7.0).all()
    # a zero vector stays zero (F.normalize's eps)
    call("dpc_embed_accumulate", torch.zeros(rows, ld, dtype=f32, device=dev), rows, nv, D, ld, esum, count)
    call("dpc_embed_finish", esum, count, D, 1e-12, out)
    _sync(dev)
    assert not out.cpu().numpy().any() and int(count.cpu()) == 0


# ---- LCEngine.embed_video ----------------------------------------------------------------------------------------------------------
def chunk_video():
    """the 36-frame video of the existing chunk case: 5 windows"""
    from dpc_amd.data import draw_lc, lc_test_windows
    video = long_video(base_frames(), 36)
    starts = lc_test_windows(36, N, SL, DS, "ucf101")
    assert len(starts) == 5
    return video, starts, draw_lc(80, 60, CROP, SIZE, N * SL, "test")


def by_hand_embedding(twin, video, starts, clip, bn):
    """forward chunk by chunk on a twin engine, ``ctx`` read after each; float64 mean over the valid rows, normalised"""
    from dpc_amd.data import video_windows_to_input
    B, dev = twin.B, twin.device
    vid = torch.from_numpy(video).to(dev)
    rows = []
    for i in range(0, len(starts), B):
        st = list(starts[i:i + B])
        nv = len(st)
        st = st + [st[-1]] * (B - nv)
        video_windows_to_input(twin.lib, vid, video.shape[0], st, clip, N, SL, DS, SIZE, None, twin.x_s2d)
        if bn == "batch":
            twin.forward(None, torch.zeros(B, dtype=torch.int64), train=True, gru_masks=torch.ones(N, twin.M, twin.D),
                         fc_mask=torch.ones(B, twin.D))
        else:
            twin.forward(None, torch.zeros(B, dtype=torch.int64), train=False)
        rows.append(twin.ctx[:nv].double().cpu().numpy().copy())
    rows = np.concatenate(rows)
    assert rows.shape[0] == len(starts) and np.isfinite(rows).all()
    return embed_reference(rows), rows.shape[0]


def embed_video_case(lib, dev, widths, dtype, B, bn, graph=False, check=True):
    """two videos through ONE engine, each against the by-hand expectation of a twin engine (so the second is unaffected by the
    first; on the MI355X, where a forward is cheap, the first goes through once more and must give the same bits); every BUF
    tensor is the same bits afterwards; returns the rows.  check=False: the rows only (another case compares them)"""
    video, starts, clip = chunk_video()
    second = np.ascontiguousarray(video[::-1])
    eng = make_engine(lib, dev, dtype, widths, B, num_class=11)
    D = eng.D
    before = {k: v.clone() for k, v in eng.BUF.items()}
    passes = (video, second) if str(dev) == "cpu" else (video, second, video)
    emb = torch.zeros(len(passes), D, dtype=torch.float32, device=dev)
    for row, v in enumerate(passes):
        eng.embed_video(v, starts, clip, emb[row], ds=DS, bn=bn, graph=graph)
    _sync(dev)
    assert before and all(torch.equal(before[k], eng.BUF[k]) for k in before), "a running buffer moved"
    got = emb.cpu().numpy()
    assert np.isfinite(got).all() and not np.array_equal(got[0], got[1])
    if len(passes) == 3:
        assert np.array_equal(got[0], got[2]), "the second video left something behind"
    if not check:
        return got[:2]
    twin = make_engine(lib, dev, dtype, widths, B, num_class=11)
    for row, v in enumerate((video, second)):
        ref, n = by_hand_embedding(twin, v, starts, clip, bn)
        err = np.abs(got[row].astype(np.float64) - ref)
        bound = embed_bound(ref, n, D)
        print(f"embed_video {dtype} B = {B} bn = {bn} graph = {graph} video {row}: worst error / bound {float((err / bound).max()):.3g}, "
              f"|row| = {np.linalg.norm(got[row].astype(np.float64)):.9f}")
        assert (err <= bound).all()
    return got[:2]


def embed_video_errors_case(lib, dev, widths):
    import pytest
    video, starts, clip = chunk_video()
    eng = make_engine(lib, dev, "f32", widths, 2, num_class=11)
    row = torch.zeros(eng.D, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="batch"):
        eng.embed_video(video, starts, clip, row, ds=DS, bn="batch", graph=True)
    with pytest.raises(ValueError, match="running"):
        eng.embed_video(video, starts, clip, row, ds=DS, bn="eval")
    with pytest.raises(ValueError, match="out_row"):
        eng.embed_video(video, starts, clip, torch.zeros(eng.D + 1, dtype=torch.float32, device=dev), ds=DS)
    with pytest.raises(ValueError, match="without windows"):
        eng.embed_video(video, [], clip, row, ds=DS)


# ---- the entry ---------------------------------------------------------------------------------------------------------------------
F_ENTRY = 18                                # 2 windows per video: one chunk at B = 2
ENTRY_LABELS = (0, 1, 2, 3, 0, 1, 2, 2)     # videos 2 and 7 are byte-identical copies with the same label
COPIES = (2, 7)


def entry_files(tmp):
    """eight short videos in four classes (two of them the same bytes), and a checkpoint of the engine the entry builds"""
    videos = variants(long_video(base_frames(), F_ENTRY), 8, 23)
    videos[COPIES[1]] = videos[COPIES[0]]
    fp, lp = os.path.join(tmp, "videos.npy"), os.path.join(tmp, "labels.npy")
    np.save(fp, videos)
    np.save(lp, np.array(ENTRY_LABELS))
    return fp, lp


def entry_argv(fp, lp, ckpt, B, dtype, extra=()):
    return ["--net", "resnet18", "--img_dim", str(SIZE), "--batch_size", str(B), "--gpu", "0", "--dtype", dtype, "--num_seq", str(N),
            "--seq_len", str(SL), "--ds", str(DS), "--dataset", "ucf101", "--crop", str(CROP), "--frames", fp, "--labels", lp,
            "--retrieval", ckpt, "--retrieval_k", "1,2,5"] + list(extra)


def save_checkpoint(lib, dev, widths, dtype, B, path):
    eng = make_engine(lib, dev, dtype, widths, B)
    torch.save({"epoch": 3, "state_dict": {"module." + k: v.cpu() for k, v in eng.state_dict().items()}}, path)


def check_entry_outputs(npz_path, out, log_text, cross, bn="running"):
    """every number of the .npz and of the printed line against a numpy recomputation from the saved embeddings"""
    z = np.load(npz_path)
    assert sorted(z.files) == sorted(["query_emb", "gallery_emb", "query_labels", "gallery_labels", "top_idx", "top_sim", "first_hit", "ks",
                                      "recall", "confusion"])
    Q, G, ql, gl = z["query_emb"], z["gallery_emb"], z["query_labels"], z["gallery_labels"]
    idx, sim, ks = z["top_idx"], z["top_sim"], z["ks"].tolist()
    nq, K = idx.shape
    assert ks == [1, 2, 5] and K == 5 and Q.dtype == np.float32 and Q.shape[0] == len(ENTRY_LABELS) and np.array_equal(ql, ENTRY_LABELS)
    assert np.array_equal(G, Q) and np.array_equal(gl, ql)
    assert np.allclose(np.linalg.norm(Q.astype(np.float64), axis=1), 1.0, atol=1e-6)
    sim64 = Q.astype(np.float64) @ G.astype(np.float64).T
    skip = None if cross else np.arange(nq)
    bad, left_out = check_topk_rounding(sim64, rounding_bound(Q, G), idx, sim, K, skip)
    assert not bad, bad
    a, b = COPIES
    if cross:     # the query itself is in the gallery: its own row or its copy comes first
        assert all(idx[i, 0] == i or {i, int(idx[i, 0])} == set(COPIES) for i in range(nq)), idx[:, 0]
    else:
        assert idx[a, 0] == b and idx[b, 0] == a and sim[a, 0] >= 1 - 1e-6 and sim[b, 0] >= 1 - 1e-6
        assert not (idx == np.arange(nq)[:, None]).any()
    hits, first, conf = recall_reference(idx, ql, gl, ks, 101)
    assert np.array_equal(z["first_hit"], first) and np.array_equal(z["confusion"], conf) and z["confusion"].dtype == np.int64
    assert np.array_equal(z["recall"], hits.astype(np.float64) / nq)
    if not cross:
        assert z["recall"][0] >= 2 / 8
    line = " ".join("R@{}: {:.4f}".format(k, r) for k, r in zip(ks, hits / nq)) + "  ({} queries, {} gallery videos, {}, bn {})".format(
        nq, nq, "cross" if cross else "leave-one-out", bn)
    assert re.search("^" + re.escape(line) + "$", out, re.M), (line, out)
    assert "(retrieval checkpoint epoch 3)" in out and re.search(r"^0 videos skipped \(too short", out, re.M)
    if log_text is not None:
        assert re.fullmatch(r"## Epoch 3:\ntime: \d{4}(_\d\d){5}\n" + re.escape(line) + r"\n\n", log_text), log_text
    print(f"entry ({'cross' if cross else 'leave-one-out'}): {line}; {left_out:.0%} of the queries left out of the list comparison")
