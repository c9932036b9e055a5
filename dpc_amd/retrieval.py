"""Nearest-neighbour video retrieval over the kernels of csrc/retrieval.hip: "how good is this checkpoint?" without a fine-tuning run.

One L2-normalised embedding per video (``LCEngine.embed_video``: the mean over the video's test windows of the spatial mean of the
last ConvGRU state, then ``F.normalize``), cosine neighbours looked up in a gallery (``knn_topk``), recall@k -- does one of the k
nearest gallery videos carry the query's class? -- and the 1-NN confusion matrix (``recall_at_k``).  Thin, validating wrappers over
the C ABI: every arithmetic op is a kernel, nothing crosses to the host, and CPU tensors raise unless the simulator handle of the
CPU test tier is passed.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L

MAX_K, MAX_SLABS, MAX_D = 64, 64, 256


def _lib_for(lib: Optional[L.Lib], t: torch.Tensor) -> L.Lib:
    return L.lib_for(t.device, lib)


def _rows_f32(name: str, t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 [rows, D] tensor")
    if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 4 or t.data_ptr() % 16:
        raise ValueError(f"{name}: rows must be contiguous and 16-byte aligned")
    return t


def knn_topk(lib: Optional[L.Lib], Q: torch.Tensor, G: torch.Tensor, K: int, skip: Optional[torch.Tensor] = None,
             n_slabs: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """(top_idx int32 [nq, K], top_sim f32 [nq, K]): per row of Q the K rows of G with the largest dot product, ordered by
    (similarity descending, index ascending); slots without a candidate hold -1 / -inf.  skip int32 [nq]: query i never returns row
    skip[i] (-1: none; leave-one-out passes arange).  n_slabs: 0 = chosen by the library, 1..64 forced -- the result is the same
    bits either way.  Inputs must be finite."""
    Q, G = _rows_f32("Q", Q), _rows_f32("G", G)
    lib = _lib_for(lib, Q)
    nq, D = Q.shape
    ng = G.shape[0]
    K, n_slabs = int(K), int(n_slabs)
    if G.device != Q.device or G.shape[1] != D:
        raise ValueError("Q and G must live on one device and share their width")
    if nq < 1 or ng < 1:
        raise ValueError("Q and G need at least one row each")
    if D % 32 or not 32 <= D <= MAX_D:
        raise ValueError(f"D = {D}: the similarity kernel takes multiples of 32 in [32, {MAX_D}]")
    if not 1 <= K <= MAX_K:
        raise ValueError(f"K = {K} is outside [1, {MAX_K}]")
    if not 0 <= n_slabs <= MAX_SLABS:
        raise ValueError(f"n_slabs = {n_slabs} is outside [0, {MAX_SLABS}]")
    if skip is not None and (skip.dtype != torch.int32 or tuple(skip.shape) != (nq,) or skip.device != Q.device or not skip.is_contiguous()):
        raise ValueError("skip must be a contiguous int32 [nq] tensor on the device of Q")
    ws_bytes = lib.call("dpc_knn_ws_bytes", nq, K, n_slabs)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=Q.device)
    top_sim = torch.empty(nq, K, dtype=torch.float32, device=Q.device)
    top_idx = torch.empty(nq, K, dtype=torch.int32, device=Q.device)
    lib.call("dpc_knn_topk", Q, nq, Q.stride(0), G, ng, G.stride(0), D, K, skip, n_slabs, top_sim, top_idx, ws, ws_bytes, lib.stream())
    return top_idx, top_sim


def recall_at_k(lib: Optional[L.Lib], top_idx: torch.Tensor, q_labels: torch.Tensor, g_labels: torch.Tensor, ks: Sequence[int],
                num_class: int, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """(hits int64 [len(ks)], first_hit int32 [nq], confusion int64 [num_class, num_class]) of a neighbour table: first_hit[i] = the
    0-based rank of the first neighbour with query i's label (-1: none), hits[j] = #{i : first_hit[i] < ks[j]}, confusion[label of
    the first neighbour][label of the query].  Labels int64 in [0, num_class) -- the caller's to guarantee, the kernel ignores others
    in the confusion matrix.  out = (hits, confusion) of an earlier call: this call's counts are added onto them."""
    if not isinstance(top_idx, torch.Tensor) or top_idx.dim() != 2 or top_idx.dtype != torch.int32 or not top_idx.is_contiguous():
        raise ValueError("top_idx must be a contiguous int32 [nq, K] tensor")
    lib = _lib_for(lib, top_idx)
    dev = top_idx.device
    nq, K = top_idx.shape
    ks = [int(k) for k in ks]
    num_class = int(num_class)
    if not ks or any(k < 1 or k > K for k in ks) or any(a >= b for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks = {ks} must be ascending and inside [1, K = {K}]")
    if num_class < 1 or nq < 1:
        raise ValueError("num_class and the number of queries must be positive")
    for name, t, n in (("q_labels", q_labels, nq), ("g_labels", g_labels, None)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.device != dev or not t.is_contiguous() or \
                (n is not None and t.shape[0] != n) or t.shape[0] < 1:
            raise ValueError(f"{name} must be a contiguous int64 vector on the device of top_idx" + (f" with {n} entries" if n else ""))
    ks_t = torch.tensor(ks, dtype=torch.int32).to(dev)
    if out is None:
        hits = torch.zeros(len(ks), dtype=torch.int64, device=dev)
        confusion = torch.zeros(num_class, num_class, dtype=torch.int64, device=dev)
    else:
        hits, confusion = out
        if hits.dtype != torch.int64 or tuple(hits.shape) != (len(ks),) or confusion.dtype != torch.int64 or \
                tuple(confusion.shape) != (num_class, num_class) or hits.device != dev or confusion.device != dev:
            raise ValueError("out = (hits int64 [len(ks)], confusion int64 [num_class, num_class]) on the device of top_idx")
    first_hit = torch.empty(nq, dtype=torch.int32, device=dev)
    lib.call("dpc_knn_recall", top_idx, nq, K, q_labels, g_labels, g_labels.shape[0], num_class, ks_t, len(ks), hits, first_hit, confusion,
             lib.stream())
    return hits, first_hit, confusion
