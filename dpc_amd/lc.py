"""Downstream action classifier ``LC`` (eval/model_3d_lc.py:12-65, driven by eval/test.py) on the MI355X kernels --
SURVEY.md section 8 f3.

Same 2d3d-ResNet and ConvGRU kernels as the DPC-RNN step; what differs from ``DPC_RNN``:
  * the backbone's BatchNorm3d layers track running statistics (``track_running_stats=True``, model_3d_lc.py:27-29):
    batch statistics + buffer update in train mode, running buffers in eval mode;
  * ReLU BEFORE the temporal mean (model_3d_lc.py:52-54), then the ConvGRU aggregates ALL num_seq blocks and only its last
    state is used (``context[:, -1]``, model_3d_lc.py:57-58);
  * head: spatial mean -> BatchNorm1d -> Dropout(p) -> Linear(num_class); loss = CrossEntropyLoss on the clip label,
    accuracy = top-1 (eval/test.py:244-255).

``LCEngine`` is the static-schedule engine (forward / backward / fused Adam on flat arenas, like ``DPCEngine``; its captured steps
are ``BackboneEngine.capture_train_step`` / ``capture_eval_step``, which it serves through ``_forward_loss`` and
``_backward_reaches_backbone``);
``LC`` is the drop-in ``nn.Module`` with the reference's constructor, ``forward(block) -> (output, context)`` and
state_dict keys (running buffers included), so ``--pretrain`` of a DPC checkpoint and ``--test`` files load by key.
In train mode the module's outputs carry an autograd node (``_LCOutput``), so the training lines of eval/test.py:224-255 run
unchanged over it, with ``dpc_amd.optim.Adam`` as the optimizer: one parameter group per parameter (``--train_what ft``,
eval/test.py:76-84), a 10x smaller backbone lr, or a linear probe on a frozen extractor (``requires_grad_(False)``), where the
backward stops in front of the frozen part.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from .engine import BN_EPS, BackboneEngine, LAYER_WIDTH, param_shapes
from .model import _REPLICA_ERROR, _EngineModule, _attach, _init_reference_style


def lc_param_shapes(network: str, num_class: int, widths: Sequence[int] = LAYER_WIDTH) -> "Dict[str, Tuple[int, ...]]":
    """trainable parameters of LC in the reference's registration order (model_3d_lc.py:29-45)"""
    base = param_shapes(network, widths)
    out = {k: v for k, v in base.items() if not k.startswith("network_pred.")}
    D = widths[3]
    out["final_bn.weight"] = (D,)
    out["final_bn.bias"] = (D,)
    out["final_fc.1.weight"] = (num_class, D)
    out["final_fc.1.bias"] = (num_class,)
    return out


def lc_state_dict_keys(network: str, num_class: int, widths: Sequence[int] = LAYER_WIDTH):
    """every state_dict key of the reference LC, in order: parameters interleaved with the BatchNorm buffers
    (weight, bias, running_mean, running_var, num_batches_tracked), the ConvGRU alias keys after the cell's own"""
    keys = []
    shapes = lc_param_shapes(network, num_class, widths)
    names = list(shapes)
    for i, k in enumerate(names):
        keys.append(k)
        is_bn_bias = k.endswith(".bias") and (".bn" in k or k.startswith("backbone.bn1") or "downsample.1" in k or k.startswith("final_bn"))
        if is_bn_bias:
            pre = k[: -len("bias")]
            keys += [pre + "running_mean", pre + "running_var", pre + "num_batches_tracked"]
        if k == "agg.ConvGRUCell_00.out_gate.bias":
            keys += [n.replace("agg.ConvGRUCell_00.", "agg.cell_list.0.") for n in names if n.startswith("agg.ConvGRUCell_00.")]
    return keys


class LCEngine(BackboneEngine):
    """forward / loss / backward / Adam of the LC classifier as fixed kernel sequences (no autograd graph)"""

    def __init__(self, network: str = "resnet18", sample_size: int = 128, num_seq: int = 8, seq_len: int = 5, batch: int = 4,
                 device="cuda", compute_dtype=torch.float32, widths: Sequence[int] = LAYER_WIDTH, lib: Optional[L.Lib] = None,
                 lr: float = 1e-3, wd: float = 1e-3, dropout: float = 0.5, num_class: int = 101, gru_dropout: float = 0.1,
                 seed: int = 666):
        self.num_class = int(num_class)
        self.p_drop_fc = float(dropout)
        super().__init__(lc_param_shapes(network, self.num_class, widths), network, sample_size, num_seq, seq_len, batch, device,
                         compute_dtype, widths, lib, lr, wd, gru_dropout, seed, bn_running=True)
        self._build_head()
        self._finish_buffers()

    # ---- head: ConvGRU over all N blocks (P = 0) + BatchNorm1d / Dropout / Linear / CE
    def _build_head(self):
        B, N, SQ, D, dt, NC = self.B, self.N, self.SQ, self.D, self.cdtype, self.num_class
        f32 = torch.float32
        self._build_gru(n_agg=N, n_steps=N, P=0)
        M = self.M
        self.d_hlast = self.empty((M, D), f32)
        self._ran_backbone_backward = True
        self._eval_ran = False   # an eager eval-mode forward has run (test_video(graph=True) replays only after one)
        self.d_context = self.empty((B, D), f32)   # an upstream d loss / d context (backward's d_context) is staged here
        self.BUF["final_bn.running_mean"] = torch.zeros(D, dtype=f32, device=self.device)
        self.BUF["final_bn.running_var"] = torch.ones(D, dtype=f32, device=self.device)
        self.BUF["final_bn.num_batches_tracked"] = torch.zeros((), dtype=torch.int64, device=self.device)
        self.target = torch.zeros(B, dtype=torch.int64, device=self.device)
        self.ctx, self.xhat, self.context, self.y_drop, self.dctx = (self.empty((B, D), f32) for _ in range(5))
        self.bn1d_stat = self.empty((2, D), f32)
        self.logits, self.dlogits = self.empty((B, NC), f32), self.empty((B, NC), f32)
        self.row_ws, self.result = self.empty((B, 2), f32), self.empty((2,), f32)
        Pm, gd = self.PRM, self.gru_desc
        for name, t in (("bias_1", Pm["agg.ConvGRUCell_00.out_gate.bias"]), ("bias_2", Pm["agg.ConvGRUCell_00.out_gate.bias"]),  # unused (P = 0)
                        ("d_hlast", self.d_hlast)):
            setattr(gd, name, t.data_ptr())
        hd = self.head_desc = L.LcHeadDesc()
        hd.dtype, hd.B, hd.SQ, hd.D, hd.num_class, hd.train = L.dtype_code(dt), B, SQ, D, NC, 1
        hd.p_drop, hd.momentum, hd.eps, hd.seed = self.p_drop_fc, self.BN_MOMENTUM, BN_EPS, self.seed  # own Philox stream id, same key
        G = self.G
        for name, t in (("h_last", self.H_all[N]), ("bn_weight", Pm["final_bn.weight"]), ("bn_bias", Pm["final_bn.bias"]),
                        ("bn_running_mean", self.BUF["final_bn.running_mean"]), ("bn_running_var", self.BUF["final_bn.running_var"]),
                        ("bn_num_batches", self.BUF["final_bn.num_batches_tracked"]), ("fc_weight", Pm["final_fc.1.weight"]),
                        ("fc_bias", Pm["final_fc.1.bias"]), ("target", self.target), ("ctx", self.ctx), ("xhat", self.xhat),
                        ("bn_out", self.context), ("y", self.y_drop), ("stat", self.bn1d_stat), ("logits", self.logits),
                        ("dlogits", self.dlogits), ("row_ws", self.row_ws), ("result", self.result),
                        ("g_fc_weight", G["final_fc.1.weight"]), ("g_fc_bias", G["final_fc.1.bias"]),
                        ("g_bn_weight", G["final_bn.weight"]), ("g_bn_bias", G["final_bn.bias"]), ("dctx", self.dctx),
                        ("d_hlast", self.d_hlast)):
            setattr(hd, name, t.data_ptr())

    # ---- state_dict with the running buffers, reference key order
    def load_params(self, params: Dict[str, torch.Tensor]):
        own = {k: v for k, v in params.items() if (k[7:] if k.startswith("module.") else k) not in self.BUF}
        super().load_params(own)
        for k, v in params.items():
            k2 = k[7:] if k.startswith("module.") else k
            if k2 in self.BUF:
                self.BUF[k2].copy_(v.to(self.BUF[k2].dtype).reshape(self.BUF[k2].shape))

    def state_dict(self) -> Dict[str, torch.Tensor]:
        self._not_swapped("state_dict")
        self._not_mid_cycle("state_dict")
        out = {}
        for k in lc_state_dict_keys(self.network, self.num_class, self.widths):
            if k in self.PRM:
                out[k] = self.PRM[k].detach().clone()
            elif k in self.BUF:
                out[k] = self.BUF[k].detach().clone()
            else:
                out[k] = out[k.replace("agg.cell_list.0.", "agg.ConvGRUCell_00.")]
        return out

    # ---- forward (model_3d_lc.py:47-65) + loss / accuracy (eval/test.py:244-255)
    def set_labels(self, target: torch.Tensor):
        """copy the class labels [B] of the next forward(block, None) / train_step(block, None) / captured step into ``self.target``
        (eagerly: a host tensor is a host-to-device copy, so never inside a capture)"""
        self.target.copy_(target.reshape(self.B).to(self.device, torch.int64))

    def fill_synthetic(self, seed: int, block: Optional[torch.Tensor] = None):
        """BackboneEngine.fill_synthetic (advances dev_input, draws the batch), then the batch's labels into ``self.target`` under the
        same seed and the same draw counter (csrc/labels.hip).  Follow with forward(None, None, ...) / train_step(None, None).
        Graph-safe: no host value changes between replays, the counter is read on the device."""
        super().fill_synthetic(seed, block)
        self.call("dpc_synthetic_labels", self.target, self.B, self.num_class, int(seed) & 0xFFFFFFFFFFFFFFFF, self.dev_input)

    def forward(self, block: torch.Tensor, target: Optional[torch.Tensor] = None, train: bool = False,
                gru_masks: Optional[torch.Tensor] = None, fc_mask: Optional[torch.Tensor] = None):
        """block [B,N,3,SL,H,W] f32 (None: the stem's operand as it stands), target [B] int64 class labels (None: the labels as they
        stand in ``self.target``: set_labels / fill_synthetic).  Returns (output [B,1,num_class], context [B,1,D]) as the
        reference does; ``self.result`` = device f32[2] (mean CE loss, top-1 accuracy).  gru_masks [N,M,D] / fc_mask [B,D]:
        optional explicit pre-scaled dropout masks (tests); train=True without them draws Philox masks in the kernels."""
        B, N, SQ, D, M = self.B, self.N, self.SQ, self.D, self.M
        if block is not None and (tuple(block.shape) != (B, N, 3, self.SL, self.size, self.size) or block.dtype != torch.float32):
            raise ValueError(f"block must be float32 [B,N,3,SL,H,W] = {(B, N, 3, self.SL, self.size, self.size)}")
        self.train_mode = bool(train)
        if target is not None:
            self.set_labels(target)
        if not train:
            self._eval_ran = True   # the eval-mode forward has allocated what it allocates on first use (capture_eval_step's rule)
        x = self._backbone_forward(block)
        dc = L.dtype_code(self.cdtype)
        self.call("dpc_relu_tpool_fwd", x, dc, B, N, self.feat_shape[1], SQ, D, self.feat_relu)
        gd, hd = self.gru_desc, self.head_desc
        self._keep = (gru_masks, fc_mask)  # explicit masks must outlive the launches
        if gru_masks is not None:
            gru_masks = gru_masks.to(self.device, torch.float32).contiguous()
            self._keep = (gru_masks, fc_mask)
        gd.drop_masks = gru_masks.data_ptr() if gru_masks is not None else None
        if train and (gru_masks is None or fc_mask is None):
            self.call("dpc_counter_advance", self.dev_draw)
        gd.step_dev = self.dev_draw.data_ptr() if (gru_masks is None and train and self.p_drop > 0) else None
        self.call("dpc_gru_chain_fwd", C.byref(gd))
        if fc_mask is not None:
            fc_mask = fc_mask.to(self.device, torch.float32).contiguous()
            self._keep = (gru_masks, fc_mask)
        hd.train = int(train)
        hd.drop_mask = fc_mask.data_ptr() if fc_mask is not None else None
        hd.step_dev = self.dev_draw.data_ptr()
        self.call("dpc_lc_head_fwd", C.byref(hd))
        return self.logits.view(B, 1, self.num_class), self.context.view(B, 1, D)

    def grad_wanted(self, wanted=None) -> Tuple[bool, bool]:
        """(backbone, agg): whether any ``backbone.*`` / ``agg.*`` parameter needs a gradient.  wanted: the names that do, when the
        caller knows (the module boundary passes what autograd asks for, and nothing else counts there).  None = the engine-owned
        step: a parameter needs none when the grouped Adam leaves it alone (set_param_groups: frozen, or in no group) or it is
        listed in ``no_grad_params``.  The backward stops at these two cut points only."""
        if wanted is None:
            skip = set(self.frozen_params()) | set(self.no_grad_params)
            wanted = [k for k in self.offsets if k not in skip]
        backbone = any(k.startswith("backbone.") for k in wanted)
        return backbone, backbone or any(k.startswith("agg.") for k in wanted)

    def _first_bucket(self) -> torch.Tensor:
        """nothing of stem + layer1 to exchange when the backward stopped in front of the backbone (their slices hold no gradient)"""
        return self.flat_g[:self.grad_split] if self._ran_backbone_backward else self.flat_g[:0]

    def backward(self, on_tail_ready=None, d_output: Optional[torch.Tensor] = None, d_context: Optional[torch.Tensor] = None,
                 wanted=None):
        """Gradients of the last train-mode forward w.r.t. every parameter that needs one.  Without arguments: of the mean CE loss
        (the forward's CE kernel left d loss / d logits in ``dlogits``).  Upstream form (torch autograd through LC.forward):
        d_output [B,1,num_class] = d loss / d output replaces the CE gradient, d_context [B,1,D] = d loss / d context enters at the
        BatchNorm1d output, ahead of the Dropout (``context`` is returned before it, model_3d_lc.py:60-64); either may be None (zero).

        Truncation: when no ``backbone.*`` parameter needs a gradient (grad_wanted(wanted); wanted = the parameter names autograd asks
        for at the module boundary, None = decided by the optimizer groups) the ReLU / temporal-mean backward and the
        backbone's backward are not launched; when no ``agg.*`` parameter does either, neither are the ConvGRU's.  The gradient
        slices of those parameters keep whatever they held.  The BatchNorm layers of such a frozen backbone still ran on batch
        statistics and updated their running buffers in the forward -- requires_grad = False in torch, not .eval()."""
        if not self.train_mode:
            raise L.DpcError("LCEngine.backward needs a train-mode forward (BatchNorm with batch statistics)")
        B, N, SQ, D = self.B, self.N, self.SQ, self.D
        dc = L.dtype_code(self.cdtype)
        hd = self.head_desc
        if d_output is not None or d_context is not None:
            if d_output is None:
                self.dlogits.zero_()
            else:
                self.dlogits.copy_(d_output.reshape(B, self.num_class))
            if d_context is not None:
                self.d_context.copy_(d_context.reshape(B, D))
        hd.d_bn_out = self.d_context.data_ptr() if d_context is not None else None
        self.call("dpc_lc_head_bwd", C.byref(hd))
        hd.d_bn_out = None
        need_backbone, need_agg = self.grad_wanted(wanted)
        self._ran_backbone_backward = need_backbone
        if need_agg:
            self.call("dpc_gru_chain_bwd", C.byref(self.gru_desc))
            self._gru_param_grads(dc)
        if not need_backbone:
            if on_tail_ready is not None:   # the two-bucket exchange still gets its tail (the head's gradients live there; the
                # frozen layers' slices in it travel along: one bucket, one collective); the first bucket is skipped (_first_bucket)
                self.side_join()
                on_tail_ready(self.flat_g[self.grad_split:])
            return
        self.call("dpc_relu_tpool_bwd", self.blocks[-1].out, self.d_featrelu, dc, B, N, self.feat_shape[1], SQ, D, self.d_feat)
        self._backbone_backward(self.d_feat, on_tail_ready)

    def _forward_loss(self, block: Optional[torch.Tensor], train: bool):
        """the CE kernel is the last launch of forward(); the labels are those in ``self.target``"""
        self.forward(block, None, train=train)

    def _backward_reaches_backbone(self) -> bool:
        """grad_wanted() of the engine-owned step: the optimizer's groups and no_grad_params decide.  A frozen backbone truncates
        the backward, and the two-bucket exchange of such a step has an empty first bucket (_first_bucket)"""
        return self.grad_wanted()[0]

    def train_step(self, block: torch.Tensor, target: Optional[torch.Tensor] = None, allreduce=None, **masks) -> torch.Tensor:
        """forward + CE / accuracy + backward (+ gradient all-reduce) + Adam; returns device f32[2] = loss, top-1.
        target=None: the labels as they stand in ``self.target``"""
        self._not_swapped("train_step")
        self.forward(block, target, train=True, **masks)
        if self._accum_n > 1:   # one micro-batch of the cycle (set_grad_accum)
            self._accum_micro_step(allreduce)
            return self.result
        self._backward_and_exchange(allreduce)
        self.adam_step()
        return self.result

    def _baked_scalars(self) -> tuple:
        """a captured step (engine.BackboneEngine.capture_train_step / capture_eval_step) also carries the head's dropout and seed"""
        hd = self.head_desc
        return super()._baked_scalars() + (float(hd.p_drop), int(hd.seed))

    # ---- the video-level test of eval/test.py:303-343 (csrc/lc_test.hip): per-video state, run totals and the confusion matrix on the device
    def test_reset(self):
        """zero the run totals (sum loss, sum top-1, sum top-5, videos), the confusion matrix [pred][target] and the per-video state"""
        NC, f32 = self.num_class, torch.float32
        z = lambda *shape, dt=f32: torch.zeros(*shape, dtype=dt, device=self.device)   # noqa: E731
        self.test_psum, self.test_lsum, self.test_count = z(NC), z(NC), z(1, dt=torch.int32)
        self.test_prob, self.test_res = z(NC), z(4)
        self.test_totals, self.test_confusion = z(4, dt=torch.float64), z(NC, NC, dt=torch.int64)
        self.test_label = torch.zeros(self.B, dtype=torch.int64)

    def test_video(self, frames_u8, label: int, starts, clip: dict, ds: int = 3, vlen: Optional[int] = None, graph: bool = False):
        """one video of the test protocol: frames_u8 uint8 [vlen, H0, W0, 3] (host array or tensor; uploaded ONCE), its class label,
        the window start frames (data.lc_test_windows) and the test recipe's draw (data.draw_lc(..., 'test')).  Per chunk of B windows:
        gather into the stem's operand (dpc_video_windows_to_input) -> eval-mode forward -> dpc_lc_test_accumulate with the chunk's
        valid count; the last chunk is padded by repeating its last window (finite rows; eval-mode BatchNorm uses running statistics,
        so rows do not see each other) and its padding rows are never summed.  Then dpc_lc_test_finish.  Nothing crosses to the
        host: ``test_res`` (loss, top-1, top-5, pred), ``test_prob`` (mean probability) hold this video, ``test_totals`` /
        ``test_confusion`` the run (``test_reset`` starts one).  graph=True: the per-chunk forward is a replay of capture_eval_step()
        (the label is set once per video; the gather and the accumulation, whose arguments differ per chunk, stay eager; the engine's
        first eval-mode forward is eager, as capture_eval_step asks)."""
        if not hasattr(self, "test_totals"):
            self.test_reset()
        label = int(label)
        if not 0 <= label < self.num_class:
            raise ValueError(f"label {label} is outside [0, {self.num_class})")
        self.test_label.fill_(label)
        if graph:
            self.check_graph_capture()
            self.set_labels(self.test_label)

        def forward():
            if not graph:
                self.forward(None, self.test_label, train=False)
            else:
                self._eval_forward_replayed()

        self._video_chunks(frames_u8, starts, clip, ds, vlen, forward, lambda n_valid: self.call(
            "dpc_lc_test_accumulate", self.logits, self.B, n_valid, self.num_class, self.num_class, self.test_psum, self.test_lsum,
            self.test_count))
        self.call("dpc_lc_test_finish", self.test_psum, self.test_lsum, self.test_count, self.num_class, label, self.test_prob, self.test_res,
                  self.test_totals, self.test_confusion)

    def _eval_forward_replayed(self):
        """the eval-mode forward on the operand and labels as they stand, as a replay of capture_eval_step() -- eagerly the first
        time, as capture_eval_step asks"""
        if not self._eval_ran:
            self.forward(None, None, train=False)
        else:
            self.capture_eval_step()()

    def _video_chunks(self, frames_u8, starts, clip: dict, ds: int, vlen: Optional[int], forward, reduce):
        """the chunk loop of the video-level protocols: the video is uploaded ONCE; per chunk of B windows: gather into the stem's
        operand (dpc_video_windows_to_input; the last chunk is padded by repeating its last window), forward(), reduce(valid rows)"""
        from .data import video_windows_to_input
        starts = [int(s) for s in starts]
        if not starts:
            raise ValueError("a video without windows is skipped by the caller (data.lc_test_windows returned none)")
        video = frames_u8 if isinstance(frames_u8, torch.Tensor) else torch.from_numpy(frames_u8.copy() if hasattr(frames_u8, "copy") else frames_u8)
        video = video.to(self.device)
        vlen = video.shape[0] if vlen is None else int(vlen)
        B = self.B
        for i in range(0, len(starts), B):
            st = starts[i:i + B]
            n_valid = len(st)
            st = st + [st[-1]] * (B - n_valid)
            video_windows_to_input(self.lib, video, vlen, st, clip, self.N, self.SL, ds, self.size, None, self.x_s2d)
            forward()
            reduce(n_valid)

    # ---- one L2-normalised embedding per video (csrc/retrieval.hip; dpc_amd/retrieval.py looks up its neighbours)
    def embed_video(self, frames_u8, starts, clip: dict, out_row: torch.Tensor, ds: int = 3, vlen: Optional[int] = None, graph: bool = False,
                    bn: str = "running"):
        """the embedding of one video into ``out_row`` (a row of a caller-owned f32 [videos, D] tensor on the engine's device): the chunk
        loop of test_video, after each forward dpc_embed_accumulate on ``self.ctx`` (the spatial mean of the last ConvGRU state, f32
        [B, D], before final_bn) with the chunk's valid count, then dpc_embed_finish: the mean over the windows, divided by
        max(its 2-norm, 1e-12) (F.normalize).  Nothing crosses to the host.

        bn='running': the eval-mode forward, as the video-level test uses -- right for any checkpoint of this entry, ``--train_what
        head`` included (its frozen backbone still moved its running buffers).  graph=True replays capture_eval_step() under
        test_video's rule.
        bn='batch': BatchNorm3d uses the chunk's own statistics, as the reference's DPC_RNN does in eval mode -- the only sensible
        mode for a DPC checkpoint loaded by key intersection, which carries no running statistics.  No dropout is applied (all-ones
        masks, no draw), and the running buffers and num_batches_tracked are put back bit for bit after the last chunk.  An
        embedding in this mode depends on the OTHER windows of its chunk, the repeated padding windows of a last chunk included:
        another batch size, or another cut into chunks, gives another embedding.  graph=True is refused with it."""
        if bn not in ("running", "batch"):
            raise ValueError(f"bn = {bn!r}: 'running' or 'batch'")
        if graph and bn == "batch":
            raise ValueError("graph=True replays the eval-mode step: it cannot be combined with bn='batch'")
        D, f32 = self.D, torch.float32
        if not isinstance(out_row, torch.Tensor) or out_row.dtype != f32 or tuple(out_row.shape) != (D,) or not out_row.is_contiguous() or \
                out_row.device != self.ctx.device:
            raise ValueError(f"out_row must be a contiguous float32 [{D}] row on {self.ctx.device}")
        if not hasattr(self, "emb_sum"):
            self.emb_sum = torch.zeros(D, dtype=f32, device=self.device)
            self.emb_count = torch.zeros(1, dtype=torch.int32, device=self.device)
        if graph:
            self.check_graph_capture()
        saved = None
        if bn == "batch":
            if not hasattr(self, "_ones_masks"):
                self._ones_masks = (torch.ones(self.N, self.M, D, dtype=f32, device=self.device), torch.ones(self.B, D, dtype=f32, device=self.device))
            saved = {k: v.clone() for k, v in self.BUF.items()}

        def forward():
            if bn == "batch":
                self.forward(None, None, train=True, gru_masks=self._ones_masks[0], fc_mask=self._ones_masks[1])
            elif not graph:
                self.forward(None, None, train=False)
            else:
                self._eval_forward_replayed()

        try:
            self._video_chunks(frames_u8, starts, clip, ds, vlen, forward, lambda n_valid: self.call(
                "dpc_embed_accumulate", self.ctx, self.B, n_valid, D, D, self.emb_sum, self.emb_count))
        finally:
            if saved is not None:
                for k, v in saved.items():
                    self.BUF[k].copy_(v)
        self.call("dpc_embed_finish", self.emb_sum, self.emb_count, D, 1e-12, out_row)


class _LCOutput(torch.autograd.Function):
    """(output, context) of a train-mode LC.forward with an autograd node, built like model._DPCScore: the backward runs the engine's
    hand-written backward from the upstream gradients and hands autograd fresh views of the gradient arena"""

    @staticmethod
    def forward(ctx, model, block, target, masks, *params):
        eng = model._engine
        model._fwd_generation += 1   # the engine keeps ONE set of saved activations: the node is valid until the next forward, for one backward
        gru_masks, fc_mask = masks if masks is not None else (None, None)
        out, context = eng.forward(block, target, train=True, gru_masks=gru_masks, fc_mask=fc_mask)
        ctx.model, ctx.generation, ctx.used = model, model._fwd_generation, False
        ctx.set_materialize_grads(False)   # an output the loss does not use arrives as None, not as a zero tensor
        return out.clone(), context.clone()

    @staticmethod
    def backward(ctx, d_output, d_context):
        model = ctx.model
        eng = model._engine
        if ctx.generation != model._fwd_generation:
            raise RuntimeError("dpc_amd.LC: backward of an output whose saved activations were overwritten by a later forward (the "
                               "engine holds one step's activations; call backward before the next forward)")
        if ctx.used:
            raise RuntimeError("dpc_amd.LC: trying to backward through the graph a second time (activations are consumed in place "
                               "by the backward kernels)")
        ctx.used = True
        names = model._param_names
        params = model._params()
        # what autograd asks for decides where the backward stops -- never the optimizer's groups: a parameter that requires a
        # gradient gets a real one whether or not the last optimizer step left it out
        wanted = [ctx.needs_input_grad[4 + i] for i in range(len(names))]
        aliased = any(q.grad is not None and q.grad.data_ptr() == eng.G[k].data_ptr() for k, q in zip(names, params))
        old = eng.flat_g.clone() if aliased else None   # .grad still set (no zero_grad): torch accumulates; the kernels overwrite the arena
        if d_output is None and d_context is None:
            d_output = torch.zeros_like(eng.logits)
        eng.backward(d_output=d_output, d_context=d_context, wanted=[k for k, w in zip(names, wanted) if w])
        need_backbone, need_agg = eng.grad_wanted([k for k, w in zip(names, wanted) if w])
        src = eng.flat_g
        if old is not None:   # autograd gets a copy of the new gradients; the arena (= the live .grad tensors) gets its old values back
            src = eng.flat_g.clone()
            eng.flat_g.copy_(old)
        grads = []
        for k, w in zip(names, wanted):
            o, n = eng.offsets[k]
            ran = need_backbone if k.startswith("backbone.") else (need_agg if k.startswith("agg.") else True)
            grads.append(src[o:o + n].view(eng.shapes[k]) if (w and ran) else None)   # requires_grad = False: None, as torch gives
        return (None, None, None, None) + tuple(grads)


class LC(_EngineModule):
    """drop-in for eval/model_3d_lc.py:12: ``LC(sample_size, num_seq, seq_len, network, dropout, num_class)``,
    ``forward(block) -> (output [B,1,num_class], context [B,1,D])``.  In train mode both carry an autograd node, so the reference's
    loop runs as written (eval/test.py:229-255): ``loss = criterion(output.view(B*N, D), target); optimizer.zero_grad();
    loss.backward(); optimizer.step()`` -- ``loss.backward()`` runs the engine's backward kernels from whatever gradient arrives at
    ``output`` and ``context``; afterwards every parameter's ``.grad`` is a view of the gradient arena (it accumulates if ``.grad``
    was still set), and ``dpc_amd.optim.Adam`` (parameter groups, frozen parameters) is the fused arena update.  A parameter with
    ``requires_grad = False`` gets ``None``; when no ``backbone.*`` (and no ``agg.*``) parameter requires a gradient the backward
    stops in front of the backbone (the ConvGRU) -- decided by ``requires_grad`` alone, never by which parameters an optimizer holds -- BatchNorm layers of such a frozen extractor still use batch statistics and update
    their running buffers in train mode, as in torch.  One backward per forward, before the next forward.  Eval mode builds no graph
    (the reference validates under ``no_grad``).  ``engine.train_step(block, target)`` remains the engine-owned step."""
    _SAVED_AS = "eval/test.py:205-214"

    def __init__(self, sample_size, num_seq, seq_len, network="resnet18", dropout=0.5, num_class=101,
                 compute_dtype=torch.float32, widths=LAYER_WIDTH, seed: int = 0, _simulator: Optional[L.Lib] = None):
        super().__init__(sample_size, num_seq, seq_len, network, compute_dtype, widths, _simulator)
        self.num_class, self.dropout = num_class, dropout
        self._forced_masks = None    # tests: (gru_masks [N,M,D], fc_mask [B,D]), pre-scaled keep values for both dropouts
        self._fwd_generation = 0
        self._param_list = None
        shapes = lc_param_shapes(network, num_class, widths)
        self._param_names = list(shapes)
        init = _init_reference_style(shapes, torch.Generator().manual_seed(seed))
        for k in lc_state_dict_keys(network, num_class, widths):
            if k.startswith("agg.cell_list.0."):
                continue
            if k in shapes:
                _attach(self, k, nn.Parameter(init[k]))
            else:
                C_ = shapes[k.rsplit(".", 1)[0] + ".weight"][0]
                v = torch.zeros(C_) if k.endswith("running_mean") else (torch.ones(C_) if k.endswith("running_var") else torch.zeros((), dtype=torch.int64))
                _attach(self, k, v, buffer=True)
        self.agg.cell_list = nn.ModuleList([self.agg.ConvGRUCell_00])

    def _params(self):
        """the Parameters in the engine's order (the objects never change: _ensure_engine re-points their .data)"""
        if self._param_list is None:
            named = dict(self.named_parameters())
            self._param_list = [named[k] for k in self._param_names]
        return self._param_list

    def _make_engine(self, B, dev):
        return LCEngine(self.network, self.sample_size, self.num_seq, self.seq_len, B, dev, self.compute_dtype,
                        self.widths, self._simulator, dropout=self.dropout, num_class=self.num_class)

    def __deepcopy__(self, memo):
        """a fresh module with the same constructor arguments, cloned parameter / buffer values and no engine (as DPC_RNN.__deepcopy__)"""
        new = type(self)(self.sample_size, self.num_seq, self.seq_len, self.network, self.dropout, self.num_class, self.compute_dtype,
                         self.widths, _simulator=self._simulator)
        new.load_state_dict({k: v.detach().clone() for k, v in self.state_dict().items()})
        mine = dict(self.named_parameters())
        for k, q in new.named_parameters():   # --train_what ft / last freeze parameters: the copy keeps that
            q.requires_grad_(mine[k].requires_grad)
        new.train(self.training)
        memo[id(self)] = new
        return new

    def forward(self, block, target: Optional[torch.Tensor] = None):
        if getattr(self, "_is_replica", False):   # nn.DataParallel over several devices (eval/test.py:63): see dpc_amd.model._REPLICA_ERROR
            raise RuntimeError(_REPLICA_ERROR.replace("dpc_amd.DPC_RNN", "dpc_amd.LC").replace("dpc_amd.main", "dpc_amd.lc_main").replace("dpc/main.py", "eval/test.py"))
        if block.device.type != "cuda" and self._simulator is None:
            raise L.DpcError("dpc_amd.LC runs on MI355X only: move the module and the input to a cuda (HIP) device")
        self._ensure_engine(block)
        self._engine.packed_for_step = -1  # the parameters may have been changed through the module since the last forward
        if target is None:
            target = torch.zeros(block.shape[0], dtype=torch.int64)
        if not self.training:
            out, ctx = self._engine.forward(block.float(), target, train=False)
            return out.clone(), ctx.clone()
        return _LCOutput.apply(self, block.float(), target, self._forced_masks, *self._params())
