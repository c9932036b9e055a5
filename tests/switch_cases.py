"""The off-default arms of the environment switches (docs/switches.md), each run against the kernel references of tests/kcases.py.

Most library switches are `static` reads, once per process, so every set of arms runs in a fresh child process that is started with
its environment:   python tests/switch_cases.py <cpu|cuda:0> <set>   (tests/test_switches_emu.py: the host SIMT simulator,
tests/test_switches_gpu.py: libdpc_hip.so on an MI355X).  The child runs the set's cases through the unmodified kcases.case_*
functions -- their bounds are the only ones: tol(), rejects_dropped_tap, rejects_dropped_row, the poison rule -- prints one line per
case and a final `switch set <name> ok`.

ARMS below is the one table both tiers and the completeness check (test_switches_emu.py) read.  An arm is

    name       what docs/switches.md calls it
    set        the child it runs in.  Arms that feed the same dispatch decision never share a child (DPC_IGEMM_WS, _PLANE,
               _TGROUP, _PAR, DPC_IGEMM_WSD, the two split-K extremes)
    env        the switch itself: part of the child's environment
    call_env   a switch the library reads on every call (PER_CALL): set around the arm's own cases only
    thr        threshold variables this arm's child needs on top of THRESHOLDS (a value of None removes one)
    cases      Case(fn, args, kw, names, thr, ns): kcases.case_<fn>(k, *args, **kw).  names = {C-ABI entry: (kernel the arm must
               select, kernel the same call selects without the switch)}: both are the full strings of dpc_last_kernel, pinned.
               thr: per-call threshold variables set around the case in the arm AND in the baseline child.  ns: (split-K slabs
               without the switch, relation the arm must show: ">" more, "1" exactly one, "=" unchanged)

How an arm proves that it acted: the baseline child (set "baseline": only THRESHOLDS in its environment) runs every case of the
table and must see the second name of every pair, the arm's child the first, and no pair holds the same name twice
(check_table).  Arms that choose no other kernel append a note at the dispatch site when their value is off-default
(`[tgroup=0]`, `[rev]`, `[a=999]`, `[wgs=7]`); every default name is unchanged.  Split-K arms are held by the slab count.
The BatchNorm grid / unroll arms change launch dimensions and an unroll template argument only: `names` pins what shows."""
import contextlib
import ctypes as C
import io
import json
import os
import sys
import time
from collections import namedtuple

# the test tiers' thresholds (tests/test_ws_emu.py) so that small shapes reach every kernel and one workgroup walks several
# tiles; the two grid caps make the end-to-front sweeps of bn_relu_maxpool_fwd / pack_input_s2d more than one sweep long
THRESHOLDS = {"DPC_IGEMM_WS_MINROWS": "1", "DPC_IGEMM_WS_GM": "2", "DPC_HALO_WS_GM": "3", "DPC_IGEMM_GM_CAP": "32",
              "DPC_IGEMM_WS_PAR_MINCO": "64", "DPC_WSD_MINPLANES": "1", "DPC_POOL_FWD_GRID": "8", "DPC_PACK_GRID": "1"}
# read by the library on every call: these alone may change inside a live process
PER_CALL = {"DPC_BN_NT_MB", "DPC_BN_UNROLL", "DPC_BN_SMALL_UNROLL", "DPC_BN_APPLY_GRID", "DPC_BN_BWD_GRID", "DPC_BN_SMALL_GRID",
            "DPC_GEMM_WS_MIN", "DPC_SCORE_GEMM2"}

Case = namedtuple("Case", "fn args kw names thr ns", defaults=({}, {}, {}, None))
Arm = namedtuple("Arm", "name set env call_env thr cases", defaults=({}, {}, {}, ()))

IG, IGX, WG, NTS = "dpc_conv_igemm", "dpc_conv_igemm_ex", "dpc_conv_wgrad", "dpc_gemm_nt_splitk"
K133, K333, S1, S122, S222, P011, P111 = (1, 3, 3), (3, 3, 3), (1, 1, 1), (1, 2, 2), (2, 2, 2), (0, 1, 1), (1, 1, 1)
NOADD = {"with_add": False}
NT1 = {"DPC_BN_NT_MB": "1"}

# ---- names as dpc_last_kernel reports them
HALO33, HALO44 = "conv_halo_kernel<bf16_t,bf16_t,3,3,8>[ws_declined=0]", "conv_halo_kernel<bf16_t,bf16_t,4,4,2>[ws_declined=0]"
HWS = "conv_halo_ws_kernel<%s>"
GEN = "igemm_kernel<T,TO,BN,%d>[T=bf16 TO=%s BN=%d]"
WS_F, WS_T, WS_PAR, WSD = "igemm_ws_kernel<false>", "igemm_ws_kernel<true>", "igemm_ws_kernel<false,true>", "igemm_wsd_kernel"
WSP_F, WSP_T = "igemm_wsp_kernel<false>", "igemm_wsp_kernel<true>"
WG2 = "wgrad2_kernel<T,NWM,NWN,%s>[T=%s nwm=%d nwn=%d padded=%d]"
WGP, WGS = "wgrad_patch_kernel<%d>", "wgrad_stem_kernel"
BNA = "bn_apply_kernel<%s>"
POOLF, PACK = "bn_relu_maxpool_fwd_kernel<%s>", "pack_input_s2d_kernel<%s>"

SPLIT_CASES = (   # (fn, args, slabs without a switch); the planner is the kernel family of the name
    ("conv_wgrad", ("bf16", 3, 64, 64, 2, 16, 16, K133, S1, P011), WGP % 16),
    ("conv_wgrad", ("bf16", 2, 64, 128, 3, 8, 8, K333, S1, P111), WGP % 8),
    # the patch planner splits every chunk apart until 512 workgroups are reached: only 4 x 4 x 3 tiles leave it something to add
    ("conv_wgrad", ("bf16", 4, 256, 256, 3, 8, 8, K333, S1, P111), WGP % 8),
    ("conv_wgrad", ("bf16", 3, 64, 128, 2, 16, 16, K133, S122, P011), WG2 % ("true", "bf16", 2, 3, 0)),
    ("conv_wgrad", ("bf16", 2, 64, 128, 1, 28, 28, K133, S122, P011), WG2 % ("true", "bf16", 2, 3, 1)),
    ("conv_wgrad", ("bf16", 5, 8, 24, 2, 6, 6, K133, S122, P011), "wgrad_kernel<T,64,64,RF>[T=bf16]"),
    ("conv_wgrad", ("f32", 2, 16, 24, 2, 8, 8, K133, S1, P011), WG2 % ("true", "f32", 1, 3, 0)),
)
SPLIT_BASE_NS = (24, 6, 6, 1, 1, 1, 1)   # slabs without a switch, case by case (the baseline child holds them)
STEM_128 = ("bf16", 1, 1, 128, 128)
STEM_128_NAMES = {IG: (HWS % "false,2,256",) * 2, WG: (WGS,) * 2}


def _split_cases(rel):
    cs = [Case(fn, args, {}, {WG: (name, name)}, {}, (ns0, rel)) for (fn, args, name), ns0 in zip(SPLIT_CASES, SPLIT_BASE_NS)]
    # wgrad_stem_kernel's planner reads no switch: its slab count must not move
    return tuple(cs) + (Case("stem", STEM_128, {}, STEM_128_NAMES, {}, (4, "=")),)


def _bn_grid_cases():
    out = []
    for args in (("bf16", 5003, 128, True, 1), ("bf16", 2011, 256, False, 2)):
        for thr in (NT1, {}):
            nt = "true" if thr and args[1] * args[2] * 2 >= 1 << 20 else "false"   # the streaming forms from DPC_BN_NT_MB megabytes on
            out.append(Case("bn_fwd_bwd", args, {}, {"dpc_bn_apply": (BNA % f"bf16_t,true,{nt},2", BNA % f"bf16_t,true,{nt},4")}, thr))
    return tuple(out)


ARMS = (
    # ------------------------------------------------------------------ set ws_off
    Arm("DPC_HALO_WS=0", "ws_off", {"DPC_HALO_WS": "0"}, cases=(
        Case("conv_fwd", ("bf16", 2, 64, 64, 2, 9, 33, K133, S1, P011), {}, {IG: (HALO33, HWS % "false,8,128")}),
        Case("conv_fwd", ("bf16", 1, 64, 40, 1, 20, 12, K133, S1, P011), {}, {IG: (HALO33, HWS % "false,8,128")}),   # ragged column tile
        Case("conv_dgrad", ("bf16", 2, 64, 64, 2, 9, 33, K133, S1, P011), {}, {IG: (HALO33, HWS % "true,8,128")}),
        Case("conv_dgrad_ex", ("bf16", 2, 64, 64, 1, 9, 33, K133, S1, P011), {}, {IGX: (HALO33, HWS % "true,8,128,true")}),
        Case("stem", ("bf16", 2, 2, 16, 72), {}, {IG: (HALO44, HWS % "false,2,256")}),
    )),
    Arm("DPC_IGEMM_WS=0", "ws_off", {"DPC_IGEMM_WS": "0"}, cases=(
        Case("conv_fwd", ("bf16", 9, 64, 128, 3, 8, 8, K333, S1, P111), {}, {IG: (GEN % (1, "bf16", 128), WS_F)}),
        Case("conv_fwd", ("bf16", 2, 64, 136, 3, 8, 8, K333, S1, P111), {}, {IG: (GEN % (1, "bf16", 128), WS_F)}),   # ragged column tile
        Case("conv_dgrad", ("bf16", 4, 128, 64, 3, 7, 7, K333, S1, P111), {}, {IG: (GEN % (1, "bf16", 128), WS_T)}),
        Case("conv_dgrad", ("bf16", 2, 128, 64, 3, 7, 9, K333, S222, P111), NOADD, {IG: (GEN % (3, "bf16", 128), WS_PAR)}),
        Case("conv_dgrad", ("bf16", 2, 64, 128, 2, 32, 32, K133, S122, P011), NOADD, {IG: (GEN % (3, "bf16", 64), WSD)}),
    )),
    Arm("DPC_WGRAD_PATCH=0", "ws_off", {"DPC_WGRAD_PATCH": "0"}, cases=(
        Case("conv_wgrad", ("bf16", 2, 64, 64, 1, 16, 16, K133, S1, P011), {}, {WG: (WG2 % ("true", "bf16", 1, 3, 0), WGP % 16)}),
        Case("conv_wgrad", ("bf16", 2, 64, 64, 2, 8, 8, K333, S1, P111), {}, {WG: (WG2 % ("true", "bf16", 1, 3, 0), WGP % 8)}),
        Case("conv_wgrad", ("bf16", 1, 64, 64, 1, 28, 28, K133, S1, P011), {}, {WG: (WG2 % ("true", "bf16", 1, 3, 1), WGP % 32)}),
    )),
    # rev only acts on streaming tensors (>= DPC_BN_NT_MB megabytes)
    Arm("DPC_BN_APPLY_REV=1", "ws_off", {"DPC_BN_APPLY_REV": "1"}, cases=(
        Case("bn_fwd_bwd", ("bf16", 5003, 128, True, 1), {}, {"dpc_bn_apply": (BNA % "bf16_t,true,true,4" + "[rev]", BNA % "bf16_t,true,true,4")}, NT1),
        Case("bn_fwd_bwd", ("f32", 4099, 64, True, 2), {}, {"dpc_bn_apply": (BNA % "float,true,true" + "[rev]", BNA % "float,true,true")}, NT1),
    )),
    # ------------------------------------------------------------------ set plane_off
    Arm("DPC_IGEMM_WS_PLANE=0", "plane_off", {"DPC_IGEMM_WS_PLANE": "0"}, cases=(
        Case("conv_fwd", ("bf16", 3, 128, 128, 2, 16, 16, K133, S1, P011), {}, {IG: (WS_F, WSP_F)}),
        Case("conv_fwd", ("bf16", 5, 64, 136, 1, 16, 16, K133, S1, P011), {}, {IG: (WS_F, WSP_F)}),   # odd tile count, ragged column tile
        Case("conv_dgrad", ("bf16", 2, 128, 128, 1, 16, 16, K133, S1, P011), {}, {IG: (WS_T, WSP_T)}),
    )),
    Arm("DPC_WGRAD2_PAD=0", "plane_off", {"DPC_WGRAD2_PAD": "0"}, cases=(
        Case("conv_wgrad", ("bf16", 2, 64, 128, 1, 28, 28, K133, S122, P011), {},
             {WG: ("wgrad_kernel<T,128,128,RF>[T=bf16]", WG2 % ("true", "bf16", 2, 3, 1))}),
    )),
    Arm("DPC_SCORE_GEMM=0", "plane_off", {"DPC_SCORE_GEMM": "0"}, cases=(
        Case("gemm_nt", ("bf16", 1024, 1024, 256), {}, {IG: (GEN % (1, "f32", 128), "score_gemm_kernel<16>")}),
        Case("gemm_nt_bf16out", (1024, 1024, 256), {}, {IG: (WS_F, "score_gemm2_kernel<16,true>")}),
    )),
    Arm("DPC_POOL_FWD_REV=1", "plane_off", {"DPC_POOL_FWD_REV": "1"}, cases=tuple(
        Case("stem_pool", (dt,) + shp, {}, {"dpc_bn_relu_maxpool_fwd": (POOLF % t + "[rev]", POOLF % t)})
        for dt, t in (("bf16", "bf16_t"), ("f32", "float"))
        for shp in ((6, 7, 10, 64), (6, 64, 64, 64), (6, 30, 22, 64)))),   # one sweep / 24 or 48 sweeps / a ragged last sweep
    Arm("DPC_PACK_REV=1", "plane_off", {"DPC_PACK_REV": "1"}, cases=(
        Case("stem", ("bf16", 2, 2, 16, 20), {}, {"dpc_pack_input_s2d": (PACK % "bf16_t" + "[rev]", PACK % "bf16_t")}),   # 320 cells: two sweeps, the second ragged
        Case("stem", ("f32", 2, 2, 16, 20), {}, {"dpc_pack_input_s2d": (PACK % "float" + "[rev]", PACK % "float")}),
    )),
    # ------------------------------------------------------------------ set tgroup_off
    Arm("DPC_IGEMM_WS_TGROUP=0", "tgroup_off", {"DPC_IGEMM_WS_TGROUP": "0"}, cases=(
        Case("conv_fwd", ("bf16", 9, 64, 128, 3, 8, 8, K333, S1, P111), {}, {IG: (WS_F + "[tgroup=0]", WS_F)}),
        Case("conv_fwd", ("bf16", 2, 64, 136, 3, 8, 8, K333, S1, P111), {}, {IG: (WS_F + "[tgroup=0]", WS_F)}),
        Case("conv_dgrad", ("bf16", 4, 128, 64, 3, 7, 7, K333, S1, P111), {}, {IG: (WS_T + "[tgroup=0]", WS_T)}),
    )),
    # five workgroups: 4 of kind A and 1 of kind B (999), 1 and 4 (1); 556 gives 2 and 3
    Arm("DPC_WSD_A_PERMILLE=999", "tgroup_off", {"DPC_WSD_A_PERMILLE": "999"}, thr={"DPC_IGEMM_WS_GM": "5"}, cases=(
        Case("conv_dgrad", ("bf16", 5, 64, 128, 1, 32, 32, K133, S122, P011), dict(NOADD, seed=11), {IG: (WSD + "[a=999]", WSD)}),
    )),
    Arm("DPC_WGRAD_STEM=0", "tgroup_off", {"DPC_WGRAD_STEM": "0"}, cases=(
        Case("stem", STEM_128, {}, {WG: (WG2 % ("true", "bf16", 1, 4, 0), WGS)}),
    )),
    Arm("DPC_SCORE_GEMM_WGS=7", "tgroup_off", {"DPC_SCORE_GEMM_WGS": "7"}, cases=(
        Case("gemm_nt", ("bf16", 1024, 1024, 256), {}, {IG: ("score_gemm_kernel<16>[wgs=7]", "score_gemm_kernel<16>")}),
    )),
    Arm("DPC_BN_BWD_GRID=3 DPC_BN_APPLY_GRID=3 DPC_BN_SMALL_GRID=3 DPC_BN_UNROLL=2 DPC_BN_SMALL_UNROLL=2", "tgroup_off",
        call_env={"DPC_BN_BWD_GRID": "3", "DPC_BN_APPLY_GRID": "3", "DPC_BN_SMALL_GRID": "3", "DPC_BN_UNROLL": "2", "DPC_BN_SMALL_UNROLL": "2"},
        cases=_bn_grid_cases()),
    # ------------------------------------------------------------------ set par_off
    Arm("DPC_IGEMM_WS_PAR=0", "par_off", {"DPC_IGEMM_WS_PAR": "0"}, cases=(
        Case("conv_dgrad", ("bf16", 2, 128, 64, 3, 7, 9, K333, S222, P111), NOADD, {IG: (GEN % (3, "bf16", 128), WS_PAR)}),
    )),
    Arm("DPC_WSD_A_PERMILLE=1", "par_off", {"DPC_WSD_A_PERMILLE": "1"}, thr={"DPC_IGEMM_WS_GM": "5"}, cases=(
        Case("conv_dgrad", ("bf16", 5, 64, 128, 1, 32, 32, K133, S122, P011), dict(NOADD, seed=11), {IG: (WSD + "[a=1]", WSD)}),
    )),
    # the 8-wave score GEMM "whenever the shape allows" (2) is the tiers' threshold for it, as in tests/test_kernels_*.py
    Arm("DPC_SCORE_GEMM2=0", "par_off", call_env={"DPC_SCORE_GEMM2": "0"}, cases=(
        Case("gemm_nt", ("bf16", 1024, 1024, 256), {}, {IG: ("score_gemm_kernel<16>", "score_gemm2_kernel<16>")}, {"DPC_SCORE_GEMM2": "2"}),
    )),
    # dpc_gemm_tn_splitk has no other kernel: its size query answers DPC_ERR_UNSUPPORTED (-3), which engine._tn_splits relies on
    Arm("DPC_GEMM_WS=0", "par_off", {"DPC_GEMM_WS": "0"}, cases=(
        Case("gemm_nt_splitk", ("bf16", 256, 256, 520), {"pad": 8},
             {NTS: (GEN % (1, "f32", 128), "gemm_ws_kernel<false>[splitk=1]")}, {"DPC_GEMM_WS_MIN": "64"}),
        Case("gemm_tn_query", (256, 256, 520, 8), {}, {"dpc_gemm_tn_splitk": ("rc=-3", "rc=0")}, {"DPC_GEMM_WS_MIN": "64"}),
    )),
    # ------------------------------------------------------------------ sets wsd_off_minco / wsd_off
    Arm("DPC_IGEMM_WSD=0 (DPC_IGEMM_WS_PAR_MINCO=64)", "wsd_off_minco", {"DPC_IGEMM_WSD": "0"}, cases=(
        Case("conv_dgrad", ("bf16", 2, 64, 128, 2, 32, 32, K133, S122, P011), NOADD, {IG: (WS_PAR, WSD)}),
    )),
    Arm("DPC_IGEMM_WSD=0", "wsd_off", {"DPC_IGEMM_WSD": "0"}, thr={"DPC_IGEMM_WS_PAR_MINCO": None}, cases=(
        Case("conv_dgrad", ("bf16", 2, 64, 128, 2, 32, 32, K133, S122, P011), NOADD, {IG: (GEN % (3, "bf16", 64), WSD)}),
    )),
    # split-K extremes: one chunk per slab / one slab
    Arm("DPC_WGRAD_MINCHUNKS=1 DPC_WGRAD_BLOCKS=100000 DPC_WGRAD_PATCH_BLOCKS=100000", "wsd_off_minco",
        {"DPC_WGRAD_MINCHUNKS": "1", "DPC_WGRAD_BLOCKS": "100000", "DPC_WGRAD_PATCH_BLOCKS": "100000"}, cases=_split_cases(">")),
    Arm("DPC_WGRAD_BLOCKS=1 DPC_WGRAD_PATCH_BLOCKS=1", "wsd_off",
        {"DPC_WGRAD_BLOCKS": "1", "DPC_WGRAD_PATCH_BLOCKS": "1"}, cases=_split_cases("1")),
)

SETS = tuple(dict.fromkeys(a.set for a in ARMS))
BASELINE = "baseline"
# GPU tier only: DPC_GEMM_WS=0 when an engine is BUILT (DPCEngine._tn_splits) -- a child of its own, nothing else in its environment
ENGINE_SET = "engine_gemm_ws_off"
ENGINE_ENV = {"DPC_GEMM_WS": "0", "DPC_GEMM_WS_MIN": "64"}


def case_id(c):
    return " ".join([c.fn, json.dumps([c.args, c.kw], separators=(",", ":")), json.dumps(c.thr, sort_keys=True)])


def set_env(name):
    """the environment a set's child is started with, on top of the caller's own"""
    env = dict(THRESHOLDS)
    if name == ENGINE_SET:
        return dict(ENGINE_ENV)
    for a in ARMS:
        if a.set == name:
            env.update(a.thr)
            env.update(a.env)
    return env


def child_env(name, base=None):
    env = dict(os.environ if base is None else base)
    for k, v in set_env(name).items():
        if v is None:
            env.pop(k, None)
        else:
            env[k] = v
    return env


def switch_names():
    """every variable the table exercises as an arm (thresholds are not arms)"""
    return {k for a in ARMS for k in list(a.env) + list(a.call_env)}


def check_table():
    """what must hold of the table itself, without running a kernel"""
    assert len(SETS) <= 8
    for s in SETS:
        seen = {}
        for a in (a for a in ARMS if a.set == s):
            for k, v in list(a.env.items()) + list(a.thr.items()):
                assert seen.setdefault(k, v) == v, f"set {s}: {k} is given two values"
            assert not (set(a.env) & PER_CALL) and set(a.call_env) <= PER_CALL, a.name
    exclusive = ("DPC_IGEMM_WS", "DPC_IGEMM_WS_PLANE", "DPC_IGEMM_WS_TGROUP", "DPC_IGEMM_WS_PAR", "DPC_IGEMM_WSD")
    for s in SETS:
        assert len({k for a in ARMS if a.set == s for k in a.env if k in exclusive}) <= 1, f"set {s} mixes arms of one dispatch decision"
        assert len({a.env["DPC_WGRAD_BLOCKS"] for a in ARMS if a.set == s and "DPC_WGRAD_BLOCKS" in a.env}) <= 1
    for a in ARMS:
        assert a.cases, a.name
        for c in a.cases:
            assert set(c.thr) <= PER_CALL, (a.name, c.thr)
            assert c.names or c.ns, f"{a.name}: {case_id(c)} can show nothing"
            acted = [arm != base for arm, base in c.names.values()]
            if c.ns is None:   # (a case with a slab relation is held by the count; "=" marks a control the switch must not move)
                # a case whose arm name equals its baseline name without a note is a test bug
                assert any(acted), f"{a.name}: {case_id(c)} pins the same names with and without the switch"


def _gemm_tn_query(k, M, N, Kd, pad):
    """dpc_gemm_tn_splitk's size query alone: 0 and a slab count where gemm_ws_kernel<true> takes the shape, else DPC_ERR_UNSUPPORTED"""
    from dpc_amd import _lib as L
    ns = C.c_int32(0)
    rc = k.lib._fn("dpc_gemm_tn_splitk")(L.BF16, M, N, Kd, None, M + pad, None, Kd + pad, None, C.byref(ns), k.lib.stream())
    k.trace["dpc_gemm_tn_splitk"] = f"rc={rc}"
    assert rc in (0, -3), rc


def _run_case(k, kc, c, which, call_env):
    import torch
    dt = {"bf16": torch.bfloat16, "f32": torch.float32}
    args = tuple(dt.get(a, a) if isinstance(a, str) else a for a in c.args)
    want = {e: pair[which] for e, pair in c.names.items()}
    kw = dict(c.kw)
    if c.fn in ("conv_fwd", "conv_dgrad", "gemm_nt", "gemm_nt_bf16out") and IG in want:
        kw["expect"] = want[IG]
    elif c.fn == "conv_dgrad_ex" and IGX in want:
        kw["expect"] = want[IGX]
    elif c.fn == "conv_wgrad" and WG in want:
        kw["expect"] = want[WG]
    elif c.fn == "gemm_nt_splitk" and NTS in want:
        kw["expect"] = want[NTS]
    elif c.fn == "stem":
        kw["expect"] = (want.get(IG), want.get(WG))
    env = dict(c.thr, **call_env)
    assert set(env) <= PER_CALL
    saved = {v: os.environ.get(v) for v in env}
    os.environ.update(env)
    k.trace.clear()
    k.ratio = (0.0, "")
    buf = io.StringIO()
    t0 = time.time()
    try:
        with contextlib.redirect_stdout(buf):
            ret = _gemm_tn_query(k, *args) if c.fn == "gemm_tn_query" else getattr(kc, "case_" + c.fn)(k, *args, **kw)
            k.sync()
    except BaseException:
        print(buf.getvalue()[-4000:])
        print(f"FAILED case {case_id(c)} kernels {json.dumps(k.trace)}", flush=True)
        raise
    finally:
        for v, old in saved.items():
            if old is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = old
    ns = ret if c.fn in ("conv_wgrad", "stem") else None
    print("case " + json.dumps({"id": case_id(c), "kernels": {e: k.trace.get(e) for e in want}, "ns": ns,
                                "row_ratio": round(k.ratio[0], 4), "row_what": k.ratio[1], "s": round(time.time() - t0, 2)}), flush=True)
    for e, name in want.items():
        assert k.trace.get(e) == name, f"{case_id(c)}: {e} ran {k.trace.get(e)!r}, the table pins {name!r}"
    if k.ratio[0] > k.worst[0]:
        k.worst = (k.ratio[0], f"{k.ratio[1]}, {case_id(c)}")
    return ns


def _engine_check():
    """DPC_GEMM_WS=0 at engine build: no slabs planned for d_feature_inf on the loader / compute GEMM (`_tn_splits is None`), and the
    head backward of one small-batch r18 step still holds against the rounding oracle (tests/head_cases.py).  With DPC_GEMM_WS_MIN=64
    alone the same engine does plan them: tests/test_head_grads_gpu.py, form "gemm_ws"."""
    import torch
    import head_cases as H
    e = H.engine("resnet18", 128, 3, 16, torch.bfloat16)
    print(f"engine: _tn_splits {e._tn_splits}", flush=True)
    assert e._tn_splits is None, e._tn_splits
    H.case(e, "r18/128/B=16 DPC_GEMM_WS=0", materialise=False)
    torch.cuda.synchronize()


def main(tier, name):
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    sys.path.insert(0, os.path.dirname(here))
    import kcases as kc
    from dpc_amd import _lib as L
    for var, v in set_env(name if name != BASELINE else "").items():   # the child really was started with the set's environment
        assert os.environ.get(var) == v, f"{var} is {os.environ.get(var)!r} in this process, the set wants {v!r}"
    t0 = time.time()
    if name == ENGINE_SET:
        assert tier != "cpu"
        _engine_check()
        print(f"switch set {name} ok ({time.time() - t0:.1f} s)")
        return

    class TraceK(kc.K):
        """K that notes, per C-ABI entry, the kernel its last call launched, and the worst error / bound of the row reductions"""
        trace, ratio, worst = {}, (0.0, ""), (0.0, "")

        def call(self, entry, *args):
            rc = super().call(entry, *args)
            self.trace[entry] = L.last_kernel(self.lib)
            return rc

    k = TraceK(L.load_emulator() if tier == "cpu" else L.load_hip(), tier)
    inner = kc.rejects_dropped_row

    def noting(got, terms, rows, what=""):
        e_ok, bound = inner(got, terms, rows, what)
        if e_ok / bound > k.ratio[0]:
            k.ratio = (e_ok / bound, what)
        return e_ok, bound
    kc.rejects_dropped_row = noting

    done = {}
    if name == BASELINE:
        for a in ARMS:
            for c in a.cases:
                if case_id(c) in done:
                    continue
                ns = done[case_id(c)] = _run_case(k, kc, c, 1, {})
                if c.ns is not None:
                    assert ns == c.ns[0], f"{case_id(c)}: {ns} slabs without a switch, the table pins {c.ns[0]}"
    else:
        assert name in SETS, name
        for a in (a for a in ARMS if a.set == name):
            print(f"arm {a.name}", flush=True)
            more = {}
            for c in a.cases:
                ns = _run_case(k, kc, c, 0, a.call_env)
                if c.ns is None:
                    continue
                base, rel = c.ns
                planner = c.names[WG][0].split("<")[0]
                if rel == "1":
                    assert ns == 1, f"{case_id(c)}: {ns} slabs where the arm asks for one"
                elif rel == "=":
                    assert ns == base, f"{case_id(c)}: {ns} slabs, {base} without the switch"
                else:
                    assert ns >= base, f"{case_id(c)}: {ns} slabs, {base} without the switch"
                    more[planner] = more.get(planner, False) or ns > base
            assert all(more.values()), f"{a.name}: no case of {[p for p, m in more.items() if not m]} got more slabs than without the switch"
    print(f"worst row reduction of the set: error / bound = {k.worst[0]:.4f} ({k.worst[1]})")
    print(f"switch set {name} ok ({time.time() - t0:.1f} s)")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
