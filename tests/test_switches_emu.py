"""CPU tier: every off-default arm of the environment switches (tests/switch_cases.py: the table, the child runner and why each
set of arms is a process of its own) against the kernel references, on the host SIMT simulator; and the check that keeps the
table complete: every DPC_* variable the sources read is documented and is either an arm or excluded for a stated reason."""
import glob
import os
import re
import subprocess
import sys

import pytest

import switch_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_is_consistent():
    sc.check_table()


@pytest.mark.parametrize("name", (sc.BASELINE,) + sc.SETS)
def test_switch_set_on_simulator(name):
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_cases.py"), "cpu", name], env=sc.child_env(name),
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and f"switch set {name} ok" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]


# ---- variables that are read by the sources and are no arm of the table, each with its reason
THRESHOLD = "threshold / grid cap the test tiers lower so that small shapes reach a kernel and walk several tiles (switch_cases.THRESHOLDS or per case)"
RUNTIME = "runtime / lifetime knob, no numerical path"
EXCLUDED = {
    "DPC_IGEMM_WS_MINROWS": THRESHOLD, "DPC_IGEMM_WS_GM": THRESHOLD, "DPC_HALO_WS_GM": THRESHOLD, "DPC_IGEMM_GM_CAP": THRESHOLD,
    "DPC_WSD_MINPLANES": THRESHOLD, "DPC_IGEMM_WS_PAR_MINCO": THRESHOLD, "DPC_BN_NT_MB": THRESHOLD, "DPC_GEMM_WS_MIN": THRESHOLD,
    "DPC_POOL_FWD_GRID": THRESHOLD, "DPC_PACK_GRID": THRESHOLD,
    "DPC_GRU_WAVES": "tests/test_kernels_emu.py, tests/test_kernels_gpu.py: the ConvGRU recurrence with 4 and 8 waves",
    "DPC_WGRAD_STREAM": "tests/test_two_stream_gpu.py: one stream against two, bit for bit",
    "DPC_STEM_FUSED": "tests/test_stem_grads_gpu.py, tests/test_engine_gpu.py: the stem_fused= argument, both forms",
    "DPC_FOLD": "engine side: tests/test_block_grads_gpu.py (fold=False engine, block by block)",
    "DPC_FOLD_RED": "engine side: tests/test_block_grads_gpu.py (engine built with DPC_FOLD_RED=0)",
    "DPC_SIDE_OFF": "engine side: tests/test_two_stream_gpu.py (named sites off, bit for bit, forks counted)",
    "DPC_SCORE_BF16": "engine side: tests/test_two_stream_gpu.py (f32 logits kept)",
    "DPC_WS_DBG": "probe builds only (#ifdef DPC_WS_PROBE): results wrong by design",
    "DPC_SF_DBG": "probe builds only (#ifdef DPC_WS_PROBE): results wrong by design",
    "DPC_KEEP_GRAPHS": RUNTIME, "DPC_KEEP_CAPTURE_EVENTS": RUNTIME, "DPC_RESERVE_CUS": RUNTIME, "DPC_RCCL_CHANNELS": RUNTIME,
    "DPC_COMPUTE_DTYPE": RUNTIME + " (selects a dtype whose paths tests/test_kernels_*.py cover)",
    "DPC_F32_MATMUL": "tests/x6_cases.py holds the bf16x6 forms kernel by kernel",
}


def _switches_read_by_the_sources():
    names = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "dpc_amd", "csrc", "*.hip"))):
        for m in re.finditer(r'(?:getenv|env_int)\(\s*"(DPC_[A-Z0-9_]+)"', open(path).read()):
            names.setdefault(m.group(1), os.path.relpath(path, ROOT))
    for path in sorted(glob.glob(os.path.join(ROOT, "dpc_amd", "*.py"))):
        for m in re.finditer(r'environ(?:\.get\(|\.setdefault\(|\.pop\(|\[)\s*["\'](DPC_[A-Z0-9_]+)["\']', open(path).read()):
            names.setdefault(m.group(1), os.path.relpath(path, ROOT))
    return names


def test_every_switch_is_documented_and_exercised_or_excluded():
    read = _switches_read_by_the_sources()
    assert len(read) > 40, sorted(read)   # the scan itself found the switches
    doc = open(os.path.join(ROOT, "docs", "switches.md")).read()
    arms = sc.switch_names()
    undocumented = sorted(n for n in read if not re.search(r"\b" + n + r"\b", doc))
    assert not undocumented, f"read by the sources, missing in docs/switches.md: {[(n, read[n]) for n in undocumented]}"
    homeless = sorted(n for n in read if n not in arms and n not in EXCLUDED)
    assert not homeless, f"neither an arm of tests/switch_cases.py nor excluded with a reason: {[(n, read[n]) for n in homeless]}"
    both = sorted(set(arms) & set(EXCLUDED))
    assert not both, f"an arm and excluded: {both}"
    stale = sorted(n for n in list(arms) + list(EXCLUDED) if n not in read)
    assert not stale, f"no source reads {stale} any more"
    assert all(len(reason) > 10 for reason in EXCLUDED.values())
