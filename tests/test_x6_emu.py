"""CPU tier of tests/x6_cases.py: first the plain-torch model of the two f32 arithmetics checks the cases themselves (the split is
exact, the model stays below half of every bound, the bound rejects the model with any one of the six piece products deleted), then
every case runs on the host SIMT simulator in both arithmetics.  Run with -s to see error, bound and kernel of every case and mode."""
import os
import subprocess

import pytest

import x6_cases as xc
from dpc_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{c.name}-{kind}" for c, kind in xc.PARAMS]


@pytest.fixture(scope="module")
def k():
    subprocess.run(["make", "-s", "-j8", "emu"], cwd=ROOT, check=True)
    k = xc.K(L.load_emulator(), "cpu")
    k.mode_before = xc.current_mode(k)
    yield k
    xc.print_results()


@pytest.mark.parametrize("case,kind", xc.PARAMS, ids=IDS)
def test_model_is_within_half_the_bound(case, kind):
    """reference() asserts x1 + x2 + x3 == x bit for bit for both operands; the GEMM view the model works on is the reference's
    operation; both arithmetics of the model use less than half of the bound"""
    r = xc.reference(case, kind)
    assert xc.gemm_view_error(case, kind) < 1e-12
    for mode in (0, 1):
        e = xc.model_error(case, kind, mode)
        print(f"x6 [model] {case.name:<22} {kind:<6} {'bf16x6' if mode else 'exact ':<6} error {e:.3e}  bound {r.bound:.3e}  ratio {e / r.bound:.3f}")
        assert e < 0.5 * r.bound, (case, kind, mode, e, r.bound)


@pytest.mark.parametrize("case,kind", xc.PARAMS, ids=IDS)
def test_bound_rejects_every_deleted_term(case, kind):
    """the model without one of the six bf16 MFMAs of mfma_f32x6 misses the bound: all six on random operands, on a probe the terms
    that probe carries"""
    r = xc.reference(case, kind)
    carried = [t for t in xc.TERMS if r.loss[t] > 0]
    assert len(carried) == (6 if kind == "random" else 3 if kind != "P22" else 4)
    for t in carried:
        e = xc.model_error(case, kind, 1, drop=t)
        assert e > r.bound, (case, kind, t, e, r.bound)


def test_probes_carry_all_six_terms():
    xc.probe_terms_seen()


@pytest.mark.parametrize("case,kind", xc.PARAMS, ids=IDS)
def test_f32_contraction(k, case, kind):
    xc.run_case(k, case, kind, "simulator")


def test_switch_is_left_as_found(k):
    """after every case above: the library multiplies as it did before, and lib._f32_mode -- which the engine trusts -- says so"""
    assert xc.current_mode(k) == k.mode_before == getattr(k.lib, "_f32_mode", 0)
