"""GPU tier: the two-stream schedule of the train step (weight gradients on a side stream beside the next unit's BatchNorm
backward, dpc_amd/engine.py: side()) is the SAME computation as the one-stream schedule: parameters and gradients bit for bit,
step after step, launched kernel by kernel and as a replayed hipGraph.  (scripts/stream_stress.py is the long-running form of this
check at the BASELINE batch sizes; profiles/r03_two_stream.txt holds its runs.)"""
import contextlib

import pytest
import torch

from dpc_amd.engine import DPCEngine
from oracle import dpc_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def build(monkeypatch, two_streams, net, size, B, P):
    monkeypatch.setenv("DPC_WGRAD_STREAM", "1" if two_streams else "0")
    e = DPCEngine(net, size, 8, 5, P, B, DEV, torch.bfloat16)
    e.load_params(O.init_params_reference_style(net, seed=3))
    assert (e._side is not None) == two_streams
    return e


@pytest.mark.parametrize("net,size,B,P,graph", [("resnet18", 128, 16, 3, False), ("resnet18", 128, 16, 3, True), ("resnet34", 224, 4, 3, True)])
def test_two_streams_bit_identical_to_one(monkeypatch, net, size, B, P, graph):
    a, b = build(monkeypatch, True, net, size, B, P), build(monkeypatch, False, net, size, B, P)
    x = torch.randn(B, 8, 3, 5, size, size, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    fa, fb = (a.capture_train_step(x), b.capture_train_step(x)) if graph else ((lambda: a.train_step(x)), (lambda: b.train_step(x)))
    for step in range(10):
        ra, rb = fa().clone(), fb().clone()
        torch.cuda.synchronize()
        assert torch.equal(ra, rb), (step, ra, rb)
        assert torch.equal(a.flat_g, b.flat_g), f"gradients differ at step {step}"
        assert torch.equal(a.flat_p, b.flat_p), f"parameters differ at step {step}"
    assert not a._busy   # every fork was joined


def _count_forks(e):
    """wraps e.side: e.entered = the sites that were entered, e.forked = those whose launches went to the side stream"""
    inner = e.side
    e.entered, e.forked = [], []

    @contextlib.contextmanager
    def side(reads=(), site=""):
        e.entered.append(site)
        with inner(reads=reads, site=site):
            if e._on_side:
                e.forked.append(site)
            yield
    e.side = side


SITES_OFF = ("pack", "head", "layer2.0.c1")


def test_side_sites_off_bit_identical_and_not_forked(monkeypatch):
    """DPC_SIDE_OFF: the named sites stay on the main stream, everything else is the default schedule -- same results, gradients and
    parameters bit for bit, and exactly the named sites no longer fork"""
    net, size, B, P, steps = "resnet18", 128, 16, 3, 10
    a = build(monkeypatch, True, net, size, B, P)
    monkeypatch.setenv("DPC_SIDE_OFF", ",".join(SITES_OFF))
    b = build(monkeypatch, True, net, size, B, P)
    monkeypatch.delenv("DPC_SIDE_OFF")
    assert a.side_off == frozenset() and b.side_off == frozenset(SITES_OFF)
    _count_forks(a)
    _count_forks(b)
    x = torch.randn(B, 8, 3, 5, size, size, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    for step in range(steps):
        ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
        torch.cuda.synchronize()
        assert torch.equal(ra, rb), (step, ra, rb)
        assert torch.equal(a.flat_g, b.flat_g), f"gradients differ at step {step}"
        assert torch.equal(a.flat_p, b.flat_p), f"parameters differ at step {step}"
    assert not a._busy and not b._busy
    assert a.entered == b.entered and a.forked == a.entered   # the default engine forks at every site
    for s in SITES_OFF:   # a misspelt name would switch nothing off
        assert a.entered.count(s) >= steps, f"site {s!r} is entered {a.entered.count(s)} times in {steps} steps: {sorted(set(a.entered))}"
        assert s not in b.forked
    named = sum(a.entered.count(s) for s in SITES_OFF)
    assert len(a.forked) - len(b.forked) == named > 0, (len(a.forked), len(b.forked), named)
    assert b.forked == [s for s in a.forked if s not in SITES_OFF]


def test_score_bf16_off_keeps_f32_logits(monkeypatch):
    """DPC_SCORE_BF16=0: no bf16 logit buffer, the train step materialises f32 logits; the default engine of the same shape has one"""
    net, size, B, P = "resnet18", 128, 16, 3
    a = build(monkeypatch, True, net, size, B, P)
    monkeypatch.setenv("DPC_SCORE_BF16", "0")
    b = build(monkeypatch, True, net, size, B, P)
    assert a.score16 is not None and b.score16 is None
    x = torch.randn(B, 8, 3, 5, size, size, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    ra, rb = a.train_step(x).clone(), b.train_step(x).clone()
    torch.cuda.synchronize()
    assert a.score_mode == "materialised (bf16 logits)" and b.score_mode == "materialised", (a.score_mode, b.score_mode)
    assert torch.isfinite(ra).all() and torch.isfinite(rb).all()
    print(f"loss / top-k  bf16 logits {ra.tolist()}  f32 logits {rb.tolist()}")
