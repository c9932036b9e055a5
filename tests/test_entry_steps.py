"""dpc_amd.entry.StepDriver, the ``--graph`` protocol both entries run their steps through, driven by a stub engine that records
what it is asked for: which steps are eager, when each kind of step is captured and with what, what is replayed, where `refill`
and `before_replay` run.  Host only: no GPU, no simulator.  (The timing events are torch.cuda's; a stand-in replaces them here.)"""
import pytest
import torch

from dpc_amd import entry


class _Engine:
    """capture_* hand out counting closures and log every request"""

    def __init__(self, log):
        self.log, self.handles = log, []

    def _handle(self, kind):
        def replay():
            replay.calls += 1
            self.log.append(("replay", kind, replay.id))
            return ("result", kind, replay.id)
        replay.calls, replay.id = 0, len(self.handles)
        self.handles.append(replay)
        return replay

    def capture_train_step(self, block, allreduce=None, warmup=2, refill=None):
        self.log.append(("capture_train", block, allreduce, warmup, refill))
        return self._handle("train")

    def capture_eval_step(self, refill=None):
        self.log.append(("capture_eval", refill))
        return self._handle("eval")


class _Event:
    made = 0

    def __init__(self, enable_timing=False):
        assert enable_timing
        _Event.made += 1
        self.recorded = 0

    def record(self):
        self.recorded += 1

    def synchronize(self):
        pass

    def elapsed_time(self, other):
        return 12.0


@pytest.fixture
def rig(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    _Event.made = 0
    log = []
    fill_t, fill_v = (lambda: log.append("refill_train")), (lambda: log.append("refill_val"))
    return log, _Engine(log), fill_t, fill_v


def _step(drv, log, train):
    """one step the way the entries take it; returns (result, replayed) and the log lines it added"""
    n = len(log)
    out = drv.step(train, lambda: log.append("eager_train" if train else "eager_val") or ("eager", train),
                   lambda: log.append("before_replay"))
    return out, log[n:]


@pytest.mark.parametrize("refills", [True, False])
def test_without_graph_every_step_is_eager(rig, refills):
    log, eng, fill_t, fill_v = rig
    drv = entry.StepDriver(eng, False, "exchange", *((fill_t, fill_v) if refills else ()))
    for _ in range(2):   # two "epochs"
        for train, n in ((True, 4), (False, 3)):
            for _ in range(n):
                (res, replayed), added = _step(drv, log, train)
                assert res == ("eager", train) and replayed is False
                name = "train" if train else "val"
                assert added == (["refill_" + name] if refills else []) + ["eager_" + name]
        assert drv.replay_line(8) is None
    assert not eng.handles and _Event.made == 0


def test_graph_warms_up_captures_once_and_replays(rig):
    log, eng, fill_t, fill_v = rig
    drv = entry.StepDriver(eng, True, "exchange", fill_t, fill_v)
    assert log == [] and _Event.made == 0   # nothing happens before the first step
    # ---- epoch 1: train steps 1-2 and validation step 1 are eager, refill in front, no before_replay
    for _ in range(2):
        (res, replayed), added = _step(drv, log, True)
        assert (res, replayed, added) == (("eager", True), False, ["refill_train", "eager_train"])
    assert _Event.made == 0
    # train step 3: one capture (the operand, the exchange, warmup=0, this kind's refill), then the replay
    (res, replayed), added = _step(drv, log, True)
    assert replayed is True and res == ("result", "train", 0)
    assert added == ["before_replay", ("capture_train", None, "exchange", 0, fill_t), ("replay", "train", 0)]
    # later train steps: the same handle, the engine is not asked, refill is not called eagerly
    for _ in range(3):
        (res, replayed), added = _step(drv, log, True)
        assert replayed is True and res == ("result", "train", 0) and added == ["before_replay", ("replay", "train", 0)]
    assert drv.replay_line(8) == "Graph replay: 4 steps, 3.000 ms/step, 2666.7 clips/s"
    assert drv.replay_line(8) is None and _Event.made == 2
    (res, replayed), added = _step(drv, log, False)
    assert (res, replayed, added) == (("eager", False), False, ["refill_val", "eager_val"])
    (res, replayed), added = _step(drv, log, False)
    assert replayed is True and res == ("result", "eval", 1)
    assert added == ["before_replay", ("capture_eval", fill_v), ("replay", "eval", 1)]
    (res, replayed), added = _step(drv, log, False)
    assert replayed is True and added == ["before_replay", ("replay", "eval", 1)]
    assert drv.replay_line(8) is None and _Event.made == 2   # validation replays are not timed
    # ---- epoch 2: the warm-up is per run -- both kinds replay at once, on the handles that exist
    for train, kind, hid in ((True, "train", 0), (True, "train", 0), (False, "eval", 1)):
        (res, replayed), added = _step(drv, log, train)
        assert replayed is True and added == ["before_replay", ("replay", kind, hid)]
    assert drv.replay_line(6) == "Graph replay: 2 steps, 6.000 ms/step, 1000.0 clips/s" and _Event.made == 4
    assert [h.calls for h in eng.handles] == [6, 3]
    assert log.count("refill_train") == 2 and log.count("refill_val") == 1 and log.count("before_replay") == 9


def test_invalidate_asks_the_engine_again_without_a_new_warm_up(rig):
    log, eng, fill_t, fill_v = rig
    drv = entry.StepDriver(eng, True, None, fill_t, fill_v)
    drv.invalidate()   # before anything was captured (lc_main sets its first learning rate): the warm-up is still due
    for train in (True, True, True, False, False):
        _step(drv, log, train)
    assert [h.calls for h in eng.handles] == [1, 1]
    drv.invalidate()
    for train, kind, hid in ((True, "train", 2), (False, "eval", 3)):
        (res, replayed), added = _step(drv, log, train)
        assert replayed is True and res == ("result", kind, hid)
        assert added[0] == "before_replay" and added[1][0] == "capture_" + kind and added[2] == ("replay", kind, hid)
        (res, replayed), added = _step(drv, log, train)   # ... once: the next step replays the new handle
        assert added == ["before_replay", ("replay", kind, hid)]
    assert [h.calls for h in eng.handles] == [1, 1, 2, 2]
    assert "eager_train" not in log[log.index(("replay", "train", 0)):] and log.count("eager_train") == 2 and log.count("eager_val") == 1


def test_before_replay_is_optional_and_one_rank_averages_to_itself(rig):
    log, eng, _, _ = rig
    drv = entry.StepDriver(eng, True)
    for _ in range(3):
        res, replayed = drv.step(True, lambda: "eager")
    assert replayed is True and log == [("capture_train", None, None, 0, None), ("replay", "train", 0)]
    t = torch.tensor([1.0, 2.0])
    assert entry.average_over_ranks(None, t, 1) is t
    from dpc_amd.main import average_over_ranks   # where tests/test_parallel_gloo.py finds it
    assert average_over_ranks is entry.average_over_ranks
