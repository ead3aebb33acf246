"""optimization.PendingUpdate, the one owner of a BertAdam update between optimizer.step() and the forward that applies it, and
engine.Plan.select_segments -- host logic only: the two update entry points of the library are replaced by a recording stand-in."""
import ctypes as C
import types

import pytest
import torch

from univl_amd import BertAdam, _lib, optimization
from univl_amd.engine import Plan, Riders
from univl_amd.optimization import ADOPTED, APPLIED, PARTIAL, PENDING, STARTED, PendingUpdate

B1, V1 = ("layer", "bert", 1), ("layer", "visual", 1)
# two "base" runs, the layers of two stacks, a key that appears twice (B1: carried once, its second run is a prologue launch) and a key
# the plan does not carry (the cross encoder); 21 chunks, every one in exactly one group
GROUPS = [("base", 0, 3), ("base", 5, 2), (("layer", "bert", 0), 3, 2), (("layer", "visual", 0), 7, 3), (B1, 10, 4), (V1, 14, 3),
          (B1, 17, 2), (("layer", "cross", 0), 19, 2)]
RIDER_KEYS = {B1, V1, ("layer", "bert", 2)}
PROLOGUE = GROUPS[:4] + GROUPS[6:]             # in launch order
NCHUNK, NSLOTS, H = 21, 4, C.c_void_p(0)


class _Recorder:
    """Stands in for univl_bert_adam / univl_bert_adam_range: records (first, count, do_prep, max_blocks) of every launch it accepts;
    `refuse`: the index of the range call it answers with an error code (nothing goes out), `throw`: of the one that raises inside."""

    def __init__(self):
        self.launches, self.whole, self.calls, self.refuse, self.throw = [], 0, 0, None, None

    def adam(self, ref, h):
        self.whole += 1
        return 0

    def adam_range(self, ref, c0, n, do_prep, max_blocks, h):
        i, self.calls = self.calls, self.calls + 1
        if i == self.throw:
            raise KeyboardInterrupt
        if i == self.refuse:
            return -1
        self.launches.append((c0, n, do_prep, max_blocks))
        return 0

    def chunks(self):
        return [c for c0, n, _, _ in self.launches for c in range(c0, c0 + n)]


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(_lib.lib(), "univl_bert_adam", r.adam, raising=False)
    monkeypatch.setattr(_lib.lib(), "univl_bert_adam_range", r.adam_range, raising=False)
    monkeypatch.setattr(optimization, "_stream", lambda: H)                     # no device here: no current stream ...
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)   # ... and nobody capturing it
    return r


def _update(auto=True):
    opt = BertAdam([torch.nn.Parameter(torch.zeros(2))], lr=1e-3)
    opt.chunk_groups = lambda: GROUPS
    model = types.SimpleNamespace(auto_ride_count=0)
    opt._update = PendingUpdate(opt, _lib.Adam(), auto, lambda: model)
    return opt, opt._update, model


def _take_all(riders, key):
    return [c for s in range(NSLOTS) for lo, n in [riders.take(key, s, NSLOTS)] for c in range(lo, lo + n)]


def test_every_transition_of_a_pending_update(rec):
    opt, u, model = _update()
    assert u.state == PENDING and opt.has_pending and opt._deferred and opt._auto_deferred
    # PENDING: flush -> APPLIED (one whole launch); everything else but adopt raises
    for bad in (u.hand_back, u.done, lambda: u.start(RIDER_KEYS, H), u.complete_after_failure):
        with pytest.raises(RuntimeError, match="pending"):
            bad()
    opt.flush()
    assert u.state == APPLIED and rec.whole == 1 and not opt.has_pending and not opt._auto_deferred
    for bad in (u.flush, u.adopt, u.hand_back, u.done, lambda: u.start(RIDER_KEYS, H), u.complete_after_failure):
        with pytest.raises(RuntimeError, match="applied"):
            bad()
    opt.flush()                                     # the optimizer's own flush: nothing pending, nothing to do
    opt.launch_deferred(groups=GROUPS)
    assert rec.whole == 1 and not rec.launches
    # PENDING -> ADOPTED -> PENDING -> ADOPTED -> STARTED -> APPLIED
    opt, u, model = _update()
    assert u.adopt(max_blocks=7) is u and u.state == ADOPTED and u.max_blocks == 7 and model.auto_ride_count == 1
    assert not opt.has_pending and not opt._deferred and not opt._auto_deferred
    for bad in (u.adopt, u.flush, u.done, u.complete_after_failure):          # adopt twice, flush of an adopted record, ...
        with pytest.raises(RuntimeError, match="adopted"):
            bad()
    opt.flush()                                     # (has_pending is False: the forward that adopted it applies it)
    assert rec.whole == 1 and u.state == ADOPTED
    u.hand_back()
    assert u.state == PENDING and opt.has_pending and opt._auto_deferred and model.auto_ride_count == 0
    u.adopt()
    riders = u.start(RIDER_KEYS, H)
    assert u.state == STARTED and isinstance(riders, Riders) and riders.ranges == {B1: (10, 4), V1: (14, 3)} and riders.max_blocks == 0
    assert [l[:2] for l in rec.launches] == [g[1:] for g in PROLOGUE] and not opt.has_pending
    for bad in (u.adopt, u.flush, u.hand_back, lambda: u.start(RIDER_KEYS, H)):         # hand back after start, ...
        with pytest.raises(RuntimeError, match="started"):
            bad()
    u.done()
    assert u.state == APPLIED and model.auto_ride_count == 1 and not opt.has_pending
    # start from PENDING was refused above; an update step(defer=True) left is not the unchanged loop's: no ride is counted
    opt, u, model = _update(auto=False)
    assert opt.has_pending and not opt._auto_deferred
    u.adopt(max_blocks=3)
    assert u.start(RIDER_KEYS, H).max_blocks == 3 and model.auto_ride_count == 0
    # launch by groups: one range launch per group, the first one prepares
    opt, u, model = _update()
    rec.launches.clear()
    seen = []
    opt.launch_deferred(groups=GROUPS, on_group=seen.append, max_blocks=5)
    assert rec.launches == [(c0, n, int(i == 0), 5) for i, (_, c0, n) in enumerate(GROUPS)] and u.state == APPLIED
    assert seen == ["base", ("layer", "bert", 0), ("layer", "visual", 0), B1, V1, B1, ("layer", "cross", 0)]


def test_nothing_rides_and_nothing_goes_out_in_front_still_prepares_once(rec):
    opt, u, _ = _update()
    opt.chunk_groups = lambda: [(B1, 0, 4)]
    riders = u.adopt().start(RIDER_KEYS, H)
    assert rec.launches == [(0, 0, 1, 0)] and riders.ranges == {B1: (0, 4)}


@pytest.mark.parametrize("prefix", range(len(PROLOGUE) + 1))
def test_failure_after_a_prefix_of_the_prologue_completes_every_chunk_once(rec, prefix):
    """The launch after `prefix` accepted ones is refused (error code: it did not go out) and start() raises; prefix == len(PROLOGUE):
    the scalar-preparing launch is not needed, start() returns and the failure comes before the plan's first launch."""
    opt, u, _ = _update()
    u.adopt()
    rec.refuse = prefix if prefix < len(PROLOGUE) else None
    if prefix < len(PROLOGUE):
        with pytest.raises(RuntimeError, match="bert_adam_range"):
            u.start(RIDER_KEYS, H)
        riders = None
    else:
        riders = u.start(RIDER_KEYS, H)
    assert u.state == STARTED and len(rec.launches) == prefix
    u.complete_after_failure(riders, ValueError("injected"))
    assert u.state == APPLIED and not opt.has_pending and u.left == []
    assert sorted(rec.chunks()) == list(range(NCHUNK))
    assert [l[2] for l in rec.launches] == [1] + [0] * (len(rec.launches) - 1)


@pytest.mark.parametrize("whole_keys", [(), (B1,), (V1,), (B1, V1)])
def test_failure_on_a_key_boundary_of_the_riders_completes_every_chunk_once(rec, whole_keys):
    opt, u, _ = _update()
    riders = u.adopt().start(RIDER_KEYS, H)
    carried = [c for key in whole_keys for c in _take_all(riders, key)]
    assert all(riders.whole(k) for k in whole_keys) and not any(riders.whole(k) for k in {B1, V1} - set(whole_keys))
    u.complete_after_failure(riders, ValueError("injected"))
    assert u.state == APPLIED and not opt.has_pending
    assert sorted(rec.chunks() + carried) == list(range(NCHUNK))
    assert [l[2] for l in rec.launches] == [1] + [0] * (len(rec.launches) - 1)
    assert len(rec.launches) == len(PROLOGUE) + 2 - len(whole_keys)


def test_a_partly_carried_key_or_an_unknown_launch_is_a_partial_update(rec, monkeypatch):
    cause = ValueError("injected")
    # one key taken at slot 0 of 4
    opt, u, _ = _update()
    riders = u.adopt().start(RIDER_KEYS, H)
    n = len(rec.launches)
    assert riders.take(B1, 0, NSLOTS) == (10, 1) and riders.pending() == [(B1, 10, 4, True), (V1, 14, 3, False)]
    with pytest.raises(RuntimeError) as ei:
        u.complete_after_failure(riders, cause)
    assert str(ei.value) == PARTIAL and ei.value.__cause__ is cause
    assert u.state == APPLIED and not opt.has_pending and len(rec.launches) == n          # nothing pending, nothing guessed
    # a launch of start() that did not return: whether it went out cannot be told
    opt, u, _ = _update()
    u.adopt()
    rec.throw = rec.calls + 2
    with pytest.raises(KeyboardInterrupt):
        u.start(RIDER_KEYS, H)
    with pytest.raises(RuntimeError) as ei:
        u.complete_after_failure(None, cause)
    assert str(ei.value) == PARTIAL and ei.value.__cause__ is cause and u.state == APPLIED and not opt.has_pending
    # somebody else's capture: nothing extra is enqueued
    opt, u, _ = _update()
    riders = u.adopt().start(RIDER_KEYS, H)
    n = len(rec.launches)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError) as ei:
        u.complete_after_failure(riders, cause)
    assert str(ei.value) == PARTIAL and len(rec.launches) == n and not opt.has_pending
    # a carrying launch of the plan that failed took its part: its key is never whole
    rd = Riders(_lib.Adam(), {B1: (10, 4)})
    _take_all(rd, B1)
    assert rd.whole(B1)
    rd.nslots[B1] = 0                                           # what Plan._run_ops records for a launch that returned an error
    assert not rd.whole(B1) and not rd.whole(V1)


def test_a_run_through_graphs_tells_nothing_until_its_last_replay(rec):
    """Plan.run_graphed: a capture takes parts no kernel has applied, a replay applies parts nobody takes -- Riders.graphed says which
    of the two the host may believe: False (under way) is a partial update whatever `used` holds, True (all replayed) is complete
    whatever it holds, and in neither case does a carried range go out again."""
    cause = ValueError("injected")
    for taken in ((), (B1, V1)):                                # a replay takes nothing, a capture everything
        for graphed in (False, True):
            opt, u, _ = _update()
            riders = u.adopt().start(RIDER_KEYS, H)
            n = len(rec.launches)
            for key in taken:
                _take_all(riders, key)
            riders.graphed = graphed
            assert riders.pending() == [(B1, 10, 4, True), (V1, 14, 3, True)] and riders.whole(B1) is graphed and riders.whole(V1) is graphed
            if graphed:
                u.complete_after_failure(riders, cause)
            else:
                with pytest.raises(RuntimeError) as ei:
                    u.complete_after_failure(riders, cause)
                assert str(ei.value) == PARTIAL and ei.value.__cause__ is cause
            assert u.state == APPLIED and not opt.has_pending and len(rec.launches) == n


def test_a_refused_completing_launch_is_a_partial_update(rec):
    opt, u, _ = _update()
    riders = u.adopt().start(RIDER_KEYS, H)
    rec.refuse = rec.calls + 1                                  # the second of the two ranges that still have to go out
    cause = ValueError("injected")
    with pytest.raises(RuntimeError) as ei:
        u.complete_after_failure(riders, cause)
    assert str(ei.value) == PARTIAL and ei.value.__cause__ is cause
    assert u.state == APPLIED and not opt.has_pending and [g[0] for g in u.left] == [V1]


def test_plan_keeps_captured_segments_per_rider_signature():
    plan = Plan()
    assert plan._segments is None and plan._seg_cache == {} and plan._rider_sig is None
    captured = []

    def run(sig, keep=4):
        if plan.select_segments(sig, keep):
            captured.append(sig)
            plan._segments = ["segments of", sig]               # what run_graphed() leaves behind
        assert plan._segments == ["segments of", sig] and plan._rider_sig == sig and sig not in plan._seg_cache

    for _ in range(3):                                          # two signatures alternate: one capture each; None is one like any other
        run(None)
        run("a")
    assert captured == [None, "a"] and "_seg_cache" in plan.__dict__ and list(plan._seg_cache) == [None]
    run("b")
    run("c")
    assert captured == [None, "a", "b", "c"] and list(plan._seg_cache) == [None, "a", "b"]
    run("d")                                                    # a fifth signature: the oldest goes
    assert list(plan._seg_cache) == ["a", "b", "c"]
    run("a")
    assert captured == [None, "a", "b", "c", "d"] and list(plan._seg_cache) == ["b", "c", "d"]
    run(None)                                                   # evicted: captured again
    assert captured[-1] is None and len(captured) == 6 and list(plan._seg_cache) == ["c", "d", "a"]
