"""The shared core of DeviceRollout, PlaneRollout and StateRollout (agent/rollout.py _RolloutBase) without a GPU and without a library
call: the one ring-ordering rule on recording stand-ins for the streams, the events and the ring; the life cycle (carry_over, record,
act below t0) on host tensors; and that the shared methods and the loop exist once."""
import types

import pytest
import torch

N, T, C = 2, 3, 2
SHAPES = [(3,), (2, 2)]


class Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_stream(self, other):
        self.log.append((self.name, "wait_stream", other.name))

    def wait_event(self, event):
        self.log.append((self.name, "wait_event", (event, event.gen)))


class Event:
    def __init__(self, log):
        self.log, self.gen = log, 0

    def record(self, stream):
        self.gen += 1
        self.log.append((stream.name, "record", (self, self.gen)))


class Ring:
    def __init__(self, log):
        self.log = log

    def pop_to(self, dst, stream=None):
        self.log.append((stream.name, "pop", dst.data_ptr()))


@pytest.fixture
def log(monkeypatch):
    """One ordered log of (stream, what, argument) for everything the stand-ins see; the launches behind the puts and finish() are
    no-ops, the push kernel logs the staging buffer it read."""
    from ddrl4nav_amd import ops
    from ddrl4nav_amd.agent import rollout as R
    entries = []
    cur = Stream("cur", entries)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: Stream("copy", entries))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: cur)
    monkeypatch.setattr(torch.cuda, "Event", lambda: Event(entries))
    monkeypatch.setattr(R, "frame_stack_push", lambda prev, newest, flags, out: entries.append(("cur", "push", newest.data_ptr())))
    monkeypatch.setattr(R, "gae_device", lambda *a, **k: None)
    monkeypatch.setattr(ops, "frame_age", lambda *a, **k: None)
    monkeypatch.setattr(ops, "frame_slot", lambda *a, **k: None)
    return entries


def _net():
    return types.SimpleNamespace(device="cpu", n_actions=6)     # neither callable nor a hot path: acting on it raises


def _build(kind, **kw):
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout, StateRollout
    if kind == "device":
        return DeviceRollout(_net(), N, horizon=T, channels=C, device="cpu", **kw)
    if kind == "plane":
        return PlaneRollout(_net(), N, horizon=T + 1, channels=C, device="cpu", **kw)
    return StateRollout(_net(), N, SHAPES, horizon=T, device="cpu", **kw)


PUTS = {
    "full": ("device", {}, lambda ro, t, ring: ro.put_frames_from_ring(t, ring)),
    "single": ("device", {}, lambda ro, t, ring: ro.put_new_frames_from_ring(t, ring, reset=True if t == 0 else None)),
    "plane": ("plane", {"act_in_place": False}, lambda ro, t, ring: ro.put_new_frames_from_ring(t, ring, reset=True if t == 0 else None)),
    "plane_in_place": ("plane", {"act_in_place": True},
                       lambda ro, t, ring: ro.put_new_frames_from_ring(t, ring, reset=True if t == 0 else None)),
    "state": ("state", {}, lambda ro, t, ring: [ro.put_state_from_ring(t, k, ring) for k in range(len(SHAPES))]),
}


@pytest.mark.parametrize("name", sorted(PUTS))
def test_the_first_ring_put_of_every_rollout_orders_the_copy_stream_once(log, name):
    """Three chained rollouts: a fresh one (first put slot 0), one behind finish(); carry_over() and one behind finish();
    carry_over(keep_step=True) (first put slot 1 in both).  Each sees exactly one wait of the copy stream for the current stream, in
    front of its first pop; the current stream waits for the copy stream after every pop."""
    kind, kw, put = PUTS[name]
    ro, ring = _build(kind, **kw), Ring(log)
    assert ro._ring_rollout == -1 and not hasattr(ro, "_ring_ordered")
    pops_per_slot = len(SHAPES) if kind == "state" else 1
    for r, (first, keep_step) in enumerate(((0, False), (1, True), (1, False))):     # keep_step: how this rollout is carried over
        del log[:]
        assert ro.rollouts == r
        for t in range(first, ro.T + 1):
            put(ro, t, ring)
        assert ro._ring_rollout == r
        copy = [e for e in log if e[0] == "copy"]
        assert [e for e in copy if e[1] == "wait_stream"] == [("copy", "wait_stream", "cur")], (name, r)
        first_pop = next(i for i, e in enumerate(copy) if e[1] == "pop")
        assert copy.index(("copy", "wait_stream", "cur")) < first_pop, (name, r)
        pops = [i for i, e in enumerate(log) if e[1] == "pop"]
        assert len(pops) == (ro.T + 1 - first) * pops_per_slot
        assert all(log[i + 1] == ("cur", "wait_stream", "copy") for i in pops), (name, r)
        assert log.count(("cur", "wait_stream", "copy")) == len(pops)
        ro.finish()
        assert ro.rollouts == r + 1
        ro.carry_over(keep_step=keep_step)
        assert ro.t0 == int(keep_step)
        assert not [e for e in log if e[1] == "pop"][len(pops):]       # finish() and carry_over() touch no ring


def test_the_staging_buffers_of_the_single_frame_put_keep_their_events(log):
    """DeviceRollout.put_new_frames_from_ring: every pop into staging buffer k other than its first is preceded, on the copy stream, by a
    wait for the event recorded after the previous push that read buffer k -- across rollouts as well."""
    ro, ring = _build("device"), Ring(log)
    for first in (0, 1, 1):
        for t in range(first, T + 1):
            ro.put_new_frames_from_ring(t, ring, reset=True if t == 0 else None)
        ro.finish()
        ro.carry_over()
    recorded = {}      # buffer -> (event, generation) recorded after the last push that read it
    waited = set()     # what the copy stream has waited for since its last pop
    seen, last_push = set(), None
    for stream, what, arg in log:
        if what == "wait_event":
            assert stream == "copy"
            waited.add((id(arg[0]), arg[1]))
        elif what == "pop":
            if arg in seen:
                assert (id(recorded[arg][0]), recorded[arg][1]) in waited, "pop into a staging buffer its last push may still read"
            seen.add(arg)
            waited = set()
        elif what == "push":
            last_push = arg
        elif what == "record":
            assert stream == "cur" and last_push is not None
            recorded[last_push], last_push = arg, None
    assert len(seen) == 2 and set(recorded) == seen           # two staging buffers, both pushed from
    assert len([e for e in log if e[1] == "pop"]) == (T + 1) + T + T


def _pools(ro):
    return [ro.values, ro._rewards, ro._dones, ro._actions, ro._logps] + ([ro._infos] if ro._infos is not None else [])


def _observation_rows(ro, t):
    """The rows that are slot t's observation (a plane slot: its frame with the H history rows in front, and its age)."""
    if hasattr(ro, "planes"):
        return [ro.planes[t:t + ro.H + 1], ro.age[t]]
    return [ro.frames[t]] if hasattr(ro, "frames") else [p[t] for p in ro.states]


@pytest.mark.parametrize("kind,kw", [("device", {}), ("plane", {"act_in_place": False}), ("plane", {"act_in_place": True}), ("state", {}),
                                     ("state", {"track_nav_status": True})])
def test_carry_over_record_and_act_below_t0(log, kind, kw):
    def marked():
        ro = _build(kind, **kw)
        for rows in _observation_rows(ro, 0) + [p[0] for p in _pools(ro)]:
            rows.fill_(0)
        for rows in _observation_rows(ro, ro.T) + [p[ro.T] for p in _pools(ro)]:
            rows.fill_(7)
        if kind == "plane":
            ro._slot_t = 2
        return ro

    ro = marked()
    assert (ro._infos is not None) == bool(kw.get("track_nav_status"))
    ro.carry_over(keep_step=True)
    assert ro.t0 == 1
    assert all(bool((rows == 7).all()) for rows in _observation_rows(ro, 0))
    assert all(bool((p[0] == 7).all()) for p in _pools(ro))
    if kind == "plane":
        assert ro._slot_t == -1
    with pytest.raises(ValueError, match="carried over from the previous rollout with its reward and done"):
        ro.record(0, torch.zeros(N), torch.zeros(N, dtype=torch.uint8), info=torch.zeros(N, dtype=torch.int32))
    kept = ro.act(0)                                            # the net is not callable: it was not asked
    assert kept.data_ptr() == ro._actions[0].data_ptr() and bool((kept == 7).all())

    ro = marked()
    ro.carry_over()
    assert ro.t0 == 0
    assert all(bool((rows == 7).all()) for rows in _observation_rows(ro, 0))
    assert all(bool((p[0] == 0).all()) for p in _pools(ro))
    if kind == "plane":
        assert ro._slot_t == -1
    ro.record(0, torch.ones(N), torch.ones(N, dtype=torch.uint8), info=torch.ones(N, dtype=torch.int32))
    assert bool((ro._rewards[0] == 1).all()) and bool((ro._dones[0] == 1).all())
    assert ro._infos is None or bool((ro._infos[0] == 1).all())


def test_the_shared_methods_and_the_loop_are_written_once():
    from ddrl4nav_amd.agent import DeviceRollout, PlaneRollout, StateRollout
    from ddrl4nav_amd.agent.rollout import _RolloutBase
    from ddrl4nav_amd.runner import device_loop
    assert issubclass(PlaneRollout, DeviceRollout) and issubclass(DeviceRollout, _RolloutBase) and issubclass(StateRollout, _RolloutBase)
    for method in ("record", "finish", "carry_over", "_value_rows", "_order_copy_stream"):
        shared = getattr(_RolloutBase, method)
        assert all(getattr(cls, method) is shared for cls in (DeviceRollout, PlaneRollout, StateRollout)), method
    frames, states = device_loop.train(None, None, None, 0), device_loop.train_states(None, None, None, 0)
    assert frames.gi_code is states.gi_code
    assert list(frames) == [] and list(states) == []
