"""PPO.learn on the Atari fast path, every frame source against every other: stacked frames or data.FramePlanes, FRAMES_IN_PLACE off or on,
the eager read-back or DEFERRED_LOSS_READBACK, with the diagnostics on, under the defaults and under two sets of minibatch knobs.  The eight
nets of a case start from identical weights and see identical content (tests/test_plane_pool_gpu.py rollouts: B = 15, where a plane stack
crosses an episode reset and K = 4 gives the uneven slices 4 / 4 / 4 / 3), so every loss dict, update_time, parameter and optimiser moment is
compared bit for bit.  The anchor to independent arithmetic is tests/test_minibatch_gpu.py.  Run with `-m gpu`."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

C, ITERS = 4, 2
KNOBS = {
    "defaults": dict(),
    "K4-shuffled-batch-norm": dict(PPO_MINIBATCHES=4, PPO_SHUFFLE=True, NORMALIZE_ADVANTAGE="batch"),
    "K2-in-order-minibatch-norm": dict(PPO_MINIBATCHES=2, NORMALIZE_ADVANTAGE="minibatch"),
}


def run_learn(net, exp):
    out = []
    for ld, update_time, last in net.learn(exp):
        assert last is True
        out.append(({k: v for k, v in ld.items() if k != "PpoBackUpTime"}, update_time))
    return out


@pytest.mark.parametrize("knobs", list(KNOBS), ids=list(KNOBS))
def test_every_frame_source_and_read_back_gives_the_same_update(knobs):
    import test_plane_pool_gpu as P
    from ddrl4nav_amd import ops
    stacked, planes, _ = P.rollouts(C)
    opts, K = KNOBS[knobs], KNOBS[knobs].get("PPO_MINIBATCHES", 1)
    first = None
    for source, in_place, deferred in itertools.product((stacked, planes), (False, True), (False, True)):
        who = (type(source).__name__, in_place, deferred)
        net = P.make_net(C, seed=3, iters=ITERS, PPO_DIAGNOSTICS=True, FRAMES_IN_PLACE=in_place, DEFERRED_LOSS_READBACK=deferred, **opts)
        assert net.frames_in_place is in_place and net.deferred_stats is deferred
        before = net.hot_path.params.clone()
        items = run_learn(net, source.batch())
        hp = net.hot_path
        assert len(items) == ITERS * K and hp.step == ITERS * K and net.update_time == ITERS * K, who
        assert all(set(ops.DIAG_KEYS) <= set(ld) for ld, _ in items), who
        assert not torch.equal(hp.params, before), who                 # the update did something
        assert net.learn_calls == (0 if knobs == "defaults" else 1), who
        got = (items, hp.step, hp.params.clone(), hp.adam_m.clone(), hp.adam_v.clone())
        if first is None:
            first = got
            continue
        assert got[0] == first[0], who                                 # floats compared with ==: the same bits
        assert got[1] == first[1], who
        for k, x, y in zip(("params", "adam_m", "adam_v"), got[2:], first[2:]):
            assert torch.equal(x, y), (who, k)


@pytest.mark.parametrize("opts", [dict(), dict(PPO_MINIBATCHES=2)], ids=["defaults", "K2"])
def test_deferred_read_back_switched_on_after_construction_refuses_target_kl(opts):
    import test_plane_pool_gpu as P
    stacked, _, _ = P.rollouts(C)
    net = P.make_net(C, seed=3, iters=ITERS, TARGET_KL=0.01, **opts)
    net.deferred_stats = True
    with pytest.raises(ValueError, match="TARGET_KL"):
        next(net.learn(stacked.batch()))
    assert net.update_time == 0
