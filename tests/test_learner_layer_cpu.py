"""The shared pieces of the learner layer above the C ABI, without a GPU: nn/base.py bind_arena, nn/minibatch.py learner_options,
nn/update_loop.py learn_columns and run().  run() is driven on a recording fake backend: the protocol after a step's launch is pinned
here once, for PPO (backend: engine.HotPath) and GenericPPO (backend: itself)."""
import types

import numpy as np
import pytest
import torch

from ddrl4nav_amd.nn import minibatch as M
from ddrl4nav_amd.nn import update_loop as U
from ddrl4nav_amd.nn.base import bind_arena


# ---- bind_arena ---------------------------------------------------------------------------------------------------------------------------
def _two_layers():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 2))


@pytest.mark.parametrize("with_grads", [False, True])
@pytest.mark.parametrize("pad", [0, 7])
def test_bind_arena_views_order_offsets(with_grads, pad):
    net = _two_layers()
    named = list(net.named_parameters())
    assert [k for k, _ in named] == ["0.weight", "0.bias", "2.weight", "2.bias"]
    before = {k: p.detach().clone() for k, p in named}
    total = 15 + 5 + 10 + 2 + pad
    params = torch.full((total,), -7.0)
    grads = torch.zeros(total + 8) if with_grads else None
    offsets = bind_arena(named, params, grads, {"2.weight": 20 + pad} if pad else None)
    assert offsets == {"0.weight": 0, "0.bias": 15, "2.weight": 20 + pad, "2.bias": 30 + pad}       # named_parameters() order, pad before 2.*
    assert list(offsets) == [k for k, _ in named]
    for k, p in net.named_parameters():
        o, n = offsets[k], p.numel()
        assert not p.requires_grad
        assert torch.equal(p.data, before[k]) and torch.equal(params[o:o + n].view(p.shape), before[k])   # the values were copied
        assert p.data.data_ptr() == params[o:o + n].data_ptr()
        p.data.mul_(2.0)                                            # a write through the view shows in the flat tensor ...
        assert torch.equal(params[o:o + n].view(p.shape), 2.0 * before[k])
        params[o:o + n] = 0.5                                       # ... and the reverse
        assert bool((p.data == 0.5).all())
        if with_grads:
            assert p.grad_view.shape == p.shape and p.grad_view.data_ptr() == grads[o:o + n].data_ptr()
            p.grad_view.fill_(3.0)
            assert bool((grads[o:o + n] == 3.0).all())
        else:
            assert not hasattr(p, "grad_view")
    assert bool((params[20:20 + pad] == -7.0).all())                # the pad is nobody's
    if with_grads:
        assert float(grads.sum()) == 3.0 * (total - pad)            # pad and statistics tail untouched


def test_bind_arena_casts_into_the_arena_dtype():
    net = _two_layers().double()
    want = [p.detach().float().clone() for p in net.parameters()]
    bind_arena(list(net.named_parameters()), torch.zeros(32))
    assert all(p.dtype == torch.float32 and torch.equal(p.data, w) for p, w in zip(net.parameters(), want))


# ---- learner_options ----------------------------------------------------------------------------------------------------------------------
ENV = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
       "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}
CALLERS = {"atari": dict(), "generic": dict(who="the operator-composed GenericPPO"), "gail": dict(who="NETWORK_TYPE='gail'", two_critics=True)}
OK, VE, NI = None, ValueError, NotImplementedError
# what the three constructors did with each knob before there was one reader (PPO.__init__, GenericPPO.__init__, GAIL.__init__ of the
# parent commit, read line by line): None = accepted.  GAIL refuses the diagnostics family before TARGET_KL is validated against
# DEFERRED_LOSS_READBACK, hence its NotImplementedError in the last row
TABLE = [
    (dict(PPO_DIAGNOSTICS=True),                         OK, OK, NI),
    (dict(TARGET_KL=0.02),                               OK, OK, NI),
    (dict(PPO_MINIBATCHES=2),                            OK, VE, VE),
    (dict(PPO_SHUFFLE=True),                             OK, VE, VE),
    (dict(NORMALIZE_ADVANTAGE="batch"),                  OK, VE, VE),
    (dict(FRAMES_IN_PLACE=True),                         OK, VE, VE),
    (dict(ACT_IN_PLACE=True),                            OK, VE, VE),
    (dict(VALUE_CLIP=0.2),                               OK, OK, VE),
    (dict(ENTROPY_BONUS_SPLIT=True),                     OK, OK, VE),
    (dict(LR_ANNEAL_UPDATES=4),                          OK, OK, OK),
    (dict(TARGET_KL=0.02, DEFERRED_LOSS_READBACK=True),  VE, VE, NI),
]
FIELD = {"PPO_DIAGNOSTICS": ("diagnostics", True), "TARGET_KL": ("target_kl", 0.02), "PPO_MINIBATCHES": ("minibatch", (2, False, None, 1e-8)),
         "PPO_SHUFFLE": ("minibatch", (1, True, None, 1e-8)), "NORMALIZE_ADVANTAGE": ("minibatch", (1, False, "batch", 1e-8)),
         "FRAMES_IN_PLACE": ("frames_in_place", True), "ACT_IN_PLACE": ("act_in_place", True), "VALUE_CLIP": ("loss_options", (0.2, False)),
         "ENTROPY_BONUS_SPLIT": ("loss_options", (0.0, True)), "LR_ANNEAL_UPDATES": ("lr_anneal", (4, 0.0, False))}


def _config_nn(**options):
    from ddrl4nav_amd.config import ConfigNN
    cfg_nn = ConfigNN(ENV)
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    return cfg_nn


def test_learner_options_defaults():
    cfg_nn = _config_nn()
    for kw in CALLERS.values():
        o = M.learner_options(cfg_nn, **kw)
        assert o[:7] == (False, None, M.DEFAULTS, False, False, (0.0, False), None)
        assert o.base_rates == (float(cfg_nn.ACTOR_LEARNING_RATE), float(cfg_nn.CRITIC_LEARNING_RATE), float(cfg_nn.LEARNING_RATE),
                                float(cfg_nn.PPO_CLIP))
        assert o._fields == ("diagnostics", "target_kl", "minibatch", "frames_in_place", "act_in_place", "loss_options", "lr_anneal",
                             "base_rates")


@pytest.mark.parametrize("row", TABLE, ids=["+".join(r[0]) for r in TABLE])
@pytest.mark.parametrize("col,caller", list(enumerate(CALLERS)), ids=list(CALLERS))
def test_learner_options_accepts_and_refuses_like_the_constructors_did(row, col, caller):
    opts, want = row[0], row[1 + col]
    cfg_nn = _config_nn(**opts)
    if want is None:
        o = M.learner_options(cfg_nn, **CALLERS[caller])
        for k in opts:
            name, value = FIELD[k]
            assert getattr(o, name) == value
        if "TARGET_KL" in opts:
            assert o.diagnostics is True          # a target implies the diagnostics
        return
    with pytest.raises(want) as e:
        M.learner_options(cfg_nn, **CALLERS[caller])
    assert type(e.value) is want
    if caller != "atari":
        assert CALLERS[caller]["who"] in str(e.value) or "DEFERRED_LOSS_READBACK" in str(e.value)
    assert any(k in str(e.value) for k in opts)


# ---- learn_columns --------------------------------------------------------------------------------------------------------------------------
def _batch(rows, B=6, dtype=np.float64):
    rng = np.random.default_rng(rows)
    col = lambda: rng.normal(size=B).astype(dtype)
    values = rng.normal(size=(rows, B)).astype(dtype) if rows else rng.normal(size=B).astype(dtype)
    return types.SimpleNamespace(values=values, actions=col(), old_logps=col(), advs=col())


@pytest.mark.parametrize("rows", [1, 2, 3])
@pytest.mark.parametrize("wants_old", [False, True])
@pytest.mark.parametrize("extra", [0, 1])
def test_learn_columns_rows(rows, wants_old, extra):
    d = _batch(rows)
    cpu = torch.device("cpu")
    if wants_old and rows < 2:
        with pytest.raises(ValueError, match="VALUE_CLIP needs the collecting policy's values as row 1 of data.values") as e:
            U.learn_columns(d, cpu, wants_old, extra)
        assert "1 row(s)" in str(e.value)
        return
    if extra and rows < 2:
        with pytest.raises(AssertionError, match="one row per critic"):
            U.learn_columns(d, cpu, wants_old, extra)
        return
    (actions, old_logps, advs, rets, old_values), extra_rets = U.learn_columns(d, cpu, wants_old, extra)
    f32 = lambda a: torch.from_numpy(np.asarray(a)).float()
    for got, want in ((actions, d.actions), (old_logps, d.old_logps), (advs, d.advs), (rets, d.values[0])):
        assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, f32(want))
    if wants_old:
        assert old_values.is_contiguous() and torch.equal(old_values, f32(d.values[1]))        # row 1, whatever follows it
    else:
        assert old_values is None
    if extra:
        assert len(extra_rets) == 1 and extra_rets[0].is_contiguous() and torch.equal(extra_rets[0], f32(d.values[-1]))   # the LAST row
    else:
        assert extra_rets == []


def test_learn_columns_refuses_a_flat_values_column_under_value_clip():
    with pytest.raises(ValueError, match="row 1 of data.values.*1 row"):
        U.learn_columns(_batch(0), torch.device("cpu"), True)
    cols, extra = U.learn_columns(_batch(1), torch.device("cpu"), False)
    assert len(cols) == 5 and extra == []


# ---- run() on a recording backend -------------------------------------------------------------------------------------------------------------
BASE_RATES = (5e-5, 1e-3, 2e-4, 0.2)
LOSS_KEYS = {"PpoTotalLoss", "ActorLoss", "VLoss", "EntLoss", "PpoBackUpTime"}
DIAG_KEYS = {"ApproxKL", "ClipFraction", "ExplainedVariance", "RatioMax"}


class Backend:
    """Appends the name of every call to `log`; the sums of step i say ApproxKL = kls[i], its statistics PpoTotalLoss = 10 + i."""

    def __init__(self, log, kls):
        self.log, self.kls, self.step = log, kls, -1
        self._options = None

    loss_options = property(lambda self: self._options)

    @loss_options.setter
    def loss_options(self, v):
        self.log.append("loss_options")
        self._options = v

    def set_rates(self, *rates):
        self.log.append(("set_rates",) + rates)

    def launch(self, actions, old_logps, advs, rets, b_global=None, old_values=None):
        assert (actions, old_logps, advs, rets, b_global, old_values) == ("a", "o", "adv", "r", 40, "vo")
        self.step += 1
        self.log.append("launch")

    def _sums(self):
        n = 4.0
        return torch.tensor([n, self.kls[self.step] * n, 1.0, 2.0, 6.0, 0.0, 1.0, 1.5], dtype=torch.float64)

    def ppo_diag(self, actions, old_logps, rets, out=None):
        assert (actions, old_logps, rets) == ("a", "o", "r")
        self.log.append("ppo_diag")
        if out is None:
            return self._sums()
        return out.copy_(self._sums())

    def diag_global(self, sums):
        self.log.append("diag_global")
        return sums.tolist()

    def allreduce_grads(self):
        self.log.append("allreduce_grads")

    def clip_adam_step(self):
        self.log.append("clip_adam_step")

    def _stats(self):
        return torch.tensor([0.5, 0.25, 0.125, 10.0 + self.step, 2.0, 1.0, 0.0, 0.0])

    def stats(self):
        self.log.append("stats")
        from ddrl4nav_amd import ops
        return ops.stats_dict(self._stats()[:6])

    def stats_async(self, row):
        self.log.append("stats_async")
        row.copy_(self._stats())


def _drive(monkeypatch, deferred=False, diag=False, target_kl=None, anneal=None, kls=(0.001, 0.002, 0.003), n_steps=3):
    log = []
    backend = Backend(log, kls)
    net = types.SimpleNamespace(update_backend=backend, diagnostics=diag, target_kl=target_kl, loss_options=(0.0, False), lr_anneal=anneal,
                                _base_rates=BASE_RATES, anneal_step=5, update_time=7, device=torch.device("cpu"),
                                _stats_rows=torch.zeros((n_steps, 8)), _diag_rows=torch.zeros((n_steps, 8), dtype=torch.float64),
                                _diag_dev=torch.zeros((n_steps, 8), dtype=torch.float64))     # sized: nothing is pinned or allocated here
    stream = types.SimpleNamespace(synchronize=lambda: log.append("synchronize"))
    monkeypatch.setattr(U.torch.cuda, "current_stream", lambda *a: stream)
    step = U.Step(backend.launch, "a", "o", "adv", "r", 40, "vo")
    items = []
    for item, update_time, last in U.run(net, (step for _ in range(n_steps)), n_steps, deferred):
        log.append("yield")
        items.append((item, update_time, last))
    return net, log, items


def _rates(u, anneal):
    return ("set_rates",) + tuple(M.annealed_rates(BASE_RATES, u, *anneal))


@pytest.mark.parametrize("anneal", [None, (8, 0.1, True)], ids=["fixed-rates", "annealed"])
@pytest.mark.parametrize("diag", [False, True], ids=["plain", "diagnostics"])
def test_run_eager_call_sequence(monkeypatch, diag, anneal):
    net, log, items = _drive(monkeypatch, diag=diag, anneal=anneal)
    want = []
    for i in range(3):
        want += ["loss_options"]
        want += [_rates(5 + i, anneal)] if anneal else []
        want += ["launch"]
        want += ["ppo_diag", "diag_global"] if diag else []
        want += ["allreduce_grads", "clip_adam_step", "stats", "yield"]
    assert log == want
    if not diag and not anneal:     # the same thing, spelled out
        assert log == ["loss_options", "launch", "allreduce_grads", "clip_adam_step", "stats", "yield"] * 3
    if diag and anneal:
        assert log[:9] == ["loss_options", ("set_rates", 5e-5 * 0.375, 1e-3 * 0.375, 2e-4 * 0.375, 0.2 * 0.375), "launch", "ppo_diag",
                           "diag_global", "allreduce_grads", "clip_adam_step", "stats", "yield"]
    assert [(set(it), ut, last) for it, ut, last in items] == [(LOSS_KEYS | (DIAG_KEYS if diag else set()), 8 + i, True) for i in range(3)]
    assert [it["PpoTotalLoss"] for it, _, _ in items] == [10.0, 11.0, 12.0]
    if diag:
        assert [it["ApproxKL"] for it, _, _ in items] == [0.001, 0.002, 0.003] and items[0][0]["RatioMax"] == 1.5
    assert (net.update_time, net.anneal_step) == (10, 8)


@pytest.mark.parametrize("anneal", [None, (8, 0.1, True)], ids=["fixed-rates", "annealed"])
@pytest.mark.parametrize("diag", [False, True], ids=["plain", "diagnostics"])
def test_run_deferred_call_sequence(monkeypatch, diag, anneal):
    net, log, items = _drive(monkeypatch, deferred=True, diag=diag, anneal=anneal)
    want = []
    for i in range(3):
        want += ["loss_options"]
        want += [_rates(5 + i, anneal)] if anneal else []      # counted at enqueue
        want += ["launch"]
        want += ["ppo_diag"] if diag else []
        want += ["allreduce_grads", "clip_adam_step", "stats_async"]
    want += ["synchronize"]                                       # the one synchronisation, before the first yield
    want += (["diag_global", "yield"] if diag else ["yield"]) * 3
    assert log == want
    if not diag and not anneal:
        assert log == ["loss_options", "launch", "allreduce_grads", "clip_adam_step", "stats_async"] * 3 + ["synchronize"] + ["yield"] * 3
    assert [(set(it), ut, last) for it, ut, last in items] == [(LOSS_KEYS | (DIAG_KEYS if diag else set()), 8 + i, True) for i in range(3)]
    assert [it["PpoTotalLoss"] for it, _, _ in items] == [10.0, 11.0, 12.0]      # every yield reads its own row
    if diag:
        assert [it["ApproxKL"] for it, _, _ in items] == [0.001, 0.002, 0.003]
    assert (net.update_time, net.anneal_step) == (10, 8)


def test_run_kl_stop_ends_the_call_before_the_step_is_applied(monkeypatch):
    """Step 2 sees ApproxKL = 0.02 > 1.5 x 0.01: no all-reduce, no Adam step, no counter, no yield for it, and step 3 is never launched."""
    net, log, items = _drive(monkeypatch, diag=True, target_kl=0.01, anneal=(8, 0.0, False), kls=(0.015, 0.02, 0.0))
    assert log == ["loss_options", _rates(5, (8, 0.0, False)), "launch", "ppo_diag", "diag_global", "allreduce_grads", "clip_adam_step", "stats",
                   "yield",
                   "loss_options", _rates(6, (8, 0.0, False)), "launch", "ppo_diag", "diag_global"]
    assert [(ut, last) for _, ut, last in items] == [(8, True)] and items[0][0]["ApproxKL"] == 0.015     # 1.5 x target itself does not stop
    assert (net.update_time, net.anneal_step) == (8, 6)
    # stopped at the first step: the counters stay where they were
    net, log, items = _drive(monkeypatch, diag=True, target_kl=0.01, kls=(0.5, 0.0, 0.0))
    assert log == ["loss_options", "launch", "ppo_diag", "diag_global"] and items == []
    assert (net.update_time, net.anneal_step) == (7, 5)


def test_run_refuses_a_kl_target_with_the_deferred_read_back(monkeypatch):
    with pytest.raises(ValueError, match="TARGET_KL needs the host after every step: not with DEFERRED_LOSS_READBACK"):
        _drive(monkeypatch, deferred=True, diag=True, target_kl=0.01)
    # nothing was launched
    log = []
    net = types.SimpleNamespace(diagnostics=True, target_kl=0.01, update_backend=Backend(log, ()))
    with pytest.raises(ValueError, match="TARGET_KL"):
        next(U.run(net, iter(()), 0, True))
    assert log == []
