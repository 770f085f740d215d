"""Host side of the imitation pre-training (nn/imitation.py): batch order, label validation, configuration, header.  No GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Set:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return np.full((1, 2, 2), i, dtype=np.uint8), np.array([i % 6], dtype=np.float32)


@pytest.mark.parametrize("n,batch", [(70, 32), (5, 5), (7, 1), (64, 16)])
def test_index_iterator_follows_iter_and_the_global_generator(n, batch):
    from ddrl4nav_amd.data.mimic_exp import batches
    loader = batches(_Set(n), batch)
    for epoch_seed in (0, 123):
        torch.manual_seed(epoch_seed)
        by_value = [[int(x[0, 0, 0]) for x in X] for X, _ in loader] + [[int(x[0, 0, 0]) for x in X] for X, _ in loader]
        state_a = torch.get_rng_state()
        torch.manual_seed(epoch_seed)
        by_index = list(loader.iter_indices()) + list(loader.iter_indices())
        state_b = torch.get_rng_state()
        assert by_index == by_value
        assert torch.equal(state_a, state_b)
        assert sorted(i for c in by_index[:len(loader)] for i in c) == list(range(n))
        assert [len(c) for c in by_index[:len(loader)]] == [batch] * (n // batch) + ([n % batch] if n % batch else [])


def test_labels_are_validated_on_the_host():
    from ddrl4nav_amd.nn.imitation import validate_labels
    y = validate_labels([0.0, 5.0, 3.0], 6)
    assert y.dtype == np.float32 and y.tolist() == [0.0, 5.0, 3.0]
    assert validate_labels(np.array([[1.0], [0.0]], dtype=np.float32), 2).shape == (2,)
    for bad in ([0.0, 6.0], [-1.0], [2.5], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="label"):
            validate_labels(bad, 6)


def test_unsupported_forms_are_refused_before_anything_else():
    from ddrl4nav_amd.nn.imitation import check_supported
    with pytest.raises(NotImplementedError, match="regression"):
        check_supported(object(), "regression")
    with pytest.raises(ValueError):
        check_supported(object(), "ranking")
    with pytest.raises(NotImplementedError, match="Gaussian"):
        check_supported(types.SimpleNamespace(actor=types.SimpleNamespace(log_std=0)), "classification")
    with pytest.raises(NotImplementedError, match="atari only"):
        check_supported(types.SimpleNamespace(actor=types.SimpleNamespace()), "classification")


def test_config_carries_the_reference_defaults():
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    assert ConfigNN.IMITATION_LEARINING_RATE == 0.0001      # the reference's spelling (config_nn.py:75)
    assert ConfigNN.IMITATION_TRAINING_EPOCH == 10000
    assert ConfigNN.IMITATION_TRAINING_BATCH == 1024
    assert ConfigNN.IMITATION_SAVING_FREQUENCY == 100
    assert ConfigNN.IMITATION_TRAINING_TYPE == "classification"
    assert BaseConfig.IMITATION_MODEL_KEY == "MODEL_IMITATION"
    assert BaseConfig.MIMIC_START is False


def test_trainer_runs_imitation_before_the_first_publish(tmp_path):
    """BackwardTrainer with MIMIC_START: the reader is built from MIMIC_START_LOAD_PATH and net.imitation_learning runs once, with
    the reference's keyword arguments, before the checkpoint load and the first nn2redis (backward.py:117-129,170-179)."""
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    from ddrl4nav_amd.server.backward import BackwardTrainer
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
           "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg, cfg_nn = BaseConfig(types.SimpleNamespace(task="t", ip="127.0.0.1"), env), ConfigNN(env)
    d = tmp_path / "mimic"
    d.mkdir()
    np.save(str(d / "0_0_0.npy"), np.zeros((84, 84), np.uint8))
    (d / "dataset.txt").write_text(str(d) + "\n0_0_0.npy||3\n")
    cfg.MIMIC_START, cfg.MIMIC_START_LOAD_PATH = True, str(d) + "/"
    events = []

    class Net:
        device = "cpu"

        def imitation_learning(self, dataset, pipe, update_key, **kw):
            events.append(("imitation", len(dataset), pipe, update_key, kw))

        def nn2redis(self, pipe, update_key, key=None):
            events.append(("publish", key))

    pipe = object()
    BackwardTrainer(Net(), cfg, cfg_nn, pipe=pipe).start()
    assert [e[0] for e in events] == ["imitation", "publish"]
    _, n, p, tag, kw = events[0]
    assert n == 1 and p is pipe and tag == cfg.TASK_NAME + cfg.UPDATE_TAG_KEY
    assert kw == {"imitation_learning_rate": 0.0001, "imitation_training_batch": 1024, "imitation_training_epoch": 10000,
                  "imitation_saving_frequency": 100, "imitation_model_key": cfg.TASK_NAME + "MODEL_IMITATION",
                  "imitation_training_type": "classification"}
    events.clear()
    cfg.MIMIC_START = False
    BackwardTrainer(Net(), cfg, cfg_nn, pipe=pipe).start()
    assert [e[0] for e in events] == ["publish"]


def test_header_declares_the_new_entry_points():
    from ddrl4nav_amd import _lib
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in ("ddrl_op_heads_bc_loss", "ddrl_op_heads_bc_ws_floats", "ddrl_op_gather_rows_u8"):
        assert re.search(r"int32_t\s+%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3
    # each declaration names the reference lines it replaces
    block = text[text.index("Imitation pre-training"):]
    assert block.count("USTC_lab/nn/base.py") >= 2


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ctypes import byref, c_int64
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED = -1, -2
    a = 0x10000
    gather = lambda src=a, n_rows=8, rb=7056, idx=a + 0x100000, n=4, dst=a + 0x200000, ls=a + 0x300000, ld=a + 0x400000: \
        lib.ddrl_op_gather_rows_u8(src, n_rows, rb, idx, n, dst, ls, ld, None)
    assert gather(src=None) == INVALID and gather(idx=None) == INVALID and gather(dst=None) == INVALID
    assert gather(n=0) == INVALID and gather(n_rows=0) == INVALID and gather(rb=0) == INVALID and gather(rb=7064) == INVALID
    assert gather(src=a + 8) == INVALID and gather(dst=a + 0x200004) == INVALID and gather(idx=a + 0x100002) == INVALID
    assert gather(ld=None) == INVALID and gather(ls=None) == INVALID
    assert gather(dst=a + 7056) == INVALID and gather(dst=a + 8 * 7056 - 16) == INVALID     # dst inside src
    bc = lambda w=a, b=a, A=6, h=a, ld_h=512, n=4, lab=a, n_total=4, dh=a, ld_dh=512, dw=a, db=a, st=a, ws=a: \
        lib.ddrl_op_heads_bc_loss(w, b, A, h, ld_h, n, lab, n_total, dh, ld_dh, dw, db, st, ws, None)
    for k in ("w", "b", "h", "lab", "dh", "dw", "db", "st", "ws"):
        assert bc(**{k: None}) == INVALID, k
    assert bc(A=1) == UNSUPPORTED and bc(A=19) == UNSUPPORTED
    assert bc(n=0) == INVALID and bc(n_total=3) == INVALID
    assert bc(ld_h=508) == INVALID and bc(ld_h=514) == INVALID and bc(ld_dh=511) == INVALID
    assert bc(h=a + 4) == INVALID and bc(dh=a + 8) == INVALID
    f = c_int64()
    assert lib.ddrl_op_heads_bc_ws_floats(6, 0, byref(f)) == INVALID and lib.ddrl_op_heads_bc_ws_floats(1, 4, byref(f)) == UNSUPPORTED
    assert lib.ddrl_op_heads_bc_ws_floats(6, 1024, byref(f)) == 0 and f.value > 0
    small = f.value
    assert lib.ddrl_op_heads_bc_ws_floats(18, 1024, byref(f)) == 0 and f.value >= small + 18 * 1024
