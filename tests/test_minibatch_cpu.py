"""Host side of the PPO minibatch epochs (nn/minibatch.py; csrc/minibatch.hip's argument checks; the header).  No GPU."""
import os
import re
import types

import numpy as np
import pytest
import torch

import minibatch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ddrl_op_moments_ws_floats", "ddrl_op_moments", "ddrl_op_moments_affine", "ddrl_op_normalize", "ddrl_op_gather_minibatch")


@pytest.mark.parametrize("B,K", [(37, 3), (5, 5), (64, 1), (65, 4)])
def test_split_covers_the_batch_with_the_stated_sizes(B, K):
    from ddrl4nav_amd.nn.minibatch import split
    ranges = split(B, K)
    assert len(ranges) == K and ranges[0][0] == 0 and ranges[-1][1] == B
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert [hi - lo for lo, hi in ranges] == [B // K + (1 if j < B % K else 0) for j in range(K)]


def test_split_refuses_more_minibatches_than_samples():
    from ddrl4nav_amd.nn.minibatch import split
    with pytest.raises(ValueError, match="PPO_MINIBATCHES"):
        split(4, 5)


def test_epoch_order_is_a_private_reproducible_permutation():
    from ddrl4nav_amd.nn.minibatch import epoch_order
    torch.manual_seed(5)
    before = torch.get_rng_state()
    a = epoch_order(123, 2, 1, 37)
    assert a.dtype == torch.int32 and a.shape == (37,) and not a.is_cuda
    assert sorted(a.tolist()) == list(range(37))
    assert torch.equal(a, epoch_order(123, 2, 1, 37))
    assert not torch.equal(a, epoch_order(123, 2, 2, 37))        # another epoch
    assert not torch.equal(a, epoch_order(123, 3, 1, 37))        # another learn call
    assert not torch.equal(a, epoch_order(124, 2, 1, 37))        # another net
    assert not torch.equal(epoch_order(123, 1, 2, 37), a)        # the three integers are not summed
    assert torch.equal(torch.get_rng_state(), before)
    assert epoch_order(2 ** 63 - 1, 0, 0, 1).tolist() == [0]


def test_options_defaults_and_validation():
    from ddrl4nav_amd.nn import minibatch as M
    ns = types.SimpleNamespace
    assert M.minibatch_options(ns()) == (1, False, None, 1e-8) == M.DEFAULTS
    assert M.minibatch_options(ns(PPO_MINIBATCHES=4, PPO_SHUFFLE=True, NORMALIZE_ADVANTAGE="batch", ADV_NORM_EPS=1e-5)) \
        == (4, True, "batch", 1e-5)
    assert M.minibatch_options(ns(NORMALIZE_ADVANTAGE="minibatch"))[2] == "minibatch"
    assert M.minibatch_options(ns(NORMALIZE_ADVANTAGE=None))[2] is None
    for bad in (dict(PPO_MINIBATCHES=0), dict(PPO_MINIBATCHES=-2), dict(PPO_MINIBATCHES=1.5), dict(NORMALIZE_ADVANTAGE="epoch"),
                dict(NORMALIZE_ADVANTAGE=True), dict(ADV_NORM_EPS=-1.0)):
        with pytest.raises(ValueError):
            M.minibatch_options(ns(**bad))


def _configs(network_type="ppo", **options):
    from ddrl4nav_amd.config import BaseConfig, ConfigNN
    env = {"env_type": "gym", "env_name": "PongNoFrameskip-v4", "env_num": 8, "int_frame_stack": 4, "discrete_action": True,
           "discrete_actions": list(range(6)), "agent_num_per_env": 1, "batch_num_per_env": 8}
    cfg_nn = ConfigNN(env)
    cfg_nn.NETWORK_TYPE = network_type
    for k, v in options.items():
        setattr(cfg_nn, k, v)
    return {"config": BaseConfig(types.SimpleNamespace(task="minibatch", ip="127.0.0.1"), env), "config_nn": cfg_nn, "config_env": env}


def test_config_contract_does_not_carry_the_knobs():
    from ddrl4nav_amd.nn.minibatch import KNOBS
    cfg_nn = _configs()["config_nn"]
    assert not any(hasattr(cfg_nn, k) for k in KNOBS)


@pytest.mark.parametrize("opt", [dict(PPO_MINIBATCHES=2), dict(PPO_SHUFFLE=True), dict(NORMALIZE_ADVANTAGE="batch"), dict(ADV_NORM_EPS=1e-5)])
def test_generic_ppo_and_gail_refuse_the_knobs(opt):
    from ddrl4nav_amd.nn.generic import GenericPPO
    from ddrl4nav_amd.runner import create_net
    c = _configs(**opt)
    with pytest.raises(ValueError, match="Atari fast path alone"):
        GenericPPO(None, None, None, None, c["config"], c["config_nn"])
    with pytest.raises(ValueError, match="Atari fast path alone"):
        create_net(_configs("gail", SHARE_CNN_NET=True, **opt), max_batch=8)
    with pytest.raises(ValueError, match="Atari fast path alone"):      # the GAIL constructor itself, whatever built its parts
        from ddrl4nav_amd.nn.gail import GAIL
        GAIL(None, types.SimpleNamespace(config=c["config"], config_nn=c["config_nn"], device="cpu"), None)


def test_header_declares_what_the_binding_binds():
    from ddrl4nav_amd import _lib
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in NEW:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
    declared = set(re.findall(r"int32_t\s+(ddrl_\w+)\s*\(", text)) | {"ddrl_status_string"}
    assert set(_lib.SIGNATURES) <= declared
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in NEW)


def test_a_library_older_than_the_binding_gets_the_rebuild_hint():
    from ddrl4nav_amd import _lib

    class Old:      # exports what an ABI 3 build before this entry point exported
        def __init__(self, version, names):
            self.ddrl_abi_version = lambda: version
            for n in names:
                setattr(self, n, types.SimpleNamespace())

    names = [n for n in _lib.SIGNATURES if n not in ("ddrl_abi_version", "ddrl_op_normalize")]
    with pytest.raises(_lib.DdrlError, match=r"does not export ddrl_op_normalize.*rebuild with `make"):
        _lib._bind(Old(3, names))
    with pytest.raises(_lib.DdrlError, match=r"ABI version 2, this binding needs 3.*rebuild"):      # the version is asked first
        _lib._bind(Old(2, []))
    _lib._bind(Old(3, names + ["ddrl_op_normalize"]))


def test_argument_checks_come_before_hip():
    """Plain integers stand in for device addresses: every refusal below is decided before the first HIP call."""
    from ctypes import byref, c_int64
    from ddrl4nav_amd import _lib
    lib = _lib.load()
    INVALID = -1
    a, M = 0x100000, 0x100000
    f = c_int64()
    assert lib.ddrl_op_moments_ws_floats(0, byref(f)) == INVALID and lib.ddrl_op_moments_ws_floats(4, None) == INVALID
    assert lib.ddrl_op_moments_ws_floats(1, byref(f)) == 0 and f.value == 6
    assert lib.ddrl_op_moments_ws_floats(1 << 40, byref(f)) == 0 and 6 < f.value <= 1 << 16      # bounded: a cap on the workgroups

    mom = lambda x=a, n=64, s=a + M, ws=a + 2 * M: lib.ddrl_op_moments(x, n, s, 0, ws, None)
    for kw in (dict(x=None), dict(s=None), dict(ws=None), dict(n=0), dict(n=-3), dict(x=a + 2), dict(s=a + M + 4), dict(ws=a + 2 * M + 4),
               dict(s=a + 8), dict(ws=a + 16), dict(ws=a + M + 8)):
        assert mom(**kw) == INVALID, kw

    aff = lambda s=a, eps=1e-8, out=a + M: lib.ddrl_op_moments_affine(s, eps, out, None)
    for kw in (dict(s=None), dict(out=None), dict(s=a + 4), dict(out=a + M + 2), dict(eps=-1.0), dict(eps=float("nan")), dict(out=a + 16)):
        assert aff(**kw) == INVALID, kw

    norm = lambda x=a, n=64, af=a + M, out=a + 2 * M: lib.ddrl_op_normalize(x, n, af, out, None)
    for kw in (dict(x=None), dict(af=None), dict(out=None), dict(n=0), dict(x=a + 1), dict(af=a + M + 2), dict(out=a + 2 * M + 3),
               dict(out=a + 4), dict(out=a - 4), dict(af=a + 2 * M + 8)):      # shifted by one float: neither in place nor apart
        assert norm(**kw) == INVALID, kw

    cols = dict(ac=a + 2 * M, ol=a + 3 * M, ad=a + 4 * M, re=a + 5 * M, acd=a + 6 * M, old=a + 7 * M, add=a + 8 * M, red=a + 9 * M)

    def gather(fr=a + 16 * M, n_rows=9, rb=7056, idx=a + M, n=5, frd=a + 24 * M, af=a + 10 * M, **kw):
        c = dict(cols, **kw)
        return lib.ddrl_op_gather_minibatch(fr, n_rows, rb, idx, n, frd, c["ac"], c["ol"], c["ad"], c["re"], c["acd"], c["old"], c["add"],
                                            c["red"], af, None)

    for kw in (dict(fr=None), dict(idx=None), dict(frd=None), dict(n=0), dict(n_rows=0), dict(rb=0), dict(rb=7064), dict(rb=8),
               dict(fr=a + 16 * M + 8), dict(frd=a + 24 * M + 4), dict(idx=a + M + 2), dict(af=a + 10 * M + 1),
               dict(ac=None), dict(acd=None), dict(ol=None), dict(old=None), dict(ad=None), dict(add=None), dict(re=None), dict(red=None),
               dict(ac=a + 2 * M + 2), dict(red=a + 9 * M + 1),
               dict(ad=None, add=None),                                              # an affine without the advantage column
               dict(frd=a + 16 * M + 7056), dict(frd=a + 16 * M + 9 * 7056 - 16),     # frames_dst inside frames
               dict(fr=a + 24 * M + 4 * 7056),                                       # frames begin inside frames_dst
               dict(acd=a + 2 * M + 4), dict(old=a + 4 * M + 32), dict(red=a + 5 * M),  # a column's destination on a source column
               dict(add=a + M + 16), dict(add=a + 10 * M + 4),                        # ... on the indices, on the affine pair
               dict(acd=a + 16 * M + 64), dict(red=a + 24 * M + 5 * 7056 - 4),        # ... inside the frames, at the end of frames_dst
               dict(old=a + 6 * M + 16)):                                             # two destinations on one another
        assert gather(**kw) == INVALID, kw
    assert gather(ac=None, acd=None, ol=None, old=None, re=None, red=None, idx=None) == INVALID     # still checked with columns left out
