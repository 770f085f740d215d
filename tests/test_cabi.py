"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports every symbol
that include/ddrl.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

import pytest

from ddrl4nav_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", src)))


def test_library_built():
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"


def test_every_declared_symbol_is_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), "symbol %s declared in include/ddrl.h is not exported" % n
    # and the binding table covers the header
    assert set(names) == set(_lib.SIGNATURES.keys())


def test_load_and_host_only_calls():
    lib = _lib.load()
    assert lib.ddrl_abi_version() == _lib.ABI_VERSION == 3
    assert lib.ddrl_status_string(-3) == b"workspace too small"
    cfg = _lib.default_config(max_batch=64)
    assert (cfg.n_actions, cfg.in_channels) == (6, 4)
    assert abs(cfg.actor_lr - 5e-5) < 1e-10 and abs(cfg.critic_lr - 1e-3) < 1e-9
    n, na = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.ddrl_param_count(ctypes.byref(cfg), ctypes.byref(n), ctypes.byref(na)))
    assert n.value == 3371847 and na.value == 1687206
    wb = ctypes.c_int64()
    _lib.check(lib.ddrl_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)))
    assert wb.value > 64 * 86528 * 4


def test_unsupported_configs_fail_loudly():
    lib = _lib.load()
    wb = ctypes.c_int64()
    for bad in (dict(n_actions=19), dict(in_channels=5), dict(in_channels=0)):
        cfg = _lib.default_config(max_batch=64, **bad)
        assert lib.ddrl_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)) == -2
    cfg = _lib.default_config(max_batch=64, share_cnn_net=2)
    assert lib.ddrl_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)) == -1
    # the kernels address the conv1 activations with 32-bit byte offsets: 83,886 samples is the last size
    cfg = _lib.default_config(max_batch=83886)
    assert lib.ddrl_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)) == 0
    cfg = _lib.default_config(max_batch=83887)
    assert lib.ddrl_workspace_bytes(ctypes.byref(cfg), ctypes.byref(wb)) == -2
    with pytest.raises(_lib.DdrlError):
        _lib.check(-2)


def test_shared_prenet_layout():
    """SHARE_CNN_NET=True: prenet + two linear heads, one Adam group (reference ppo.py:39)."""
    lib = _lib.load()
    cfg = _lib.default_config(max_batch=64, share_cnn_net=1)
    assert abs(cfg.learning_rate - 2e-4) < 1e-9 and cfg.smooth_l1_loss == 0
    n, na = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(lib.ddrl_param_count(ctypes.byref(cfg), ctypes.byref(n), ctypes.byref(na)))
    assert n.value == 1684128 + 6 * 512 + 6 + 512 + 1 and na.value == n.value


def test_no_gpu_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ddrl4nav_amd.engine import HotPath
    with pytest.raises(_lib.DdrlError):
        HotPath(max_batch=8)


def test_operator_abi_host_side_queries():
    """Shape / size queries of the operator-level ABI run on the host (no GPU needed)."""
    from ctypes import byref, c_int32, c_int64
    lib = _lib.load()
    d = _lib.ConvDesc(4, 3, 48, 48, 64, 7, 7, 1, 1, 1, 0, 0)          # NavPreNet1D.conv1 (nav_encoder.py:96)
    oh, ow, f = c_int32(), c_int32(), c_int64()
    _lib.check(lib.ddrl_op_conv_out_shape(byref(d), byref(oh), byref(ow)))
    assert (oh.value, ow.value) == (44, 44)
    d1 = _lib.ConvDesc(4, 1, 1, 960, 32, 1, 5, 2, 0, 0, 0, 0)          # conv1d1 as a 1 x 960 image
    _lib.check(lib.ddrl_op_conv_out_shape(byref(d1), byref(oh), byref(ow)))
    assert (oh.value, ow.value) == (1, 478)
    _lib.check(lib.ddrl_op_conv_pack_floats(byref(d), byref(f)))
    assert f.value >= 64 * 3 * 49
    _lib.check(lib.ddrl_op_conv_ws_floats(byref(d), byref(f)))
    assert f.value >= 64 * 3 * 49 + 64
    bad = _lib.ConvDesc(4, 3, 48, 48, 64, 7, 7, 3, 1, 1, 0, 0)         # stride 3 is not supported
    assert lib.ddrl_op_conv_out_shape(byref(bad), byref(oh), byref(ow)) == -1
    a, b = c_int64(), c_int64()
    _lib.check(lib.ddrl_op_linear_pack_floats(773, 512, byref(a), byref(b)))
    # the f32 layouts, followed by the 16-bit plane layouts of csrc/plin.hip (K >= 128, N >= 64): [column tile 128][k-groups of 16,
    # an even number][2 planes][128][16] halves + a 64-float header
    assert a.value == 800 * 512 + (4 * 50 * 4096 // 2 + 64) and b.value == 512 * 776 + (7 * 32 * 4096 // 2 + 64)
    _lib.check(lib.ddrl_op_linear_pack_floats(37, 12, byref(a), byref(b)))       # a small layer keeps the f32 layouts only
    assert a.value == 64 * 12 and b.value == 12 * 40
    assert lib.ddrl_op_linear_pack_floats(16, 6, byref(a), byref(b)) == -1  # N must be a multiple of 4
    _lib.check(lib.ddrl_op_linear_ws_floats(1024, 7616, 256, byref(f)))
    assert f.value >= 7616 * 256 + 256
    h = _lib.HeadsDesc(1, 2, 0, 0, 100, 1124, 0, 1126, 1638, 1639)
    _lib.check(lib.ddrl_op_heads_ws_floats(byref(h), 256, byref(f)))
    assert f.value > 256 * 3
    h.n_actions = 9                                                      # Gaussian heads: at most 8 action dims
    assert lib.ddrl_op_heads_ws_floats(byref(h), 256, byref(f)) == -1
    _lib.check(lib.ddrl_op_clip_adam_ws_bytes(byref(f)))
    assert f.value == 1024 * 8


# (cin, h, w, cout, kh, kw, stride, pad) -> (pack_floats, ws_floats, scratch_floats, has_forward_pool, pooled_uses_scales) at n = 1, 5, 300, 4096.
# Recorded from the library before the conv routing moved into conv_route (csrc/api_ops.hip): what callers size their buffers by.
CONV_HOST_ANSWERS = {
    (3, 48, 48, 64, 7, 7, 1, (1, 1)): [(233920, 151552, 0, 1, 0), (233920, 719872, 0, 1, 0), (233920, 7274496, 0, 1, 0), (233920, 7274496, 0, 1, 0)],
    (64, 22, 22, 128, 5, 5, 1, (1, 1)): [(829376, 819778, 1, 1, 1), (829376, 3278922, 5, 1, 1), (829376, 38527128, 300, 1, 1), (829376, 39354432, 4096, 1, 1)],
    (128, 10, 10, 256, 3, 3, 1, (1, 1)): [(1186816, 295234, 1, 1, 1), (1186816, 1180746, 5, 1, 1), (1186816, 11512216, 300, 1, 1), (1186816, 28344384, 4096, 1, 1)],
    (1, 48, 48, 64, 3, 3, 1, (1, 1)): [(44544, 11520, 0, 1, 0), (44544, 57600, 0, 1, 0), (44544, 491520, 0, 1, 0), (44544, 491520, 0, 1, 0)],
    (4, 48, 48, 64, 3, 3, 1, (1, 1)): [(46656, 42624, 0, 1, 0), (46656, 213120, 0, 1, 0), (46656, 1818624, 0, 1, 0), (46656, 1818624, 0, 1, 0)],
    (64, 24, 24, 128, 3, 3, 1, (1, 1)): [(299072, 369346, 1, 1, 1), (299072, 1698762, 5, 1, 1), (299072, 16618264, 300, 1, 1), (299072, 28368960, 4096, 1, 1)],
    (128, 12, 12, 256, 3, 3, 1, (1, 1)): [(1186880, 590402, 1, 1, 1), (1186880, 1771082, 5, 1, 1), (1186880, 11512216, 300, 1, 1), (1186880, 28344384, 4096, 1, 1)],
    (64, 9, 9, 64, 3, 3, 1, (0, 0)): [(149952, 36994, 1, 0, 0), (149952, 73930, 5, 0, 0), (149952, 4247384, 300, 0, 0), (149952, 9461824, 4096, 0, 0)],
    (1, 1, 960, 32, 1, 5, 2, (0, 0)): [(12544, 192, 0, 0, 0), (12544, 960, 0, 0, 0), (12544, 57600, 0, 0, 0), (12544, 98304, 0, 0, 0)],
    (32, 1, 478, 32, 1, 3, 2, (0, 0)): [(19072, 6208, 0, 0, 0), (19072, 31040, 0, 0, 0), (19072, 1732032, 0, 0, 0), (19072, 2383872, 0, 0, 0)],
    (32, 1, 101, 32, 1, 3, 2, (0, 0)): [(18880, 3104, 0, 0, 0), (18880, 6208, 0, 0, 0), (18880, 366272, 0, 0, 0), (18880, 2383872, 0, 0, 0)],
    (5, 9, 11, 70, 3, 2, 1, (2, 0)): [(32832, 2170, 0, 0, 0), (32832, 10850, 0, 0, 0), (32832, 559860, 0, 0, 0), (32832, 833280, 0, 0, 0)],
    (4, 20, 20, 32, 4, 4, 2, (0, 0)): [(38144, 2080, 0, 0, 0), (38144, 8320, 0, 0, 0), (38144, 395200, 0, 0, 0), (38144, 1597440, 0, 0, 0)],
    (3, 16, 16, 8, 8, 8, 4, (0, 0)): [(46528, 1544, 0, 0, 0), (46528, 1544, 0, 0, 0), (46528, 33968, 0, 0, 0), (46528, 444672, 0, 0, 0)],
}
CONV_HOST_ANSWERS_NS = (1, 5, 300, 4096)


def test_conv_host_side_answers_are_pinned():
    """Sizes and capability flags of every conv geometry of tests/test_ops_gpu.py (all kernel families + layers that have none), and of
    NavPreNet1D.conv2 read from a strided view (the answers depend on the geometry, not on the view).  A size query that disagrees
    with a launcher is a device buffer overrun, so the exact values are pinned."""
    from ctypes import byref, c_int64
    from test_ops_gpu import CONVS
    lib = _lib.load()

    def answers(d):
        a, b, c = c_int64(), c_int64(), c_int64()
        _lib.check(lib.ddrl_op_conv_pack_floats(byref(d), byref(a)))
        _lib.check(lib.ddrl_op_conv_ws_floats(byref(d), byref(b)))
        _lib.check(lib.ddrl_op_conv_scratch_floats(byref(d), byref(c)))
        return (a.value, b.value, c.value, lib.ddrl_op_conv_has_forward_pool(byref(d)), lib.ddrl_op_conv_pooled_uses_scales(byref(d)))

    assert len(CONVS) == 16
    for (_, cin, h, w, cout, kh, kw, s, pad) in CONVS:
        want = CONV_HOST_ANSWERS[(cin, h, w, cout, kh, kw, s, pad)]
        for n, row in zip(CONV_HOST_ANSWERS_NS, want):
            assert answers(_lib.ConvDesc(n, cin, h, w, cout, kh, kw, s, pad[0], pad[1], 0, 0)) == row, (cin, h, w, cout, kh, kw, s, pad, n)
    dense = 64 * 22 * 22
    for extra in (1, 4):   # dense + 1 rules out the plane kernels' 16-byte loads for a call; dense + 4 does not
        assert answers(_lib.ConvDesc(3, 64, 22, 22, 128, 5, 5, 1, 1, 1, dense + extra, 0)) == (829376, 2049350, 3, 1, 1)


# (share_cnn_net, in_channels, n_actions) -> (n_params, n_actor, [workspace bytes at each max_batch of ATARI_HOST_ANSWERS_MBS]).  Recorded from the
# library of the commit before the workspace sizes got their names in csrc/common.h: what callers allocate by.  The batches lie on
# both sides of every cap of choose_splits (pairs against 256 / 512 splits, 32-sample tiles against 5 / 10) and of the 1024 cap of the
# acting path's partial sums, and end at the last supported size.
ATARI_HOST_ANSWERS = {
    (0, 1, 2): (3357507, 1679010, [55256832, 55608064, 80756480, 297606400, 477529344, 477882112, 1557067008, 23147820288, 29596230912]),
    (0, 1, 6): (3359559, 1681062, [57353984, 57705216, 82854144, 299711744, 479642880, 479995648, 1559229696, 23150966016, 29599670272]),
    (0, 1, 18): (3365715, 1687218, [63645440, 63996672, 89147392, 306027776, 485983488, 486336256, 1565717760, 23160403200, 29609988096]),
    (0, 4, 2): (3369795, 1685154, [55256832, 55608064, 80756480, 297606400, 477529344, 477882112, 1557067008, 23147820288, 29596230912]),
    (0, 4, 6): (3371847, 1687206, [57353984, 57705216, 82854144, 299711744, 479642880, 479995648, 1559229696, 23150966016, 29599670272]),
    (0, 4, 18): (3378003, 1693362, [63645440, 63996672, 89147392, 306027776, 485983488, 486336256, 1565717760, 23160403200, 29609988096]),
    (1, 1, 2): (1679523, 1679523, [55256832, 55608064, 80756480, 350469376, 553157888, 553510656, 1632695552, 23223448832, 29671859456]),
    (1, 1, 6): (1681575, 1681575, [57353984, 57705216, 82854144, 352574720, 555271424, 555624192, 1634858240, 23226594560, 29675298816]),
    (1, 1, 18): (1687731, 1687731, [63645440, 63996672, 89147392, 358890752, 561612032, 561964800, 1641346304, 23236031744, 29685616640]),
    (1, 4, 2): (1685667, 1685667, [55256832, 55608064, 80756480, 350469376, 553157888, 553510656, 1632695552, 23223448832, 29671859456]),
    (1, 4, 6): (1687719, 1687719, [57353984, 57705216, 82854144, 352574720, 555271424, 555624192, 1634858240, 23226594560, 29675298816]),
    (1, 4, 18): (1693875, 1693875, [63645440, 63996672, 89147392, 358890752, 561612032, 561964800, 1641346304, 23236031744, 29685616640]),
}
ATARI_HOST_ANSWERS_MBS = (1, 2, 37, 512, 1024, 1025, 4096, 65536, 83886)


def test_atari_host_side_answers_are_pinned():
    """ddrl_workspace_bytes and ddrl_param_count of the Atari context over both prenet arrangements, 1 and 4 stacked frames and 2 / 6 / 18
    actions.  A size query that disagrees with carve() or with a launcher's stride is a device buffer overrun, so the exact values
    are pinned; a context serves every batch up to its max_batch, so the byte count never decreases with it."""
    from ctypes import byref, c_int64
    lib = _lib.load()

    def answers(shared, C, A, mb):
        cfg = _lib.default_config(max_batch=mb, share_cnn_net=shared, in_channels=C, n_actions=A)
        n, na, wb = c_int64(), c_int64(), c_int64()
        _lib.check(lib.ddrl_param_count(byref(cfg), byref(n), byref(na)))
        _lib.check(lib.ddrl_workspace_bytes(byref(cfg), byref(wb)))
        return wb.value, n.value, na.value

    assert len(ATARI_HOST_ANSWERS) == 12
    for (shared, C, A), (n_params, n_actor, per_mb) in ATARI_HOST_ANSWERS.items():
        for mb, nbytes in zip(ATARI_HOST_ANSWERS_MBS, per_mb):
            assert answers(shared, C, A, mb) == (nbytes, n_params, n_actor), (shared, C, A, mb)
    for shared, C, A in ((0, 4, 6), (1, 1, 18)):
        sizes = [answers(shared, C, A, mb)[0] for mb in range(1, 2049)]
        assert all(lo <= hi for lo, hi in zip(sizes, sizes[1:])), (shared, C, A)


# (K, N) -> (wt_floats, wn_floats, [(ws_floats, uses_planes) at n = 1, 127, 128, 300, 4096, 65536]).  Recorded from the library before the
# dense routing moved into linear_route (csrc/api_ops.hip): what callers size their buffers by.
LINEAR_HOST_ANSWERS = {
    (7616, 256): (3899456, 3915840, [(1950082, 0), (3900286, 0), (3900288, 1), (9750488, 1), (17557888, 1), (25329792, 1)]),
    (6400, 512): (6553664, 6553664, [(3277442, 0), (6555006, 0), (6555008, 1), (9832664, 1), (19672192, 1), (42139776, 1)]),
    (9216, 512): (9437248, 9437248, [(4719234, 0), (9438590, 0), (9438592, 1), (14158040, 1), (18884736, 1), (42139776, 1)]),
    (773, 512): (819264, 856128, [(396418, 0), (792958, 0), (792960, 1), (1982168, 1), (12689536, 1), (42139776, 1)]),
    (512, 512): (524352, 524352, [(262786, 0), (525694, 0), (525696, 1), (1314008, 1), (8413312, 1), (42139776, 1)]),
    (1536, 256): (786496, 786496, [(393602, 0), (787326, 0), (787328, 1), (1968088, 1), (12599424, 1), (25329792, 1)]),
    (1024, 192): (458816, 393280, [(196930, 0), (393982, 0), (393984, 1), (984728, 1), (6305920, 1), (19030144, 1)]),
    (516, 64): (104512, 74048, [(33218, 0), (66558, 0), (66560, 1), (166168, 1), (2125952, 1), (8519808, 1)]),
    (128, 64): (24640, 16448, [(8386, 0), (16894, 0), (16896, 1), (42008, 1), (536704, 1), (4358272, 1)]),
    (127, 64): (8192, 8192, [(8322, 0), (16766, 0), (16768, 0), (41688, 0), (532608, 0), (4325504, 0)]),
    (128, 60): (7680, 7680, [(7870, 0), (15862, 0), (15864, 0), (39428, 0), (503680, 0), (4094080, 0)]),
    (4, 128): (4096, 512, [(770, 0), (16638, 0), (16768, 0), (39128, 0), (532608, 0), (8519808, 0)]),
    (37, 12): (768, 480, [(586, 0), (1906, 0), (1920, 0), (4328, 0), (57472, 0), (917632, 0)]),
}
LINEAR_HOST_ANSWERS_NS = (1, 127, 128, 300, 4096, 65536)


def test_linear_host_side_answers_are_pinned():
    """Sizes and the family flag of the dense layers of the nav / MLP / GAIL nets and of the layers at the edges of the plane kernels'
    domain (K >= 128, N >= 64, n >= 128).  A size query that disagrees with a launcher is a device buffer overrun, so the exact values
    are pinned; a workspace sized for n rows serves every launch of fewer rows, so ws_floats never decreases with n."""
    from ctypes import byref, c_int64
    lib = _lib.load()

    def ws_floats(n, K, N):
        f = c_int64()
        _lib.check(lib.ddrl_op_linear_ws_floats(n, K, N, byref(f)))
        return f.value

    assert len(LINEAR_HOST_ANSWERS) == 13
    for (K, N), (wt, wn, per_n) in LINEAR_HOST_ANSWERS.items():
        a, b = c_int64(), c_int64()
        _lib.check(lib.ddrl_op_linear_pack_floats(K, N, byref(a), byref(b)))
        assert (a.value, b.value) == (wt, wn), (K, N)
        for n, row in zip(LINEAR_HOST_ANSWERS_NS, per_n):
            assert (ws_floats(n, K, N), lib.ddrl_op_linear_uses_planes(n, K, N)) == row, (K, N, n)
        for ns in (range(1, 1025), range(1024, 65536 + 1, 1024)):
            sizes = [ws_floats(n, K, N) for n in ns]
            assert all(lo <= hi for lo, hi in zip(sizes, sizes[1:])), (K, N)


def test_clean_build_stays_within_its_time_budget(tmp_path):
    """Every HIP source compiles from scratch in well under five minutes (hipcc cross-compiles gfx950 without a GPU): the driver's
    build() check and a fresh checkout depend on it.  (Round 5: a scheduling experiment -- one sched_group_barrier-pinned region over
    a whole stage of pconv.hip's weight gradient -- compiled correctly but took hipcc 11 minutes for that one file.)"""
    import shutil
    import subprocess
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dst = tmp_path / "ddrl4nav_amd" / "csrc"
    dst.parent.mkdir(parents=True)
    shutil.copytree(os.path.join(root, "ddrl4nav_amd", "csrc"), dst, ignore=shutil.ignore_patterns("*.o", "*.so", ".pytest_cache", "_scratch*"))
    (tmp_path / "include").mkdir()
    shutil.copy(os.path.join(root, "include", "ddrl.h"), tmp_path / "include" / "ddrl.h")
    t0 = time.time()
    r = subprocess.run(["make", "-C", str(dst), "-j", str(min(8, os.cpu_count() or 1))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (dst / "libddrl_hip.so").exists()
    print("clean build: %.0f s" % (time.time() - t0))


def test_removed_environment_switches_are_reported_once():
    """a launch script that still sets a switch removed in round 5 (DDRL_ALLREDUCE_OVERLAP, DDRL_ENC_STREAMS, ...) must not be
    ignored silently: loading the library warns once per variable and names the replacement (ddrl4nav_amd/_lib.py:REMOVED_SWITCHES)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import warnings; warnings.simplefilter('always'); from ddrl4nav_amd import _lib; _lib.load(); _lib.load()"
    env = dict(os.environ, DDRL_ALLREDUCE_OVERLAP="1", DDRL_ENC_STREAMS="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.count("DDRL_ALLREDUCE_OVERLAP is set but was removed") == 1 and "DDRL_ALLREDUCE=overlap" in r.stderr
    assert r.stderr.count("DDRL_ENC_STREAMS is set but was removed") == 1 and "encoder_streams" in r.stderr
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env={k: v for k, v in os.environ.items() if not k.startswith("DDRL_")},
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "was removed" not in r.stderr
