"""What the arena's host-side tests share (tests/test_nav_env_cpu.py, test_fleet_env_cpu.py, test_nav_status_cpu.py, test_truncation_cpu.py,
test_ped_avoid_cpu.py; test_nav_expert_cpu.py for the header): the header against the binding table, and one description of the two
reset and seven step entries of the C ABI -- argument order, fake addresses, byte sizes -- from which the keyword closures, the overlap
cases and the refusals every step entry shares are made.  Plain integers stand in for device addresses: every refusal is decided
before the first HIP call.  A new arena entry is described here; its test appends what is its own."""
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def header_declares(names, counts):
    """Every name is declared in include/ddrl.h with as many arguments as the binding table gives it (`counts`, spelled out by the
    caller) and exported by the loaded library; the ABI version is 3 in all three places.  -> (the header's text, the library)."""
    from ddrl4nav_amd import _lib
    text = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in names:
        m = re.search(r"int32_t\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        args = 0 if m.group(1).strip() == "void" else m.group(1).count(",") + 1
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == args, name
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == list(counts)
    assert re.search(r"#define\s+DDRL_ABI_VERSION\s+3\b", text) and _lib.ABI_VERSION == 3
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in names) and lib.ddrl_abi_version() == 3
    return text, lib


# ---- the arena entries ------------------------------------------------------------------------------------------------------------------
# The fabricated call: n = 8 envs, or 4 worlds x 2 robots = 8 rows.  st: the state; la, ve, im: the observation; rw, dn, info: reward,
# done and info word; act: the actions; fl, fv, fi: the terminal observation; e0: env0 / world0; ms: max_steps; pm: ped_model.
A, M = 0x10000000, 0x1000000
POINTERS = ("st", "la", "ve", "im", "rw", "dn", "info", "act", "fl", "fv", "fi", "mask")
BASE = {k: A + i * M for i, k in enumerate(POINTERS)}
ALIGN = dict(st=16, la=16, ve=4, im=16, rw=4, dn=1, info=4, act=4, fl=16, fv=4, fi=16, mask=1)
DEFAULTS = dict(BASE, mask=None, n=8, nw=4, nr=2, e0=0, seed=1, nobs=10, nped=5, ms=500, pm=1)
_NAV, _FLEET, _OBS, _FINAL = ("st", "n"), ("st", "nw", "nr"), ("la", "ve", "im"), ("fl", "fv", "fi")
_ARENA = ("e0", "seed", "nobs", "nped")
ENTRIES = {}                                                            # name: its arguments in order, without the stream
for _env, _lead in (("nav", _NAV), ("fleet", _FLEET)):
    _step = _lead + _ARENA + ("ms", "act") + _OBS + ("rw", "dn")
    ENTRIES["ddrl_op_%s_env_reset" % _env] = _lead + _ARENA + ("mask",) + _OBS
    ENTRIES["ddrl_op_%s_env_step" % _env] = _step + (("info",) if _env == "fleet" else ())
    ENTRIES["ddrl_op_%s_env_step_final" % _env] = _step + ("info",) + _FINAL
    ENTRIES["ddrl_op_%s_env_step_model" % _env] = _lead + _ARENA + ("ms", "pm", "act") + _OBS + ("rw", "dn", "info") + _FINAL
ENTRIES["ddrl_op_nav_env_step_info"] = ENTRIES["ddrl_op_nav_env_step"] + ("info",)
OPTIONAL = {"ddrl_op_fleet_env_step": ("info",), "ddrl_op_nav_env_step_model": ("info",) + _FINAL,
            "ddrl_op_fleet_env_step_model": ("info",) + _FINAL}          # pointers that may be null


def sizes(name):
    """Bytes behind each pointer of the fabricated call."""
    fleet = "fleet" in name
    return dict(st=4 * 384 if fleet else 8 * 256, la=8 * 3840, ve=8 * 20, im=8 * 27648, rw=32, dn=8, info=32, act=64, fl=8 * 3840, fv=8 * 20,
                fi=8 * 27648, mask=4 if fleet else 8)


def caller(lib, name):
    """call(**changes) -> the entry's return value for the fabricated call with `changes` (by argument name) applied."""
    def call(**changes):
        assert set(changes) <= set(ENTRIES[name]), (name, changes)
        values = dict(DEFAULTS, **changes)
        return getattr(lib, name)(*[values[a] for a in ENTRIES[name]], None)
    return call


def outputs(name):
    return tuple(a for a in ENTRIES[name] if a in POINTERS and a not in ("act", "mask"))


def overlaps(names, size):
    """For each ordered pair (p, q) of `names`: q moved onto p's first byte, and onto p's last aligned unit."""
    out = []
    for p, q in itertools.permutations(names, 2):
        out.append({q: BASE[p]})
        if size[p] > ALIGN[q] and size[p] % ALIGN[q] == 0:
            out.append({q: BASE[p] + size[p] - ALIGN[q]})
    return out


def common_refusals(name, without=()):
    """What every step entry refuses: a null where a pointer is required, populations, max_steps and the index range, every misaligned
    base, every output and the actions on either end of every other of them.  without: optional outputs
    the call is to leave null, so that nothing can lie on them."""
    outs, size = tuple(p for p in outputs(name) if p not in without), sizes(name)
    bad = [{p: None} for p in outs + ("act",) if p not in OPTIONAL.get(name, ())]
    bad += [dict(nobs=-1), dict(nobs=11), dict(nped=-1), dict(nped=-2), dict(nped=6), dict(ms=0), dict(ms=-3), dict(ms=-5), dict(e0=-1),
            dict(e0=-3), dict(e0=2 ** 32), dict(e0=2 ** 32 - 3)]
    bad += [{p: BASE[p] + off} for p in outs + ("act",) for off in (1, 2, 4, 8, 12) if off % ALIGN[p]]
    bad += overlaps(outs + ("act",), size)
    return bad + [{"act": BASE[p] - size["act"] + 4} for p in outs]     # and the actions' last word on every output's first bytes


def refused(call, cases, **always):
    for kw in cases:
        assert call(**dict(always, **kw)) == INVALID, (always, kw)
