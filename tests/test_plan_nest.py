"""CPU: what the nest of opt-in planner entry points must keep, whatever sits behind it -- the header's parameter counts against the
binding, the ladder of the ten nested exports (every level's argtypes behind ctx end with the level below's), and, on an engine whose
library is a recorder, for each of the twelve `HipEngine.*_plan` methods: the export it ends in, that export's arguments, the size
export and the workspace slot, the name in its messages, and the same call through `opt_in_plan`.

The actuator's prev / prefix must be device tensors (`is_cuda`): every case here runs with `actuator=None`, and the levels with an
actuator model are held by tests/test_gpu_actuator.py and the GPU files of the levels above it."""
import ctypes
import os
import re

import pytest
import torch

from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the nested exports, inner to outer, and what each puts in front of the level below (the header's order)
LADDER = [("scored", ["score", "update", "params"]), ("constrained", ["constraints"]), ("knot", ["knots", "phase"]),
          ("tracking", ["track", "targets", "T", "offset"]), ("actuated", ["actuator", "prev", "prefix", "advance"]),
          ("uncertain", ["uncertainty"]), ("valued", ["value"]), ("rewarded", ["reward"]), ("guided", ["policy"]), ("critic", ["critic"])]
STRUCTS = ("score", "constraints", "knots", "track", "actuator", "uncertainty", "value", "reward", "policy", "critic")
TAIL = 15      # obs, cp_obs, cp_act, init_mean, init_var, carry, carry_valid, m, n, seed, call, workspace, plan_out, best_return_out, stream


def head_of(level):
    """the names of cadm_<level>_plan's parameters between ctx and obs"""
    names = []
    for lv, front in LADDER:
        names = front + names
        if lv == level:
            return names
    return ["params"]      # cadm_icem_plan, cadm_mppi_plan


def declared():
    """export -> its parameter count in include/cadm_hip.h"""
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for name, params in re.findall(r"\b(cadm_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------- header and binding
def test_every_export_takes_as_many_arguments_as_the_header_declares():
    decl = declared()
    assert sorted(decl) == sorted(_lib.SIGNATURES)
    bad = {k: (n, len(_lib.SIGNATURES[k][1])) for k, n in decl.items() if n != len(_lib.SIGNATURES[k][1])}
    assert not bad, "header count != binding count: %r" % bad


def test_each_nested_export_ends_with_the_level_below():
    below = None
    for lv, front in LADDER:
        args = _lib.SIGNATURES["cadm_%s_plan" % lv][1]
        assert args[0] is ctypes.c_void_p and len(args) == 1 + len(head_of(lv)) + TAIL
        if below is not None:
            assert args[1 + len(front):] == below[1:], lv
        below = args
    # the two innermost take their own params struct in front of the same tail
    for lv in ("icem", "mppi"):
        assert _lib.SIGNATURES["cadm_%s_plan" % lv][1][2:] == _lib.SIGNATURES["cadm_scored_plan"][1][4:]


# ---------------------------------------------------------------------------------------------------------------------- the engine's ladder
M, N, H, A, K_TERMS, T = 2, 8, 3, 2, 2, 2


class Recorder:
    """stands where the library stands: every cadm_* call is kept and answers 0 (a size export: 4096)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("cadm_"):
            raise AttributeError(name)

        def export(*args):
            self.calls.append((name, args))
            return 4096 if name.endswith("_workspace_bytes") else 0
        return export


class Engine(HipEngine):
    stream = None

    def __init__(self):
        self.lib, self.device, self._ctx = Recorder(), torch.device("cpu"), None
        self.H, self.A, self.p, self.D, self.num_elites = H, A, 4, 5, 2
        self._loop_ws, self.whos = {}, []
        self._check = lambda rc, what="": self.whos.append(what)

    def ensure_rollout(self, noise=None, m=1, n_local=1):
        pass


def terms(level, given):
    """name -> value of every leading argument of `<level>_plan`; given: every term but the actuator model, under TERMINATE constraints
    and the MPPI update; else none, under the elite refit"""
    if level in ("icem", "mppi"):
        return dict(params=HipEngine.mppi_params(1.0, keep_elites=0) if level == "mppi" else HipEngine.icem_params())
    full = dict(score=HipEngine.score_params("mean_std", 0.5), constraints=HipEngine.constraint_params([dict(dim=0, lo=-1.0)], "terminate", 2.0),
                knots=HipEngine.knot_params(2), phase=torch.zeros(M, dtype=torch.int32), track=HipEngine.track_params([dict(dim=0), dict(dim=1)]),
                targets=torch.zeros(M, T, K_TERMS), offset=torch.zeros(M, dtype=torch.int32), actuator=None, prev=None, prefix=None,
                advance=True, uncertainty=HipEngine.uncertainty_params("epistemic", 0.1), value=HipEngine.value_params((4,)),
                reward=HipEngine.reward_params("next_obs", (4,)), policy=HipEngine.policy_params((4,), n_samples=3),
                critic=HipEngine.critic_params((4,)), params=HipEngine.mppi_params(1.0))
    if not given:
        full = dict({k: None for k in full}, advance=True, params=HipEngine.icem_params())
    return {k: full[k] for k in head_of(level) if k not in ("T", "update")}


INPUTS = (torch.zeros(M, 5), None, None, torch.zeros(M, H, A), torch.ones(M, H, A), N)      # obs, cp_obs, cp_act, init_mean, init_var, n


def inputs():
    return INPUTS


def run(eng, level, t, **kw):
    """one call of `<level>_plan`; returns (export name, its arguments)"""
    del eng.lib.calls[:], eng.whos[:]
    getattr(eng, level + "_plan")(*t.values(), *inputs(), seed=7, call=9, **kw)
    plans = [c for c in eng.lib.calls if c[0].endswith("_plan")]
    assert len(plans) == 1 and eng.whos == [plans[0][0]]
    return plans[0]


def answering(level, t):
    """the level whose export answers: from `actuated_plan` outwards a level whose own struct is None hands the call to the one below"""
    order = [lv for lv, _ in LADDER]
    i = order.index(level) if level in order else -1
    while i >= order.index("actuated") and t[LADDER[i][1][0]] is None:
        i -= 1
    return order[i] if i >= 0 else level


def expected_workspace(level, t):
    """(slot, size export, its integer arguments behind ctx) of the level that answers"""
    if level in ("icem", "mppi"):
        return (level == "mppi", False), "cadm_%s_workspace_bytes" % level, (M, N, 0)
    mppi = isinstance(t["params"], _lib.MppiParams)
    cons = t.get("constraints")
    term = cons is not None and cons.mode == _lib.CONSTRAIN_MODES["terminate"]
    unc, P = t.get("uncertainty") is not None, 0 if t.get("policy") is None else 3
    if level in ("uncertain", "valued", "rewarded", "guided", "critic"):
        tag = dict(uncertain="unc", valued="val", rewarded="rew", guided="pol", critic="crt")[level]
        flags = dict(unc=(term, False), val=(term, False, unc), rew=(term, False, unc), pol=(term, False, unc, P), crt=(term, False, unc, P))[tag]
        return (mppi, tag) + flags, "cadm_%s_workspace_bytes" % level, (M, N, 0, int(mppi)) + tuple(int(f) for f in flags)
    if t.get("track") is not None:
        return (mppi, "track", term), "cadm_tracking_workspace_bytes", (M, N, 0, int(mppi), int(term))
    if cons is not None:
        return (mppi, True), "cadm_constrained_workspace_bytes", (M, N, 0, int(mppi))
    return (mppi, False), "cadm_%s_workspace_bytes" % ("mppi" if mppi else "icem"), (M, N, 0)


def same(arg, want):
    """is the argument the export received the one the caller gave"""
    if want is None:
        return arg is None
    if isinstance(want, ctypes.Structure):
        return arg._obj is want
    if isinstance(want, torch.Tensor):
        return arg.value == want.data_ptr()
    return arg == want


LEVELS = ["icem", "mppi"] + [lv for lv, _ in LADDER]
CASES = [(lv, g) for lv in LEVELS for g in (False, True) if g or lv not in ("icem", "mppi")]


@pytest.mark.parametrize("level,given", CASES)
def test_every_level_ends_in_its_export_with_its_workspace(level, given):
    eng, t, decl = Engine(), terms(level, given), declared()
    name, args = run(eng, level, t)
    got = answering(level, t)
    assert name == "cadm_%s_plan" % got
    assert len(args) == decl[name] == len(_lib.SIGNATURES[name][1])
    # the head: ctx, then the structs and tensors in the declared order
    head = head_of(got)
    assert args[0] is None and len(args) == 1 + len(head) + TAIL
    mppi = isinstance(t["params"], _lib.MppiParams)
    for k, arg in zip(head, args[1:]):
        if k == "update":
            assert arg == int(mppi)
        elif k == "T":
            assert arg == (T if t["track"] is not None else 0)
        elif k == "params" and got not in ("icem", "mppi"):
            prm = arg._obj      # always a cadm_mppi_params: an icem_params result is wrapped
            assert isinstance(prm, _lib.MppiParams) and (prm is t["params"] if mppi else prm.icem.decay == t["params"].decay)
        elif k == "advance":
            assert arg == 1
        elif k in ("prev", "prefix"):
            assert arg is None
        else:
            assert same(arg, t[k]), k
    obs = args[1 + len(head)]
    assert args[-8:-4] == (M, N, 7, 9) and obs.value == INPUTS[0].data_ptr() and args[-1] is None and args[-2] is None
    # the workspace: one size call, its slot
    slot, size, ints = expected_workspace(got, {k: t.get(k) for k in head + ["params"]})
    sizes = [c for c in eng.lib.calls if c[0].endswith("_workspace_bytes")]
    assert sizes == [(size, (None,) + ints)]
    assert list(eng._loop_ws) == [slot] and eng._loop_ws[slot][0] == (M, N, 0)
    assert args[-4].value == eng._loop_ws[slot][1].data_ptr() and eng._loop_ws[slot][1].numel() == 4096
    # a second call finds the slot
    run(eng, level, t)
    assert [c[0] for c in eng.lib.calls if c[0].endswith("_workspace_bytes")] == []


@pytest.mark.parametrize("level,given", CASES)
def test_every_level_names_itself_in_its_refusals(level, given):
    eng, t = Engine(), terms(level, given)
    got = answering(level, t)
    if "phase" in t:
        bad = dict(t, phase=torch.zeros(M + 1, dtype=torch.int32))
        with pytest.raises(ValueError) as e:
            run(eng, level, bad)
        assert str(e.value).startswith("%s_plan: phase" % got)
    if got in ("icem", "mppi"):
        t["params"] = HipEngine.mppi_params(1.0, keep_elites=1) if got == "mppi" else HipEngine.icem_params(keep_elites=1)
    elif isinstance(t["params"], _lib.MppiParams):
        t["params"] = HipEngine.mppi_params(1.0, keep_elites=1)
    else:
        t["params"] = HipEngine.icem_params(keep_elites=1)
    with pytest.raises(ValueError) as e:
        run(eng, level, t)
    assert str(e.value).startswith("%s_plan: keep_elites=1 needs carry" % got)
    assert not [c for c in eng.lib.calls if c[0].endswith("_plan")]


def normal(args):
    return tuple(("ref", id(a._obj)) if hasattr(a, "_obj") else a.value if isinstance(a, ctypes.c_void_p) else a for a in args)


@pytest.mark.parametrize("level", [lv for lv in LEVELS if lv != "actuated"])
def test_opt_in_plan_reaches_the_same_call(level):
    """a `PlanOptions` whose outermost struct is `<level>`'s goes through `opt_in_plan` to the call `<level>_plan` makes itself
    (`actuated`: with no actuator model there is nothing for the options to hold, the GPU tests have it)"""
    eng, t = Engine(), terms(level, True)
    out = torch.empty(M, H, A)
    direct = run(eng, level, t, out=out)
    fields = dict(score="score_params", constraints="constraint_params", knots="knot_params", track="track_params",
                  uncertainty="uncertainty_params", value="value_params", reward="reward_params", policy="policy_params",
                  critic="critic_params", params="params")
    opt = PlanOptions.from_kwargs(use_cem=True, cem_add_mean=True)._replace(update="mppi" if level != "icem" else "cem",
                                                         **{fields[k]: v for k, v in t.items() if k in fields})
    del eng.lib.calls[:], eng.whos[:]
    eng.opt_in_plan(opt, *inputs(), phase=t.get("phase"), targets=t.get("targets"), target_offset=t.get("offset"), seed=7, call=9, out=out)
    plans = [c for c in eng.lib.calls if c[0].endswith("_plan")]
    assert len(plans) == 1 and plans[0][0] == direct[0] == "cadm_%s_plan" % level
    assert normal(plans[0][1]) == normal(direct[1])
    assert eng.whos == [direct[0]]
