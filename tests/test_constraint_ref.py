"""CPU: the numpy restatement of the state constraints (tests/constraint_ref.py) against a brute-force loop, every validation rule of
`PlanOptions.from_kwargs` and `HipEngine.constraint_params`, and the `cadm_constraint_params` struct as the header lays it out."""
import ctypes
import os
import re

import numpy as np
import pytest

import constraint_ref as cref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.env_spec import EnvDecl
from cadm_amd.planner import PlanOptions
from forecast_ref import step_rewards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_env():
    return EnvDecl(5, 2, preproc=["id"] * 5, postproc=["add"] * 5,
                   reward=[dict(kind="linear", dim=0), dict(kind="square", dim=3, w=-0.5, when="next_obs"),
                           dict(kind="inside", dim=1, w=1.0, lo=-0.5, hi=0.5, when="next_obs")], ctrl_cost=0.01, bonus=1.0)


def problem(seed, H=4, m=2, n=3, p=4, D=5, A=2):
    rng = np.random.default_rng(seed)
    traj = rng.standard_normal((H, m, n, p, D)).astype(np.float32)
    return (traj, rng.standard_normal((m, D)).astype(np.float32), rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32),
            rng.uniform(-20, 20, (m, n, p)).astype(np.float32))


CONS = [dict(dim=1, lo=-1.0, hi=1.2), dict(dim=4, lo=-1.5)]


def test_reference_equals_the_brute_force_loop():
    env = small_env()
    traj, obs, acts, rows = problem(1)
    traj[2, 0, 1, 3, 1] = np.float32(1.2)           # exactly hi: violates
    traj[0, 1, 2, 0, 4] = np.float32(-1.5)          # exactly lo: violates
    traj[1, 1, 0, 2, 1] = np.nan                    # NaN in a constrained dim
    traj[3, 0, 0, 1, 4] = np.inf                    # +inf under a one-sided bound
    traj[2, 1, 1, 1, 0] = np.nan                    # an unconstrained dim: not looked at
    first, viol = cref.counters(traj, CONS)
    r = step_rewards(env, traj, obs, acts)
    bf_first, bf_viol, bf_pen, bf_term = cref.brute_force(traj, CONS, rows, 4.0, step_reward=r)
    np.testing.assert_array_equal(first, bf_first)
    np.testing.assert_array_equal(viol, bf_viol)
    assert first[0, 1, 3] <= 2 and first[1, 2, 0] == 0 and first[1, 0, 2] <= 1 and viol[0, 0, 1] >= 1
    frac = (viol > 0).mean()
    assert 0.2 < frac < 0.9 and (first == 0).any() and (first == 3).any() and (first == 4).any()
    pen = cref.penalty_rows(rows, viol, 4.0)
    assert pen.dtype == np.float32
    np.testing.assert_array_equal(pen.view(np.uint32), bf_pen.view(np.uint32))
    np.testing.assert_array_equal(pen[viol == 0].view(np.uint32), rows[viol == 0].view(np.uint32))
    term = cref.terminate_rows(env, traj, obs, acts, rows, first, 4.0)
    ok = ~np.isnan(bf_term)
    np.testing.assert_array_equal(term[ok], bf_term[ok])
    np.testing.assert_array_equal(np.isnan(term), np.isnan(bf_term))
    np.testing.assert_array_equal(term[first == 4], rows[first == 4].astype(np.float64))


def test_terminate_reads_nothing_after_the_first_violation():
    env = small_env()
    traj, obs, acts, rows = problem(2)
    first, _ = cref.counters(traj, CONS)
    mi, ni, j = [int(v[0]) for v in np.nonzero(first == 1)]
    want = cref.terminate_rows(env, traj, obs, acts, rows, first, 2.0)
    blown = traj.copy()
    blown[2:, mi, ni, j] = np.nan
    f2, v2 = cref.counters(blown, CONS)
    assert f2[mi, ni, j] == 1 and v2[mi, ni, j] == 3
    got = cref.terminate_rows(env, blown, obs, acts, rows, f2, 2.0)
    assert np.isfinite(got[mi, ni, j]) and got[mi, ni, j] == want[mi, ni, j]
    r = step_rewards(env, traj, obs, acts).astype(np.float64)
    assert got[mi, ni, j] == (r[mi, ni, 0, j] + r[mi, ni, 1, j]) - 2.0      # the step that leaves still pays
    pen = cref.penalty_rows(np.full_like(rows, np.nan), v2, 4.0)
    assert np.isnan(pen).all()


# ---------------------------------------------------------------------------------------------------------------------- validation
def test_plan_options_defaults_and_the_opt_in_route():
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_constraints=None, cem_constraint_mode="penalty", cem_constraint_weight=None) is None
    opt = PlanOptions.from_kwargs(use_cem=True, cem_constraints=CONS, cem_constraint_weight=3.0)
    assert opt is not None and opt.score_params is None and opt.update == "cem" and opt.keep_elites == 0
    assert opt.constraints == (tuple(CONS), "penalty", 3.0)
    c = opt.constraint_params
    assert isinstance(c, _lib.ConstraintParams) and (c.n, c.mode, c.weight) == (2, 0, 3.0)
    assert list(c.dim[:2]) == [1, 4] and c.lo[0] == -1.0 and c.hi[0] == np.float32(1.2) and c.lo[1] == -1.5 and c.hi[1] == np.inf
    opt = PlanOptions.from_kwargs(use_cem=True, cem_constraints=dict(dim=0, hi=2.0), cem_constraint_mode="terminate", cem_constraint_weight=0.0,
                                  cem_score="cvar", cem_risk=0.5, cem_update="mppi")
    assert (opt.constraint_params.n, opt.constraint_params.mode, opt.constraint_params.weight) == (1, 1, 0.0)
    assert opt.constraint_params.lo[0] == -np.inf and opt.score_params.mode == 3 and opt.update == "mppi"
    plain = PlanOptions.from_kwargs(use_cem=True, cem_noise_beta=1.0)
    assert plain.constraints is None and plain.constraint_params is None


@pytest.mark.parametrize("kw,msg", [
    (dict(use_cem=False, cem_constraints=CONS, cem_constraint_weight=1.0), "need use_cem=True"),
    (dict(cem_constraint_mode="terminate"), "they need cem_constraints"),
    (dict(cem_constraint_weight=1.0), "they need cem_constraints"),
    (dict(cem_constraints=CONS), "need a cem_constraint_weight"),
    (dict(cem_constraints=CONS, cem_constraint_weight=-1.0), "finite and >= 0"),
    (dict(cem_constraints=CONS, cem_constraint_weight=float("nan")), "finite and >= 0"),
    (dict(cem_constraints=CONS, cem_constraint_weight=float("inf")), "finite and >= 0"),
    (dict(cem_constraints=CONS, cem_constraint_weight=1.0, cem_constraint_mode="stop"), "'penalty' or 'terminate'"),
    (dict(cem_constraints=[], cem_constraint_weight=1.0), "expected 1 .. 16"),
    (dict(cem_constraints=[dict(dim=0, lo=0.0)] * 17, cem_constraint_weight=1.0), "expected 1 .. 16"),
    (dict(cem_constraints=[dict(dim=0)], cem_constraint_weight=1.0), "at least one of lo and hi"),
    (dict(cem_constraints=[dict(lo=0.0)], cem_constraint_weight=1.0), "expected dict"),
    (dict(cem_constraints=[dict(dim=0, lo=0.0, weight=2.0)], cem_constraint_weight=1.0), "expected dict"),
    (dict(cem_constraints=[(0, 0.0, 1.0)], cem_constraint_weight=1.0), "expected dict"),
    (dict(cem_constraints=5, cem_constraint_weight=1.0), "must be a list"),
    (dict(cem_constraints=[dict(dim=-1, lo=0.0)], cem_constraint_weight=1.0), "observation index"),
    (dict(cem_constraints=[dict(dim=1.5, lo=0.0)], cem_constraint_weight=1.0), "observation index"),
    (dict(cem_constraints=[dict(dim=0, lo=1.0, hi=1.0)], cem_constraint_weight=1.0), "must be below"),
    (dict(cem_constraints=[dict(dim=0, lo=2.0, hi=1.0)], cem_constraint_weight=1.0), "must be below"),
    (dict(cem_constraints=[dict(dim=0, lo=1.0, hi=1.0 + 1e-9)], cem_constraint_weight=1.0), "in float32"),
    (dict(cem_constraints=[dict(dim=0, lo=float("nan"))], cem_constraint_weight=1.0), "NaN"),
    (dict(cem_constraints=[dict(dim=0, lo=-np.inf, hi=np.inf)], cem_constraint_weight=1.0), "both sides are infinite"),
    (dict(cem_constraints=[dict(dim=0, lo=-np.inf)], cem_constraint_weight=1.0), "both sides are infinite"),
])
def test_plan_options_refusals(kw, msg):
    kw = dict(dict(use_cem=True), **kw)
    with pytest.raises(ValueError, match=msg):
        PlanOptions.from_kwargs(**kw)


def test_plan_options_keeps_its_other_refusals():
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_constraints=CONS, cem_constraint_weight=1.0)
    with pytest.raises(ValueError, match="cem_risk configures"):
        PlanOptions.from_kwargs(use_cem=True, cem_risk=1.0, cem_constraints=CONS, cem_constraint_weight=1.0)


def test_constraint_params_directly():
    c = HipEngine.constraint_params([dict(dim=np.int64(3), lo=0.1, hi=None)], "terminate", 2)
    assert (c.n, c.mode, c.weight, c.dim[0]) == (1, 1, 2.0, 3) and c.lo[0] == np.float32(0.1) and c.hi[0] == np.inf
    assert HipEngine.constraint_params(CONS, 1, 0.5).mode == 1 and HipEngine.constraint_params(CONS, weight=0.5).mode == 0
    for mode in (2, -1, "Penalty"):
        with pytest.raises(ValueError, match="'penalty' or 'terminate'"):
            HipEngine.constraint_params(CONS, mode, 1.0)
    with pytest.raises(ValueError, match="finite and >= 0"):
        HipEngine.constraint_params(CONS, "penalty")
    with pytest.raises(ValueError, match="observation index"):
        HipEngine.constraint_params([dict(dim=True, lo=0.0)], "penalty", 1.0)


def test_the_forecast_iteration_word_is_the_library_s():
    from cadm_amd import planner
    src = open(os.path.join(ROOT, "cadm_amd", "csrc", "planner.h")).read()
    assert int(re.search(r"#define CADM_FORECAST_IT (0x[0-9A-Fa-f]+)", src).group(1), 16) == planner.FORECAST_IT


def test_struct_layout_matches_the_header():
    names = [f[0] for f in _lib.ConstraintParams._fields_]
    assert names == ["n", "mode", "weight", "dim", "lo", "hi"]
    assert ctypes.sizeof(_lib.ConstraintParams) == (3 + 3 * 16) * 4
    assert [getattr(_lib.ConstraintParams, k).offset for k in names] == [0, 4, 8, 12, 76, 140]
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    body = re.search(r"typedef struct cadm_constraint_params \{(.*?)\} cadm_constraint_params;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[CADM_MAX_CONSTRAINTS\])?;", body) == names
    assert re.search(r"#define CADM_MAX_CONSTRAINTS (\d+)", src).group(1) == "16" == str(_lib.MAX_CONSTRAINTS)
    assert re.search(r"#define CADM_CONSTRAIN_PENALTY (\d+)", src).group(1) == "0" and _lib.CONSTRAIN_MODES["penalty"] == 0
    assert re.search(r"#define CADM_CONSTRAIN_TERMINATE (\d+)", src).group(1) == "1" and _lib.CONSTRAIN_MODES["terminate"] == 1
    sig = _lib.SIGNATURES
    assert len(sig["cadm_constrain_returns"][1]) == 12 and len(sig["cadm_constrained_plan"][1]) == len(sig["cadm_scored_plan"][1]) + 1
    assert len(sig["cadm_constrained_workspace_bytes"][1]) == 5 and sig["cadm_constrained_workspace_bytes"][0] is ctypes.c_size_t
