"""CPU: the numpy restatement of the actuator model (tests/actuator_ref.py) on the properties the GPU tests rely on -- the float32
emulation of the kernel's cost chain inside the derived bound, idempotence, the inert case, and why the plan needs a last pass --, the
`cadm_actuator_params` struct and the ctypes signatures as the header lays them out, and every construction-time refusal of
`PlanOptions.from_kwargs` for `cem_action_delay` / `cem_action_rate_limit` / `cem_action_rate_cost` / `cem_action_advance`."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import actuator_ref as aref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CASES = [(2, 24, 5, 6, 0), (2, 24, 5, 6, 1), (2, 24, 5, 6, 4), (4, 7, 3, 3, 2), (4, 1, 5, 6, 1)]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def brute_force(seqs, delay, dl, w, prev, prefix, lb=-1.0, ub=1.0):
    """the definition's loop, one chain at a time, on numpy float32 scalars; the cost in python floats"""
    u = np.array(seqs, dtype=F, copy=True)
    m, n, H, A = u.shape
    cost = np.zeros((m, n))
    for mi in range(m):
        for c in range(n):
            for a in range(A):
                last, ca = F(prev[mi, a]), 0.0
                for t in range(H):
                    x = u[mi, c, t, a]
                    if t < delay and not np.isnan(prefix[mi, t, a]):
                        y = F(prefix[mi, t, a])
                    elif np.isfinite(dl[a]) and not np.isnan(last):
                        y = min(max(x, F(last - dl[a])), F(last + dl[a]))
                        y = F(min(max(y, F(lb)), F(ub)))
                    else:
                        y = x
                    if not np.isnan(last):
                        ca += float(w[a]) * (float(y) - float(last)) ** 2
                    u[mi, c, t, a] = y
                    last = y
                cost[mi, c] += ca
    return u, cost


@pytest.mark.parametrize("m,n,H,A,d", CASES, ids=["m%d-n%d-H%d-A%d-d%d" % c for c in CASES])
def test_restatement_against_brute_force(m, n, H, A, d):
    """The vectorised restatement == the definition's loop, the sequences bit for bit; the float32 emulation of the kernel's cost chain
    stays inside the bound the GPU test holds the kernel to; a second pass changes no bit and costs the same."""
    seqs, dl, w, prev, prefix = aref.make_case(m, n, H, A, d, seed=m + n + d, nan_env=m - 1, outside=True)
    u, cost, S = aref.actuate(seqs, d, dl, w, prev, prefix)
    bu, bc = brute_force(seqs, d, dl, w, prev, prefix)
    np.testing.assert_array_equal(_bits(u), _bits(bu))
    np.testing.assert_allclose(cost, bc, rtol=1e-12, atol=1e-300)
    np.testing.assert_array_equal(cost, S)                    # the terms are non-negative
    assert (cost > 0).any() and np.isfinite(cost).all()
    err, lim = np.abs(aref.cost_f32(u, w, prev).astype(np.float64) - cost), aref.bound(S, H, A)
    assert (err <= lim).all(), "worst |err| / bound %.3f" % (err / np.maximum(lim, 1e-300)).max()
    print("\nfloat32 chain against float64: worst |err| / bound %.3f" % (err[lim > 0] / lim[lim > 0]).max())
    again, cost2, _ = aref.actuate(u, d, dl, w, prev, prefix)
    np.testing.assert_array_equal(_bits(again), _bits(u))
    np.testing.assert_array_equal(cost2, cost)
    # what the definition promises: pins are facts, free steps stay in the window and -- with the window inside it or not -- in the box
    pinned = np.zeros((m, H, A), bool)
    pinned[:, :d] = ~np.isnan(prefix)
    for c in range(n):
        np.testing.assert_array_equal(_bits(u[:, c][pinned]), _bits(np.concatenate([prefix, np.zeros((m, H - d, A), F)], axis=1)[pinned]))
        assert aref.window_ok(u[:, c], dl, prev, free=~pinned).all()
    limited = np.isfinite(dl)[None, None, None] & ~np.isnan(prev)[:, None, None] & ~pinned[:, None]
    assert (np.abs(u[np.broadcast_to(limited, u.shape)]) <= 1.0).all()
    assert np.isnan(prev[m - 1]).all()
    np.testing.assert_array_equal(_bits(u[m - 1, :, 0][:, np.isnan(prefix[m - 1, 0]) if d else slice(None)]),
                                  _bits(seqs[m - 1, :, 0][:, np.isnan(prefix[m - 1, 0]) if d else slice(None)]))      # unknown prev: step 0 is free


def test_inert_parameters_copy():
    seqs, _, _, prev, _ = aref.make_case(2, 24, 5, 6, 0, seed=1)
    seqs[0, 0, 0, 0], seqs[1, 2, 3, 4] = -0.0, np.nan
    u, cost, _ = aref.actuate(seqs, 0, np.inf, 0.0, prev, None)
    np.testing.assert_array_equal(_bits(u), _bits(seqs))
    assert (cost[np.isfinite(cost)] == 0).all() and np.isnan(cost[1, 2]) and np.isnan(cost).sum() == 1
    u, cost, _ = aref.actuate(seqs, 0, 0.25, 1.0, None, None)      # nothing known about step 0: it is free, and costs nothing
    np.testing.assert_array_equal(_bits(u[:, :, 0]), _bits(seqs[:, :, 0]))


def test_a_mean_of_feasible_sequences_needs_the_last_pass():
    """The mean of three feasible sequences, formed in float32, violates the float32 window check by a few ulps at some step, and
    misses some pinned value (a third of the sum of three copies need not be the value) -- and passes the check, pins restored, after
    one more pass, which moves it by a few ulps only.  This is what justifies the plan's last pass in the loop."""
    m, K, H, A, d = 4, 3, 30, 6, 2
    rng = np.random.default_rng(0)
    dl, w = np.full(A, 0.1, F), np.ones(A, F)
    prev = rng.uniform(-0.9, 0.9, (m, A)).astype(F)
    prefix = rng.uniform(-1, 1, (m, d, A)).astype(F)
    u, _, _ = aref.actuate(rng.uniform(-1, 1, (m, K, H, A)).astype(F), d, dl, w, prev, prefix)
    acc3 = ((u[:, 0] + u[:, 1]).astype(F) + u[:, 2]).astype(F)      # three elites: a divisor that is no power of two
    mean3 = (acc3 / F(3)).astype(F)
    free = np.ones((m, H, A), bool)
    free[:, :d] = False
    bad = ~aref.window_ok(mean3, dl, prev, free=free)
    assert bad.any(), "the float32 mean of feasible sequences passed the exact check everywhere"
    last = np.concatenate([prev[:, None], mean3[:, :-1]], axis=1)
    over = np.abs(mean3.astype(np.float64) - last) - 0.1
    assert over[bad].max() <= 8 * np.spacing(F(1.0)), "violations are rounding, not more: %g" % over[bad].max()
    assert not np.array_equal(_bits(mean3[:, :d]), _bits(prefix)), "a mean of three copies of a pinned value reproduced every one"
    fixed, _, _ = aref.actuate(mean3[:, None], d, dl, w, prev, prefix)
    assert aref.window_ok(fixed[:, 0], dl, prev, free=free).all()
    np.testing.assert_array_equal(_bits(fixed[:, 0, :d]), _bits(prefix))
    assert np.abs(fixed[:, 0, d:].astype(np.float64) - mean3[:, d:]).max() <= H * 8 * np.spacing(F(1.0))
    print("\n%d of %d free steps of a float32 mean violate the exact window, by at most %.2g" % (bad.sum(), free.sum(), over[bad].max()))


def test_struct_and_signatures_match_the_header():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    assert int(re.search(r"#define CADM_MAX_ACT_DIMS (\d+)", src).group(1)) == _lib.MAX_ACT_DIMS == 32
    body = re.search(r"typedef struct cadm_actuator_params \{(.*?)\} cadm_actuator_params;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[CADM_MAX_ACT_DIMS\])?;", body)
    want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, want[t] * 32 if arr else want[t]) for t, n, arr in fields] == [(n, t) for n, t in _lib.ActuatorParams._fields_]
    assert ctypes.sizeof(_lib.ActuatorParams) == (2 + 2 * 32) * 4
    assert re.search(r"#define CADM_ABI_VERSION 2\b", src)
    kinds = {"cadm_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "int": ctypes.c_int,
             "uint32_t": ctypes.c_uint32}
    for name in ("cadm_actuate_actions", "cadm_actuated_workspace_bytes", "cadm_actuated_plan"):
        ret, args = re.search(r"^(int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M).groups()
        got = []
        for a in args.split(","):
            typ = re.sub(r"\bconst\b", "", a).strip().rsplit(" ", 1)[0].replace(" ", "")
            got.append(kinds[typ] if typ in kinds else ctypes.POINTER(getattr(_lib, {"cadm_actuator_params*": "ActuatorParams", "cadm_track_params*": "TrackParams",
                       "cadm_knot_params*": "KnotParams", "cadm_constraint_params*": "ConstraintParams", "cadm_score_params*": "ScoreParams",
                       "cadm_mppi_params*": "MppiParams"}[typ])))
        res, sig = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t), name
        assert len(sig) == len(got) and all(x is y for x, y in zip(sig, got)), name
    # the loop entry is cadm_tracking_plan's arguments behind the actuator's four
    assert _lib.SIGNATURES["cadm_actuated_plan"][1][5:] == _lib.SIGNATURES["cadm_tracking_plan"][1][1:]


def test_plan_options_accept_and_refuse():
    """Any of the three kwargs off its default takes the opt-in route by itself and is folded into the struct the library reads; every
    default still gives None; what is refused is refused without an engine."""
    kw = dict(use_cem=True, n_forwards=5, action_dim=6)
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_action_delay=0, cem_action_rate_limit=None, cem_action_rate_cost=None, cem_action_advance=True, **kw) is None
    for one in (dict(cem_action_delay=1), dict(cem_action_rate_limit=0.1), dict(cem_action_rate_cost=[0.0] * 6)):
        opt = PlanOptions.from_kwargs(**one, **kw)
        assert opt is not None and isinstance(opt.actuator_params, _lib.ActuatorParams) and opt.action_advance is True
        assert opt.update == "cem" and opt.track_params is None and opt.knot_params is None
    opt = PlanOptions.from_kwargs(cem_action_delay=np.int64(4), cem_action_rate_limit=[0.1, math.inf, 0.3, 1, 2, 3], cem_action_rate_cost=2, **kw)
    ap = opt.actuator_params
    assert (ap.delay, ap.n_dims) == (4, 6) and list(ap.rate_limit[:3]) == [F(0.1), math.inf, F(0.3)] and ap.rate_limit[6] == math.inf
    assert list(ap.rate_w) == [2.0] * 32 and opt.actuator == (4, (0.1, math.inf, 0.3, 1.0, 2.0, 3.0), 2.0)
    ap = PlanOptions.from_kwargs(cem_action_rate_cost=[1, 2, 3, 4, 5, 6], **kw).actuator_params
    assert (ap.delay, ap.n_dims) == (0, 6) and list(ap.rate_w[:7]) == [1, 2, 3, 4, 5, 6, 0] and list(ap.rate_limit) == [math.inf] * 32
    assert PlanOptions.from_kwargs(cem_action_rate_limit=0.5, **kw).actuator_params.n_dims == 0      # a scalar fits any A
    assert PlanOptions.from_kwargs(cem_action_delay=1, cem_action_advance=False, **kw).action_advance is False
    both = PlanOptions.from_kwargs(cem_action_delay=1, cem_knots=2, cem_update="mppi", cem_tracking=dict(dim=0), cem_return="best",
                                   cem_constraints=[dict(dim=0, lo=0.0)], cem_constraint_weight=1.0, cem_score="cvar", cem_risk=0.5, **kw)
    assert all(x is not None for x in (both.actuator_params, both.knot_params, both.track_params, both.constraint_params, both.score_params))
    assert PlanOptions.from_kwargs(use_cem=True, cem_knots=2).actuator_params is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_action_delay=3).actuator_params.delay == 3      # no horizon given: the library checks it
    for delay in (-1, 5, 6, 1.0, 1.5, "1", True, None):
        with pytest.raises(ValueError, match="action delay"):
            PlanOptions.from_kwargs(cem_action_delay=delay, **kw)
    for lim in (0.0, -0.1, float("nan"), [0.1, 0.1, 0.1, 0.1, 0.1, 0.0], [0.1] * 5 + [float("nan")], -math.inf):
        with pytest.raises(ValueError, match="rate_limit must be > 0"):
            PlanOptions.from_kwargs(cem_action_rate_limit=lim, **kw)
    for cost in (-1.0, float("nan"), math.inf, [1.0] * 5 + [-0.5], [1.0] * 5 + [math.inf]):
        with pytest.raises(ValueError, match="rate_cost must be finite and >= 0"):
            PlanOptions.from_kwargs(cem_action_rate_cost=cost, **kw)
    for name in ("cem_action_rate_limit", "cem_action_rate_cost"):
        for val in ([0.1] * 5, [0.1] * 7, [], [0.1] * 33, [[0.1] * 6]):
            with pytest.raises(ValueError, match="entries|scalar or \\[A\\]"):
                PlanOptions.from_kwargs(**{name: val}, **kw)
        with pytest.raises(ValueError, match="number or a list"):
            PlanOptions.from_kwargs(**{name: "fast"}, **kw)
    with pytest.raises(ValueError, match="entries"):      # two arrays that disagree, no action_dim to check against
        PlanOptions.from_kwargs(use_cem=True, cem_action_rate_limit=[0.1] * 3, cem_action_rate_cost=[0.1] * 4)
    with pytest.raises(ValueError, match="up to 32 action dims"):
        PlanOptions.from_kwargs(use_cem=True, cem_action_delay=1, action_dim=33)
    with pytest.raises(ValueError, match="cem_action_advance configures the actuator model"):
        PlanOptions.from_kwargs(cem_action_advance=False, use_cem=True)
    with pytest.raises(ValueError, match="True or False"):
        PlanOptions.from_kwargs(cem_action_delay=1, cem_action_advance=0, **kw)
    with pytest.raises(ValueError, match="use_cem=True"):
        PlanOptions.from_kwargs(cem_action_delay=1, n_forwards=5, action_dim=6)
    with pytest.raises(NotImplementedError, match="discrete"):
        PlanOptions.from_kwargs(cem_action_rate_cost=1.0, discrete=True, use_cem=True)

    class TwoRanks:
        pass
    import torch.distributed as dist
    orig = dist.get_world_size
    dist.get_world_size = lambda group=None: 2
    try:
        with pytest.raises(NotImplementedError, match="more than one rank"):
            PlanOptions.from_kwargs(cem_action_delay=1, process_group=TwoRanks(), **kw)
    finally:
        dist.get_world_size = orig


def test_model_methods_refuse_without_an_engine():
    """What the model's actuator methods refuse, they refuse before they touch the engine (a stand-in object carries the options alone)."""
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Model
    opt = PlanOptions.from_kwargs(use_cem=True, cem_action_delay=2, n_forwards=5, action_dim=6)
    stub = types.SimpleNamespace(_opt=opt, engine=None, action_space_dims=6, n_forwards=5, _act_prev=None, _act_prefix=None,
                                 _require_actuator=lambda who: Model._require_actuator(stub, who))
    for kw in (dict(prev=np.zeros((2, 5))), dict(committed=np.zeros((2, 1, 6))), dict(prev=np.zeros((2, 6)), committed=np.zeros((3, 2, 6)))):
        with pytest.raises(ValueError, match="set_applied_actions: (prev|committed)"):
            Model.set_applied_actions(stub, **kw)
    assert Model.set_applied_actions(stub) is None and stub._act_prev is None
    assert Model.actuator_state(stub) is None
    for fn, args in ((Model.set_applied_actions, (np.zeros((2, 6)),)), (Model.actuator_state, ()), (Model.action_cost, (np.zeros((2, 5, 6)),))):
        for o in (None, PlanOptions.from_kwargs(use_cem=True, cem_knots=2)):
            none = types.SimpleNamespace(_opt=o)
            none._require_actuator = lambda who, none=none: Model._require_actuator(none, who)
            with pytest.raises(ValueError, match="no actuator model"):
                fn(none, *args)
