"""CPU: the numpy restatement of the tracking targets (tests/tracking_ref.py) on the properties the GPU tests rely on, every validation
rule of `PlanOptions.from_kwargs` for `cem_tracking` / `cem_target_advance`, the `cadm_track_params` struct as the header lays it out, and
the model's `set_targets` shape checks as far as they run without an engine."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import tracking_ref as tref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(s, K, T) for s in tref.SHAPES for K in (1, 16) for T in (1, tref.SHAPES[s][0], tref.SHAPES[s][0] - 1, tref.SHAPES[s][0] + 3)]


def _first(shape, seed):
    H, m, n, p = tref.SHAPES[shape][:4]
    first = np.random.default_rng(seed).integers(0, H + 1, (m, n, p)).astype(np.int32)
    first.reshape(-1)[:2] = 0, H      # (rows (0, 0, 0) and (0, 0, 1) where p > 1)
    return first


@pytest.mark.parametrize("shape,K,T", CASES, ids=["%s-K%d-T%d" % c for c in CASES])
def test_restatement_against_brute_force(shape, K, T):
    """The vectorised restatement == plain loops on python floats (to float64 rounding of another summation order), with and without
    `first`; the float32 emulation of the kernel's chain stays inside the bound the GPU test holds the kernel to."""
    H = tref.SHAPES[shape][0]
    traj, rows, terms, targets, offset = tref.make_case(shape, K, T)
    for first in (None, _first(shape, K + T)):
        out, cost, S, counted = tref.tracking(traj, rows, terms, targets, offset, first)
        bo, bc, bS, bn = tref.brute_force(traj, rows, terms, targets, offset, first)
        np.testing.assert_array_equal(counted, bn)
        np.testing.assert_allclose(cost, bc, rtol=1e-12, atol=0)
        np.testing.assert_allclose(S, bS, rtol=1e-12, atol=0)
        np.testing.assert_allclose(out, bo, rtol=1e-12, atol=1e-12)
        assert (S >= np.abs(cost) * (1 - 1e-12)).all()
        f32, c32 = tref.float32_chain(traj, rows, terms, targets, offset, first)
        err, lim = np.abs(f32.astype(np.float64) - out), tref.bound(S, out, H, K)
        assert (err <= lim).all() and (np.abs(c32.astype(np.float64) - cost) <= tref.bound(S, None, H, K)).all()
        skipped = counted == 0
        np.testing.assert_array_equal(f32[skipped].view(np.uint32), rows[skipped].view(np.uint32))
        if (~skipped).any():
            print("[%s K=%d T=%d first=%s] float32 chain: worst error / bound %.3f" % (shape, K, T, first is not None,
                                                                                       float((err[~skipped] / lim[~skipped]).max())))


def test_nan_targets_skip():
    """A NaN target skips its (step, term): the result equals that of the terms and rows that remain; an env whose targets are all NaN
    counts nothing and keeps its rows; the skipped share of the K = 16 cases lies in 10 .. 30 % on the envs that have targets."""
    for shape in tref.SHAPES:
        H, m = tref.SHAPES[shape][:2]
        traj, rows, terms, targets, offset = tref.make_case(shape, 16, H)
        out, cost, S, counted = tref.tracking(traj, rows, terms, targets, offset)
        live = [mi for mi in range(m) if not (m == 4 and mi == tref.ALL_NAN_ENV)]
        share = 1.0 - counted[live].mean() / (H * 16)
        assert 0.1 <= share <= 0.3, "%s: %.2f of the (step, term) pairs are skipped" % (shape, share)
        if m == 4:
            assert (counted[tref.ALL_NAN_ENV] == 0).all() and (cost[tref.ALL_NAN_ENV] == 0).all()
            np.testing.assert_array_equal(out[tref.ALL_NAN_ENV], rows[tref.ALL_NAN_ENV].astype(np.float64))
        # dropping term 0 == making its targets NaN
        gone = targets.copy()
        gone[:, :, 0] = np.nan
        a = tref.tracking(traj, rows, terms, gone, offset)
        b = tref.tracking(traj, rows, terms[1:], targets[:, :, 1:], offset)
        np.testing.assert_allclose(a[1], b[1], rtol=1e-12)
        np.testing.assert_array_equal(a[3], b[3])
    # a NaN in a tracked dim at a counted step reaches the row; in another dim it does not
    traj, rows, terms, targets, offset = tref.make_case("hopper-45", 1, 1, kinds=("square",))
    targets[:] = 0.5
    d = terms[0]["dim"]
    bad = traj.copy()
    bad[1, 0, 2, 3, d] = np.nan
    bad[2, 0, 4, 1, (d + 1) % 11] = np.inf
    out = tref.tracking(bad, rows, terms, targets, offset)[0]
    assert np.isnan(out[0, 2, 3]) and np.isfinite(np.delete(out.reshape(-1), 2 * 5 + 3)).all()


def test_constant_goal_and_offset_clamp():
    """T = 1 is the goal held over the horizon; a reference shorter than the horizon holds its last row; a negative offset holds the
    first row, one beyond T the last."""
    shape = "halfcheetah-320"
    H, m = tref.SHAPES[shape][:2]
    traj, rows, terms, targets, _ = tref.make_case(shape, 16, H + 3)
    targets = np.nan_to_num(targets, nan=0.25)
    zero = np.zeros(m, np.int32)
    run = lambda tg, off: tref.tracking(traj, rows, terms, tg, off)[1]
    np.testing.assert_array_equal(run(targets[:, :1], zero), run(np.repeat(targets[:, :1], H, axis=1), zero))
    np.testing.assert_array_equal(run(targets[:, 0], None), run(targets[:, :1], zero))                  # [m,K] is T = 1
    short = targets[:, :3]
    held = np.concatenate([short, np.repeat(short[:, -1:], H - 3, axis=1)], axis=1)
    np.testing.assert_array_equal(run(short, zero), run(held, zero))
    np.testing.assert_array_equal(run(targets, zero - 2), run(np.concatenate([targets[:, :1]] * 2 + [targets], axis=1), zero))
    np.testing.assert_array_equal(run(targets, zero + H + 7), run(targets[:, -1:], zero))
    np.testing.assert_array_equal(run(targets, zero + 2), run(targets[:, 2:], zero))
    assert tref.target_rows(4, 6, -2).tolist() == [0, 0, 0, 1, 2, 3] and tref.target_rows(4, 6, 2).tolist() == [2, 3, 3, 3, 3, 3]
    assert tref.target_rows(1, 3, 5).tolist() == [0, 0, 0]


def test_first_cut():
    """Steps t > first are not counted -- the step at `first` still pays: the result is that of the trajectory cut there, whatever it
    holds behind; first = H counts every step, first = 0 the first alone."""
    shape = "halfcheetah-320"
    H, m, n, p = tref.SHAPES[shape][:4]
    traj, rows, terms, targets, offset = tref.make_case(shape, 16, H)
    first = _first(shape, 3)
    out, cost, S, counted = tref.tracking(traj, rows, terms, targets, offset, first)
    junk = traj.copy()
    behind = np.arange(H)[:, None, None, None] > first[None]
    junk[behind] = np.nan
    again = tref.tracking(junk, rows, terms, targets, offset, first)
    np.testing.assert_array_equal(out, again[0])
    full = tref.tracking(traj, rows, terms, targets, offset)
    np.testing.assert_array_equal(out[first == H], full[0][first == H])
    only0 = tref.tracking(traj[:1], rows, terms, targets, offset)      # (a one-step horizon: step 0 alone)
    np.testing.assert_array_equal(cost[first == 0], only0[1][first == 0])
    assert (counted[first < H - 1] <= full[3][first < H - 1]).all()


def test_plan_options_accept_and_refuse():
    """`cem_tracking` alone takes the opt-in route and is folded into the struct the library reads; every default still gives None; what
    is refused is refused without an engine."""
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_tracking=None, cem_target_advance=True) is None
    terms = [dict(dim=3, w=2.0), dict(dim=0, kind="abs"), dict(dim=17, kind="huber", w=0.0, delta=0.5)]
    opt = PlanOptions.from_kwargs(use_cem=True, cem_tracking=terms)
    assert opt is not None and opt.target_advance is True and opt.tracking == tuple(terms) and opt.knot_params is None and opt.constraint_params is None
    tp = opt.track_params
    assert isinstance(tp, _lib.TrackParams) and tp.n == 3
    assert list(tp.dim[:3]) == [3, 0, 17] and list(tp.kind[:3]) == [0, 1, 2] and list(tp.w[:3]) == [2.0, 1.0, 0.0] and tp.delta[2] == 0.5
    assert opt.update == "cem" and opt.keep_elites == 0 and opt.score_params is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_tracking=dict(dim=1), cem_target_advance=False).target_advance is False
    assert PlanOptions.from_kwargs(use_cem=True, cem_tracking=dict(dim=1)).track_params.n == 1
    both = PlanOptions.from_kwargs(use_cem=True, cem_tracking=terms, cem_knots=2, cem_update="mppi", cem_constraints=[dict(dim=0, lo=0.0)],
                                   cem_constraint_weight=1.0)
    assert both.track_params is not None and both.knot_params is not None and both.constraint_params is not None
    assert PlanOptions.from_kwargs(use_cem=True, cem_knots=2).track_params is None      # the fields are appended with defaults
    assert PlanOptions._fields[-3:] == ("tracking", "track_params", "target_advance")
    with pytest.raises(ValueError, match="use_cem=True"):
        PlanOptions.from_kwargs(cem_tracking=terms)
    with pytest.raises(ValueError, match="needs cem_tracking"):
        PlanOptions.from_kwargs(use_cem=True, cem_target_advance=False)
    with pytest.raises(ValueError, match="True or False"):
        PlanOptions.from_kwargs(use_cem=True, cem_tracking=terms, cem_target_advance=1)
    with pytest.raises(NotImplementedError, match="discrete"):
        PlanOptions.from_kwargs(use_cem=True, cem_tracking=terms, discrete=True)
    bad = [[], [dict(dim=0)] * 17, [dict(w=1.0)], [dict(dim=-1)], [dict(dim=1.5)], [dict(dim=True)], [dict(dim=0, kind="cube")],
           [dict(dim=0, kind=3)], [dict(dim=0, w=-1.0)], [dict(dim=0, w=float("nan"))], [dict(dim=0, w=float("inf"))],
           [dict(dim=0, kind="huber")], [dict(dim=0, kind="huber", delta=0.0)], [dict(dim=0, kind="huber", delta=float("inf"))],
           [dict(dim=0, kind="square", delta=1.0)], [dict(dim=0, weight=1.0)], [dict(dim=0, target=1.0)], ["dim"], 5]
    for t in bad:
        with pytest.raises(ValueError, match="tracking"):
            PlanOptions.from_kwargs(use_cem=True, cem_tracking=t)
    assert HipEngine.track_params([dict(dim=0, kind=_lib.TRACK_KINDS["abs"])]).kind[0] == 1
    assert len(HipEngine.track_params([dict(dim=k) for k in range(16)]).dim) == 16


def test_struct_matches_the_header():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    assert int(re.search(r"#define CADM_MAX_TRACK_TERMS (\d+)", src).group(1)) == _lib.MAX_TRACK_TERMS == 16
    for name, code in _lib.TRACK_KINDS.items():
        assert int(re.search(r"#define CADM_TRACK_%s (\d+)" % name.upper(), src).group(1)) == code
    body = re.search(r"typedef struct cadm_track_params \{(.*?)\} cadm_track_params;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[CADM_MAX_TRACK_TERMS\])?;", body)
    want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, want[t] * 16 if arr else want[t]) for t, n, arr in fields] == [(n, t) for n, t in _lib.TrackParams._fields_]
    assert ctypes.sizeof(_lib.TrackParams) == (1 + 4 * 16) * 4


def test_set_targets_shape_checks_without_an_engine():
    """What `set_targets` refuses, it refuses before it touches the engine (a stand-in object carries the options alone)."""
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Model
    opt = PlanOptions.from_kwargs(use_cem=True, cem_tracking=[dict(dim=0), dict(dim=4, kind="abs")])
    stub = types.SimpleNamespace(_opt=opt, engine=None, _targets=None, _target_offset=None)
    for targets in (np.zeros((2, 3)), np.zeros((2, 5, 1)), np.zeros((2,)), np.zeros((0, 2)), np.zeros((2, 0, 2)), np.zeros((2, 2, 2, 2))):
        with pytest.raises(ValueError, match="set_targets: targets"):
            Model.set_targets(stub, targets)
    with pytest.raises(ValueError, match="set_targets: offset"):
        Model.set_targets(stub, np.zeros((2, 5, 2)), offset=np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="no cem_tracking"):
        Model.set_targets(types.SimpleNamespace(_opt=None), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="no cem_tracking"):
        Model.set_targets(types.SimpleNamespace(_opt=PlanOptions.from_kwargs(use_cem=True, cem_knots=2)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="no cem_tracking"):
        Model.tracking_cost(types.SimpleNamespace(_opt=None), np.zeros((2, 18)), np.zeros((2, 5, 6)))
    assert stub._targets is None and stub._target_offset is None
    Model.clear_targets(stub)
    assert stub._targets is None
