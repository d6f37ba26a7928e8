"""CPU: the uncertainty cost's numpy restatement (tests/uncertainty_ref.py) against plain loops, the float32 emulation of the kernel's
chain (csrc/uncertainty.hip) within the derived bound -- so the bound is neither vacuous nor broken before a GPU sees it --, and the
option checks of `PlanOptions.from_kwargs(cem_uncertainty=...)` / `HipEngine.uncertainty_params`, which need no engine."""
import math

import numpy as np
import pytest

import uncertainty_ref as uref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

F = np.float32
GEOMETRIES = [(5, 5, 11), (20, 5, 18), (4, 1, 18), (6, 2, 7)]      # (p, E, D)


def _traj(seed, H, m, n, p, D, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((H, m, n, p, D)) * scale * rng.uniform(0.5, 2.0, D) + offset * rng.standard_normal(D)).astype(F)


def _first(seed, H, m, n, p):
    first = np.random.default_rng(seed).integers(0, H + 1, (m, n, p)).astype(np.int32)
    first[0, 0], first[-1, -1] = 0, H
    return first


def brute_force(traj, E, kind, w, form, cap, first):
    """the quantity by loops over (env, candidate, step, dim) on python floats"""
    H, m, n, p, D = traj.shape
    q = p // E
    step, cost = np.zeros((m, n, H)), np.zeros((m, n))
    for mi in range(m):
        for c in range(n):
            cut = H if first is None else int(min(first[mi, c]))
            for t in range(H):
                u = 0.0
                for d in range(D):
                    if not w[d] > 0:
                        continue
                    v = [float(traj[t, mi, c, j, d]) for j in range(p)]
                    if kind == "epistemic":
                        v = [sum(v[e * q:(e + 1) * q]) / q for e in range(E)]
                    mu = sum(v) / len(v)
                    u += float(w[d]) * sum((a - mu) ** 2 for a in v) / len(v)
                if form == "std":
                    u = math.sqrt(u)
                if cap is not None and u > float(F(cap)):
                    u = float(F(cap))
                step[mi, c, t] = u
                if t <= cut:
                    cost[mi, c] += u
    return step, cost


@pytest.mark.parametrize("p,E,D", GEOMETRIES)
def test_restatement_against_plain_loops(p, E, D):
    H, m, n = 4, 2, 3
    traj = _traj(p + D, H, m, n, p, D)
    for kind in uref.KINDS:
        for form, cap, first, style in (("var", None, None, "broadcast"), ("std", 2.5, _first(1, H, m, n, p), "per-dim"), ("var", 0.5, None, "one-hot-4")):
            w = uref.make_w(style, D, seed=3)
            step, cost, _, _ = uref.cost(traj, E, kind, w, form, cap, first)
            bs, bc = brute_force(traj, E, kind, uref.weights(w, D), form, cap, first)
            np.testing.assert_allclose(step, bs, rtol=1e-11, atol=1e-13)
            np.testing.assert_allclose(cost, bc, rtol=1e-11, atol=1e-13)
            assert (cost > 0).any() or (kind == "epistemic" and E == 1)
    if E == 1:
        assert (uref.cost(traj, E, "epistemic")[1] == 0).all()
        assert (uref.emulate32(traj, E, "epistemic")[1] == 0).all()


@pytest.mark.parametrize("p,E,D", GEOMETRIES)
def test_float32_chain_within_the_bound(p, E, D):
    """The emulated chain against float64 at value scales 0.01 .. 30 and offsets up to 100, both kinds and forms, with and without a
    `first` cut and a cap: inside the UNDOUBLED bound everywhere, and not by orders of magnitude (the bound is not vacuous)."""
    H, m, n = 5, 2, 7
    worst = 0.0
    for k, (scale, offset) in enumerate(((0.01, 0.0), (1.0, 1.0), (30.0, 5.0), (0.3, 100.0))):
        traj = _traj(10 * k + p, H, m, n, p, D, scale, offset)
        for kind in uref.KINDS:
            for form in uref.FORMS:
                for first, cap, style in ((None, None, "broadcast"), (_first(k, H, m, n, p), None, "per-dim"), (None, scale, "one-hot-1")):
                    w = uref.make_w(style, D, seed=k)
                    step, cost, B, S = uref.cost(traj, E, kind, w, form, cap, first)
                    s32, c32 = uref.emulate32(traj, E, kind, w, form, cap, first)
                    lim = uref.bound(B, S, H, first)
                    es, ec = np.abs(s32 - step), np.abs(c32 - cost)
                    assert (es <= B).all(), "step: worst |err| / bound %.3f" % (es / B).max()
                    assert (ec <= lim).all(), "cost: worst |err| / bound %.3f" % (ec / lim).max()
                    if E > 1 or kind == "total":
                        worst = max(worst, float((es[B > 0] / B[B > 0]).max()), float((ec[lim > 0] / lim[lim > 0]).max()))
    assert 1e-4 < worst <= 1.0, worst


def test_nan_reaches_the_cost_only_from_weighted_dims_at_counted_steps():
    H, m, n, p, E, D = 4, 2, 3, 10, 5, 6
    traj = _traj(2, H, m, n, p, D)
    w = uref.make_w("per-dim", D, seed=1)
    first = np.full((m, n, p), H, np.int32)
    first[1, 2, 4] = 1
    base = uref.emulate32(traj, E, "total", w, first=first)
    bad = traj.copy()
    bad[:, :, :, :, 0] = np.nan                  # a zero-weight dim
    bad[2:, 1, 2, 3, 1] = 1e30                   # behind candidate (1, 2)'s cut: its square overflows float32
    for fn in (uref.emulate32, lambda *a, **k: uref.cost(*a, **k)[:2]):
        step, cost = fn(bad, E, "total", w, first=first)
        assert np.isfinite(cost).all() and (step[1, 2, 2:] > 1e38).all()
    assert np.isinf(uref.emulate32(bad, E, "total", w, first=first)[0][1, 2, 2:]).all()
    np.testing.assert_array_equal(uref.emulate32(bad, E, "total", w, first=first)[1].view(np.uint32), base[1].view(np.uint32))
    bad[1, 1, 2, 3, 1] = np.nan                  # at the cut: counted
    step, cost = uref.emulate32(bad, E, "total", w, first=first)
    assert np.isnan(cost[1, 2]) and np.isfinite(np.delete(cost.reshape(-1), 5)).all()
    # a cap is a comparison: it holds a NaN, and stops an inf
    step, cost = uref.emulate32(bad, E, "total", w, cap=3.0, first=first)
    assert np.isnan(step[1, 2, 1]) and (step[1, 2, 2:] == F(3.0)).all()


# ---------------------------------------------------------------------------------------------------------------------- the options
def test_none_is_the_default_route():
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_uncertainty=None) is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_uncertainty=None) is None
    opt = PlanOptions.from_kwargs(cem_noise_beta=1.0, use_cem=True)
    assert opt.uncertainty is None and opt.uncertainty_params is None
    # the two fields have defaults and sit in front of the tracking ones, which stay the last three (tests/test_tracking_ref.py), as the
    # actuator's do: keyword constructions and positional ones up to the actuator's fields keep working
    assert PlanOptions._fields[-5:-3] == ("uncertainty", "uncertainty_params")
    assert PlanOptions(*range(18)).uncertainty_params is None and PlanOptions(*range(18)).action_advance == 17


def test_options_from_kwargs():
    opt = PlanOptions.from_kwargs(use_cem=True, cem_uncertainty=dict(kind="epistemic", weight=0.5))
    assert opt is not None and opt.uncertainty == ("epistemic", 0.5, None, "var", None)
    prm = opt.uncertainty_params
    assert (prm.kind, prm.form, prm.weight, prm.n_dims, prm.w[0]) == (_lib.UNC_KINDS["epistemic"], _lib.UNC_FORMS["var"], 0.5, 0, 1.0)
    assert math.isinf(prm.cap) and prm.cap > 0
    assert opt.actuator_params is None and opt.track_params is None and opt.update == "cem"
    opt = PlanOptions.from_kwargs(use_cem=True, obs_dim=3, cem_uncertainty=dict(kind="total", weight=-2, w=[0, 1.5, 0], form="std", cap=4))
    assert opt.uncertainty == ("total", -2.0, (0.0, 1.5, 0.0), "std", 4.0)
    prm = opt.uncertainty_params
    assert (prm.kind, prm.form, prm.weight, prm.cap, prm.n_dims, list(prm.w[:4])) == (1, 1, -2.0, 4.0, 3, [0.0, 1.5, 0.0, 0.0])
    opt = PlanOptions.from_kwargs(use_cem=True, obs_dim=3, cem_uncertainty=dict(kind="total", weight=0.0, w="delta_std"))
    assert opt.uncertainty[2] == "delta_std" and opt.uncertainty_params.n_dims == 0      # (the model fills the weights in)
    assert PlanOptions.from_kwargs(use_cem=True, cem_uncertainty=dict(kind="total", weight=1, w=2.0)).uncertainty_params.w[0] == 2.0
    assert ct_size() == 4 * (5 + _lib.MAX_UNC_DIMS)


def ct_size():
    import ctypes
    return ctypes.sizeof(_lib.UncertaintyParams)


BAD = [dict(kind="aleatoric", weight=1.0), dict(kind=2, weight=1.0), dict(kind="total", weight=math.nan), dict(kind="total", weight=math.inf),
       dict(kind="total", weight="much"), dict(kind="total", weight=1.0, form="variance"), dict(kind="total", weight=1.0, cap=0.0),
       dict(kind="total", weight=1.0, cap=-1.0), dict(kind="total", weight=1.0, cap=math.nan), dict(kind="total", weight=1.0, w=-1.0),
       dict(kind="total", weight=1.0, w=[1.0, math.nan, 1.0]), dict(kind="total", weight=1.0, w=[1.0, math.inf, 1.0]),
       dict(kind="total", weight=1.0, w=[0.0, 0.0, 0.0]), dict(kind="total", weight=1.0, w=0.0), dict(kind="total", weight=1.0, w=[1.0, 1.0]),
       dict(kind="total", weight=1.0, w=[[1.0] * 3]), dict(kind="total", weight=1.0, w="obs_std"), dict(kind="total"), dict(weight=1.0),
       dict(kind="total", weight=1.0, limit=3.0), ("total", 1.0), dict(kind="total", weight=1.0, w=[1.0] * (_lib.MAX_UNC_DIMS + 1))]


@pytest.mark.parametrize("bad", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_options_raise(bad):
    with pytest.raises(ValueError, match="uncertainty"):
        PlanOptions.from_kwargs(use_cem=True, obs_dim=3, cem_uncertainty=bad)


def test_refusals_match_the_other_options(monkeypatch):
    import torch.distributed as dist
    u = dict(kind="epistemic", weight=1.0)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        PlanOptions.from_kwargs(use_cem=True, process_group=object(), cem_uncertainty=u)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="need use_cem=True"):
        PlanOptions.from_kwargs(cem_uncertainty=u)
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_uncertainty=u)
    with pytest.raises(ValueError, match="up to %d observation dims" % _lib.MAX_UNC_DIMS):
        HipEngine.uncertainty_params("total", 1.0, obs_dim=_lib.MAX_UNC_DIMS + 1)
    prm = HipEngine.uncertainty_params(_lib.UNC_KINDS["total"], 1.0, form=_lib.UNC_FORMS["std"], cap=np.float32(2.0))
    assert (prm.kind, prm.form, prm.cap) == (1, 1, 2.0)
