"""CPU: the numpy restatement of the MPPI update (tests/mppi_ref.py) held to known answers, and the new exports of the built library
as far as they go without a ctx."""
import ctypes

import numpy as np
import pytest

import icem_ref
import mppi_ref

M, N, H, A = 2, 37, 5, 3


def _data(seed=0):
    rng = np.random.default_rng(seed)
    mean = rng.uniform(-0.5, 0.5, (M, H, A))
    var = rng.uniform(0.05, 0.3, (M, H, A))
    actions = rng.uniform(-1.0, 1.0, (M, N, H, A))
    cand = rng.standard_normal((M, N)) * 3.0
    return mean, var, actions, cand


def test_equal_returns_give_the_plain_mean_and_biased_variance():
    mean, var, actions, cand = _data()
    cand[:] = 1.75
    for relative in (False, True):      # (relative: lambda_eff == 0 -> every weight 1)
        nm, nv, plan = mppi_ref.mppi_update(mean, var, actions, cand, 0.7, relative, alpha=0.0)
        np.testing.assert_allclose(nm, actions.mean(axis=1), rtol=0, atol=1e-15)
        np.testing.assert_allclose(nv, actions.var(axis=1), rtol=0, atol=1e-15)
        np.testing.assert_array_equal(plan, np.clip(nm, -1.0, 1.0))
    # the blend: alpha of the old, 1 - alpha of the new
    nm, nv, _ = mppi_ref.mppi_update(mean, var, actions, cand, 0.7, alpha=0.25)
    np.testing.assert_allclose(nm, 0.25 * mean + 0.75 * actions.mean(axis=1), rtol=0, atol=1e-15)
    np.testing.assert_allclose(nv, 0.25 * var + 0.75 * actions.var(axis=1), rtol=0, atol=1e-15)


def test_weighted_statistics_by_hand():
    """Two candidates with returns 0 and -lambda ln 3: weights 1 and 1/3."""
    lam = 0.4
    actions = np.array([[[[1.0]], [[-1.0]]]])                         # [1, 2, 1, 1]
    cand = np.array([[0.0, -lam * np.log(3.0)]])
    nm, nv, _ = mppi_ref.mppi_update(np.zeros((1, 1, 1)), np.zeros((1, 1, 1)), actions, cand, lam, alpha=0.0)
    assert abs(nm[0, 0, 0] - 0.5) <= 1e-15                            # (1 - 1/3) / (4/3)
    assert abs(nv[0, 0, 0] - 0.75) <= 1e-15                           # (0.25 + 2.25 / 3) / (4/3)


def test_a_constant_added_to_all_returns_changes_nothing():
    mean, var, actions, cand = _data(1)
    for relative in (False, True):
        a = mppi_ref.mppi_update(mean, var, actions, cand, 0.9, relative)
        b = mppi_ref.mppi_update(mean, var, actions, cand + 1000.0, 0.9, relative)
        for x, y in zip(a, b):
            np.testing.assert_allclose(x, y, rtol=0, atol=1e-11)      # (1000 + R rounds R to 1e-13: 1e-13 / lambda on a weight)


def test_relative_is_invariant_to_a_positive_scale_of_the_returns():
    mean, var, actions, cand = _data(2)
    a = mppi_ref.mppi_update(mean, var, actions, cand, 0.2, True)
    for scale in (1e-3, 8.0, 1e6):                                    # (8: exact; the others to rounding)
        b = mppi_ref.mppi_update(mean, var, actions, cand * scale, 0.2, True)
        for x, y in zip(a, b):
            np.testing.assert_allclose(x, y, rtol=0, atol=1e-13)
    c = mppi_ref.mppi_update(mean, var, actions, cand * 8.0, 0.2, False)      # the absolute form is not
    assert np.abs(c[0] - mppi_ref.mppi_update(mean, var, actions, cand, 0.2, False)[0]).max() > 1e-3


def test_a_far_best_candidate_is_the_mean():
    """Every other candidate >= 200 lambda below the best: their weights are below exp(-200) = 1.4e-87, mu is the best sequence."""
    mean, var, actions, cand = _data(3)
    lam = 0.05
    best = np.array([5, 30])
    cand = np.minimum(cand, 0.0) - 200.0 * lam
    cand[np.arange(M), best] = 0.0
    nm, nv, _ = mppi_ref.mppi_update(mean, var, actions, cand, lam, alpha=0.0)
    np.testing.assert_array_equal(nm, actions[np.arange(M), best])
    assert nv.max() <= 1e-80


def test_non_finite_returns_are_ignored():
    mean, var, actions, cand = _data(4)
    bad = cand.copy()
    bad[0, [1, 7, 20]] = [np.nan, np.inf, -np.inf]
    keep = np.setdiff1d(np.arange(N), [1, 7, 20])
    for relative in (False, True):
        got = mppi_ref.mppi_update(mean, var, actions, bad, 0.8, relative)
        want0 = mppi_ref.mppi_update(mean[:1], var[:1], actions[:1, keep], cand[:1, keep], 0.8, relative)
        want1 = mppi_ref.mppi_update(mean[1:], var[1:], actions[1:], cand[1:], 0.8, relative)
        for g, w0, w1 in zip(got, want0, want1):
            np.testing.assert_allclose(g[0], w0[0], rtol=0, atol=1e-15)
            np.testing.assert_array_equal(g[1], w1[0])
    # an env whose returns are all NaN keeps its distribution; the other env is unaffected
    bad = cand.copy()
    bad[1] = np.nan
    nm, nv, plan = mppi_ref.mppi_update(mean * 3.0, var, actions, bad, 0.8)
    np.testing.assert_array_equal(nm[1], mean[1] * 3.0)
    np.testing.assert_array_equal(nv[1], var[1])
    np.testing.assert_array_equal(plan[1], np.clip(mean[1] * 3.0, -1.0, 1.0))
    assert np.abs(plan[1]).max() == 1.0
    np.testing.assert_array_equal(nm[0], mppi_ref.mppi_update(mean[:1] * 3.0, var[:1], actions[:1], cand[:1], 0.8)[0][0])


def test_generic_over_dtype():
    mean, var, actions, cand = (x.astype(np.float32) for x in _data(5))
    nm, nv, plan = mppi_ref.mppi_update(mean, var, actions, cand, 1.5)
    assert nm.dtype == nv.dtype == plan.dtype == np.float32
    ref = mppi_ref.mppi_update(*(x.astype(np.float64) for x in (mean, var, actions, cand)), 1.5)
    assert np.abs(nm - ref[0]).max() <= 1e-5 and np.abs(nv - ref[1]).max() <= 1e-5


def test_top_elites_order_and_ties():
    cand = np.array([[1.0, 3.0, 3.0, -2.0, 3.0, 0.5]])
    np.testing.assert_array_equal(mppi_ref.top_elites(cand, 4), [[1, 2, 4, 0]])


def test_loop_runs_on_the_icem_cases():
    """`mppi_loop` on one whole-loop case of icem_ref: the schedule, the carried elites and the mean candidate are icem_loop's; a tiny
    temperature refits towards the best candidate of each iteration."""
    from helpers import oracle_problem
    case = (6, True, 1.0, 1.5)
    c = icem_ref.LOOP
    prob, z, xi, carry, valid = icem_ref.loop_case(case)
    o = oracle_problem(prob, np.float64)
    kw = dict(noise_beta=case[2], K=c["K"], decay=case[3], add_mean_last=True, z=z, xi=xi, carry=carry.astype(np.float64), carry_valid=valid)
    plan, info, ncarry, nvalid = mppi_ref.mppi_loop(o, c["E"], c["p"], c["n"], c["iters"], c["num_elites"], temperature=0.5, relative=True, **kw)
    assert plan.shape == (c["m"], 6, prob["A"]) and np.isfinite(plan).all() and np.abs(plan).max() <= 1.0
    assert [x["actions"].shape[1] for x in info] == [64, 42, 28]
    np.testing.assert_array_equal(info[0]["actions"][1, :c["K"], :-1], carry[1, :, 1:].astype(np.float64))
    np.testing.assert_array_equal(info[-1]["actions"][:, :c["K"]], info[-2]["kept"])
    np.testing.assert_array_equal(info[-1]["actions"][:, c["K"]], np.clip(info[-2]["mean"], -1.0, 1.0))
    np.testing.assert_array_equal(ncarry, info[-1]["kept"])
    np.testing.assert_array_equal(nvalid, [1, 1])
    # the first iteration sees the same candidates as the CEM loop (same draws, same carry) and ranks the same elites
    ref = icem_ref.icem_loop(o, c["E"], c["p"], c["n"], c["iters"], c["num_elites"], **kw)
    np.testing.assert_array_equal(info[0]["elites"], ref[1][0]["elites"])
    assert not np.array_equal(info[0]["mean"], ref[1][0]["mean"])
    sharp = mppi_ref.mppi_loop(o, c["E"], c["p"], c["n"], 1, c["num_elites"], temperature=1e-6, relative=True, alpha=0.0, **dict(kw, add_mean_last=False))
    first = sharp[1][0]
    np.testing.assert_allclose(first["mean"], first["actions"][np.arange(c["m"]), first["elites"][:, 0]], rtol=0, atol=1e-12)


def test_new_exports_are_bound_and_refuse_null_arguments_without_a_gpu():
    import os
    from cadm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cadm_mppi_refit", "cadm_mppi_plan", "cadm_mppi_workspace_bytes"):
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in _lib.SIGNATURES, "%s is not bound" % name
    assert [f[0] for f in _lib.MppiParams._fields_] == ["icem", "temperature", "relative"]
    assert ctypes.sizeof(_lib.MppiParams) == ctypes.sizeof(_lib.IcemParams) + 8
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    prm = _lib.MppiParams()
    prm.temperature = 1.0
    calls = {
        "cadm_mppi_refit": lambda: lib.cadm_mppi_refit(None, P, P, 1, 1, 1.0, 0, P, P, None, None),
        "cadm_mppi_plan": lambda: lib.cadm_mppi_plan(None, ctypes.byref(prm), P, None, None, P, P, None, None, 1, 1, 0, 0, P, P, None, None),
    }
    for name, fn in calls.items():
        assert fn() == -1, name
        assert lib.cadm_last_error().decode().startswith(name + ":"), name
    assert lib.cadm_mppi_plan(None, None, P, None, None, P, P, None, None, 1, 1, 0, 0, P, P, None, None) == -1
    assert lib.cadm_mppi_workspace_bytes(None, 1, 1, 0) == 0
