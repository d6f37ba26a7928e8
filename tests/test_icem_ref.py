"""CPU: the numpy restatement of the iCEM planner's noise synthesis (tests/icem_ref.py) held to its own maths, and the argument
checks of the new exports that need no ctx."""
import ctypes

import numpy as np
import pytest

import icem_ref

HS = (5, 6, 30)
BETAS = (0.0, 0.5, 2.0)


@pytest.mark.parametrize("H", HS + (1, 2, 3))
def test_white_synthesis_is_orthonormal(H):
    S = icem_ref.synthesis_matrix(H, 0.0)
    assert np.abs(S @ S.T - np.eye(H)).max() <= 1e-12
    assert np.abs(S.T @ S - np.eye(H)).max() <= 1e-12


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("beta", BETAS)
def test_unit_variance_and_lag1_correlation(H, beta):
    S = icem_ref.synthesis_matrix(H, beta)
    cov = S @ S.T
    assert np.abs(np.diag(cov) - 1.0).max() <= 1e-12
    r1 = icem_ref.rho1(H, beta)
    assert np.abs(np.diag(cov, 1) - r1).max() <= 1e-12      # the same for every t
    assert abs(cov[H - 1, 0] - r1) <= 1e-12                  # (the synthesis is circular)
    if beta == 0.0:
        assert abs(r1) <= 1e-12
    else:
        assert r1 > 0.0


def test_beta_orders_the_correlation():
    assert 0.0 < icem_ref.rho1(30, 0.5) < icem_ref.rho1(30, 2.0) < 1.0


def test_h1_is_the_plain_draw():
    assert icem_ref.synthesis_matrix(1, 0.0).shape == (1, 1)
    for beta in BETAS:
        assert abs(icem_ref.synthesis_matrix(1, beta)[0, 0] - 1.0) <= 1e-15


def test_colored_actions_layout_and_clip():
    rng = np.random.default_rng(0)
    m, n, H, A = 2, 3, 5, 4
    mean = rng.uniform(-0.9, 0.9, (m, H, A))
    var = np.full((m, H, A), 4.0)
    xi = rng.standard_normal((m, n, A, H))
    got = icem_ref.colored_actions(mean, var, xi, 1.0)
    assert got.shape == (m, n, H, A) and got.min() >= -1.0 and got.max() <= 1.0
    z = icem_ref.synthesis_matrix(H, 1.0) @ xi[1, 2, 3]
    sd = np.minimum((mean[1, :, 3] + 1.0) / 2.0, (1.0 - mean[1, :, 3]) / 2.0)
    np.testing.assert_allclose(got[1, 2, :, 3], np.clip(mean[1, :, 3] + sd * z, -1.0, 1.0), rtol=0, atol=1e-15)


def test_spectral_draws_are_standard_normal_and_keyed():
    a = icem_ref.spectral_draws(3, 7, 1, 2, 64, 6, 6)
    assert a.shape == (2, 64, 6, 6) and a.dtype == np.float32
    np.testing.assert_array_equal(a, icem_ref.spectral_draws(3, 7, 1, 2, 64, 6, 6))
    assert not np.array_equal(a, icem_ref.spectral_draws(3, 7, 2, 2, 64, 6, 6))
    assert not np.array_equal(a, icem_ref.spectral_draws(3, 8, 1, 2, 64, 6, 6))
    N = a.size
    assert abs(a.mean()) <= 4.0 / np.sqrt(N) and abs(a.var() - 1.0) <= 4.0 * np.sqrt(2.0 / N)
    odd = icem_ref.spectral_draws(3, 7, 1, 2, 64, 6, 5)
    np.testing.assert_array_equal(odd[..., :4], a[..., :4])      # slots x_0, (x_1, y_1), x_2 share counters; y_2 / the Nyquist slot differ
    assert not np.array_equal(odd[..., 4], a[..., 5])


def test_candidate_schedule():
    assert [icem_ref.n_candidates(64, 1.5, it, 8, 3) for it in range(4)] == [64, 42, 28, 18]
    assert [icem_ref.n_candidates(64, 4.0, it, 8, 3) for it in range(3)] == [64, 16, 16]
    assert icem_ref.n_candidates(10, 1.0, 0, 8, 3) == 10      # never more than the workspace holds
    assert icem_ref.n_candidates(200, 1.25, 4, 50, 15) == 100


def test_new_exports_refuse_null_arguments_without_a_gpu():
    import os
    from cadm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P = ctypes.c_void_p(ctypes.addressof(buf))
    prm = _lib.IcemParams()
    calls = {
        "cadm_sample_actions_colored": lambda: lib.cadm_sample_actions_colored(None, P, P, None, 1.0, 0, 0, 0, 1, 1, P, None),
        "cadm_icem_keep": lambda: lib.cadm_icem_keep(None, P, P, 1, 1, 1, P, None),
        "cadm_icem_inject": lambda: lib.cadm_icem_inject(None, P, None, 1, 1, 1, 0, P, None),
        "cadm_icem_track_best": lambda: lib.cadm_icem_track_best(None, P, P, P, 1, 1, P, P, None),
        "cadm_icem_plan": lambda: lib.cadm_icem_plan(None, ctypes.byref(prm), P, None, None, P, P, None, None, 1, 1, 0, 0, P, P, None, None),
    }
    for name, fn in calls.items():
        assert fn() == -1, name
        assert lib.cadm_last_error().decode().startswith(name + ":"), name
    assert lib.cadm_icem_workspace_bytes(None, 1, 1, 0) == 0


@pytest.mark.parametrize("case", icem_ref.LOOP_CASES, ids=["H%d-%s-beta%g-decay%g" % (c[0], "cadm" if c[1] else "vanilla", c[2], c[3]) for c in icem_ref.LOOP_CASES])
def test_loop_seeds_rank_the_same_in_float32_and_float64(case):
    """The condition of the whole-loop GPU test (tests/test_gpu_icem.py): at the seeds of icem_ref.LOOP_SEEDS the float32 and the
    float64 oracle pick the same elites in the same order in every iteration, and no two of the 9 best returns are closer than
    LOOP_MIN_GAP of the returns' scale."""
    assert case in icem_ref.LOOP_SEEDS
    a = icem_ref.loop_reference(*case, np.float32)
    b = icem_ref.loop_reference(*case, np.float64)
    c = icem_ref.LOOP
    ns = [icem_ref.n_candidates(c["n"], case[3], it, c["num_elites"], c["K"]) for it in range(c["iters"])]
    assert ns == ([64, 42, 28] if case[3] == 1.5 else [64, 64, 64])
    for it, (x, y) in enumerate(zip(a[1], b[1])):
        np.testing.assert_array_equal(x["elites"], y["elites"], err_msg="iteration %d" % it)
        top = -np.sort(-y["cand"], axis=1)[:, :c["num_elites"] + 1]
        assert np.abs(np.diff(top, axis=1)).min() > icem_ref.LOOP_MIN_GAP * np.abs(y["cand"]).max()
        assert y["actions"].shape[1] == ns[it]
    assert np.abs(a[0] - b[0]).max() <= 1e-5
    # env 1 started from carried elites (moved one step on), env 0 did not; the last iteration holds the clipped mean in slot K
    first, last = b[1][0], b[1][-1]
    prob, z, xi, carry, valid = icem_ref.loop_case(*case)
    np.testing.assert_array_equal(first["actions"][1, :c["K"], :-1], carry[1, :, 1:].astype(np.float64))
    assert not np.array_equal(first["actions"][0, :c["K"], :-1], carry[0, :, 1:].astype(np.float64))
    np.testing.assert_array_equal(last["actions"][:, c["K"]], np.clip(b[1][-2]["mean"], -1.0, 1.0))
    np.testing.assert_array_equal(last["actions"][:, :c["K"]], b[1][-2]["kept"])
