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


@pytest.mark.parametrize("H", [2, 3, 4])
def test_spectral_slot_layout_at_short_horizons(H):
    """The slot layout of the restated draws at H = 2 (x_0 and the Nyquist draw, no pair), 3 (x_0 and one pair) and 4 (x_0, one pair,
    the Nyquist draw) is the one csrc/icem.hip states: x_0 in slot 0, (x_k, y_k) at (2k - 1, 2k), the Nyquist draw in slot H - 1.  The
    draw of counter k is restated here from oracle/philox.py on its own."""
    from oracle import philox
    seed, call, it, m, n, A = 5, 2, 1, 2, 7, 3
    got = icem_ref.spectral_draws(seed, call, it, m, n, A, H).reshape(m * n * A, H)
    q = np.arange(m * n * A, dtype=np.uint64)
    lo, hi = q.astype(np.uint32), np.zeros(q.shape, np.uint32)

    def draw(k):
        r = philox.philox4x32_10(philox._ctr(lo, np.uint32(k), hi, np.uint32(icem_ref.STREAM_ICEM | (it << 8))), philox._key(seed, call, q.shape))
        return philox.box_muller(philox.u01(r[..., 0]), philox.u01(r[..., 1]))
    want = {2: [draw(0)[0], draw(1)[0]], 3: [draw(0)[0], draw(1)[0], draw(1)[1]], 4: [draw(0)[0], draw(1)[0], draw(1)[1], draw(2)[0]]}[H]
    for slot, w in enumerate(want):
        np.testing.assert_array_equal(got[:, slot], w, err_msg="slot %d" % slot)
    assert len({tuple(got[:, s]) for s in range(H)}) == H      # (no slot repeats another)
    # and the synthesis reads them that way: slot 0 weighs every step alike, the Nyquist slot alternates, a pair turns with t
    S = icem_ref.synthesis_matrix(H, 1.0)
    assert np.ptp(S[:, 0]) == 0.0
    if H % 2 == 0:
        np.testing.assert_array_equal(np.sign(S[:, H - 1]), np.where(np.arange(H) % 2 == 0, 1.0, -1.0))
        assert np.ptp(np.abs(S[:, H - 1])) == 0.0
    if H > 2:
        th = 2.0 * np.pi * np.arange(H) / H
        np.testing.assert_allclose(S[:, 1] / np.hypot(S[0, 1], S[0, 2]), np.cos(th), rtol=0, atol=1e-15)
        np.testing.assert_allclose(S[:, 2] / np.hypot(S[0, 1], S[0, 2]), -np.sin(th), rtol=0, atol=1e-15)


def test_decay_that_is_no_float32_number():
    """n = icem_ref.DECAY_11_N: floor(n / decay^it) differs between float32(1.1), which the library receives, and float64 1.1 at some
    it < 3, above the 2 num_elites floor -- a loop that used the float64 value would run another candidate count."""
    n, KE, K = icem_ref.DECAY_11_N, 8, 3
    f32 = [int(np.floor(n / float(np.float32(1.1)) ** it)) for it in range(3)]
    f64 = [int(np.floor(n / 1.1 ** it)) for it in range(3)]
    assert f32 != f64 and min(f32 + f64) > 2 * KE and max(f32 + f64) <= n
    assert [icem_ref.n_candidates(n, 1.1, it, KE, K) for it in range(3)] == f32 == [77, 69, 63]
    assert f64 == [77, 70, 63]


def test_key_order_and_best_candidate_with_non_finite_returns():
    """The elite order of the device (make_key) ranks a positive NaN above +inf; the best candidate of an iteration is the greatest
    non-NaN return, ties to the lower index."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    cand = np.array([1.0, nan, 3.0, inf, -inf, 3.0, -0.0, 0.0], np.float32)
    np.testing.assert_array_equal(icem_ref.key_order(cand), [1, 3, 2, 5, 0, 6, 7, 4])
    np.testing.assert_array_equal(icem_ref.key_order(cand, 3), [1, 3, 2])
    np.testing.assert_array_equal(icem_ref.key_order(np.array([-nan, 2.0, -inf], np.float32).view(np.float32)), [1, 2, 0])
    assert icem_ref.best_candidate(cand) == 3
    assert icem_ref.best_candidate(np.array([nan, 2.0, nan, 2.0], np.float32)) == 1
    assert icem_ref.best_candidate(np.array([nan, -0.0, 0.0], np.float32)) == 1
    assert icem_ref.best_candidate(np.array([nan, -inf], np.float32)) == 1
    assert icem_ref.best_candidate(np.array([nan, nan], np.float32)) == -1
    # over iterations: a tie keeps the earlier sequence; NaN never replaces; -inf replaces "nothing yet"
    acts = np.arange(2 * 4 * 1 * 1, dtype=np.float32).reshape(2, 4, 1, 1)
    br, bs = np.full(2, np.nan, np.float32), np.full((2, 1, 1), np.nan, np.float32)
    icem_ref.track_best(np.array([[nan, 1.0, 1.0, 0.5], [nan, nan, -inf, nan]], np.float32), acts, br, bs)
    np.testing.assert_array_equal(br, [1.0, -inf])
    np.testing.assert_array_equal(bs[:, 0, 0], [1.0, 6.0])
    icem_ref.track_best(np.array([[1.0, nan, 0.0, 0.0], [nan, nan, nan, nan]], np.float32), acts, br, bs)
    np.testing.assert_array_equal(bs[:, 0, 0], [1.0, 6.0])
    icem_ref.track_best(np.array([[1.0, nan, 0.0, 2.0], [-inf, nan, nan, -1e30]], np.float32), acts, br, bs)
    np.testing.assert_array_equal(bs[:, 0, 0], [3.0, 7.0])


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


@pytest.mark.parametrize("case", icem_ref.LOOP_CASES, ids=[icem_ref.case_id(c) for c in icem_ref.LOOP_CASES])
def test_loop_seeds_rank_the_same_in_float32_and_float64(case):
    """The condition of the whole-loop GPU test (tests/test_gpu_icem.py): at the seeds of icem_ref.LOOP_SEEDS the float32 and the
    float64 oracle pick the same elites in the same order in every iteration, and no two of the 9 best returns are closer than
    LOOP_MIN_GAP of the returns' scale."""
    assert case in icem_ref.LOOP_SEEDS
    a = icem_ref.loop_reference(case, np.float32)
    b = icem_ref.loop_reference(case, np.float64)
    lower, upper = icem_ref.case_env_bounds(case)[1]
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
    prob, z, xi, carry, valid = icem_ref.loop_case(case)
    np.testing.assert_array_equal(first["actions"][1, :c["K"], :-1], carry[1, :, 1:].astype(np.float64))
    assert not np.array_equal(first["actions"][0, :c["K"], :-1], carry[0, :, 1:].astype(np.float64))
    np.testing.assert_array_equal(last["actions"][:, c["K"]], np.clip(b[1][-2]["mean"], lower, upper))
    np.testing.assert_array_equal(last["actions"][:, :c["K"]], b[1][-2]["kept"])
    assert b[0].min() >= lower and b[0].max() <= upper
