"""GPU: the MPPI refit (csrc/mppi.hip, `cadm_mppi_refit`) off the geometry of tests/test_gpu_mppi.py: n below one group and one past a
group, more than 256 groups (the second pass of the weights kernel's W loop), scalar loads with a second element tile, alpha = 0 and 1,
bounds other than +-1, and the ctx-owned scratch buffer made to grow.  (The MPPI loop at other envs, bounds, alpha, one CEM iteration
and a NaN observation: tests/test_gpu_icem_envelope.py, which runs every loop case with both updates.)

halfcheetah (A = 6), hidden (32,) * 4, ensemble 5, particles 5.  Numpy restatement: tests/mppi_ref.py at float64.  Bars: the mean within
1e-5 absolute, the variance within 1e-5 of its largest element -- except at n = 16 448, where the bar is the rounding chain's own bound."""
import numpy as np
import pytest

import mppi_ref
from cadm_amd import synth
from helpers import make_engine

pytestmark = pytest.mark.gpu

HID = (32,) * 4
KE, ITERS, A = 8, 3, 6
BAR = 1e-5


def _np(t):
    return t.detach().cpu().numpy()


def _engine(H, m=2, **kw):
    prob = synth.make_problem(env="halfcheetah", context=False, E=5, m=m, H=H, seed=3, hidden_sizes=HID, trained_like=True)
    return prob, make_engine(prob, p=5, num_elites=KE, num_cem_iters=ITERS, **kw)


def _data(H, n, seed, m=2, lo=-1.0, hi=1.0):
    """Actions in [lo, hi]; returns in [-3, 3] with both ends present where n allows (as tests/test_gpu_mppi.py)."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.7 * lo, 0.7 * hi, (m, H, A)).astype(np.float32)
    var = rng.uniform(0.02, 0.3, (m, H, A)).astype(np.float32)
    actions = rng.uniform(lo, hi, (m, n, H, A)).astype(np.float32)
    cand = rng.uniform(-3.0, 3.0, (m, n)).astype(np.float32)
    if n >= 5:
        cand[:, 3], cand[:, n - 2] = -3.0, 3.0
    return mean, var, actions, cand


def _refit(eng, mean, var, actions, cand, lam, relative):
    tm, tv = eng._t(mean).clone(), eng._t(var).clone()
    plan = eng.mppi_refit(eng._t(cand), eng._t(actions), tm, tv, temperature=lam, relative=relative, want_plan=True)
    return _np(tm), _np(tv), _np(plan)


def _reference(eng, mean, var, actions, cand, lam, relative, lo=-1.0, hi=1.0):
    return mppi_ref.mppi_update(*(np.asarray(x, np.float64) for x in (mean, var, actions, cand)), float(np.float32(lam)), relative,
                                alpha=float(np.float32(eng.cfg.alpha)), lower=lo, upper=hi)


def _errors(got, ref):
    return np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max() / max(np.abs(ref[1]).max(), 1e-30), np.abs(got[2] - ref[2]).max()


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("relative", [False, True], ids=["absolute", "relative"])
@pytest.mark.parametrize("n", [1, 5, 65])
@pytest.mark.parametrize("H", [5, 6])
def test_small_candidate_counts(gpu, H, n, relative):
    """n = 1 and 5 (less than a run / a group), n = 65 (the second group holds one candidate), scalar and 16-byte loads.  n = 1: the
    new mean is the one candidate blended by alpha -- one rounding per product and sum, restated in float32 -- and the variance
    term is exactly 0.  Measured on an MI355X, worst over the 12 cases: mean 1.7e-07; var 2.7e-07 of its largest element."""
    prob, eng = _engine(H)
    mean, var, actions, cand = _data(H, n, 10 * H + n)
    lam = float(np.float32(1.0 / 24.0 if relative else 0.25))
    got = _refit(eng, mean, var, actions, cand, lam, relative)
    em, ev, ep = _errors(got, _reference(eng, mean, var, actions, cand, lam, relative))
    print("\n[H=%d n=%d %s] mean %.2e, var %.2e of its largest element" % (H, n, "relative" if relative else "absolute", em, ev))
    assert em <= BAR and ev <= BAR and ep <= BAR
    if n == 1:
        al = np.float32(eng.cfg.alpha)
        np.testing.assert_array_equal(got[0], mean * al + (np.float32(1.0) - al) * actions[:, 0])
        np.testing.assert_array_equal(got[1], var * al)


N_BIG = 16448
ARG_BIG = 24.0
BAR_BIG = (2 * (15 + (N_BIG + 63) // 64) + 4) * 2.0 ** -24 + ARG_BIG * 2.0 ** -23      # the chain of csrc/mppi.hip's header: 3.5e-5
assert (N_BIG + 63) // 64 == 257 and 3.4e-5 < BAR_BIG < 3.6e-5


@pytest.mark.parametrize("relative", [False, True], ids=["absolute", "relative"])
@pytest.mark.parametrize("H", [5, 6])
def test_more_than_256_groups(gpu, H, relative):
    """n = 16 448 = 257 groups: the weights kernel's W loop takes a second pass (group 256).  m = 1, exponent arguments up to 24.
    Bar: the header's chain, (2 (15 + 257) + 4) 2^-24 + 24 x 2^-23 = 3.5e-5 (1e-5 is not guaranteed at this n), on the mean
    (absolute) and on the variance (of its largest element).  Bit-identical run to run; env 0 of an m = 2 call == the m = 1 call.
    A W that lacks the last group's weights (it holds a best candidate: weight 1) would scale mu and v by ~1e-3, far above the bar.
    Measured on an MI355X, worst over the 4 cases: mean 1.4e-08, var 8.3e-07 of its largest element (the bar: 3.5e-05)."""
    prob, eng = _engine(H, m=1)
    mean, var, actions, cand = _data(H, N_BIG, 40 + H)
    lam = float(np.float32(1.0 / ARG_BIG if relative else 6.0 / ARG_BIG))
    one = _refit(eng, mean[:1], var[:1], actions[:1], cand[:1], lam, relative)
    em, ev, ep = _errors(one, _reference(eng, mean[:1], var[:1], actions[:1], cand[:1], lam, relative))
    print("\n[H=%d n=%d %s] mean %.2e, var %.2e of its largest element (bar %.2e)" % (H, N_BIG, "relative" if relative else "absolute", em, ev, BAR_BIG))
    assert em <= BAR_BIG and ev <= BAR_BIG and ep <= BAR_BIG
    again = _refit(eng, mean[:1], var[:1], actions[:1], cand[:1], lam, relative)
    two = _refit(eng, mean, var, actions, cand, lam, relative)
    for x, y, z in zip(one, again, two):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x[0], z[0])
    # the last group matters: a W without its weights scales v by W / (W - that share), far more than the bar
    w = np.exp((cand[0].astype(np.float64) - 3.0) / (lam * (6.0 if relative else 1.0)))
    assert w[256 * 64:].sum() / w.sum() > 10 * BAR_BIG


def test_scalar_loads_with_a_second_element_tile(gpu):
    """H = 171: H A = 1026 is no multiple of 4 (scalar loads) and the second element tile is 2 wide; n = 130.
    Measured on an MI355X: mean 9.3e-08, var 1.3e-07."""
    H, n = 171, 130
    prob, eng = _engine(H)
    assert (H * A) % 4 != 0 and H * A - 1024 == 2
    mean, var, actions, cand = _data(H, n, 7)
    got = _refit(eng, mean, var, actions, cand, 0.25, False)
    em, ev, ep = _errors(got, _reference(eng, mean, var, actions, cand, 0.25, False))
    print("\n[H=171 n=130] mean %.2e, var %.2e of its largest element" % (em, ev))
    assert em <= BAR and ev <= BAR and ep <= BAR
    assert np.abs(got[0][:, -1] - mean[:, -1]).max() > 0.05      # (the 2-wide tile was refitted, not left)


@pytest.mark.parametrize("H", [5, 6])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_refit_alpha_0_and_1(gpu, alpha, H):
    """alpha from the engine config.  alpha = 1: mean and var come back bit-equal to the inputs; alpha = 0: they are mu and v.
    Measured on an MI355X (alpha = 0): mean 4.1e-08, var 1.1e-07."""
    n = 130
    prob, eng = _engine(H, alpha=alpha)
    mean, var, actions, cand = _data(H, n, 50 + H)
    got = _refit(eng, mean, var, actions, cand, 0.25, False)
    if alpha == 1.0:
        np.testing.assert_array_equal(got[0], mean)
        np.testing.assert_array_equal(got[1], var)
        np.testing.assert_array_equal(got[2], np.clip(mean, -1.0, 1.0))
        return
    ref = mppi_ref.mppi_update(*(np.asarray(x, np.float64) for x in (np.zeros_like(mean), np.zeros_like(var), actions, cand)), 0.25, False, alpha=0.0)
    em, ev, ep = _errors(got, ref)
    print("\n[H=%d alpha=0] mean %.2e, var %.2e of its largest element" % (H, em, ev))
    assert em <= BAR and ev <= BAR and ep <= BAR


@pytest.mark.parametrize("H", [5, 6])
def test_refit_with_bounds(gpu, H):
    """Bounds (-2, 2): actions drawn in [-2, 2], the plan clipped to the bounds (a mean pushed outside them is), alpha = 0.5.
    Measured on an MI355X: mean 7.9e-08, var 1.4e-07."""
    n, lo, hi = 130, -2.0, 2.0
    prob, eng = _engine(H, lower_bound=lo, upper_bound=hi, alpha=0.5)
    mean, var, actions, cand = _data(H, n, 60 + H, lo=lo, hi=hi)
    mean[0, 0, 0], mean[1, H - 1, 5] = 9.0, -9.0
    assert np.abs(actions).max() > 1.5
    got = _refit(eng, mean, var, actions, cand, 0.25, False)
    em, ev, ep = _errors(got, _reference(eng, mean, var, actions, cand, 0.25, False, lo, hi))
    print("\n[H=%d bounds (-2, 2)] mean %.2e, var %.2e of its largest element" % (H, em, ev))
    assert em <= BAR and ev <= BAR and ep <= BAR
    assert got[2][0, 0, 0] == 2.0 and got[2][1, H - 1, 5] == -2.0 and np.abs(got[2]).max() == 2.0 and np.abs(got[2]).min() < 1.0
    np.testing.assert_array_equal(got[2], np.clip(got[0], np.float32(lo), np.float32(hi)))


def test_scratch_growth(gpu):
    """One engine: refit at n = 64, at n = 1030 (the ctx frees its scratch buffer and allocates a larger one), at n = 64 again: the
    first and third results are the same bits, and a fresh engine's."""
    H = 6
    prob, eng = _engine(H)
    small, big = _data(H, 64, 1), _data(H, 1030, 2)
    first = _refit(eng, *small, 0.25, False)
    grown = _refit(eng, *big, 0.25, False)
    third = _refit(eng, *small, 0.25, False)
    _, fresh_eng = _engine(H)
    fresh = _refit(fresh_eng, *small, 0.25, False)
    for x, y, z in zip(first, third, fresh):
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, z)
    em, ev, ep = _errors(grown, _reference(eng, *big, 0.25, False))
    assert em <= BAR and ev <= BAR and ep <= BAR
    np.testing.assert_array_equal(grown[0], _refit(fresh_eng, *big, 0.25, False)[0])
