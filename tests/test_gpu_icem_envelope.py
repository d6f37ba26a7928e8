"""GPU: the iCEM planner (csrc/icem.hip) off the one geometry of tests/test_gpu_icem.py: short and long horizons, A != 6, sequence counts
that are no multiple of 64, bounds other than +-1, the grid-stride path of keep / inject, one CEM iteration, the floor and the cap of the
candidate schedule, other envs, and non-finite returns.

Everything runs on hidden (32,) * 4 (zero-padded on the compiled-in 128-wide kernel: no on-demand build), ensemble 5, particles 5,
trained-like weights.  Numpy restatements: tests/icem_ref.py, used at float64.  Bars: 1e-5 absolute on actions, means and plans;
helpers.assert_close at 1e-5 on returns; "bit for bit" where the text says so."""
import ctypes as ct

import numpy as np
import pytest
import torch

import icem_ref
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import make_engine

pytestmark = pytest.mark.gpu

HID = (32,) * 4
KE, K, ITERS = 8, 3, 3
BOUNDS = [(-1.0, 1.0), (-0.5, 2.0), (0.25, 0.75)]      # (the last two: tests/test_gpu_cem_constants.py BOUNDS)
NAN = np.float32(np.nan)


def _np(t):
    return t.detach().cpu().numpy()


def _engine(H, env="halfcheetah", context=False, m=2, seed=3, **kw):
    prob = synth.make_problem(env=env, context=context, E=5, m=m, H=H, seed=seed, hidden_sizes=HID, trained_like=True)
    kw.setdefault("num_elites", KE)
    kw.setdefault("num_cem_iters", ITERS)
    return prob, make_engine(prob, p=5, **kw)


def _mean_var(rng, m, H, A, lo, hi):
    """Means inside the bounds, ON both bounds and outside both; var above and below the bound term, and exactly 0 on some elements."""
    w = hi - lo
    mean = rng.uniform(lo + 0.1 * w, hi - 0.1 * w, (m, H, A)).astype(np.float32)
    var = rng.uniform(0.01 * w * w, 0.05 * w * w, (m, H, A)).astype(np.float32)
    f = mean.reshape(-1)
    f[0], f[1 % f.size], f[2 % f.size], f[3 % f.size] = lo, hi, lo - 0.3 * w, hi + 0.2 * w
    v = var.reshape(-1)
    v[4 % v.size], v[5 % v.size] = 0.0, 3.0 * w * w
    v[-1] = 0.0
    return mean, var


# ---------------------------------------------------------------------------------------------------------------------- 1
SAMPLER = [("halfcheetah", 2), ("halfcheetah", 3), ("halfcheetah", 4), ("pendulum", 5), ("ant", 5), ("slim_humanoid", 5)]


@pytest.mark.parametrize("lo,hi", BOUNDS, ids=["%g_%g" % b for b in BOUNDS])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("env,H", SAMPLER, ids=["%s-H%d" % s for s in SAMPLER])
def test_colored_sampler_injected(gpu, env, H, m, lo, hi):
    """`cadm_sample_actions_colored` on injected draws against the float64 restatement, every element <= 1e-5: H = 2 (Nyquist term, no
    pair), 3 (one pair), 4 (both); A = 1, 8, 17; n = 37, so that m n A is no multiple of 64 (threads pass the barrier idle) except by
    accident of A; three bounds; means on and outside the bounds; var = 0, where the action is exactly clip(mean).
    Measured on an MI355X, worst over the 36 cases: 2.1e-07."""
    n, beta = 37, 1.5
    prob, eng = _engine(H, env=env, m=m, lower_bound=lo, upper_bound=hi)
    A = prob["A"]
    rng = np.random.default_rng(1000 * H + 10 * A + m)
    mean, var = _mean_var(rng, m, H, A, lo, hi)
    xi = rng.standard_normal((m, n, A, H)).astype(np.float32)
    got = _np(eng.sample_actions_colored(mean, var, n, beta, xi=xi))
    ref = icem_ref.colored_actions(mean, var, xi, beta, lower=lo, upper=hi)
    err = np.abs(got - ref).max()
    print("\n[%s H=%d m=%d bounds (%g, %g)] m n A = %d: max abs %.2e" % (env, H, m, lo, hi, m * n * A, err))
    assert got.shape == (m, n, H, A) and got.min() >= np.float32(lo) and got.max() <= np.float32(hi)
    assert err <= 1e-5
    zero = np.broadcast_to((var == 0.0)[:, None], got.shape)
    assert zero.any()
    np.testing.assert_array_equal(got[zero], np.broadcast_to(np.clip(mean, np.float32(lo), np.float32(hi))[:, None], got.shape)[zero])
    if mean.size > 6:      # (pendulum at m = 1 has 5 elements: every one of them is a planted edge)
        assert np.abs(got - np.clip(mean, lo, hi)[:, None]).max() > 0.05 * (hi - lo)      # elsewhere the noise is there


@pytest.mark.parametrize("H", [2, 3, 4])
def test_colored_sampler_device_rng_short_horizons(gpu, H):
    """The device's own draws at H = 2, 3, 4 -- three different maps from Philox counters to spectral slots -- against the float64
    synthesis of the restated draws (tests/test_icem_ref.py holds their slot layout to the kernel's comment), m n A = 3 x 37 x 6.
    Measured on an MI355X: 9.4e-08 (H = 2), 2.0e-07 (H = 3), 1.3e-07 (H = 4)."""
    m, n, beta, seed, call, it = 3, 37, 1.5, 11, 5, 2
    prob, eng = _engine(H, m=m)
    A = prob["A"]
    mean, var = _mean_var(np.random.default_rng(H), m, H, A, -1.0, 1.0)
    got = _np(eng.sample_actions_colored(mean, var, n, beta, seed=seed, call=call, it=it))
    ref = icem_ref.colored_actions(mean, var, icem_ref.spectral_draws(seed, call, it, m, n, A, H), beta)
    err = np.abs(got - ref).max()
    print("\n[H=%d] device RNG vs restated draws: max abs %.2e" % (H, err))
    assert err <= 1e-5
    np.testing.assert_array_equal(got, _np(eng.sample_actions_colored(mean, var, n, beta, seed=seed, call=call, it=it)))


@pytest.mark.parametrize("beta", [0.0, 2.5])
@pytest.mark.parametrize("H", [32, 172])
def test_colored_sampler_long_horizon(gpu, H, beta):
    """The kernel's header says accuracy does not depend on H (integer angle reduction, double-precision tables): injected draws at
    H = 32 and H = 172, n = 64, m = 1, held to the same 1e-5.
    Measured on an MI355X: H = 32: 2.9e-07 (beta 0), 3.2e-07 (beta 2.5); H = 172: 4.7e-07, 8.5e-07 -- some 2 - 3 x what a float32 numpy
    evaluation of the same synthesis is off by on the same inputs (1.5e-07, 1.8e-07; 2.0e-07, 3.1e-07; printed by the test): the error
    grows slowly with the number of terms summed, an order of magnitude inside the bar at the longest horizon tried."""
    m, n = 1, 64
    prob, eng = _engine(H, m=m)
    A = prob["A"]
    rng = np.random.default_rng(H + int(beta))
    mean, var = _mean_var(rng, m, H, A, -1.0, 1.0)
    xi = rng.standard_normal((m, n, A, H)).astype(np.float32)
    got = _np(eng.sample_actions_colored(mean, var, n, beta, xi=xi))
    ref = icem_ref.colored_actions(mean, var, xi, beta)
    err = np.abs(got - ref).max()
    f32 = np.abs(icem_ref.colored_actions_f32(mean, var, xi, beta) - ref).max()
    print("\n[H=%d beta=%g] max abs %.2e (a float32 numpy evaluation of the same synthesis: %.2e)" % (H, beta, err, f32))
    assert err <= 1e-5


def test_colored_sampler_refuses_a_horizon_beyond_its_lds(gpu):
    """H = 247 needs 65 708 bytes of LDS (H <= 246 fits 65 536): the sampler and the loop with noise_beta > 0 return CADM_EINVAL naming
    the horizon before any launch; the same engine plans with noise_beta = 0 (white noise needs no LDS)."""
    H, m, n = 247, 1, 16
    prob, eng = _engine(H, m=m)
    lib, ctx = eng.lib, eng._ctx
    buf = torch.zeros(m * n * H * prob["A"], dtype=torch.float32, device=eng.device)
    P = ct.c_void_p(buf.data_ptr())
    assert lib.cadm_sample_actions_colored(ctx, P, P, None, 1.0, 0, 0, 0, m, n, P, None) == -1
    msg = lib.cadm_last_error().decode()
    assert msg.startswith("cadm_sample_actions_colored:") and "horizon" in msg and "LDS" in msg, msg
    with pytest.raises(Exception, match="horizon"):
        eng.icem_plan(HipEngine.icem_params(noise_beta=1.0), prob["obs"], None, None, prob["init_mean"], prob["init_var"], n, seed=1, call=1)
    assert lib.cadm_last_error().decode().startswith("cadm_icem_plan:")
    with pytest.raises(Exception, match="horizon"):
        eng.mppi_plan(HipEngine.mppi_params(noise_beta=1.0), prob["obs"], None, None, prob["init_mean"], prob["init_var"], n, seed=1, call=1)
    assert lib.cadm_last_error().decode().startswith("cadm_mppi_plan:")
    out = _np(eng.icem_plan(HipEngine.icem_params(noise_beta=0.0), prob["obs"], None, None, prob["init_mean"], prob["init_var"], n, seed=1, call=1))
    assert out.shape == (m, H, prob["A"]) and np.isfinite(out).all() and 0 < np.abs(out).max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- 2
def test_keep_inject_grid_stride(gpu):
    """m K H A = 120 x 50 x 30 x 6 = 1 080 000 elements > 4096 x 256: every thread of keep / inject takes a second element."""
    m, n, KK, H = 120, 50, 50, 30
    prob, eng = _engine(H, m=1, num_elites=KK)
    A = prob["A"]
    assert m * KK * H * A > 4096 * 256
    rng = np.random.default_rng(1)
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    el = np.stack([rng.permutation(n) for _ in range(m)]).astype(np.int32)
    ta = eng._t(acts)
    kept = _np(eng.icem_keep(ta, eng._t(el, dtype=torch.int32), KK))
    np.testing.assert_array_equal(kept, acts[np.arange(m)[:, None], el])
    src = rng.uniform(-1, 1, (m, KK, H, A)).astype(np.float32)
    np.testing.assert_array_equal(_np(eng.icem_inject(ta.clone(), eng._t(src))), src)      # (K == n: every slot replaced)
    valid = (rng.uniform(size=m) < 0.5).astype(np.int32)
    assert 0 < valid.sum() < m
    got = _np(eng.icem_inject(ta.clone(), eng._t(src), valid=eng._t(valid, dtype=torch.int32), shift=1))
    want = acts.copy()
    want[valid == 1, :, :H - 1] = src[valid == 1, :, 1:]
    np.testing.assert_array_equal(got, want)


def test_elite_ids_out_of_range_touch_nothing(gpu):
    """Elite ids -1 and n: `icem_keep` leaves the matching rows of a pre-filled buffer alone (and gathers the others); `track_best`
    ends its walk at such an id and leaves best_ret / best_seq as they were, whatever the later elites are."""
    m, n, H = 2, 37, 5
    prob, eng = _engine(H, m=m)
    A = prob["A"]
    rng = np.random.default_rng(2)
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    el = np.stack([rng.permutation(n)[:KE] for _ in range(m)]).astype(np.int32)
    el[0, 0], el[0, 2], el[1, 0], el[1, KE - 1] = -1, n, n, -1
    kept = torch.full((m, KE, H, A), 7.0, dtype=torch.float32, device=eng.device)
    rc = eng.lib.cadm_icem_keep(eng._ctx, ct.c_void_p(eng._t(acts).data_ptr()), ct.c_void_p(eng._t(el, dtype=torch.int32).data_ptr()), m, n, KE,
                                ct.c_void_p(kept.data_ptr()), eng.stream)
    assert rc == 0
    want = acts[np.arange(m)[:, None], np.clip(el, 0, n - 1)]
    want[(el < 0) | (el >= n)] = 7.0
    np.testing.assert_array_equal(_np(kept), want)
    cand = rng.standard_normal((m, n)).astype(np.float32) + np.float32(10.0)      # (every return beats the stored one)
    best_ret, best_seq = eng._t(np.array([0.5, -0.5], np.float32)), eng._t(np.full((m, H, A), 0.25, np.float32))
    eng.icem_track_best(eng._t(cand), eng._t(el, dtype=torch.int32), eng._t(acts), best_ret, best_seq)
    np.testing.assert_array_equal(_np(best_ret), [0.5, -0.5])
    np.testing.assert_array_equal(_np(best_seq), np.full((m, H, A), 0.25, np.float32))


@pytest.mark.parametrize("env,H", [("halfcheetah", 1), ("pendulum", 5)])
def test_inject_shift_at_h1_and_a1(gpu, env, H):
    """shift = 1 at H = 1: every element is the last step, the actions are unchanged.  A = 1, H = 5: steps [0, H - 1) take steps [1, H).
    K = num_elites and K = 1 through keep and inject."""
    m, n = 2, 37
    prob, eng = _engine(H, env=env, m=m)
    A = prob["A"]
    rng = np.random.default_rng(3 + H)
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    el = np.stack([rng.permutation(n)[:KE] for _ in range(m)]).astype(np.int32)
    for KK in (1, KE):
        kept = _np(eng.icem_keep(eng._t(acts), eng._t(el, dtype=torch.int32), KK))
        np.testing.assert_array_equal(kept, acts[np.arange(m)[:, None], el[:, :KK]])
        src = rng.uniform(-1, 1, (m, KK, H, A)).astype(np.float32)
        got = _np(eng.icem_inject(eng._t(acts).clone(), eng._t(src), shift=1))
        want = acts.copy()
        want[:, :KK, :H - 1] = src[:, :, 1:]
        np.testing.assert_array_equal(got, want)
        if H == 1:
            np.testing.assert_array_equal(got, acts)
        got = _np(eng.icem_inject(eng._t(acts).clone(), eng._t(src)))
        np.testing.assert_array_equal(got[:, :KK], src)
        np.testing.assert_array_equal(got[:, KK:], acts[:, KK:])


# ---------------------------------------------------------------------------------------------------------------------- 3
def _carry(eng, m, KK, H, A, valid=None):
    if KK == 0:
        return None, None
    v = torch.zeros((m,), dtype=torch.int32, device=eng.device) if valid is None else eng._t(np.asarray(valid, np.int32), dtype=torch.int32)
    return torch.zeros((m, KK, H, A), dtype=torch.float32, device=eng.device), v


def _both(eng, prob, n, update, call, mean, var, ca, va, cb, vb, want_ret=True, **kw):
    """One call of the fused loop and of the stepwise loop: (plan a, best return a, plan b, info, extra)."""
    args = (prob["obs"], prob["cp_obs"] if prob["cp"] is not None else None, prob["cp_act"] if prob["cp"] is not None else None)
    if update == "mppi":
        prm = HipEngine.mppi_params(temperature=0.5, relative=True, **kw)
        a, ra = eng.mppi_plan(prm, *args, mean, var, n, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
    else:
        a, ra = eng.icem_plan(HipEngine.icem_params(**kw), *args, mean, var, n, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
    b, info, extra = hplanner.icem_plan(eng, *args, mean, var, n, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True, update=update,
                                        temperature=0.5, relative=True, **kw)
    return _np(a), _np(ra), _np(b), info, extra


def _two_calls(eng, prob, n, update="cem", valid=None, lo=-1.0, hi=1.0, **kw):
    """Fused == stepwise, bit for bit, over two consecutive calls (plan, best return, carry); returns the per-call (plan, info, extra,
    carry before the call)."""
    m, H, A, KK = prob["m"], prob["H"], prob["A"], kw.get("keep_elites", 0)
    (ca, va), (cb, vb) = _carry(eng, m, KK, H, A, valid), _carry(eng, m, KK, H, A, valid)
    if KK and valid is not None:
        ca.uniform_(lo, hi)
        cb.copy_(ca)
    mean, var = prob["init_mean"], prob["init_var"]
    out = []
    for call in (1, 2):
        before = None if ca is None else _np(ca).copy()
        a, ra, b, info, extra = _both(eng, prob, n, update, call, mean, var, ca, va, cb, vb, **kw)
        assert a.shape == (m, H, A) and np.isfinite(a).all() and a.min() >= np.float32(lo) and a.max() <= np.float32(hi)
        np.testing.assert_array_equal(a, b, err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(ra, _np(extra["best_ret"]), err_msg="best return of call %d" % call)
        if KK:
            np.testing.assert_array_equal(_np(ca), _np(cb), err_msg="carry after call %d" % call)
            np.testing.assert_array_equal(_np(va), np.ones(m))
        out.append((a, info, extra, before))
        mean = np.concatenate([a[:, 1:], np.zeros((m, 1, A), np.float32)], axis=1)
    return out


@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_one_cem_iteration(gpu, update):
    """num_cem_iters = 1: iteration 0 is also the last -- the carry is read and rewritten, and the mean candidate injected, in the
    same iteration.  Call 2's slots [0, K) hold call 1's carry moved one step on; slot K holds clip(mean)."""
    H, n = 5, 64
    prob, eng = _engine(H, context=True, num_cem_iters=1)
    A = prob["A"]
    calls = _two_calls(eng, prob, n, update, keep_elites=K, add_mean_last=True, noise_beta=1.0, return_best=True)
    (p1, info1, _, _), (p2, info2, _, before2) = calls
    assert len(info1) == len(info2) == 1
    acts2 = _np(info2[0]["actions"])
    np.testing.assert_array_equal(before2, _np(info1[0]["kept"]))
    np.testing.assert_array_equal(acts2[:, :K, :H - 1], before2[:, :, 1:])
    mean2 = np.concatenate([p1[:, 1:], np.zeros((2, 1, A), np.float32)], axis=1)
    np.testing.assert_array_equal(acts2[:, K], np.clip(mean2, -1.0, 1.0))
    np.testing.assert_array_equal(_np(info1[0]["actions"])[:, K], np.clip(prob["init_mean"], -1.0, 1.0).astype(np.float32))


SCHEDULE = [(64, 4.0, [64, 16, 16]), (12, 1.5, [12, 12, 12]), (icem_ref.DECAY_11_N, 1.1, [77, 69, 63])]


@pytest.mark.parametrize("n,decay,counts", SCHEDULE, ids=["floor", "cap", "decay1.1"])
def test_candidate_schedule_floor_cap_and_float32_decay(gpu, n, decay, counts):
    """The 2 num_elites floor (64 -> 16 -> 16 at decay 4), the n cap (n = 12 < 2 num_elites: 12 every iteration) and decay = 1.1, no
    float32 number (n = 77: float64 1.1 would give 70 in iteration 1; tests/test_icem_ref.py): fused == stepwise, whose per-iteration
    candidate counts are asserted.  (A fused loop on another count draws and scores other candidates: another plan, carry and return.)"""
    H = 6
    prob, eng = _engine(H)
    for _, info, _, _ in _two_calls(eng, prob, n, keep_elites=K, decay=decay, add_mean_last=True, noise_beta=1.0):
        assert [x["actions"].shape[1] for x in info] == counts
        assert [eng.icem_candidates(n, decay, it, K) for it in range(ITERS)] == counts


@pytest.mark.parametrize("update", ["cem", "mppi"])
@pytest.mark.parametrize("m,valid", [(1, [1]), (3, [1, 0, 1])])
def test_env_counts_and_mixed_carry_valid(gpu, m, valid, update):
    """m = 1, and m = 3 with carry_valid = [1, 0, 1]: only the flagged envs start from the carry."""
    H, n = 5, 64
    prob, eng = _engine(H, context=True, m=m)
    (p1, info1, _, before1), _ = _two_calls(eng, prob, n, update, valid=valid, keep_elites=K, noise_beta=1.0)
    acts = _np(info1[0]["actions"])
    for mi in range(m):
        same = np.array_equal(acts[mi, :K, :H - 1], before1[mi, :, 1:])
        assert same == bool(valid[mi]), "env %d" % mi


@pytest.mark.parametrize("best", [False, True], ids=["mean", "best"])
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_bounds_through_the_loop(gpu, update, best):
    """Bounds (-0.5, 2.0), a warm start partly outside them, add_mean_last: the mean candidate is clip(mean) and the plan lies inside
    the bounds; under cem_return = "mean" the plan is clip(last mean)."""
    H, n, lo, hi = 6, 64, -0.5, 2.0
    prob, eng = _engine(H, lower_bound=lo, upper_bound=hi)
    prob["init_mean"] = np.random.default_rng(8).uniform(-0.9, 2.4, prob["init_mean"].shape).astype(np.float32)
    for a, info, extra, _ in _two_calls(eng, prob, n, update, valid=[1, 1], lo=lo, hi=hi, keep_elites=K, add_mean_last=True, noise_beta=1.0, return_best=best):
        last_in = _np(info[-2]["mean"])
        np.testing.assert_array_equal(_np(info[-1]["actions"])[:, K], np.clip(last_in, np.float32(lo), np.float32(hi)))
        for x in info:
            assert _np(x["actions"]).min() >= np.float32(lo) and _np(x["actions"]).max() <= np.float32(hi)
        if not best:
            np.testing.assert_array_equal(a, np.clip(_np(info[-1]["mean"]), np.float32(lo), np.float32(hi)))
    assert np.abs(_np(info[-1]["mean"])).max() > 0


@pytest.mark.parametrize("update", ["cem", "mppi"])
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_alpha_through_the_loop(gpu, alpha, update):
    """alpha from the engine config.  alpha = 1: the distribution never moves, the mean plan is clip(init_mean) bit for bit."""
    H, n = 5, 64
    prob, eng = _engine(H, alpha=alpha)
    prob["init_mean"] = np.random.default_rng(9).uniform(-1.3, 1.3, prob["init_mean"].shape).astype(np.float32)
    (a, info, _, _), _ = _two_calls(eng, prob, n, update, noise_beta=1.0)
    if alpha == 1.0:
        np.testing.assert_array_equal(a, np.clip(prob["init_mean"], -1.0, 1.0))
        np.testing.assert_array_equal(_np(info[-1]["var"]), prob["init_var"].astype(np.float32))
    else:
        assert np.abs(_np(info[0]["mean"]) - prob["init_mean"]).max() > 0.05


@pytest.mark.parametrize("update", ["cem", "mppi"])
@pytest.mark.parametrize("env,H", [("pendulum", 5), ("ant", 5), ("slim_humanoid", 3)])
def test_other_envs(gpu, env, H, update):
    """pendulum (H A = 5), ant (40: MPPI's 16-byte loads at A != 6), slim_humanoid (51: its scalar loads): fused == stepwise."""
    prob, eng = _engine(H, env=env, context=True)
    for a, info, _, _ in _two_calls(eng, prob, 64, update, keep_elites=K, decay=1.5, add_mean_last=True, noise_beta=1.0, return_best=update == "cem"):
        assert all(np.isfinite(_np(x["cand"])).all() for x in info)
        assert np.abs(a).max() > 0


# ---------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_a_nan_observation_does_not_leak_across_envs(gpu, update):
    """The same call twice, the second time with env 0's observation NaN (an input the library documents): env 1's plan, carry and best
    return are the same bits.  Env 0, whose returns are all NaN: no best sequence (NaN, and a NaN best return) under either update;
    iCEM, run with cem_return = "best", plans NaN (its elites -- whatever the NaN keys rank as -- have finite sequences, which is what
    it carries); MPPI, run with cem_return = "mean", keeps mean / var in every iteration and plans clip(init_mean)."""
    H, n, m = 5, 64, 2
    prob, eng = _engine(H, context=True, m=m)
    A = prob["A"]
    prob["init_mean"] = np.random.default_rng(5).uniform(-1.2, 1.2, prob["init_mean"].shape).astype(np.float32)
    bad = dict(prob)
    bad["obs"] = prob["obs"].copy()
    bad["obs"][0] = np.nan
    res = []
    for pr in (prob, bad):
        (ca, va), (cb, vb) = _carry(eng, m, K, H, A), _carry(eng, m, K, H, A)
        a, ra, b, info, extra = _both(eng, pr, n, update, 1, prob["init_mean"], prob["init_var"], ca, va, cb, vb, keep_elites=K, noise_beta=1.0,
                                      return_best=update == "cem")
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ra, _np(extra["best_ret"]))
        np.testing.assert_array_equal(_np(ca), _np(cb))
        res.append((a, ra, _np(ca), info, _np(extra["best_seq"])))
    (a0, r0, c0, _, s0), (a1, r1, c1, info, s1) = res
    np.testing.assert_array_equal(a0[1], a1[1])
    np.testing.assert_array_equal(c0[1], c1[1])
    np.testing.assert_array_equal(s0[1], s1[1])
    assert r0[1] == r1[1] and np.isfinite(r1[1]) and np.isfinite(a0).all()
    assert all(np.isnan(_np(x["cand"])[0]).all() and np.isfinite(_np(x["cand"])[1]).all() for x in info)
    assert np.isnan(r1[0]) and np.isnan(s1[0]).all() and np.isfinite(c1).all()
    if update == "cem":
        assert np.isnan(a1[0]).all()
    else:
        np.testing.assert_array_equal(a1[0], np.clip(prob["init_mean"][0], -1.0, 1.0))
        for x in info:
            np.testing.assert_array_equal(_np(x["mean"])[0], prob["init_mean"][0])
            np.testing.assert_array_equal(_np(x["var"])[0], prob["init_var"][0].astype(np.float32))


def test_mixed_returns_through_the_stepwise_exports(gpu):
    """Injected returns, no rollout: n = 37, num_elites = 8, three iterations of refit -> track-best -> keep.

    What `cadm_cem_refit`'s elites_out orders today (pinned, not changed: the reference path rests on it): a positive NaN ranks above
    +inf, then the returns descending, -inf last; `icem_keep` therefore carries NaN-return candidates first (their sequences are finite).

    cem_return = "best": the sequence with the greatest non-NaN return scored in the call, ties to the earliest iteration, then the
    lowest index; NaN only if every return of the call is NaN.  Env 0: one NaN in EVERY iteration (elite 0 each time: with track-best
    reading elite 0 only, the plan was NaN although finite candidates were scored), the best finite return tied between iterations 1
    and 2 and inside iteration 1.  Env 1: NaN, +inf and -inf in iteration 0 (+inf is the greatest non-NaN return), 9 NaN returns in
    iteration 1 (more than num_elites: the arg-max over the candidates), all NaN in iteration 2.  Env 2: every return NaN."""
    m, n, H = 3, 37, 5
    prob, eng = _engine(H, m=m)
    A = prob["A"]
    rng = np.random.default_rng(12)
    cands = [rng.standard_normal((m, n)).astype(np.float32) for _ in range(ITERS)]
    acts = [rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32) for _ in range(ITERS)]
    top = np.float32(5.0)
    cands[0][0, 7] = NAN
    cands[1][0, [3, 20, 30]] = [NAN, top, top]
    cands[2][0, [0, 11]] = [top, NAN]
    cands[0][1, [4, 9, 33]] = [NAN, np.inf, -np.inf]
    cands[1][1, :9] = NAN
    cands[1][1, [15, 22]] = [np.float32(7.0), np.float32(7.0)]
    cands[2][1] = NAN
    for c in cands:
        c[2] = NAN
    best_ret = eng._t(np.full(m, np.nan, np.float32))
    best_seq = eng._t(np.full((m, H, A), np.nan, np.float32))
    rbest, rseq = np.full(m, np.nan, np.float32), np.full((m, H, A), np.nan, np.float32)
    mean, var = eng._t(np.zeros((m, H, A), np.float32)), eng._t(np.full((m, H, A), 0.25, np.float32))
    for it in range(ITERS):
        tc, ta = eng._t(cands[it]), eng._t(acts[it])
        el = eng.cem_refit(tc.unsqueeze(0), ta, mean, var, want_elites=True)
        want_el = np.stack([icem_ref.key_order(cands[it][mi], KE) for mi in range(m)])
        np.testing.assert_array_equal(_np(el), want_el, err_msg="elite order, iteration %d" % it)
        kept = _np(eng.icem_keep(ta, el, K))
        np.testing.assert_array_equal(kept, acts[it][np.arange(m)[:, None], want_el[:, :K]])
        assert np.isfinite(kept).all()
        eng.icem_track_best(tc, el, ta, best_ret, best_seq)
        icem_ref.track_best(cands[it], acts[it], rbest, rseq)
        np.testing.assert_array_equal(_np(best_ret), rbest, err_msg="best return after iteration %d" % it)
        np.testing.assert_array_equal(_np(best_seq), rseq, err_msg="best sequence after iteration %d" % it)
        if it == 0:
            np.testing.assert_array_equal(want_el[0, 0], 7)                     # the NaN is elite 0 ...
            np.testing.assert_array_equal(want_el[1, :2], [4, 9])               # ... ahead of +inf
            assert want_el[1, -1] != 33 and icem_ref.key_order(cands[0][1])[-1] == 33      # -inf ranks last of all
            np.testing.assert_array_equal(rseq[0], acts[0][0, want_el[0, 1]])   # env 0: the best finite candidate, not nothing
    # known answers, spelled out
    got_ret, got_seq = _np(best_ret), _np(best_seq)
    assert got_ret[0] == top
    np.testing.assert_array_equal(got_seq[0], acts[1][0, 20])      # earliest iteration (1, not 2), then the lowest index (20, not 30)
    assert got_ret[1] == np.inf
    np.testing.assert_array_equal(got_seq[1], acts[0][1, 9])
    assert np.isnan(got_ret[2]) and np.isnan(got_seq[2]).all()
    # more than num_elites NaN returns, alone: the arg-max over the candidates, ties to the lower index
    br, bs = eng._t(np.full(m, np.nan, np.float32)), eng._t(np.full((m, H, A), np.nan, np.float32))
    tc, ta = eng._t(cands[1]), eng._t(acts[1])
    el = eng.cem_refit(tc.unsqueeze(0), ta, mean, var, want_elites=True)
    assert np.isnan(cands[1][1][_np(el)[1]]).all()
    eng.icem_track_best(tc, el, ta, br, bs)
    assert _np(br)[1] == np.float32(7.0)
    np.testing.assert_array_equal(_np(bs)[1], acts[1][1, 15])
    # a call whose non-NaN returns are all -inf plans its first such candidate
    low = np.full((m, n), NAN)
    low[:, [6, 8]] = -np.inf
    br, bs = eng._t(np.full(m, np.nan, np.float32)), eng._t(np.full((m, H, A), np.nan, np.float32))
    tc = eng._t(low)
    el = eng.cem_refit(tc.unsqueeze(0), ta, mean, var, want_elites=True)
    eng.icem_track_best(tc, el, ta, br, bs)
    np.testing.assert_array_equal(_np(br), np.full(m, -np.inf, np.float32))
    np.testing.assert_array_equal(_np(bs), acts[1][:, 6])
