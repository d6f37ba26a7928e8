"""GPU: the plan forecast -- the statistics kernel (cadm_forecast_stats) on synthetic trajectories, its divergence rule and rewards,
the composite (cadm_plan_forecast) against the oracle's trajectory, the refusals, and the classes' forecast / return_forecast.

Shapes: (a) hopper_like D = 11, p = 5, E = 5, H = 3, m = 3, n = 2 -- one particle per member, an odd D, spans of 55 floats that leave
16-byte alignment; (b) halfcheetah D = 18, p = 20, E = 5, H = 8, m = 2, n = 1; (c) E = 1, p = 4; (d) p = 1.  The composite runs
halfcheetah with context at E = 5, p = 10, H = 8, m = 3, n = 2 (the compiled-in 200 x 4 kernel) and hopper_like, both with injected
noise.
At the kernel's size limits (section 6): the last p its LDS carve accepts and the first it refuses, for halfcheetah (p = 323 / 324: the
per-particle loops take a second stride of the 256 threads) and slim_humanoid (p = 133 / 134); particles that agree, wholly and
inside a member; order statistics full of ties.  Ant, slim_humanoid and pendulum: tests/test_gpu_behind_rollout_envs.py.

Bounds of the isolated kernel, from its particle-0 form (every deviation x_j - x_0 - mean carries at most p + 2 roundings of size
2^-24 R, R = max_j |x_j - x_0|): means within (p + 4) 2^-24 max_j |x_j| of float64, variances within 4 (p + 4) 2^-24 R^2."""
import ctypes as ct

import numpy as np
import pytest
import torch

from cadm_amd import _lib, synth
from cadm_amd._lib import ptr
from cadm_amd.env_spec import EnvDecl
from behind_rollout import synth_traj
from forecast_ref import forecast_ref, reward_bound, step_rewards
from helpers import make_engine, oracle_problem, spec_oracle
from oracle import envs as oenvs
from oracle import nets as onets
from oracle import planner as oplanner

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
VARS = ("var_total", "var_epistemic", "var_aleatoric")
STATE = ("mean", "member_mean") + VARS + ("lo", "hi")
REWARD = ("reward_mean", "reward_var", "reward_member", "returns")
ALL = STATE + REWARD + ("diverged_step",)


def hopper_like():          # tests/test_gpu_horizon.py's declaration (same geometry: one JIT module serves both files)
    return EnvDecl(11, 3, preproc=["drop", "sincos", "id", "id", "sincos", "id", "id", "id", "id", "id", "id"],
                   postproc=["add"] * 5 + ["replace"] + ["add"] * 5,
                   reward=[dict(kind="linear", dim=5), dict(kind="square", dim=3, w=-0.5, when="next_obs"),
                           dict(kind="abs", dim=10, w=-0.1), dict(kind="inside", dim=0, w=1.0, lo=-0.5, hi=0.5, when="next_obs"),
                           dict(kind="outside", dim=2, w=-1.0, lo=-0.2, hi=0.2), dict(kind="linear", dim=4, w=0.3, when="next_obs"),
                           dict(kind="square", dim=7, w=-0.05), dict(kind="abs", dim=6, w=0.2, when="next_obs"),
                           dict(kind="outside", dim=9, w=-0.5, lo=-1.0, hi=1.0, when="next_obs"),
                           dict(kind="inside", dim=8, w=0.25, lo=-0.3, hi=0.8)],
                   ctrl_cost=0.001, bonus=1.0)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def hc(gpu):
    """halfcheetah with context, E = 5, p = 10, engine horizon 8: the isolated kernel's (b), (c), (d) and the composite."""
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=3, H=8, seed=51)
    eng = make_engine(prob, p=10)
    yield prob, eng
    eng.close()


@pytest.fixture(scope="module")
def hop(gpu):
    """hopper_like (tests/test_gpu_horizon.py's declaration) with context, E = 5, p = 5, engine horizon 3: shape (a)."""
    spec = hopper_like()
    prob = synth.make_problem(env=spec, context=True, E=5, m=3, H=3, seed=52)
    eng = make_engine(prob, p=5)
    yield spec, prob, eng
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 1
def check_state_stats(got, traj, E, what):
    H, m, n, p, D = traj.shape
    ref = forecast_ref(traj, np.zeros((m, D), np.float32), np.zeros((m, n, H, 1), np.float32), E)
    x = np.transpose(traj.astype(np.float64), (1, 2, 0, 3, 4))                    # [m,n,H,p,D]
    bm = (p + 4) * U24 * np.abs(x).max(3)
    bv = 4 * (p + 4) * U24 * np.abs(x - x[:, :, :, :1]).max(3) ** 2
    worst = {}
    for k in ("mean", "member_mean"):
        err = np.abs(got[k] - ref[k])
        worst[k] = (err / bm).max()
        assert (err <= bm).all(), "%s %s: worst |err| / bound %.3f" % (what, k, worst[k])
    for k in VARS:
        err = np.abs(got[k] - ref[k])
        worst[k] = (err / np.maximum(bv, 1e-300)).max() if bv.max() > 0 else 0.0
        assert (err <= bv).all(), "%s %s: worst |err| / bound %.3f" % (what, k, worst[k])
    ident = np.abs(got["var_total"].astype(np.float64) - (got["var_epistemic"].astype(np.float64) + got["var_aleatoric"]))
    worst["identity"] = (ident / np.maximum(2 * bv, 1e-300)).max() if bv.max() > 0 else 0.0
    assert (ident <= 2 * bv).all(), "%s: total = epistemic + aleatoric, worst |err| / bound %.3f" % (what, worst["identity"])
    print("%s: worst |err| / bound %s" % (what, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert (got["diverged_step"] == H).all()


def check_order_stats(eng, traj, obs, acts, E, what):
    p = traj.shape[3]
    srt = np.sort(np.transpose(traj, (1, 2, 0, 3, 4)), axis=3)
    for k in sorted({1, min(2, p), p}):
        got = _np(eng.forecast_stats(traj, obs, acts, band_k=k, E=E))
        assert np.array_equal(_bits(got["lo"]), _bits(srt[:, :, :, k - 1])), "%s: lo, band_k = %d" % (what, k)
        assert np.array_equal(_bits(got["hi"]), _bits(srt[:, :, :, p - k])), "%s: hi, band_k = %d" % (what, k)


def test_statistics_kernel_shape_a(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    check_state_stats(_np(eng.forecast_stats(traj, obs, acts)), traj, 5, "(a) D=11 p=5 E=5")
    check_order_stats(eng, traj, obs, acts, 5, "(a)")


def test_statistics_kernel_shape_b(hc):
    prob, eng = hc
    traj, obs, acts = synth_traj(2, 8, 2, 1, 20, 18, 6)
    got = _np(eng.forecast_stats(traj, obs, acts))
    check_state_stats(got, traj, 5, "(b) D=18 p=20 E=5")
    check_order_stats(eng, traj, obs, acts, 5, "(b)")
    again = _np(eng.forecast_stats(traj, obs, acts))
    for k in ALL:
        assert np.array_equal(_bits(got[k]), _bits(again[k])), "run to run: %s" % k


def test_statistics_kernel_one_member_and_one_particle(hc):
    prob, eng = hc
    traj, obs, acts = synth_traj(3, 3, 2, 2, 4, 18, 6)                               # (c) E = 1, p = 4
    got = _np(eng.forecast_stats(traj, obs, acts, E=1))
    check_state_stats(got, traj, 1, "(c) E=1 p=4")
    check_order_stats(eng, traj, obs, acts, 1, "(c)")
    assert (got["var_epistemic"] == 0).all()
    traj, obs, acts = synth_traj(4, 3, 2, 2, 1, 18, 6)                               # (d) p = 1
    got = _np(eng.forecast_stats(traj, obs, acts, E=1))
    x = np.transpose(traj, (1, 2, 0, 3, 4))[:, :, :, 0]
    for k in VARS + ("reward_var",):
        assert (got[k] == 0).all(), "(d) %s is not exactly 0" % k
    for k in ("mean", "lo", "hi"):
        assert np.array_equal(_bits(got[k]), _bits(x)), "(d) %s differs from the input bits" % k
    assert np.array_equal(_bits(got["member_mean"][0]), _bits(x))


# ---------------------------------------------------------------------------------------------------------------------- 2
def test_divergence(hop):
    spec, prob, eng = hop
    clean, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    base = _np(eng.forecast_stats(clean, obs, acts))
    planted = clean.copy()
    planted[1, 0, 1, 3, 7] = np.inf            # sequence (0, 1) at step 1
    planted[2, 2, 0, 0, 0] = np.nan            # sequence (2, 0) at step 2
    got = _np(eng.forecast_stats(planted, obs, acts))
    want = np.full((3, 2), 3, np.int32)
    want[0, 1], want[2, 0] = 1, 2
    np.testing.assert_array_equal(got["diverged_step"], want)
    for k in STATE + REWARD:
        g, b = got[k], base[k]
        if k in ("member_mean", "reward_member"):                                  # [E, m, n, ...] -> [m, n, E, ...]
            g, b = np.moveaxis(g, 0, 2), np.moveaxis(b, 0, 2)
        for mi in range(3):
            for ni in range(2):
                d = want[mi, ni]
                if k == "returns":
                    assert np.isnan(g[mi, ni]).all() if d < 3 else np.array_equal(_bits(g[mi, ni]), _bits(b[mi, ni])), (k, mi, ni)
                    continue
                gs, bs = (g[mi, ni][:, :d], b[mi, ni][:, :d]) if k in ("member_mean", "reward_member") else (g[mi, ni][:d], b[mi, ni][:d])
                ga = g[mi, ni][:, d:] if k in ("member_mean", "reward_member") else g[mi, ni][d:]
                assert np.array_equal(_bits(gs), _bits(bs)), "%s of sequence (%d, %d) before step %d changed" % (k, mi, ni, d)
                assert np.isnan(ga).all(), "%s of sequence (%d, %d) from step %d on is not NaN" % (k, mi, ni, d)


# ---------------------------------------------------------------------------------------------------------------------- 3
def check_rewards(eng, env, terms_env, traj, obs, acts, E, what):
    """Per-particle step rewards r_j: the env's closure on float32 arrays; b_j = `reward_bound` ((T + 3) 2^-23 sum |terms|; pendulum:
    plus its angle's rounding) bounds each of them.
    The kernel's own step rewards are read with E = p: a member of one particle reports that particle's reward bit for bit
    (reward_member), and is held to b_j with nothing added.  With the engine's E, a mean of rewards (reward_mean, reward_member) is
    held to the mean of its particles' b_j, a return to H times the largest b_j of its steps; a variance moves by at most
    mean_j (2 |r_j - rbar| 2 b + (2 b)^2), b = max_j b_j, plus its own rounding 4 (p + 4) 2^-24 R^2 (as for the states)."""
    H, m, n, p, D = traj.shape
    r32 = step_rewards(env, traj, obs, acts)
    b = reward_bound(terms_env, traj, obs, acts)                                     # [m,n,H,p]
    r = r32.astype(np.float64)
    each = _np(eng.forecast_stats(traj, obs, acts, E=p))
    err = np.abs(np.moveaxis(each["reward_member"], 0, 3) - r)
    print("%s per-particle step rewards: worst |err| / bound %.3f, %d of %d bit-equal to the float32 reference"
          % (what, (err / b).max(), (np.moveaxis(each["reward_member"], 0, 3) == r32).sum(), r32.size))
    assert (err <= b).all(), "%s per-particle step rewards: worst |err| / bound %.3f" % (what, (err / b).max())
    got = _np(eng.forecast_stats(traj, obs, acts, E=E))
    ref = forecast_ref(traj, obs, acts, E, rewards=r32)
    lim = dict(reward_mean=b.mean(3), reward_member=np.moveaxis(b.reshape(m, n, H, E, p // E).mean(4), 3, 0), returns=H * b.max(2))
    bmax, R = b.max(3), np.abs(r - r[..., :1]).max(3)
    lim["reward_var"] = (2 * np.abs(r - r.mean(3, keepdims=True)) * 2 * bmax[..., None] + (2 * bmax[..., None]) ** 2).mean(3) + 4 * (p + 4) * U24 * R ** 2
    for k in REWARD:
        err = np.abs(got[k] - ref[k])
        print("%s %s: worst |err| / bound %.3f" % (what, k, (err / lim[k]).max()))
        assert (err <= lim[k]).all(), "%s %s: worst |err| / bound %.3f" % (what, k, (err / lim[k]).max())


def test_rewards_halfcheetah(hc):
    prob, eng = hc
    traj, obs, acts = synth_traj(2, 8, 2, 1, 20, 18, 6)
    check_rewards(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, 5, "halfcheetah (b)")


def test_rewards_declared_env(hop):
    spec, prob, eng = hop
    traj, obs, acts = synth_traj(1, 3, 3, 2, 5, 11, 3)
    traj = (traj * np.float32(0.4)).astype(np.float32)          # values on both sides of the inside / outside thresholds
    r32 = step_rewards(spec, traj, obs, acts)
    assert len({round(float(v), 3) for v in r32.reshape(-1)}) > 50
    check_rewards(eng, spec, spec, traj, obs, acts, 5, "hopper_like (a)")


# ---------------------------------------------------------------------------------------------------------------------- 4
def check_composite(eng, prob, o, env, terms_env, seed, what):
    E, p, H, m, n, D, A = prob["E"], eng.p, eng.H, 3, 2, prob["D"], prob["A"]
    rng = np.random.default_rng(seed)
    acts = rng.uniform(-1, 1, (m, n, H, A)).astype(np.float32)
    eps = rng.standard_normal((H, m, n, p, D)).astype(np.float32)
    got = _np(eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], acts, eps=eps))
    T_ctx = oplanner.context_table_indexed(onets.context_forward(o["cp"], o["cp_obs"], o["cp_act"], o["st"]), 0)
    _, t_ref = oplanner.rollout_indexed(env, o["ff"], o["st"], o["obs"], T_ctx, acts, eps, E, p, False, return_traj=True)
    assert (got["diverged_step"] == H).all()
    ref = forecast_ref(t_ref, o["obs"], acts, E)
    # the project's trajectory bar (helpers.assert_close: every value within 1e-5 max(|x_ref|, rms(x_ref))): a mean of values moves
    # by at most the mean of their deltas; plus the kernel's own rounding of a mean (test 1)
    x = np.transpose(t_ref.astype(np.float64), (1, 2, 0, 3, 4))                   # [m,n,H,p,D]
    dl = 1e-5 * np.maximum(np.abs(x), np.sqrt((x ** 2).mean()))
    rnd = (p + 4) * U24 * np.abs(x).max(3)
    lim = dict(mean=dl.mean(3) + rnd, member_mean=np.moveaxis(dl.reshape(m, n, H, E, p // E, D).mean(4), 3, 0) + rnd[None])
    for k in ("mean", "member_mean"):
        err = np.abs(got[k] - ref[k])
        print("%s %s vs the oracle's trajectory: worst |err| / bound %.3f" % (what, k, (err / lim[k]).max()))
        assert (err <= lim[k]).all(), "%s %s: %d entries outside the trajectory bar, worst |err| / bound %.3f" % (
            what, k, (err > lim[k]).sum(), (err / lim[k]).max())
    # the forecast's rewards account for the return the planner scored
    lim_ret = H * reward_bound(terms_env, t_ref, o["obs"], acts).max(2)
    err = np.abs(got["returns"].astype(np.float64) - got["rollout_returns"])
    print("%s returns vs rollout_returns: worst |err| / bound %.3f" % (what, (err / lim_ret).max()))
    assert (err <= lim_ret).all(), "%s: returns vs rollout_returns, worst |err| / bound %.3f" % (what, (err / lim_ret).max())
    return acts


def test_composite_halfcheetah(hc):
    prob, eng = hc
    acts = check_composite(eng, prob, oracle_problem(prob, np.float32), oenvs.make_env("halfcheetah"), "halfcheetah", 7, "halfcheetah")
    # device noise: the same (seed, call) gives the same bits, another call does not
    a = _np(eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], acts, seed=7, call=3))
    b = _np(eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], acts, seed=7, call=3))
    c = _np(eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], acts, seed=7, call=4))
    for k in ALL + ("rollout_returns",):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), "device noise, same (seed, call): %s differs" % k
    assert not np.array_equal(a["mean"], c["mean"]) and not np.array_equal(a["returns"], c["returns"])
    assert (a["var_aleatoric"] > 0).all() and (a["var_epistemic"] > 0).all()


def test_composite_declared_env(gpu):
    spec = hopper_like()
    prob = synth.make_problem(env=spec, context=True, E=5, m=3, H=8, seed=53)
    eng = make_engine(prob, p=10)
    check_composite(eng, prob, spec_oracle(prob, spec), spec, spec, 8, "hopper_like")
    eng.close()


def test_composite_deterministic_engine(hc):
    """Without noise the particles of a member agree -- provided they read the same context: with reference_quirks on, particle j reads
    encoder j % E (core/utils.py:434-435), so a member's particles differ by their context alone; quirks off, they are identical."""
    prob, _ = hc
    eng = make_engine(prob, p=10, deterministic=True, quirks=False)
    acts = np.random.default_rng(9).uniform(-1, 1, (3, 2, 8, 6)).astype(np.float32)
    got = _np(eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], acts))
    assert (got["var_aleatoric"] == 0).all(), "identical particles of a member must give exactly 0"
    assert (got["var_epistemic"] > 0).all()
    eng.close()
    # quirks on (the default): the two particles of a member read different encoders, and that shows as spread inside a member
    eng = make_engine(prob, p=10, deterministic=True)
    got = _np(eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], acts))
    assert (got["var_aleatoric"] > 0).any() and (got["var_epistemic"] > 0).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 5
def raw_outputs(eng, ctx, traj, obs, acts, p, E, band_k):
    """cadm_forecast_stats called directly, every output pre-filled with 7: (return code, message, the outputs on the device)."""
    H, m, n = traj.shape[0], traj.shape[1], traj.shape[2]
    out, c = eng._forecast_outputs(m, n, H, max(p, 1), max(E, 1))
    for v in out.values():
        v.fill_(7)
    t, o, a = eng._t(traj), eng._t(obs), eng._t(acts)
    rc = eng.lib.cadm_forecast_stats(ctx, ptr(t), ptr(o), ptr(a), m, n, H, p, E, band_k, ct.byref(c), eng.stream)
    msg = eng.lib.cadm_last_error().decode()
    torch.cuda.synchronize()
    return rc, msg, out


def raw_stats(eng, ctx, traj, obs, acts, p, E, band_k):
    """(return code, message, whether an output was written)"""
    rc, msg, out = raw_outputs(eng, ctx, traj, obs, acts, p, E, band_k)
    return rc, msg, any(bool((v != 7).any()) for v in out.values())


def test_refusals(hc, hop):
    prob, eng = hc
    traj, obs, acts = synth_traj(5, 2, 1, 1, 10, 18, 6)
    for p, E, k, word in ((10, 5, 0, "band_k"), (10, 5, 11, "band_k"), (10, 4, 1, "multiple of E"), (10, 0, 1, "multiple of E")):
        rc, msg, wrote = raw_stats(eng, eng._ctx, traj, obs, acts, p, E, k)
        assert rc == -1 and word in msg and not wrote, (p, E, k, rc, msg, wrote)
    with pytest.raises(_lib.CadmError, match="band_k"):
        eng.forecast_stats(traj, obs, acts, band_k=11)
    with pytest.raises(_lib.CadmError, match="band_k"):
        eng.plan_forecast(prob["obs"], prob["cp_obs"], prob["cp_act"], np.zeros((3, 1, 8, 6), np.float32), band_k=0)
    # an oversize p * D: two tiles of 400 * 18 floats are 57.6 KB
    big = np.zeros((1, 1, 1, 400, 18), np.float32)
    rc, msg, wrote = raw_stats(eng, eng._ctx, big, obs, acts[:, :, :1], 400, 5, 1)
    assert rc == -1 and "LDS" in msg and "49152" in msg and not wrote, (rc, msg, wrote)
    # a discrete engine
    dprob = synth.make_problem(env="cartpole", context=True, E=5, m=1, H=4, seed=1)
    deng = make_engine(dprob, p=5)
    dtraj, dobs, dacts = synth_traj(6, 4, 1, 1, 5, 4, 2)
    rc, msg, wrote = raw_stats(deng, deng._ctx, dtraj, dobs, dacts, 5, 5, 1)
    assert rc == -1 and "discrete" in msg and not wrote, (rc, msg, wrote)
    with pytest.raises(_lib.CadmError, match="discrete"):
        deng.plan_forecast(dprob["obs"], dprob["cp_obs"], dprob["cp_act"], dacts)
    deng.close()
    # a spec ctx before cadm_set_env_spec
    spec, sprob, seng = hop
    raw = ct.c_void_p()
    assert seng.lib.cadm_ctx_create(ct.byref(seng.cfg), ct.byref(raw)) == 0
    straj, sobs, sacts = synth_traj(7, 3, 1, 1, 5, 11, 3)
    rc, msg, wrote = raw_stats(seng, raw, straj, sobs, sacts, 5, 5, 1)
    seng.lib.cadm_ctx_destroy(raw)
    assert rc == -4 and "cadm_set_env_spec" in msg and not wrote, (rc, msg, wrote)


# ---------------------------------------------------------------------------------------------------------------------- 6
# The kernel's LDS carve (forecast.hip: forecast_stats_kernel) against the bytes the host asks for (forecast_lds_bytes), with
# ts = p * D rounded up to a multiple of 4 floats: two tiles, 2 * ts floats; ret and rew, 2 * p floats; the `bad` word, 4 bytes of the
# 16 the host adds.  The budget is 49152 bytes.
#     halfcheetah   p = 323, D = 18: ts = 5816, (2 * 5816 + 2 * 323) * 4 + 16 = 49128 bytes -- accepted; the kernel's last word, `bad`,
#                   sits at byte 49112
#                   p = 324:         ts = 5832, (2 * 5832 + 2 * 324) * 4 + 16 = 49264 bytes -- refused
#     slim_humanoid p = 133, D = 45: ts = 5988, (2 * 5988 + 2 * 133) * 4 + 16 = 48984 bytes -- accepted
#                   p = 134:         ts = 6032, (2 * 6032 + 2 * 134) * 4 + 16 = 49344 bytes -- refused
# Without the 2 * p term the host would ask for 46544 bytes at p = 323 while the kernel's carve reaches byte 49116, and would accept
# every p up to 341: a change of either side has to keep these figures in step.
@pytest.fixture(scope="module")
def hum(gpu):
    """slim_humanoid (D = 45, A = 17) with a small network: the statistics kernel never reads the model"""
    prob = synth.make_problem(env="slim_humanoid", context=True, E=5, m=1, H=2, seed=55, hidden_sizes=(32,) * 4)
    eng = make_engine(prob, p=5)
    yield prob, eng
    eng.close()


def check_at_the_last_accepted_p(eng, env, kind, traj, obs, acts, E, what):
    H, m, n, p, D = traj.shape
    got = _np(eng.forecast_stats(traj, obs, acts, E=E))
    check_state_stats(got, traj, E, what)
    check_order_stats(eng, traj, obs, acts, E, what)
    check_rewards(eng, env, kind, traj, obs, acts, E, what)
    # one particle more: refused on the host before any launch, nothing written
    E1 = next(e for e in range(2, p + 2) if (p + 1) % e == 0)
    big = np.zeros((1, 1, 1, p + 1, D), np.float32)
    rc, msg, wrote = raw_stats(eng, eng._ctx, big, obs[:1], acts[:1, :1, :1], p + 1, E1, 1)
    assert rc == -1 and "LDS" in msg and "49152" in msg and not wrote, (rc, msg, wrote)
    return msg


def test_last_accepted_p_halfcheetah(hc):
    """p = 323 = 17 * 19 particles of D = 18 dims, E = 17: 49128 of the 49152 bytes, and the per-particle loops (ret, rew, the reward
    threads, the returns) take a second stride of the 256-thread workgroup.  p = 324 is refused.
    Measured on an MI355X: worst |err| / bound -- mean 0.003, member_mean 0.006, variances 0.001; every one of the 1292 step rewards
    bit-equal to the float32 closure; reward_mean 0.055, reward_member 0.124, returns 0.087."""
    prob, eng = hc
    traj, obs, acts = synth_traj(31, 2, 1, 2, 323, 18, 6)
    msg = check_at_the_last_accepted_p(eng, oenvs.make_env("halfcheetah"), "halfcheetah", traj, obs, acts, 17, "halfcheetah p=323 E=17")
    assert "49264" in msg, msg
    # the returns of the particles behind the first stride: r_0 + r_1 of the float32 closure, within the two steps' bounds
    got = _np(eng.forecast_stats(traj, obs, acts, E=17))
    r = step_rewards(oenvs.make_env("halfcheetah"), traj, obs, acts).astype(np.float64)
    b = reward_bound("halfcheetah", traj, obs, acts)
    assert (np.abs(got["returns"] - r.sum(2))[..., 256:] <= 2 * b.max(2)[..., 256:]).all()


def test_last_accepted_p_slim_humanoid(hum):
    """p = 133 = 7 * 19 particles of D = 45 dims, E = 7: 48984 bytes; spans of 5985 floats, unaligned for three sequence-steps of four.
    p = 134 is refused.  Dim 1 is redrawn around the alive bonus's interval.
    Measured on an MI355X: worst |err| / bound -- mean 0.010, member_mean 0.017, variances 0.003; every one of the 532 step rewards
    bit-equal to the float32 closure; reward_mean 0.011, reward_member 0.096, returns 0.052."""
    prob, eng = hum
    traj, obs, acts = synth_traj(32, 2, 1, 2, 133, 45, 17)
    traj[..., 1] = (1.5 + 0.5 * np.random.default_rng(98).standard_normal(traj.shape[:-1])).astype(np.float32)
    obs[0, 1] = 1.2
    msg = check_at_the_last_accepted_p(eng, oenvs.make_env("slim_humanoid"), "slim_humanoid", traj, obs, acts, 7, "slim_humanoid p=133 E=7")
    assert "49344" in msg, msg


def test_particles_that_agree(hc):
    """forecast.hip's header: particles that agree give exactly their value as every mean and exactly 0 as every variance.
    (1) all p = 20 particles of a sequence equal; (2) equal inside each of the 5 members (4 particles each: c + c + c + c is exact
    in float32), the members differing."""
    prob, eng = hc
    H, m, n, p, E, D = 8, 2, 2, 20, 5, 18
    one, obs, acts = synth_traj(33, H, m, n, 1, D, 6)
    traj = np.ascontiguousarray(np.broadcast_to(one, (H, m, n, p, D)))
    got = _np(eng.forecast_stats(traj, obs, acts, E=E))
    x = np.transpose(one, (1, 2, 0, 3, 4))[:, :, :, 0]                               # [m,n,H,D]
    assert (got["diverged_step"] == H).all()
    for k in ("mean", "lo", "hi"):
        assert np.array_equal(_bits(got[k]), _bits(x)), "(1) %s differs from the particles' bits" % k
    for e in range(E):
        assert np.array_equal(_bits(got["member_mean"][e]), _bits(x)), "(1) member_mean[%d]" % e
        assert np.array_equal(_bits(got["reward_member"][e]), _bits(got["reward_mean"])), "(1) reward_member[%d]" % e
    for k in VARS + ("reward_var",):
        assert (got[k] == 0).all(), "(1) %s is not exactly 0" % k
    r1 = step_rewards(oenvs.make_env("halfcheetah"), one, obs, acts)[..., 0]       # [m,n,H]
    assert (np.abs(got["reward_mean"] - r1) <= reward_bound("halfcheetah", one, obs, acts)[..., 0]).all()
    for j in range(p):
        assert np.array_equal(_bits(got["returns"][..., j]), _bits(got["returns"][..., 0])), "(1) returns of particle %d" % j
    mem, obs, acts = synth_traj(34, H, m, n, E, D, 6)
    traj = np.ascontiguousarray(np.repeat(mem, p // E, axis=3))                     # particle j holds member j // 4's values
    got = _np(eng.forecast_stats(traj, obs, acts, E=E))
    assert (got["var_aleatoric"] == 0).all(), "(2) identical particles of a member must give exactly 0"
    assert (got["var_epistemic"] > 0).all()
    check_state_stats(got, traj, E, "(2) particles equal inside a member")


def test_order_statistics_with_ties(hc):
    """A trajectory of the four values -1, -0.0, +0.0, 1: every dim of every step is full of ties, and the two zeros compare equal.
    lo / hi equal np.sort's by value; every entry is written (each rank 0 .. p - 1 is taken by exactly one particle)."""
    prob, eng = hc
    H, m, n, p, D = 3, 2, 2, 20, 18
    rng = np.random.default_rng(35)
    traj = np.array([-1.0, -0.0, 0.0, 1.0], np.float32)[rng.integers(0, 4, (H, m, n, p, D))]
    traj[0, 0, 0, :, 0] = 0.0
    traj[0, 0, 0, ::2, 0] = -0.0                  # only zeros, of both signs
    traj[0, 0, 0, :, 1] = 1.0                     # only one value
    assert np.signbit(traj[traj == 0]).any() and not np.signbit(traj[traj == 0]).all()
    _, obs, acts = synth_traj(36, H, m, n, 1, D, 6)
    srt = np.sort(np.transpose(traj, (1, 2, 0, 3, 4)), axis=3)
    for k in (1, 2, p):
        rc, msg, out = raw_outputs(eng, eng._ctx, traj, obs, acts, p, 5, k)
        assert rc == 0, msg
        got = _np(out)
        for name in ALL:
            assert (got[name] != 7).all(), "band_k = %d: an entry of %s was not written" % (k, name)
        assert np.array_equal(got["lo"], srt[:, :, :, k - 1]), "lo, band_k = %d" % k
        assert np.array_equal(got["hi"], srt[:, :, :, p - k]), "hi, band_k = %d" % k


# ---------------------------------------------------------------------------------------------------------------------- 7
FORECAST_SHAPES = dict(mean="mHD", std_total="mHD", std_epistemic="mHD", std_aleatoric="mHD", lo="mHD", hi="mHD", member_mean="EmHD",
                       reward_mean="mH", reward_std="mH", reward_member="EmH", returns="mp", rollout_returns="mp", return_mean="m",
                       diverged_step="m")


def _models(n, **kw):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDM
    from cadm_amd.envs import make_env_spec
    base = dict(hidden_nonlinearity="swish", n_forwards=8, n_candidates=64, ensemble_size=5, n_particles=10, use_cem=True, state_diff=1,
                normalize_input=False, seed=5)
    base.update(kw)
    return [CaDM("dyn", make_env_spec("halfcheetah"), **base) for _ in range(n)]


ROUTES = dict(cem={}, icem=dict(cem_noise_beta=2.0, cem_keep_elites=3), mppi=dict(cem_update="mppi", cem_temperature=0.5),
              scored=dict(cem_score="mean_std", cem_risk=1.0))


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_get_action_with_forecast_leaves_the_plans_alone(gpu, route):
    """Default CEM (numpy inputs: the first call takes the checked path, the later ones the staged host path), iCEM, MPPI, scored."""
    kw = ROUTES[route]
    model, twin = _models(2, **kw)
    rng = np.random.default_rng(0)
    m, H, D, A, Hh = 2, 8, 18, 6, 10
    obs, cpo, cpa = rng.standard_normal((m, D)), 0.1 * rng.standard_normal((m, D * Hh)), rng.uniform(-1, 1, (m, A * Hh))
    mean, var = np.zeros((m, H, A)), np.full((m, H, A), 0.25)
    fc = None
    for i in range(3):
        want = twin.get_action(obs, cpo, cpa, mean, var)
        if i == 1:
            plan, fc = model.get_action(obs, cpo, cpa, mean, var, return_forecast=True)
            again = model.forecast(obs, plan, cpo, cpa)                             # the same (seed, call): the same bits
            wide = model.forecast(obs, np.stack([plan, plan], 1), cpo, cpa, band_k=2)
        else:
            plan = model.get_action(obs, cpo, cpa, mean, var)
        np.testing.assert_array_equal(plan, want, err_msg="%s call %d" % (route, i))
        assert model._call == twin._call
        mean = np.concatenate([plan[:, 1:], np.zeros((m, 1, A))], 1)
    dims = dict(m=m, H=H, D=D, E=5, p=10)
    assert sorted(fc) == sorted(FORECAST_SHAPES)
    for k, sh in FORECAST_SHAPES.items():
        assert fc[k].shape == tuple(dims[c] for c in sh), k
        assert np.array_equal(fc[k], again[k], equal_nan=True), "forecast() of the returned plan: %s differs" % k
    assert (fc["diverged_step"] == H).all() and np.isfinite(fc["mean"]).all() and (fc["std_total"] > 0).all()
    np.testing.assert_allclose(fc["std_total"] ** 2, fc["std_epistemic"] ** 2 + fc["std_aleatoric"] ** 2, rtol=1e-4)
    np.testing.assert_allclose(fc["return_mean"], fc["returns"].mean(-1), rtol=1e-6)
    assert (fc["lo"] <= fc["mean"]).all() and (fc["mean"] <= fc["hi"]).all()
    assert wide["mean"].shape == (m, 2, H, D) and wide["member_mean"].shape == (5, m, 2, H, D) and wide["returns"].shape == (m, 2, 10)
    assert (wide["lo"] <= wide["hi"]).all()


def test_forecast_refusals_and_the_controller(gpu):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDM
    from cadm_amd.envs import make_env_spec
    from cadm_amd.policies.mpc_controller import MPCController
    (model,) = _models(1)
    rng = np.random.default_rng(1)
    m, H, D, A, Hh = 2, 8, 18, 6, 10
    obs, cpo, cpa = rng.standard_normal((m, D)), 0.1 * rng.standard_normal((m, D * Hh)), rng.uniform(-1, 1, (m, A * Hh))
    mean, var = np.zeros((m, H, A)), np.full((m, H, A), 0.25)
    with pytest.raises(ValueError, match="random-shooting"):
        model.get_action(obs, cpo, cpa, return_forecast=True)
    with pytest.raises(ValueError, match="forecast"):
        model.forecast(obs, np.zeros((m, H + 1, A)), cpo, cpa)
    disc = CaDM("dyn", make_env_spec("cartpole"), hidden_nonlinearity="swish", n_forwards=4, n_candidates=32, ensemble_size=5, n_particles=5,
                use_cem=False, state_diff=1, normalize_input=False)
    with pytest.raises(ValueError, match="discrete"):
        disc.get_action(np.zeros((1, 4)), np.zeros((1, 40)), np.zeros((1, 20)), return_forecast=True)
    with pytest.raises(ValueError, match="discrete"):
        disc.forecast(np.zeros((1, 4)), np.zeros((1, 4, 2)), np.zeros((1, 40)), np.zeros((1, 20)))
    # the controller: opt-in keeps the forecast, the default never asks the engine for one
    calls = []
    real = model.engine.plan_forecast
    model.engine.plan_forecast = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    plain = MPCController("mpc", model.env, model, use_cem=True, n_candidates=64, horizon=H, num_rollouts=m, context=True)
    plan, _ = plain.get_actions(obs, cpo, cpa, mean, var)
    assert not calls and plain.last_forecast is None and plan.shape == (m, H, A)
    asking = MPCController("mpc", model.env, model, use_cem=True, n_candidates=64, horizon=H, num_rollouts=m, context=True, forecast=True)
    plan, _ = asking.get_actions(obs, cpo, cpa, mean, var)
    assert len(calls) == 1 and plan.shape == (m, H, A)
    assert sorted(asking.last_forecast) == sorted(FORECAST_SHAPES) and asking.last_forecast["mean"].shape == (m, H, D)
    np.testing.assert_array_equal(asking.last_forecast["mean"], model.forecast(obs, plan, cpo, cpa)["mean"])
