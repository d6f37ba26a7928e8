"""GPU: open-loop prediction error along the horizon -- the statistics kernel (cadm_horizon_error), the composite over a
device-resident windowed dataset (cadm_eval_horizon) and the classes' evaluate_horizon.

Shapes: E = 5, p = 10, halfcheetah with context (the compiled-in 200 x 4 kernel), engine horizon 8, F = 4, N = 150 windows: blocks
of 64, 64 and a ragged 22.  future_bool holds all-valid windows, prefixes of every length, one all-invalid window and one window
with a hole (1, 1, 0, 1).  Truth is drawn independently of the model, normal, at the per-dim scale of the oracle trajectory: no
entry of a statistic is a difference of nearly equal numbers."""
import numpy as np
import pytest
import torch

from cadm_amd import _lib, synth
from cadm_amd.env_spec import EnvDecl
from helpers import make_engine, oracle_problem, spec_oracle
from horizon_ref import RTOL, check_against_oracle, make_mask, stats64
from oracle import nets as onets
from oracle import planner as oplanner

pytestmark = pytest.mark.gpu

E, P_, H_ENG, F, N = 5, 10, 8, 4, 150
KEYS = ("se", "spread", "se_member", "count", "diverged")


def hopper_like():          # tests/test_gpu_env_spec.py's declaration (same geometry: one JIT module serves both files)
    return EnvDecl(11, 3, preproc=["drop", "sincos", "id", "id", "sincos", "id", "id", "id", "id", "id", "id"],
                   postproc=["add"] * 5 + ["replace"] + ["add"] * 5,
                   reward=[dict(kind="linear", dim=5), dict(kind="square", dim=3, w=-0.5, when="next_obs"),
                           dict(kind="abs", dim=10, w=-0.1), dict(kind="inside", dim=0, w=1.0, lo=-0.5, hi=0.5, when="next_obs"),
                           dict(kind="outside", dim=2, w=-1.0, lo=-0.2, hi=0.2), dict(kind="linear", dim=4, w=0.3, when="next_obs"),
                           dict(kind="square", dim=7, w=-0.05), dict(kind="abs", dim=6, w=0.2, when="next_obs"),
                           dict(kind="outside", dim=9, w=-0.5, lo=-1.0, hi=1.0, when="next_obs"),
                           dict(kind="inside", dim=8, w=0.25, lo=-0.3, hi=0.8)],
                   ctrl_cost=0.001, bonus=1.0)


def small_vanilla():        # the shape of tests/test_gpu_env_spec.py's vanilla env
    return EnvDecl(7, 1, preproc=["id", "id", "sincos", "id", "drop", "id", "id"],
                   reward=[dict(kind="linear", dim=0, when="next_obs"), dict(kind="square", dim=2, w=-0.1, when="next_obs"),
                           dict(kind="outside", dim=1, w=-1.0, lo=-1.5, hi=1.5, when="next_obs")], ctrl_cost=0.01)


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_stats_close(got, ref, what):
    np.testing.assert_array_equal(got["count"], ref["count"], err_msg=what + " count")
    np.testing.assert_array_equal(got["diverged"], ref["diverged"], err_msg=what + " diverged")
    for k in ("se", "spread", "se_member"):
        err = np.abs(got[k] - ref[k]) / np.maximum(np.abs(ref[k]), 1e-300)
        err = np.where(ref[k] == 0, np.abs(got[k]), err)
        print("%s %s: worst relative error %.2e" % (what, k, err.max()))
        assert err.max() <= RTOL, "%s %s: relative error %.3e > %.1e" % (what, k, err.max(), RTOL)


def assert_identical(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s differs" % (what, k)


class Case:
    """One model + dataset + oracle trajectory, built once and left unchanged."""

    def __init__(self, env, seed):
        self.prob = prob = synth.make_problem(env=env, context=True, E=E, m=N, H=H_ENG, seed=seed)
        D, A = prob["D"], prob["A"]
        rng = np.random.default_rng(seed + 100)
        self.acts8 = rng.uniform(-1, 1, (N, 1, H_ENG, A)).astype(np.float32)       # the engine's 8 steps; the windows hold the first 4
        self.eps8 = rng.standard_normal((H_ENG, N, 1, P_, D)).astype(np.float32)
        self.mask = make_mask(N, F)
        o = oracle_problem(prob, np.float32) if isinstance(env, str) else spec_oracle(prob, env)
        T = oplanner.context_table_indexed(onets.context_forward(o["cp"], o["cp_obs"], o["cp_act"], o["st"]), 0)
        _, t_ref = oplanner.rollout_indexed(o["env"], o["ff"], o["st"], o["obs"], T, self.acts8[:, :, :F].copy(), self.eps8[:F].copy(), E, P_,
                                            False, return_traj=True)
        self.t_ref = t_ref.reshape(F, N, P_, D)                                    # fp32 oracle, H = 4
        scale = np.sqrt((self.t_ref.astype(np.float64) ** 2).mean(axis=(0, 1, 2)))
        self.truth = (rng.standard_normal((N, F, D)) * scale).astype(np.float32)
        obs = rng.standard_normal((N, F, D)).astype(np.float32)
        obs[:, 0] = prob["obs"].astype(np.float32)
        self.ds = dict(obs=obs.reshape(N, F * D), act=self.acts8[:, 0, :F].reshape(N, F * A).copy(), obs_next=self.truth.reshape(N, F * D),
                       cp_obs=prob["cp_obs"], cp_act=prob["cp_act"], future_bool=self.mask)

    def engine(self, **kw):
        return make_engine(self.prob, p=P_, **kw)

    def dev(self, eng):
        return {k: eng._t(v) for k, v in self.ds.items()}


@pytest.fixture(scope="module")
def hc(gpu):
    c = Case("halfcheetah", 41)
    eng = c.engine()
    ctx = eng.context_forward(c.prob["cp_obs"], c.prob["cp_act"])
    _, traj = eng.rollout_returns(c.prob["obs"], ctx, c.acts8, eps=c.eps8, want_traj=True)
    c.traj4 = traj[:F].contiguous()                                                # 4 steps of the 8-step engine
    c.iso = _np(eng.horizon_error(c.traj4, c.truth, c.mask))                       # statistics kernel in isolation
    c.comp = _np(eng.eval_horizon(c.dev(eng), N, F, eps=c.eps8[:F].copy()))        # composite, one chunk
    c.eng = eng
    return c


# ---------------------------------------------------------------------------------------------------------------------- 1
def test_statistics_kernel_matches_float64_restatement(hc):
    ref = stats64(hc.traj4.cpu().numpy().reshape(F, N, P_, -1), hc.truth, hc.mask, E)
    assert ref["count"].min() > 0 and ref["count"][0] > ref["count"][-1] and ref["diverged"].sum() == 0
    assert_stats_close(hc.iso, ref, "model trajectory")
    # cut into launches of 64, 64, 22 and of 128, 22 windows: the same bits
    for calls in ((64, 64, 22), (128, 22)):
        assert_identical(_np(hc.eng.horizon_error(hc.traj4, hc.truth, hc.mask, calls=calls)), hc.iso, "launches %r" % (calls,))


def test_statistics_kernel_odd_dim(hc):
    """D = 11: a window's p * D values are no multiple of 16 bytes times anything convenient; no model needed."""
    D = 11
    rng = np.random.default_rng(3)
    traj = (rng.standard_normal((F, N, 1, P_, D)) * rng.uniform(0.5, 3.0, D) + rng.standard_normal(D)).astype(np.float32)
    truth = (rng.standard_normal((N, F, D)) * 2.0).astype(np.float32)
    for n in (N, 131):                                      # 131 * 10 * 11 floats per step: steps 1 and 3 start off 16-byte alignment
        got = _np(hc.eng.horizon_error(traj[:, :n].copy(), truth[:n], hc.mask[:n]))
        assert_stats_close(got, stats64(traj[:, :n, 0], truth[:n], hc.mask[:n], E), "D = 11, m = %d" % n)


# ---------------------------------------------------------------------------------------------------------------------- 2
def test_composite_matches_oracle_and_the_isolated_kernel(hc):
    check_against_oracle(hc, hc.comp, "halfcheetah")
    # 4 steps of the 8-step engine == the composite's 4-step launch, row for row
    assert_identical(hc.comp, hc.iso, "composite vs rollout_returns + horizon_error")


def test_composite_on_a_declared_env(gpu):
    c = Case(hopper_like(), 43)
    eng = c.engine()
    check_against_oracle(c, _np(eng.eval_horizon(c.dev(eng), N, F, eps=c.eps8[:F].copy())), "hopper_like")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 3
def test_chunk_invariance_and_determinism(hc):
    eng, dev = hc.eng, hc.dev(hc.eng)
    for chunk in (64, 128, 4096):
        assert_identical(_np(eng.eval_horizon(dev, N, F, chunk=chunk, eps=hc.eps8[:F].copy())), hc.comp, "chunk %d" % chunk)
    a = _np(eng.eval_horizon(dev, N, F, seed=7, call=3))
    b = _np(eng.eval_horizon(dev, N, F, seed=7, call=3))
    assert_identical(a, b, "device noise, same (seed, call)")
    c = _np(eng.eval_horizon(dev, N, F, seed=7, call=4))
    assert not np.array_equal(a["spread"], c["spread"])
    np.testing.assert_array_equal(a["count"], c["count"])
    with pytest.raises(_lib.CadmError, match="n_forwards"):
        eng.eval_horizon(dev, N, H_ENG + 1)


# ---------------------------------------------------------------------------------------------------------------------- 4
def test_closed_form_constant_delta(gpu):
    """All weights zero, deterministic: the mean head is its bias (powers of two, the same for every member), so every step adds
    delta_d = bias_d * delta_std_d + delta_mean_d (halfcheetah: dim 0 is replaced by it, the others add it).  Truth = that trajectory
    + b_d: mse = b_d^2, spread = 0, every member's mse = mse."""
    prob = synth.make_problem(env="halfcheetah", context=True, E=E, m=N, H=H_ENG, seed=5)
    D, A = prob["D"], prob["A"]
    for k, v in prob["ff"].items():
        if not k.endswith("logvar"):
            prob["ff"][k] = np.zeros_like(v)
    rng = np.random.default_rng(6)
    bias = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], D)
    prob["ff"]["output_mu_bias"] = np.tile(bias[None, None, :], (E, 1, 1))
    eng = make_engine(prob, p=P_, deterministic=True)
    f32 = np.float32
    delta = (bias.astype(f32) * (prob["stats"]["delta_std"].astype(f32) + f32(1e-10)) + prob["stats"]["delta_mean"].astype(f32)).astype(f32)
    x = prob["obs"].astype(f32)
    steps = []
    for _ in range(F):
        nxt = (x + delta).astype(f32)
        nxt[:, 0] = delta[0]
        steps.append(nxt)
        x = nxt
    b = rng.uniform(2.0, 4.0, D).astype(f32) * rng.choice([-1.0, 1.0], D).astype(f32)
    truth = (np.stack(steps, 1) + b).astype(f32)                                   # [N,F,D]
    mask = make_mask(N, F)
    obs = rng.standard_normal((N, F, D)).astype(f32)
    obs[:, 0] = prob["obs"]
    ds = dict(obs=obs.reshape(N, -1), act=rng.uniform(-1, 1, (N, F * A)).astype(f32), obs_next=truth.reshape(N, -1), cp_obs=prob["cp_obs"],
              cp_act=prob["cp_act"], future_bool=mask)
    out = _np(eng.eval_horizon({k: eng._t(v) for k, v in ds.items()}, N, F, chunk=64))
    count = (np.cumprod(mask, axis=1) > 0).sum(0)
    np.testing.assert_array_equal(out["count"], count)
    assert out["diverged"].sum() == 0
    mse_expected = count[:, None] * b.astype(np.float64)[None] ** 2
    err = np.abs(out["se"] / mse_expected - 1)
    print("closed form: worst relative error of se %.2e" % err.max())
    assert err.max() <= RTOL
    assert (out["spread"] == 0).all()
    for e in range(E):
        assert np.array_equal(out["se_member"][e], out["se"])
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 5
def test_non_finite_rows_are_counted_and_left_out(hc):
    rng = np.random.default_rng(9)
    D = 18
    clean = (rng.standard_normal((F, N, 1, P_, D)) * 2.0 + 1.0).astype(np.float32)
    truth = (rng.standard_normal((N, F, D)) * 2.0).astype(np.float32)
    mask = np.ones((N, F), np.float32)
    mask[100, 3] = 0.0
    planted = clean.copy()
    planted[2:, 3, 0, 4, 7] = np.nan                         # one particle of window 3 from step 2 on
    planted[0, 70, 0, 0, 0] = np.inf                         # window 70 at step 0
    planted[0, 70, 0, 9, 17] = -np.inf
    eng = hc.eng
    got = _np(eng.horizon_error(planted, truth, mask))
    base = _np(eng.horizon_error(clean, truth, mask))
    np.testing.assert_array_equal(got["diverged"], [1, 0, 1, 1])
    np.testing.assert_array_equal(got["count"], base["count"] - got["diverged"])
    assert_stats_close(got, stats64(planted[:, :, 0], truth, mask, E), "planted")
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    # step 1 holds no planted value: untouched, bit for bit
    for k in KEYS:
        assert np.array_equal(got[k][..., 1, :] if got[k].ndim > 1 else got[k][1], base[k][..., 1, :] if base[k].ndim > 1 else base[k][1])
    # a diverged (window, step) is in no sum: the same bits as a clean run whose mask drops exactly those pairs
    m3 = mask.copy()
    m3[3, 2:] = 0.0
    drop3 = _np(eng.horizon_error(clean, truth, m3))
    m70 = mask.copy()
    m70[70, 0] = 0.0
    drop70 = _np(eng.horizon_error(clean, truth, m70))
    for k in ("se", "spread", "se_member"):
        assert np.array_equal(got[k][..., 2:, :], drop3[k][..., 2:, :]), k
        assert np.array_equal(got[k][..., 0, :], drop70[k][..., 0, :]), k
    # blocks that hold neither window: their windows alone give the same bits with and without the planted values elsewhere
    tail = _np(eng.horizon_error(planted[:, 128:].copy(), truth[128:], mask[128:]))
    assert_identical(tail, _np(eng.horizon_error(clean[:, 128:].copy(), truth[128:], mask[128:])), "block 2")


# ---------------------------------------------------------------------------------------------------------------------- 6
def _windows(rng, n, D, A, Hh, f):
    obs = rng.standard_normal((n, f * D))
    fb = np.ones((n, f))
    for i in range(0, n, 4):
        fb[i, (i // 4) % f + 1:] = 0.0
    fb[2] = 0.0
    return dict(obs=obs, act=rng.uniform(-1, 1, (n, f * A)), obs_next=obs + 0.1 * rng.standard_normal((n, f * D)),
                cp_obs=0.1 * rng.standard_normal((n, D * Hh)), cp_act=rng.uniform(-1, 1, (n, A * Hh)), future_bool=fb)


def test_class_api(gpu):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDM
    from cadm_amd.envs import EnvSpec
    D, A, Hh, f, H = 18, 6, 10, 4, 8
    kw = dict(hidden_nonlinearity="swish", n_forwards=H, n_candidates=64, ensemble_size=E, n_particles=P_, use_cem=True, batch_size=64,
              history_length=Hh, future_length=f, seed=3)
    rng = np.random.default_rng(0)
    w = _windows(rng, 200, D, A, Hh, f)
    args = (w["obs"], w["act"], w["obs_next"], w["cp_obs"], w["cp_act"], w["future_bool"])
    models = [CaDM("dyn", EnvSpec("halfcheetah"), **kw) for _ in range(2)]
    with pytest.raises(RuntimeError, match="statistics"):
        models[0].evaluate_horizon(*args)
    for mdl in models:
        mdl.fit(*args, epochs=2)
    model, twin = models
    held = _windows(rng, 150, D, A, Hh, f)
    hargs = (held["obs"], held["act"], held["obs_next"], held["cp_obs"], held["cp_act"], held["future_bool"])
    n_ds, call = model._dataset["obs"].shape[0], model._call
    res = model.evaluate_horizon(*hargs)
    res2 = model.evaluate_horizon(*hargs, chunk=64)
    assert sorted(res) == ["count", "diverged", "member_mse", "mse", "rmse", "spread"]
    assert res["mse"].shape == (f, D) and res["member_mse"].shape == (E, f, D) and res["spread"].shape == (f, D)
    assert res["count"].shape == res["diverged"].shape == res["rmse"].shape == (f,)
    np.testing.assert_array_equal(res["count"], (np.cumprod(held["future_bool"], axis=1) > 0).sum(0))
    assert res["diverged"].sum() == 0
    assert np.isfinite(res["mse"]).all() and np.isfinite(res["rmse"]).all() and (res["spread"] > 0).all()
    assert not np.array_equal(res["spread"], res2["spread"])           # its own call counter moved on
    assert model._dataset["obs"].shape[0] == n_ds and model._call == call
    # count == 0 -> NaN
    none = dict(held, future_bool=np.zeros_like(held["future_bool"]))
    r0 = model.evaluate_horizon(none["obs"], none["act"], none["obs_next"], none["cp_obs"], none["cp_act"], none["future_bool"])
    assert (r0["count"] == 0).all() and np.isnan(r0["mse"]).all() and np.isnan(r0["rmse"]).all()
    # planning is the same with or without evaluations in between
    o, cpo, cpa = rng.standard_normal((2, D)), 0.1 * rng.standard_normal((2, D * Hh)), rng.uniform(-1, 1, (2, A * Hh))
    mean, var = np.zeros((2, H, A)), np.full((2, H, A), 0.25)
    np.testing.assert_array_equal(model.get_action(o, cpo, cpa, mean, var), twin.get_action(o, cpo, cpa, mean, var))
    # windows longer than the planning horizon
    long = CaDM("dyn", EnvSpec("halfcheetah"), **dict(kw, future_length=9))
    long.set_normalization(model.normalization)
    lw = _windows(rng, 70, D, A, Hh, 9)
    with pytest.raises(ValueError, match="n_forwards"):
        long.evaluate_horizon(lw["obs"], lw["act"], lw["obs_next"], lw["cp_obs"], lw["cp_act"], lw["future_bool"])


def test_vanilla_class_on_a_declared_env(gpu):
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Vanilla
    spec = small_vanilla()
    D, A = 7, 1
    model = Vanilla("dyn", spec, hidden_nonlinearity="swish", n_forwards=5, n_candidates=64, ensemble_size=5, n_particles=5, use_cem=True,
                    batch_size=32, normalize_input=True, deterministic=True)
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((200, D))
    act, nxt = rng.uniform(-1, 1, (200, A)), obs + 0.1 * rng.standard_normal((200, D))
    model.fit(obs, act, nxt, epochs=2)
    res = model.evaluate_horizon(obs[:130], act[:130], nxt[:130])
    assert sorted(res) == ["count", "diverged", "member_mse", "mse", "rmse", "spread"]
    assert res["mse"].shape == (1, D) and res["member_mse"].shape == (5, 1, D) and res["count"].tolist() == [130]
    assert np.isfinite(res["mse"]).all() and np.isfinite(res["spread"]).all() and (res["spread"] >= 0).all()
