"""Shared helpers for the test-suite (tests may import both the product and the oracle)."""
import functools

import numpy as np

from cadm_amd import synth
from oracle import envs as oenvs
from oracle import nets as onets


def oracle_problem(prob, dtype):
    """Cast a synth problem to oracle inputs of the given dtype."""
    o = dict(env=oenvs.make_env(prob["env"]),
             ff=onets.cast_params(prob["ff"], dtype),
             cp=None if prob["cp"] is None else onets.cast_params(prob["cp"], dtype),
             back=None if prob.get("back") is None else onets.cast_params(prob["back"], dtype),
             st=onets.cast_stats(prob["stats"], dtype))
    for k in ("obs", "cp_obs", "cp_act", "init_mean", "init_var"):
        o[k] = prob[k].astype(dtype)
    return o


make_engine = synth.make_engine   # product code (cadm_amd/synth.py); re-exported for the tests


def trunc_z(rng, shape):
    z = rng.standard_normal(shape)
    bad = np.abs(z) >= 2.0
    while bad.any():
        z[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(z) >= 2.0
    return z


def rel_err(a, b):
    """norm-wise relative error max|a-b| / max|b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def assert_close(a, b, rtol=1e-5, what=""):
    """|a-b| <= rtol * max(|b|, scale) elementwise with scale = rms(b): the 1e-5 relative bar of
    BASELINE.json with an absolute floor that tolerates cancellation in fp32 dot products."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.sqrt(np.mean(b * b))), 1e-30)
    bound = rtol * np.maximum(np.abs(b), scale)
    bad = np.abs(a - b) > bound
    assert not bad.any(), "%s: %d/%d elements off, worst |diff|=%.3e (bound %.3e), rel_err=%.3e" % (
        what, int(bad.sum()), bad.size, float(np.abs(a - b).max()), float(bound.flat[np.abs(a - b).argmax()]), rel_err(a, b))


def floored_rel(a, b):
    """The smallest rtol `assert_close(a, b, rtol)` passes with: max |a-b| / max(|b|, rms(b))."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.sqrt(np.mean(b * b))), 1e-30)
    return float((np.abs(a - b) / np.maximum(np.abs(b), scale)).max())


def floor_reliance(a, b, rtol=1e-5):
    """How much of `assert_close`'s verdict leans on its rms floor: (elements that violate the PURE relative bound
    |a-b| <= rtol*|b|, total elements, largest |b|/rms among those).  Elements far below the tensor's rms are sums that
    cancelled: no fp32 evaluation order reproduces them to 1e-5 of themselves."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(float(np.sqrt(np.mean(b * b))), 1e-30)
    bad = np.abs(a - b) > rtol * np.abs(b)
    worst = float((np.abs(b)[bad] / scale).max()) if bad.any() else 0.0
    return int(bad.sum()), int(bad.size), worst


def f16_split_saturating(x):
    """What the rollout kernels feed the matrix pipe for a value x: hi = sat(f16(x)), lo = sat(f16(x - hi)) with f16 overflow saturating
    at +-65504 (MODE.FP16_OVFL, csrc/rollout_env.h: fp16_saturate_on), returned as hi + lo in fp32: x to 2^-22 inside the f16 range,
    at most +-131008 beyond it."""
    x = np.asarray(x, np.float32)
    big = np.float32(65504.0)

    def sat(v):
        with np.errstate(over="ignore", invalid="ignore"):
            h = v.astype(np.float16).astype(np.float32)
        return np.where(np.isinf(h) & np.isfinite(v), np.sign(v) * big, h).astype(np.float32)
    hi = sat(x)
    with np.errstate(invalid="ignore"):
        lo = sat((x - hi).astype(np.float32))
    return (hi + lo).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# the fused training step against the oracle: what tests/test_gpu_train.py and tests/test_gpu_train_state.py share
# ------------------------------------------------------------------------------------------------------------------------------
WD = (0.000025, 0.00005, 0.000075, 0.000075, 0.0001)      # run_cadm_pets.py:223
CWD = (0.000025, 0.00005, 0.000075)                        # run_cadm_pets.py:232


def _cfg(prob, det, back_coeff):
    return dict(deterministic=det, back_coeff=back_coeff, weight_decay_coeff=1.0, weight_decays=WD,
                context_weight_decays=CWD, n_hidden=len(prob["hidden_sizes"]), n_cp_hidden=len(prob["cp_hidden_sizes"]))


def _oracle_nets(prob, dtype, requires_grad=True):
    from oracle import train as otrain
    ff = otrain.to_torch(prob["ff"], dtype, requires_grad)
    back = otrain.to_torch(prob["back"], dtype, requires_grad) if prob.get("back") is not None else None
    cp = otrain.to_torch(prob["cp"], dtype, requires_grad) if prob["cp"] is not None else None
    st = otrain.to_torch(prob["stats"], dtype)
    return ff, back, cp, st


def _dev_batch(eng, batch, context, with_back):
    keys = ["obs", "act", "delta"] + (["obs_next", "back_delta"] if with_back else []) + (["cp_obs", "cp_act"] if context else [])
    return {k: eng._t(batch[k]) for k in keys}


def _dev_engine(prob, p, **kw):
    """An engine on the DEVELOPER library: the product's objects plus the hook that reads Adam's moment buffers."""
    from cadm_amd import _lib
    return make_engine(prob, p=p, lib=_lib.load_dev(), **kw)


def _grad_report(g_hip, g_ref):
    """(max |d| / max |ref|,  max elementwise |d| / |ref| over |ref| >= 0.25 rms(ref))"""
    scale = max(np.abs(g_ref).max(), 1e-300)
    d = np.abs(g_hip - g_ref)
    big = np.abs(g_ref) >= 0.25 * np.sqrt(np.mean(g_ref ** 2))
    return d.max() / scale, (d[big] / np.abs(g_ref[big])).max() if big.any() else 0.0


def _check_gradients(eng, grads, what):
    """Every gradient tensor the fused step produced, read back DIRECTLY (Adam's first moment after one step with beta1 = 0 is
    the gradient, exactly: m = 0 m + 1 g) and compared element by element with torch.autograd on the fp64 oracle:
    <= 1e-5 of the tensor's max, and <= 1e-4 PURE relative on every element with |g| >= 0.25 rms (fp32 forward / backward over a
    256-row batch: roundoff-scale bars; a sign or scale error in any slice of any tensor fails them)."""
    checked, worst = 0, (0.0, 0.0, "")
    for net in eng.net_names():
        for name in eng.nets[net]:
            g_ref = grads[net][name]
            if g_ref is None:      # TF skips variables without a gradient (backward model's logvar head, dynamics.py:213-240)
                continue
            g_hip = eng.dev_read_adam_moment(net, name).cpu().numpy().astype(np.float64)
            assert np.isfinite(g_hip).all()
            to_max, pure = _grad_report(g_hip, g_ref.numpy())
            assert to_max <= 1e-5, "%s %s/%s gradient: max err %.2e of the tensor's max" % (what, net, name, to_max)
            assert pure <= 1e-4, "%s %s/%s gradient: pure relative err %.2e on |g| >= 0.25 rms" % (what, net, name, pure)
            if to_max > worst[0]:
                worst = (to_max, pure, "%s/%s" % (net, name))
            checked += 1
    print("%s: %d gradient tensors, worst %.2e of max (pure-relative %.2e) at %s" % ((what, checked) + worst))
    return checked


# ------------------------------------------------------------------------------------------------------------------------------
# the context encoder under non-identity history statistics (state_diff = False: the history holds raw observations): what
# tests/test_context_stats_inputs.py, tests/test_gpu_context_stats.py and tests/test_gpu_context.py share
# ------------------------------------------------------------------------------------------------------------------------------
RAW_GEOMETRIES = [  # env, E, Hh, cp_sizes, C
    ("halfcheetah", 5, 10, (256, 128, 64), 10),       # the reference's encoder
    ("pendulum", 5, 1, (8, 6), 3),                    # input width 4, layers narrower than one 64-unit group, odd widths
    ("halfcheetah", 3, 3, (320, 100, 30), 10),        # a layer wider than 256; widths not multiples of 4 / 64
    ("ant", 7, 2, (64,), 7),                          # one hidden layer, odd output width, E = 7
    ("slim_humanoid", 2, 10, (256, 128, 64), 10),     # input width 620
    ("halfcheetah", 5, 10, (1024, 512), 16),          # two row tiles do not fit in LDS: the launcher falls back to ONE at every m
    ("halfcheetah", 5, 3, (70, 50, 30), 10),          # no width a multiple of 4 behind the input, fewer than four 64-unit groups per layer
]


def raw_history_problem(env, E, Hh, cp_sizes, C, m, seed, zero_std_cols=(), **kw):
    """(prob, cp_obs [m, D Hh], cp_act [m, A Hh]): a trained-like synth problem whose statistics are those of a model built with
    state_diff = False -- every history column has its own mean (5 N(0,1)) and spread (U(0.5, 2)) -- and histories at that scale,
    cp_obs = mean + std N(0,1).  A column of `zero_std_cols` has std 0 and sits exactly on its mean: what np.std of a constant
    column gives `fit`.  Statistics and histories are float32 values (held in float64 arrays): the float64 oracle then sees the
    numbers the device sees, and a zero-std column normalises to exactly 0 in every precision instead of to a rounding error
    divided by 1e-10.  `kw` goes to synth.make_problem (trained_like=False: the reference's initialiser); prob["cp_obs"] / prob["cp_act"] are the returned histories."""
    prob = synth.make_problem(env=env, E=E, m=m, Hh=Hh, cp_hidden_sizes=cp_sizes, C=C, seed=seed, **dict(dict(trained_like=True), **kw))
    rng = np.random.default_rng(seed + 1000)
    st = synth.norm_stats(rng, prob["D"], prob["A"], prob["P"], Hh, state_diff=False, discrete=prob["discrete"])
    st["cp_obs_mean"] = 5.0 * st["cp_obs_mean"]
    st["cp_obs_std"][list(zero_std_cols)] = 0.0
    for k in st:
        st[k] = st[k].astype(np.float32).astype(np.float64)
    prob["stats"] = st
    cp_obs, _ = raw_histories(prob, (m,), rng)
    cp_act = rng.uniform(-1, 1, (m, prob["A"] * Hh)).astype(np.float32).astype(np.float64)
    prob["cp_obs"], prob["cp_act"] = cp_obs, cp_act
    return prob, cp_obs, cp_act


def raw_histories(prob, lead, rng):
    """(cp_obs [*lead, D Hh] at the scale of prob's cp_obs statistics, cp_act [*lead, A Hh] ~ U(-1, 1)) as float32 values."""
    st = prob["stats"]
    cp_obs = st["cp_obs_mean"] + st["cp_obs_std"] * rng.standard_normal(tuple(lead) + (prob["D"] * prob["Hh"],))
    cp_act = rng.uniform(-1, 1, tuple(lead) + (prob["A"] * prob["Hh"],))
    return cp_obs.astype(np.float32).astype(np.float64), cp_act.astype(np.float32).astype(np.float64)


def raw_train_batch(prob, B, seed):
    """synth.make_train_batch with the history's cp_obs redrawn at raw scale from prob's own statistics."""
    batch = synth.make_train_batch(prob, B=B, seed=seed)
    batch["cp_obs"], _ = raw_histories(prob, (prob["E"], B), np.random.default_rng(seed + 2000))
    return batch


def rolled_stats(stats, key):
    """The statistics with one vector moved by one column: what a kernel that reads the neighbouring column computes with."""
    out = dict(stats)
    out[key] = np.roll(stats[key], 1)
    return out


def identity_history_stats(stats):
    out = dict(stats)
    out["cp_obs_mean"], out["cp_obs_std"] = np.zeros_like(stats["cp_obs_mean"]), np.ones_like(stats["cp_obs_std"])
    return out


def context_row_tiles(E, m, n_cus):
    """csrc/context.hip launch_context_batched: the row tiles per workgroup (16 rows each) the launcher tries FIRST for m >= 48 rows
    per member.  (Layers too wide for two tiles in LDS fall back to one: RAW_GEOMETRIES' (1024, 512).)"""
    wg2 = E * ((m + 31) // 32)
    return 1 if (n_cus < wg2 < 2 * n_cus + n_cus // 2) or wg2 <= n_cus // 4 else 2


def two_tile_m(E, n_cus):
    """The smallest m = 1 (mod 32) whose batched call takes two row tiles: its last 32-row tile holds ONE row, the second half empty."""
    m = 33
    while context_row_tiles(E, m, n_cus) != 2:
        m += 32
        assert m < 1 << 16, "no two-tile m for E = %d on %d CUs" % (E, n_cus)
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# user-declared envs (cadm_amd/env_spec.py EnvDecl): what tests/test_gpu_env_spec.py and tests/test_gpu_env_spec_envelope.py share
# ------------------------------------------------------------------------------------------------------------------------------
SPEC_WD = (0.000025, 0.00005, 0.000075, 0.000075, 0.0001)
SPEC_CWD = (0.000025, 0.00005, 0.000075)
FLAVOURS = ("1", "2", "3", "4")      # cooperative kernel with one / two row tiles, wave-tile kernel with 8 / 4 tiles per workgroup


def _np(t):
    return t.detach().cpu().numpy()


# the opt-in planner: what tests/test_gpu_icem.py, tests/test_gpu_mppi.py and tests/test_gpu_risk.py share
@functools.lru_cache(maxsize=None)
def planner_engine(H, context=False, p=5, env="halfcheetah"):
    """(problem, engine), cached: hidden (32,) * 4, ensemble 5, m = 2, num_elites = 8, 3 CEM iterations."""
    prob = synth.make_problem(env=env, context=context, E=5, m=2, H=H, seed=3, hidden_sizes=(32,) * 4, trained_like=env == "halfcheetah")
    return prob, make_engine(prob, p=p, num_elites=8, num_cem_iters=3)


def plan_model(context, H, hidden=(32,) * 4, n_candidates=64, n_particles=5, m=2, **kw):
    """(model, problem): a CaDM (context) or vanilla model with a synthetic halfcheetah problem's weights and statistics; kw: more kwargs."""
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDMModel
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as VanillaModel
    from cadm_amd.envs import make_env_spec
    env = kw.pop("env", None) or make_env_spec("halfcheetah")
    base = dict(name="dyn", env=env, hidden_sizes=hidden, hidden_nonlinearity="swish", n_forwards=H, n_candidates=n_candidates, ensemble_size=5,
                n_particles=n_particles, use_cem=True, normalize_input=True, seed=7)
    base.update(kw)
    prob = synth.make_problem(env="halfcheetah", context=context, E=5, m=m, H=H, seed=9, hidden_sizes=hidden, trained_like=True)
    st = prob["stats"]
    if context:
        model = CaDMModel(**base)
        model.engine.set_net("context_model", prob["cp"])
    else:
        model = VanillaModel(**base)
    model.engine.set_net("ff_model", prob["ff"])
    nz = {"obs": (st["obs_mean"], st["obs_std"]), "delta": (st["delta_mean"], st["delta_std"]), "act": (st["act_mean"], st["act_std"])}
    if context:
        nz.update({"cp_obs": (st["cp_obs_mean"], st["cp_obs_std"]), "cp_act": (st["cp_act_mean"], st["cp_act_std"]),
                   "back_delta": (st["back_delta_mean"], st["back_delta_std"])})
    model.set_normalization(nz)
    return model, prob


def plan_act(model, prob, context, mean, var):
    if context:
        return model.get_action(prob["obs"], prob["cp_obs"], prob["cp_act"], mean, var)
    return model.get_action(prob["obs"], mean, var)


def zero_carry(eng, m, K, H):
    """(carry [m,K,H,A] float32, carry_valid [m] int32) of a planner that has carried nothing yet; (None, None) for K = 0."""
    import torch
    if K == 0:
        return None, None
    return torch.zeros((m, K, H, eng.A), dtype=torch.float32, device=eng.device), torch.zeros((m,), dtype=torch.int32, device=eng.device)


def spec_oracle(prob, spec, dt=np.float32):
    """A synth problem of a spec env as oracle inputs (the oracle is duck-typed on env objects: the spec is its env)."""
    o = dict(env=spec, ff=onets.cast_params(prob["ff"], dt), cp=None if prob["cp"] is None else onets.cast_params(prob["cp"], dt),
             st=onets.cast_stats(prob["stats"], dt))
    for k in ("obs", "cp_obs", "cp_act", "init_mean", "init_var"):
        o[k] = prob[k].astype(dt)
    return o


class flavour:
    """`with flavour(eng, "3"):` forces one rollout flavour on a developer-library engine, and hands back the launch plan after."""

    def __init__(self, eng, fl):
        self.eng, self.fl = eng, fl

    def __enter__(self):
        self.eng.dev_set_rollout("xdl", row_tiles=int(self.fl))
        return self.eng

    def __exit__(self, *exc):
        self.eng.dev_set_rollout("xdl", row_tiles=0)


def run_flavour(eng, fl, obs, ctx, acts, **kw):
    """(returns [m,n,p], trajectory [H,m,n,p,D]) of one rollout call in flavour `fl`, as numpy."""
    import torch
    with flavour(eng, fl):
        rows, traj = eng.rollout_returns(obs, ctx, acts, want_traj=True, **kw)
        torch.cuda.synchronize()
        return _np(rows), _np(traj)


def threshold_jump(spec, H, p):
    """Largest change of a candidate's return from indicator terms (inside / outside) taking the other side of a threshold once per
    step: their weights summed, over H steps, averaged over p particles."""
    return sum(abs(t[3]) for t in spec.terms if t[0] in ("inside", "outside")) * H / p


def close_but_jumps(got, want, jump, what):
    """Candidate returns against the oracle's.  An indicator term (inside / outside) jumps by its weight where a state sits on its
    threshold: a particle whose state lands within rounding of it may take the other side in the oracle.  Such a candidate is off by
    a multiple of w / p -- allowed for at most 1 % of the candidates, everything else at the usual 1e-4 bar."""
    bad = np.abs(got - want) > 1e-4 * np.maximum(np.abs(want), np.sqrt(np.mean(want ** 2)))
    assert bad.sum() <= 0.01 * bad.size, "%s: %d/%d candidates off" % (what, bad.sum(), bad.size)
    assert (np.abs(got - want)[bad] <= jump + 1e-3).all(), "%s: off by more than one threshold flip" % what


def check_spec_training_step(spec, prob, E, det, what, B=48, predict=False):
    """One training step of a spec env against oracle/train: the three losses at rtol 5e-5, and every gradient (linearised Adam:
    g = w_before - w_after) within 2e-3 of its tensor's max against fp64 autograd.  `predict`: also predict_heads against the oracle's
    one-step forward pass (float64).  The oracle's obs_preproc is picked by env name, so it is handed the spec's preprocessed
    observations under an identity-preproc name: the same network inputs."""
    import torch
    from cadm_amd import synth
    from oracle import train as otrain
    context = prob["cp"] is not None
    batch = synth.make_train_batch(prob, B=B, seed=2)
    cfg = dict(deterministic=det, back_coeff=0.5, weight_decay_coeff=1.0, weight_decays=SPEC_WD, context_weight_decays=SPEC_CWD,
               n_hidden=len(prob["hidden_sizes"]), n_cp_hidden=len(prob["cp_hidden_sizes"]))
    keys = ["obs", "act", "delta", "obs_next", "back_delta"] + (["cp_obs", "cp_act"] if context else [])
    tb = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    tb["obs"] = torch.tensor(spec.obs_preproc(batch["obs"]), dtype=torch.float64)
    tb["obs_next"] = torch.tensor(spec.obs_preproc(batch["obs_next"]), dtype=torch.float64)

    def oracle_nets(rg):
        return (otrain.to_torch(prob["ff"], torch.float64, rg), otrain.to_torch(prob["back"], torch.float64, rg),
                otrain.to_torch(prob["cp"], torch.float64, rg) if context else None, otrain.to_torch(prob["stats"], torch.float64))
    eng = make_engine(prob, p=E, deterministic=det)
    eng.train_configure(1e-3, SPEC_WD, SPEC_CWD, 1.0, 0.5, max_batch=B)
    got = _np(eng.train_step({k: eng._t(batch[k]) for k in keys}, train=False))
    ff, back, cp, st = oracle_nets(False)
    ref = otrain.train_losses("slim_humanoid", ff, back, cp, st, tb, cfg)       # (identity obs_preproc)
    np.testing.assert_allclose(got, [float(ref["mse"]), float(ref["back_mse"]), float(ref["recon"])], rtol=5e-5, atol=5e-5)
    if predict:
        mu, lv = eng.predict_heads(batch["obs"], batch["act"], batch["cp_obs"] if context else None, batch["cp_act"] if context else None)
        o = {k: onets.cast_params(prob[k], np.float64) for k in ("ff",) + (("cp",) if context else ())}
        s = onets.cast_stats(prob["stats"], np.float64)
        feats = [onets.normalize(spec.obs_preproc(batch["obs"]), s["obs_mean"], s["obs_std"]),
                 onets.normalize(batch["act"], s["act_mean"], s["act_std"])]
        if context:
            feats.append(onets.context_forward_bs(o["cp"], batch["cp_obs"], batch["cp_act"], s))
        _, mu_ref, lv_ref = onets.dynamics_forward(o["ff"], np.concatenate(feats, -1), s["delta_mean"], s["delta_std"],
                                                   np.zeros((E, B, prob["D"])), det)
        assert_close(_np(mu), mu_ref, 2e-5, "%s predict mu" % what)
        if not det:
            assert_close(_np(lv), lv_ref, 2e-5, "%s predict logvar" % what)
    eng.close()
    eng = make_engine(prob, p=E, deterministic=det)
    eng.train_configure(1e6, SPEC_WD, SPEC_CWD, 1.0, 0.5, max_batch=B, beta1=0.0, beta2=0.0, epsilon=1e6)    # linearised Adam
    before = {nn: {k: v.clone() for k, v in eng.nets[nn].items()} for nn in eng.net_names()}
    eng.train_step({k: eng._t(batch[k]) for k in keys}, train=True)
    ff, back, cp, st = oracle_nets(True)
    out = otrain.train_losses("slim_humanoid", ff, back, cp, st, tb, cfg)
    grads = otrain.grads_of(out["loss"], {"ff_model": ff, "backward_model": back, "context_model": cp})
    for net in eng.net_names():
        for pname, w0 in before[net].items():
            g_ref = grads[net][pname]
            g_hip = (w0 - eng.nets[net][pname]).cpu().numpy().astype(np.float64)
            if g_ref is None:
                assert np.abs(g_hip).max() == 0.0
                continue
            g_ref = g_ref.numpy()
            err = np.abs(g_hip - g_ref).max() / max(np.abs(g_ref).max(), 1e-12)
            assert err < 2e-3, "%s %s/%s gradient off: %.3e" % (what, net, pname, err)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the corners of the kernels' envelope (include/cadm_hip.h CADM_SPEC_MAX_*: D <= 48, A <= 24, P <= 64, 32 reward terms), as plain
# declarations: tests/test_env_spec.py restates the closures from these lists, tests/test_gpu_env_spec_envelope.py runs them
# ------------------------------------------------------------------------------------------------------------------------------
_WIDEST_SINCOS = (1, 4, 6, 11, 15, 20, 26, 30, 32, 34, 37, 39, 42, 43, 45, 46, 47)      # 17 dims on both sides of dim 32
_WIDEST_REPLACE = (0, 13, 33, 40, 47)
CORNER_DECLS = {
    # D = 48, A = 24, P = 30 id + 17 sincos x 2 = 64 (dim 40 dropped).  32 terms: every kind on both states, several terms on dims 35
    # and 47 and on pair 17, terms on pairs 16..23 (return slots shared with pairs 0..7).  The first term reads dim 35 (pair 17): the
    # ctrl cost and bonus ride on slot 1, which pair 1's own terms (dims 2, 3) share.
    "widest": dict(
        obs_dim=48, act_dim=24,
        preproc=["drop" if d == 40 else "sincos" if d in _WIDEST_SINCOS else "id" for d in range(48)],
        postproc=["replace" if d in _WIDEST_REPLACE else "add" for d in range(48)],
        reward=[dict(kind="linear", dim=35, w=0.8),
                dict(kind="square", dim=34, w=-0.3),
                dict(kind="abs", dim=35, w=0.2, when="next_obs"),
                dict(kind="inside", dim=47, w=0.5, lo=-0.4, hi=0.6),
                dict(kind="outside", dim=47, w=-0.7, lo=-1.2, hi=1.1, when="next_obs"),
                dict(kind="linear", dim=46, w=0.4, when="next_obs"),
                dict(kind="square", dim=3, w=-0.05),
                dict(kind="abs", dim=2, w=-0.15, when="next_obs"),
                dict(kind="linear", dim=0, w=1.0),
                dict(kind="inside", dim=1, w=0.3, lo=-0.5, hi=0.5, when="next_obs"),
                dict(kind="outside", dim=5, w=-0.25, lo=-1.5, hi=1.5),
                dict(kind="square", dim=32, w=-0.1, when="next_obs"),
                dict(kind="linear", dim=33, w=-0.6),
                dict(kind="abs", dim=40, w=0.35),
                dict(kind="linear", dim=40, w=0.12, when="next_obs"),
                dict(kind="square", dim=41, w=-0.08),
                dict(kind="inside", dim=44, w=0.9, lo=0.0, hi=2.0),
                dict(kind="outside", dim=38, w=-0.45, lo=-0.8, hi=0.9, when="next_obs"),
                dict(kind="linear", dim=20, w=0.22),
                dict(kind="abs", dim=21, w=-0.33),
                dict(kind="square", dim=30, w=0.07, when="next_obs"),
                dict(kind="linear", dim=31, w=-0.18, when="next_obs"),
                dict(kind="inside", dim=12, w=0.6, lo=-1.0, hi=0.2, when="next_obs"),
                dict(kind="outside", dim=18, w=-0.2, lo=-0.3, hi=0.3),
                dict(kind="abs", dim=47, w=0.11),
                dict(kind="linear", dim=47, w=0.27, when="next_obs"),
                dict(kind="square", dim=36, w=-0.04),
                dict(kind="linear", dim=39, w=0.5, when="next_obs"),
                dict(kind="abs", dim=43, w=-0.09, when="next_obs"),
                dict(kind="square", dim=45, w=-0.06),
                dict(kind="linear", dim=35, w=-0.2),
                dict(kind="outside", dim=26, w=-0.3, lo=-2.0, hi=2.0, when="next_obs")],
        ctrl_cost=0.02, bonus=0.5),
    # the smallest env: one dim, one action, one feature, no reward terms (ctrl cost only, on pair 0)
    "tiny": dict(obs_dim=1, act_dim=1, preproc=["id"], reward=[], ctrl_cost=0.1),
    # two dims, the first dropped, the second sin / cos: P = 2 from one dim
    "tiny_sincos": dict(obs_dim=2, act_dim=2, preproc=["drop", "sincos"], postproc=["add", "replace"],
                        reward=[dict(kind="square", dim=1, w=-0.5)], ctrl_cost=0.03, bonus=0.25),
    # odd D = 47: the last pair (23, return slot 7, Philox group 11) holds dim 46 alone, which is sin / cos, replaced, and read by a
    # pre-step and a next-obs term.  P = 1 drop, 4 sincos, 42 id = 50.
    "odd_tail": dict(
        obs_dim=47, act_dim=13,
        preproc=["drop" if d == 0 else "sincos" if d in (3, 20, 35, 46) else "id" for d in range(47)],
        postproc=["replace" if d in (5, 46) else "add" for d in range(47)],
        reward=[dict(kind="linear", dim=2, w=1.0), dict(kind="square", dim=46, w=-0.2, when="next_obs"),
                dict(kind="abs", dim=46, w=0.3), dict(kind="inside", dim=45, w=0.4, lo=-0.5, hi=0.5, when="next_obs"),
                dict(kind="linear", dim=33, w=-0.1)],
        ctrl_cost=0.01, bonus=0.2),
    # the first term reads the next state: the ctrl cost and bonus ride on its pair (6), which has no pre-step term of its own
    "first_next": dict(
        obs_dim=20, act_dim=5,
        preproc=["drop" if d == 0 else "sincos" if d in (7, 13) else "id" for d in range(20)],
        postproc=["replace" if d == 13 else "add" for d in range(20)],
        reward=[dict(kind="linear", dim=13, w=0.5, when="next_obs"), dict(kind="square", dim=4, w=-0.1),
                dict(kind="inside", dim=19, w=0.3, lo=-0.5, hi=1.0), dict(kind="abs", dim=12, w=-0.2, when="next_obs")],
        ctrl_cost=0.05, bonus=1.5),
}


def corner_spec(name):
    from cadm_amd.env_spec import EnvDecl
    return EnvDecl(**CORNER_DECLS[name])


def check_class_api_on_spec(spec, tmp_path, epochs):
    """The class API on a user's simulator that declares its closures by a spec (wrapped the way the reference's NormalizedEnv wraps
    an env): fit, plan through MPCController (finite, inside [-1, 1]), warm-started replan, predict, context, and save / load / replan
    bit for bit."""
    from cadm_amd.caller import DevicePlannerState
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel
    from cadm_amd.policies.mpc_controller import MPCController
    from cadm_amd.samplers.model_sample_processor import ModelSampleProcessor

    class UserSim:                                       # a user's simulator: declares its closures, is no built-in class
        cadm_env_spec = spec
        observation_space, action_space, proc_observation_space_dims = spec.observation_space, spec.action_space, spec.proc_obs_dim
        obs_preproc, obs_postproc, targ_proc, reward = spec.obs_preproc, spec.obs_postproc, spec.targ_proc, spec.reward

    class Normalized:                                    # the reference's NormalizedEnv wrapper shape
        def __init__(self, e):
            self.wrapped_env = e
            for k in ("observation_space", "action_space", "proc_observation_space_dims", "obs_preproc", "obs_postproc", "targ_proc", "reward"):
                setattr(self, k, getattr(e, k))
    env = Normalized(UserSim())
    D, A, Hh, F, H = spec.obs_dim, spec.act_dim, 10, 10, 6
    kw = dict(hidden_nonlinearity="swish", context_out_dim=10, n_forwards=H, n_candidates=64, ensemble_size=5, n_particles=10, use_cem=True,
              batch_size=32, state_diff=1, normalize_input=True, back_coeff=0.5, weight_decays=SPEC_WD, weight_decay_coeff=1.0,
              context_weight_decays=SPEC_CWD + (0.0001,), history_length=Hh, future_length=F)
    model = MLPEnsembleCEMDynamicsModel("dyn", env, **kw)
    assert model.engine.spec == spec
    rng = np.random.default_rng(0)
    paths = []
    for L in (30, 45, 12):
        obs = rng.standard_normal((L, D)).astype(np.float32)
        paths.append(dict(observations=obs, actions=rng.uniform(-1, 1, (L, A)).astype(np.float32), rewards=rng.standard_normal(L),
                          cp_obs=0.1 * rng.standard_normal((L, D * Hh)).astype(np.float32),
                          cp_act=rng.uniform(-1, 1, (L, A * Hh)).astype(np.float32)))
    d = ModelSampleProcessor(context=True, future_length=F).process_samples(paths)
    model.fit(d["concat_obs"], d["concat_act"], d["concat_next_obs"], d["cp_observations"], d["cp_actions"], d["concat_bool"], epochs=epochs)
    policy = MPCController("mpc", env, model, use_cem=True, n_candidates=64, horizon=H, num_rollouts=2, context=True)
    o, cpo, cpa = rng.standard_normal((2, D)), 0.1 * rng.standard_normal((2, D * Hh)), rng.uniform(-1, 1, (2, A * Hh))
    mean, var = np.zeros((2, H, A)), np.full((2, H, A), 0.25)
    plan, _ = policy.get_actions(o, cpo, cpa, mean, var)
    assert plan.shape == (2, H, A) and np.isfinite(plan).all() and np.abs(plan).max() <= 1.0
    warm = np.concatenate([plan[:, 1:], np.zeros((2, 1, A))], axis=1)          # the samplers' CEM warm start
    plan2, _ = policy.get_actions(o, cpo, cpa, warm, var)
    assert np.isfinite(plan2).all()
    assert DevicePlannerState(model, 2).eng.spec == spec          # the device-resident caller state builds on the same engine
    mu, sd = model.predict(o, plan[:, 0], cpo, cpa, return_std=True)
    assert np.isfinite(mu).all() and np.isfinite(sd).all() and (sd > 0).all()
    cp = model.get_context_pred(cpo, cpa)
    assert np.isfinite(np.asarray(cp)).all()
    path = str(tmp_path / "params")
    model.save(path)
    model2 = MLPEnsembleCEMDynamicsModel("dyn", env, **kw)
    model2.load(path)
    model._call = model2._call = 7
    a1 = model.get_action(o, cpo, cpa, warm, var)
    a2 = model2.get_action(o, cpo, cpa, warm, var)
    assert np.isfinite(a1).all() and np.abs(a1).max() <= 1.0
    np.testing.assert_array_equal(a1, a2)
