"""GPU: the open-loop prediction error (csrc/horizon.hip) off the one geometry of tests/test_gpu_horizon.py.

1  The statistics kernel `cadm_horizon_error` at every width of its LDS tile (WT = 16, 8, 4, 2, 1) and at the edges of its
   parameters -- horizon_ref.SHAPES, one row each -- against the float64 restatement within horizon_ref.kernel_bound, counts exact;
   on the rows horizon_ref.INVARIANT_ROWS the bitwise invariants (launch cuts, strided truth, the three load paths) and on
   horizon_ref.NONFINITE_ROWS non-finite values on every load path; the refusals of what does not fit.
2  The composite `cadm_eval_horizon` on ant, slim humanoid, pendulum and cartpole, on a vanilla stochastic and a deterministic
   E = 1, p = 1 engine, at F = H and F = 1: against the fp32 oracle's trajectory (the propagated 1e-5 bar) and bitwise against
   rollout_returns + horizon_error; device-drawn noise against the oracle's Philox streams fed to the same composite.
3  evaluate_horizon of the classes on cartpole and on a vanilla stochastic halfcheetah, equal to the engine call they make.

tests/test_horizon_ref.py (CPU) shows the bars of 1 on the references alone.  Measured on an MI355X: 1 at most 0.435 of its bar (one
window; every other row below 0.14), 2 at most 0.016 of the propagated trajectory bar, device-drawn noise at most 0.019 of its."""
import types

import numpy as np
import pytest
import torch

from cadm_amd import _lib, synth
from cadm_amd._lib import ptr
from helpers import make_engine, oracle_problem
from horizon_ref import (IDS, INVARIANT_ROWS, NONFINITE_ROWS, SHAPES, chain, check_against_oracle, kernel_bound, make_mask, oracle_bound,
                         row_inputs, row_mask, stats64, worst_ratio)
from oracle import nets as onets
from oracle import philox as ophilox
from oracle import planner as oplanner

pytestmark = pytest.mark.gpu

KEYS = ("se", "spread", "se_member", "count", "diverged")
SUMS = ("se", "spread", "se_member")
FILL = 1e30              # what surrounds the arrays under test: finite, and visible in any sum that reads it
INV = [SHAPES[i] for i in INVARIANT_ROWS]
INV_IDS = [IDS[i] for i in INVARIANT_ROWS]


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_identical(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s differs" % (what, k)


@pytest.fixture(scope="module")
def eng(gpu):
    """One halfcheetah engine for every row of 1: the statistics kernel reads no model."""
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=5, seed=1)
    e = make_engine(prob, p=10)
    yield e
    e.close()


def at_offset(eng, traj, k):
    """`traj` copied into a larger device buffer k floats behind its 16-byte aligned start: a contiguous view (engine._t hands it on
    as it is), so the kernel reads from ptr + 4 k."""
    big = torch.full((traj.size + 8,), FILL, dtype=torch.float32, device=eng.device)
    view = big[k:k + traj.size].view(traj.shape)
    view.copy_(torch.from_numpy(traj))
    assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
    return view


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("row", SHAPES, ids=IDS)
def test_statistics_kernel_at_its_tile_widths_and_edges(eng, row):
    """Worst |diff| / bound on an MI355X, in table order: 0.058, 0.059, 0.048, 0.060, 0.074, 0.045, 0.063, 0.079, 0.044, 0.135, 0.435
    -- digit for digit what the float32 restatement gives on the host (tests/test_horizon_ref.py): the library is built without
    contraction of a * b + c, so the kernel's roundings are the restatement's."""
    traj, truth = row_inputs(row)
    mask = row_mask(row)
    got = _np(eng.horizon_error(traj, truth, mask, E=row["E"]))
    ref = stats64(traj, truth, mask, row["E"])
    assert ref["count"].min() > 0
    np.testing.assert_array_equal(got["count"], ref["count"])
    np.testing.assert_array_equal(got["diverged"], 0)
    assert got["se_member"].shape == (row["E"], row["F"], row["D"])
    worst = worst_ratio(got, ref, kernel_bound(traj, truth, mask, row["E"], chain(row)))
    print("%s: kernel vs float64, worst |diff| / bound %.3f" % (row["what"], worst))
    assert worst <= 1.0, "%s: worst |diff| / bound %.3f" % (row["what"], worst)
    if row["p"] == 1:                            # one particle: exactly no spread, the member is the ensemble, bit for bit
        assert (got["spread"].view(np.uint32) == 0).all()
        assert np.array_equal(got["se_member"][0].view(np.uint32), got["se"].view(np.uint32))


@pytest.mark.parametrize("row", [r for r in SHAPES if r["m"] < 20], ids=[i for i, r in zip(IDS, SHAPES) if r["m"] < 20])
def test_all_invalid_mask_gives_exact_zeros(eng, row):
    traj, truth = row_inputs(row)
    got = _np(eng.horizon_error(traj, truth, np.zeros((row["m"], row["F"]), np.float32), E=row["E"]))
    for k in KEYS:
        assert (got[k].view(np.uint32) == 0).all(), "%s is not all +0" % k


@pytest.mark.parametrize("row", INV, ids=INV_IDS)
def test_launch_cuts_strided_truth_and_load_paths_give_the_same_bits(eng, row):
    traj, truth = row_inputs(row)
    mask = row_mask(row)
    m, f, d, e = row["m"], row["F"], row["D"], row["E"]
    base = _np(eng.horizon_error(traj, truth, mask, E=e))
    # one launch per block of 64 windows
    calls = [64] * (m // 64) + ([m % 64] if m % 64 else [])
    assert_identical(_np(eng.horizon_error(traj, truth, mask, calls=calls, E=e)), base, "launches %r" % (calls,))
    # truth rows F D + 7 floats apart, the padding never read
    wide = np.full((m, f * d + 7), FILL, np.float32)
    wide[:, :f * d] = truth.reshape(m, f * d)
    assert_identical(_np(eng.horizon_error(traj, wide, mask, E=e, truth_ld=f * d + 7)), base, "truth_ld = F D + 7")
    assert_identical(_np(eng.horizon_error(traj, wide, mask, calls=calls, E=e, truth_ld=f * d + 7)), base, "truth_ld = F D + 7, launches")
    # the same values read from ptr, ptr + 4, + 8, + 12: the vector path (and its scalar tail) at offset 0, the scalar path elsewhere
    for k in range(4):
        assert_identical(_np(eng.horizon_error(at_offset(eng, traj, k), truth, mask, E=e)), base, "buffer offset %d floats" % k)


@pytest.mark.parametrize("row", [SHAPES[i] for i in NONFINITE_ROWS], ids=[IDS[i] for i in NONFINITE_ROWS])
def test_non_finite_values_on_every_load_path(eng, row):
    """A NaN in the last element of window 10's span and an Inf in the first element of window 11's (step 0), a NaN in the ragged last
    tile (window m - 1, last step): each flags its own window and no other, whichever path loaded it, and a flagged (window, step) is
    in no sum -- the same bits as a clean run whose mask drops exactly those pairs (a mask drops the steps behind as well, so each
    step is compared with the mask that drops its own pairs)."""
    clean, truth = row_inputs(row)
    mask = row_mask(row)
    m, f, e = row["m"], row["F"], row["E"]
    planted = clean.copy()
    planted[0, 10, -1, -1] = np.nan
    planted[0, 11, 0, 0] = np.inf
    planted[f - 1, m - 1, row["p"] // 2, 0] = np.nan
    assert (mask[[10, 11, m - 1]] == 1).all() and (m - 1) % 64 < 16          # (the last block holds fewer windows than any tile width)
    base = _np(eng.horizon_error(clean, truth, mask, E=e))
    first, last = mask.copy(), mask.copy()
    first[10, 0] = first[11, 0] = 0.0
    last[m - 1, f - 1] = 0.0
    drop_first, drop_last = _np(eng.horizon_error(clean, truth, first, E=e)), _np(eng.horizon_error(clean, truth, last, E=e))
    want_div = np.zeros(f, np.int32)
    want_div[0] += 2
    want_div[f - 1] += 1
    for k in (0, 1):
        got = _np(eng.horizon_error(at_offset(eng, planted, k), truth, mask, E=e))
        what = "buffer offset %d" % k
        np.testing.assert_array_equal(got["diverged"], want_div, err_msg=what)
        np.testing.assert_array_equal(got["count"], base["count"] - want_div, err_msg=what)
        assert all(np.isfinite(got[s]).all() for s in SUMS), what
        for s in SUMS:
            bits = lambda o, h: o[s][..., h, :].view(np.uint32)
            assert np.array_equal(bits(got, 0), bits(drop_first, 0)), "%s: %s step 0" % (what, s)
            assert np.array_equal(bits(got, f - 1), bits(drop_last, f - 1)), "%s: %s last step" % (what, s)
            for h in range(1, f - 1):
                assert np.array_equal(bits(got, h), bits(base, h)), "%s: %s step %d holds no planted value" % (what, s, h)


@pytest.mark.parametrize("p,d,ld_off,names", [(185, 64, 0, ("does not fit", "p (185)")), (10, 65, 0, ("D (65)",)),
                                              (10, 18, -1, ("truth_row_stride",))], ids=["p185-D64", "D65", "truth_ld-below-FD"])
def test_refusals_leave_the_outputs_alone(eng, p, d, ld_off, names):
    m, f, e = 3, 2, 5
    ld = f * d + ld_off
    dev = eng.device
    traj, truth, mask = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (f * m * p * d, m * f * d, m * f))
    partials = torch.zeros(f * ((2 + e) * d + 2), dtype=torch.float32, device=dev)
    out = dict(se=torch.full((f, d), -7.0, device=dev), spread=torch.full((f, d), -7.0, device=dev),
               se_member=torch.full((e, f, d), -7.0, device=dev), count=torch.full((f,), -7, dtype=torch.int32, device=dev),
               diverged=torch.full((f,), -7, dtype=torch.int32, device=dev))
    rc = eng.lib.cadm_horizon_error(ptr(traj), ptr(truth), ld, ptr(mask), m, f, p, e, d, 0, ptr(partials), 1, ptr(out["se"]), ptr(out["spread"]),
                                    ptr(out["se_member"]), ptr(out["count"]), ptr(out["diverged"]), 1, eng.stream)
    msg = eng.lib.cadm_last_error().decode()
    assert rc == -1 and msg.startswith("cadm_horizon_error:") and all(n in msg for n in names), "rc %d: %r" % (rc, msg)
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())
    with pytest.raises(_lib.CadmError, match="cadm_horizon_error"):      # the same through the wrapper
        eng.horizon_error(traj.view(f, m, p, d), truth[:m * ld].view(m, ld) if ld_off else truth.view(m, f, d), mask.view(m, f), E=e,
                          truth_ld=ld if ld_off else None)


# ---------------------------------------------------------------------------------------------------------------------- 2
H_ENG = 5


class Comp:
    """One model + dataset + fp32 oracle trajectory (tests/test_gpu_horizon.py's Case at any kind, E, p, F), built once and left
    unchanged.  Truth is drawn independently of the model at the oracle trajectory's per-dim scale."""

    def __init__(self, kind, context, e, p, seed, n=70, f=3, det=False):
        self.kind, self.context, self.e, self.p, self.n, self.f, self.det = kind, context, e, p, n, f, det
        self.prob = prob = synth.make_problem(env=kind, context=context, E=e, m=n, H=H_ENG, seed=seed)
        D, A = prob["D"], prob["A"]
        self.D = D
        rng = np.random.default_rng(seed + 100)
        acts = rng.uniform(-1, 1, (n, 1, H_ENG, A)).astype(np.float32)
        if kind == "pendulum":                   # a third of the torques beyond the clip at +-2 (behind_rollout.kind_inputs)
            acts = (acts * np.float32(3.0)).astype(np.float32)
            assert (np.abs(acts) > 2.0).mean() > 0.1
        if kind == "cartpole":                   # discrete: the windows hold one-hot actions, as `fit` receives them
            acts = np.eye(A, dtype=np.float32)[rng.integers(0, A, (n, 1, H_ENG))]
        self.acts = acts
        self.eps = rng.standard_normal((H_ENG, n, 1, p, D)).astype(np.float32)
        self.mask = make_mask(n, f)
        self.o = oracle_problem(prob, np.float32)
        self.T = oplanner.context_table_indexed(onets.context_forward(self.o["cp"], self.o["cp_obs"], self.o["cp_act"], self.o["st"]), 0) if context else None
        self.t_ref = self.oracle_traj(self.eps[:f])
        scale = np.sqrt((self.t_ref.astype(np.float64) ** 2).mean(axis=(0, 1, 2)))
        self.truth = (rng.standard_normal((n, f, D)) * scale).astype(np.float32)
        obs = rng.standard_normal((n, f, D)).astype(np.float32)
        obs[:, 0] = prob["obs"].astype(np.float32)
        self.ds = dict(obs=obs.reshape(n, f * D), act=acts[:, 0, :f].reshape(n, f * A).copy(), obs_next=self.truth.reshape(n, f * D),
                       future_bool=self.mask)
        if context:
            self.ds.update(cp_obs=prob["cp_obs"], cp_act=prob["cp_act"])

    def oracle_traj(self, eps):
        """[F,n,p,D]: the fp32 oracle's F-step rollout of every window under noise eps [F,n,1,p,D]"""
        o = self.o
        _, t = oplanner.rollout_indexed(o["env"], o["ff"], o["st"], o["obs"], self.T, self.acts[:, :, :self.f].copy(), eps.astype(np.float32).copy(),
                                        self.e, self.p, self.det, return_traj=True)
        assert t.dtype == np.float32
        return t.reshape(self.f, self.n, self.p, self.D)

    def engine(self):
        return make_engine(self.prob, p=self.p, deterministic=self.det)

    def dev(self, eng):
        return {k: eng._t(v) for k, v in self.ds.items()}


COMPOSITES = [   # kind, context, E, p, F, deterministic, seed
    ("ant", True, 5, 10, 3, False, 51),                  # P != D
    ("slim_humanoid", True, 5, 15, 3, False, 52),        # D odd
    ("pendulum", True, 5, 5, 3, False, 53),              # D = 3, torques beyond the clip
    ("cartpole", True, 5, 5, 3, False, 54),              # discrete: one-hot actions
    ("halfcheetah", False, 5, 5, 3, False, 55),          # vanilla stochastic: no cp_obs / cp_act in the dataset
    ("halfcheetah", False, 1, 1, 3, True, 56),           # deterministic, one particle
    ("halfcheetah", True, 5, 10, 5, False, 57),          # F = H
    ("halfcheetah", True, 5, 10, 1, False, 57),          # F = 1
]


@pytest.mark.parametrize("kind,context,e,p,f,det,seed", COMPOSITES,
                         ids=["%s-%s-E%d-p%d-F%d" % (c[0], "ctx" if c[1] else "vanilla", c[2], c[3], c[4]) for c in COMPOSITES])
def test_composite_on_every_kind_and_at_its_corners(gpu, kind, context, e, p, f, det, seed):
    c = Comp(kind, context, e, p, seed, f=f, det=det)
    eng = c.engine()
    dev = c.dev(eng)
    assert ("cp_obs" in dev) == context and c.mask.shape == (c.n, f)
    eps = None if det else c.eps[:f].copy()
    comp = _np(eng.eval_horizon(dev, c.n, f, eps=eps))
    # (a) the fp32 oracle's trajectory, within the propagated 1e-5 trajectory bar
    with np.errstate(divide="ignore", invalid="ignore"):         # (its report divides by a reference that is 0 for one particle)
        check_against_oracle(c, comp, "%s E=%d p=%d F=%d" % (kind, e, p, f), e=e)
    # (b) F steps of the H-step engine + the statistics kernel: the same bits
    ctx = eng.context_forward(c.prob["cp_obs"], c.prob["cp_act"]) if context else None
    _, traj = eng.rollout_returns(c.prob["obs"], ctx, c.acts, eps=None if det else c.eps, want_traj=True)
    assert traj.shape[0] == H_ENG
    iso = _np(eng.horizon_error(traj[:f].contiguous(), c.truth, c.mask))
    assert_identical(comp, iso, "composite vs rollout_returns + horizon_error")
    assert comp["count"].min() > 0
    if det:
        assert (comp["spread"].view(np.uint32) == 0).all()
        assert np.array_equal(comp["se_member"][0].view(np.uint32), comp["se"].view(np.uint32))
    else:
        assert (comp["spread"] > 0).all()
    eng.close()


def test_device_noise_is_the_oracles_streams(gpu):
    """The composite's device-drawn noise is, chunk by chunk, the oracle's Philox stream of iteration word 2 x chunk index with rows
    keyed inside the launch: the composite fed those streams gives the same statistics.  Drawn and injected normals differ by
    Box-Muller ulps (tests/test_gpu_planner.py allows 4e-6 absolute), so the bar is the propagated trajectory bar plus twice what
    +-4e-6 on the streams does to the fp32 oracle's own statistics.  Measured on an MI355X: device-drawn against injected differ by at most 3.0e-7 relative
(0.019 of the bar, se_member at chunk 128); the +-4e-6 on the streams moves the oracle's statistics by up to 1.2e-6 relative."""
    n, f, p, e = 150, 5, 10, 5
    c = Comp("halfcheetah", True, e, p, 47, n=n, f=f)
    eng = c.engine()
    dev = c.dev(eng)
    rng = np.random.default_rng(8)
    for chunk in (64, 128):
        streams = np.concatenate([ophilox.eps_normals(7, 3, 2 * ci, min(chunk, n - w0), 1, p, f, c.D)
                                  for ci, w0 in enumerate(range(0, n, chunk))], axis=1)
        assert streams.shape == (f, n, 1, p, c.D) and streams.dtype == np.float32
        drawn = _np(eng.eval_horizon(dev, n, f, chunk=chunk, seed=7, call=3))
        fed = _np(eng.eval_horizon(dev, n, f, chunk=chunk, eps=streams.copy()))
        t_a = c.oracle_traj(streams)
        t_b = c.oracle_traj(streams + np.float32(4e-6) * rng.choice([-1.0, 1.0], streams.shape).astype(np.float32))
        s_a, s_b = stats64(t_a, c.truth, c.mask, e), stats64(t_b, c.truth, c.mask, e)
        bound = oracle_bound(t_a, c.truth, c.mask, e)
        case = types.SimpleNamespace(t_ref=t_a, truth=c.truth, mask=c.mask)
        check_against_oracle(case, fed, "chunk %d, fed the oracle's streams" % chunk, e=e)
        np.testing.assert_array_equal(drawn["count"], fed["count"])
        assert drawn["diverged"].sum() == 0
        for k in SUMS:
            sens = np.abs(s_a[k] - s_b[k])
            bar = bound[k] + 2 * sens
            diff = np.abs(drawn[k].astype(np.float64) - fed[k])
            print("chunk %d %s: device-drawn vs injected, worst |diff| / bar %.3f (worst relative %.2e; the streams' +-4e-6 moves the oracle by "
                  "up to %.2e relative)" % (chunk, k, (diff / bar).max(), (diff / np.abs(fed[k])).max(), (sens / np.abs(s_a[k])).max()))
            assert (diff <= bar).all(), "chunk %d %s: worst |diff| / bar %.3f" % (chunk, k, (diff / bar).max())
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 3
def _equals_the_engine_call(model, dev_arrays, fb, res, seed):
    """mse / spread / member_mse of the class are the engine's sums over the counts, exactly, for the (seed, call) the class used."""
    eng = model.engine
    dev = {k: eng._t(v) for k, v in dev_arrays.items()}
    dev["future_bool"] = eng._t(np.asarray(fb) > 0)
    out = _np(eng.eval_horizon(dev, fb.shape[0], fb.shape[1], seed=seed, call=model._eval_call))
    cnt = out["count"].astype(np.float64)[:, None]
    np.testing.assert_array_equal(res["count"], out["count"])
    np.testing.assert_array_equal(res["mse"], out["se"].astype(np.float64) / cnt)
    np.testing.assert_array_equal(res["spread"], out["spread"].astype(np.float64) / cnt)
    np.testing.assert_array_equal(res["member_mse"], out["se_member"].astype(np.float64) / cnt[None])


def test_class_on_cartpole(gpu):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDM
    from cadm_amd.envs import EnvSpec
    D, A, Hh, f, n, e = 4, 2, 10, 3, 80, 5
    model = CaDM("dyn", EnvSpec("cartpole"), hidden_nonlinearity="swish", n_forwards=5, n_candidates=64, ensemble_size=e, n_particles=5,
                 use_cem=False, batch_size=64, history_length=Hh, future_length=f, seed=3)
    rng = np.random.default_rng(20)
    onehot = lambda steps: np.eye(A)[rng.integers(0, A, (n, steps))].reshape(n, steps * A)
    obs = 0.1 * rng.standard_normal((n, f * D))
    w = dict(obs=obs, act=onehot(f), obs_next=obs + 0.05 * rng.standard_normal((n, f * D)), cp_obs=0.1 * rng.standard_normal((n, D * Hh)),
             cp_act=onehot(Hh))
    fb = make_mask(n, f).astype(np.float64)
    args = (w["obs"], w["act"], w["obs_next"], w["cp_obs"], w["cp_act"], fb)
    model.fit(*args, epochs=1)
    res = model.evaluate_horizon(*args, seed=11)
    assert sorted(res) == ["count", "diverged", "member_mse", "mse", "rmse", "spread"]
    assert res["mse"].shape == res["spread"].shape == (f, D) and res["member_mse"].shape == (e, f, D)
    assert res["count"].shape == res["diverged"].shape == res["rmse"].shape == (f,)
    np.testing.assert_array_equal(res["count"], (np.cumprod(fb, axis=1) > 0).sum(0))
    assert res["count"].min() > 0 and res["diverged"].sum() == 0
    assert all(np.isfinite(res[k]).all() for k in res) and (res["spread"] > 0).all()
    _equals_the_engine_call(model, w, fb, res, 11)


def test_vanilla_stochastic_class_on_halfcheetah(gpu):
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Vanilla
    from cadm_amd.envs import EnvSpec
    D, A, n, e = 18, 6, 80, 5
    model = Vanilla("dyn", EnvSpec("halfcheetah"), hidden_nonlinearity="swish", n_forwards=5, n_candidates=64, ensemble_size=e, n_particles=5,
                    use_cem=True, batch_size=32, normalize_input=True, deterministic=False, seed=4)
    rng = np.random.default_rng(21)
    obs = rng.standard_normal((n, D))
    act, nxt = rng.uniform(-1, 1, (n, A)), obs + 0.1 * rng.standard_normal((n, D))
    model.fit(obs, act, nxt, epochs=1)
    res = model.evaluate_horizon(obs, act, nxt, seed=12)
    assert res["mse"].shape == res["spread"].shape == (1, D) and res["member_mse"].shape == (e, 1, D) and res["count"].tolist() == [n]
    assert all(np.isfinite(res[k]).all() for k in res) and (res["spread"] > 0).all() and res["diverged"].sum() == 0
    _equals_the_engine_call(model, dict(obs=obs, act=act, obs_next=nxt), np.ones((n, 1)), res, 12)
