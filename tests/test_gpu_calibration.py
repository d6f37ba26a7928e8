"""GPU: calibration of the predictive distribution -- the statistics kernel (cadm_calibration_stats, csrc/calibration.hip), the
composite over a device-resident windowed dataset (cadm_eval_calibration) and the classes' evaluate_calibration.

1  The kernel against the float64 restatement (tests/calibration_ref.py) on the rows calibration_ref.ROWS of horizon_ref.SHAPES --
   tile widths 8, 1 and 16, p = 1, p / E = 1 with D = 1, E = 9, eleven blocks, one window: integers equal, crps / z2 / nll within
   calibration_ref.kernel_bound (built from the kernel header's rounding chains, never from a measured error), count / diverged
   equal to cadm_horizon_error's on the same tensors.
2  Planted windows with hand-written expectations: rank 0, rank p, a tie, coinciding particles, NaN and Inf on both load paths, a
   masked-out window.
3  Launch cuts, repeated runs and an unaligned buffer give the same bits.
4  The composite equals rollout_returns + calibration_stats chunk by chunk (same seed / call / iteration words), is invariant to
   the chunk size under injected noise, and counts what cadm_eval_horizon counts.  (Rank counts are never compared with the
   oracle's trajectory: a 1e-5 move flips a comparison.)
5  evaluate_calibration of both classes.
6  The refusals of the two entry points, each before any launch.
tests/test_calibration_ref.py (CPU) shows what the restatement itself tells apart."""
import ctypes as ct

import numpy as np
import pytest
import torch

from cadm_amd import _lib, synth
from cadm_amd._lib import ptr
from calibration_ref import INTS, ROWS, SHAPES, SUMS, WT, kernel_bound, make_mask, row_inputs, stats64, worst_ratio
from helpers import make_engine
from horizon_ref import IDS, row_mask

pytestmark = pytest.mark.gpu

KEYS = INTS + SUMS
FILL = 1e30              # what surrounds the arrays under test: finite, and visible in any sum that reads it


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_identical(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s differs" % (what, k)


def assert_matches_reference(got, traj, truth, mask, e, wt, what):
    ref = stats64(traj, truth, mask, e)
    for k in INTS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg="%s %s" % (what, k))
    worst = worst_ratio(got, ref, kernel_bound(traj, truth, mask, e, wt))
    print("%s: kernel vs float64, worst |diff| / bound %.3f" % (what, worst))
    assert worst <= 1.0, "%s: worst |diff| / bound %.3f" % (what, worst)
    return ref


@pytest.fixture(scope="module")
def eng(gpu):
    """One halfcheetah engine for 1, 2, 3 and 6: the statistics kernel reads no model."""
    prob = synth.make_problem(env="halfcheetah", context=True, E=5, m=1, H=5, seed=1)
    e = make_engine(prob, p=10)
    yield e
    e.close()


def at_offset(eng, traj, k):
    """`traj` in a larger device buffer k floats behind its 16-byte aligned start: the kernel reads from ptr + 4 k."""
    big = torch.full((traj.size + 8,), FILL, dtype=torch.float32, device=eng.device)
    view = big[k:k + traj.size].view(traj.shape)
    view.copy_(torch.from_numpy(traj))
    assert view.data_ptr() % 16 == 4 * k and view.is_contiguous()
    return view


# ---------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", ROWS, ids=[IDS[i] for i in ROWS])
def test_kernel_against_the_float64_restatement(eng, i):
    row = SHAPES[i]
    traj, truth = row_inputs(row)
    mask = row_mask(row)
    p, e, d, f = row["p"], row["E"], row["D"], row["F"]
    got = _np(eng.calibration_stats(traj, truth, mask, E=e))
    assert got["rank_hist"].shape == (f, d, p + 1) and got["rank_hist_member"].shape == (e, f, d, p // e + 1)
    ref = assert_matches_reference(got, traj, truth, mask, e, WT[i], row["what"])
    assert ref["count"].min() > 0
    assert (got["rank_hist"].sum(-1) == got["count"][:, None]).all() and (got["rank_hist_member"].sum(-1) == got["count"][None, :, None]).all()
    hor = _np(eng.horizon_error(traj, truth, mask, E=e))
    np.testing.assert_array_equal(got["count"], hor["count"])
    np.testing.assert_array_equal(got["diverged"], hor["diverged"])
    if p == 1:               # one particle: every pair is degenerate, its CRPS is |x - y|, and the member is the ensemble
        assert (got["degenerate"] == got["count"][:, None]).all() and (got["z2"].view(np.uint32) == 0).all() and (got["nll"].view(np.uint32) == 0).all()
        assert np.array_equal(got["rank_hist_member"][0], got["rank_hist"])
    else:
        assert got["degenerate"].sum() == 0 and got["ties"].sum() == 0


# ---------------------------------------------------------------------------------------------------------------------- 2
P2, E2, D2, M2, F2 = 6, 3, 4, 70, 2


def edge_inputs():
    rng = np.random.default_rng(12)
    traj = (rng.standard_normal((F2, M2, P2, D2)) * 2.0 + 1.0).astype(np.float32)
    truth = (rng.standard_normal((M2, F2, D2)) * 2.0).astype(np.float32)
    mask = np.ones((M2, F2), np.float32)
    truth[1, 0] = traj[0, 1].min(0) - 1.0                    # window 1: below every particle
    truth[2, 0] = traj[0, 2].max(0) + 1.0                    # window 2: above every particle
    traj[0, 3, :, 1] = [5.0, 1.0, 3.0, 3.0, 0.0, 4.0]       # window 3, dim 1: truth equals particles 2 and 3; two are strictly below
    truth[3, 0, 1] = 3.0
    traj[0, 4] = traj[0, 4, 0]                               # window 4: the particles coincide in every dim
    mask[5] = 0.0                                            # window 5: masked out
    mask[6, 1] = 0.0                                         # window 6: step 0 only
    traj[0, 10, P2 - 1, D2 - 1] = np.nan                     # window 10, step 0 (block 0)
    traj[1, 66, 0, 0] = np.inf                               # window 66, step 1 (block 1)
    return traj, truth, mask


def only(mask, w):
    """step 0 of window w and nothing else"""
    m = np.zeros_like(mask)
    m[w, 0] = 1.0
    return m


def test_planted_edges(eng):
    traj, truth, mask = edge_inputs()
    pe = P2 // E2
    run = lambda mk, k=0: _np(eng.calibration_stats(at_offset(eng, traj, k), truth, mk, E=E2))
    zero_but = lambda got, keep: all((got[k] == 0).all() for k in KEYS if k not in keep)

    got = run(only(mask, 1))                                 # rank 0
    assert (got["rank_hist"][0, :, 0] == 1).all() and got["rank_hist"].sum() == D2
    assert (got["rank_hist_member"][:, 0, :, 0] == 1).all() and got["rank_hist_member"].sum() == E2 * D2
    assert got["count"].tolist() == [1, 0] and zero_but(got, ("rank_hist", "rank_hist_member", "count") + SUMS)

    got = run(only(mask, 2))                                 # rank p
    assert (got["rank_hist"][0, :, P2] == 1).all() and got["rank_hist"].sum() == D2
    assert (got["rank_hist_member"][:, 0, :, pe] == 1).all() and got["rank_hist_member"].sum() == E2 * D2

    got = run(only(mask, 3))                                 # a tie: the rank counts strictly-less only
    assert got["ties"].tolist() == [[0, 1, 0, 0], [0, 0, 0, 0]] and got["rank_hist"][0, 1, 2] == 1 and got["rank_hist"][0, 1].sum() == 1
    # members (5, 1), (3, 3), (0, 4) against 3: ranks 1, 0, 1
    assert got["rank_hist_member"][:, 0, 1].tolist() == [[0, 1, 0], [1, 0, 0], [0, 1, 0]]

    got = run(only(mask, 4))                                 # coinciding particles: degenerate, in crps as |x - y|, in neither z2 nor nll
    assert got["degenerate"].tolist() == [[1] * D2, [0] * D2] and got["count"].tolist() == [1, 0]
    assert (got["z2"].view(np.uint32) == 0).all() and (got["nll"].view(np.uint32) == 0).all()
    want = np.abs(traj[0, 4, 0].astype(np.float64) - truth[4, 0])
    assert (np.abs(got["crps"][0] - want) <= (P2 + 4) * 2.0 ** -24 * want).all() and (got["crps"][1] == 0).all()

    for w, step in ((10, 0), (66, 1)):                       # non-finite: diverged, and in nothing else
        mk = np.zeros_like(mask)
        mk[w] = 1.0
        for k in (0, 1):
            got = run(mk, k)
            assert got["diverged"].tolist() == [1 - step, step] and got["count"].tolist() == [step, 1 - step]
            assert got["rank_hist"].sum() == D2 and got["rank_hist"][step].sum() == 0 and np.isfinite(got["crps"]).all()

    got = run(only(mask, 5) * 0.0)                           # nothing valid: every output exactly zero
    assert zero_but(got, ())

    full = run(mask)                                         # everything at once, on both load paths
    assert full["count"].tolist() == [M2 - 2, M2 - 3] and full["diverged"].tolist() == [1, 1]
    assert full["ties"].sum() == 1 and full["degenerate"].sum() == D2
    assert_matches_reference(full, traj, truth, mask, E2, 16, "planted windows")
    assert_identical(run(mask, 1), full, "buffer offset 1 float")
    hor = _np(eng.horizon_error(traj, truth, mask, E=E2))
    np.testing.assert_array_equal(full["count"], hor["count"])
    np.testing.assert_array_equal(full["diverged"], hor["diverged"])


# ---------------------------------------------------------------------------------------------------------------------- 3
def test_launch_cuts_runs_and_alignment_give_the_same_bits(eng):
    row = dict(p=10, E=5, D=11, m=130, F=3)                  # 130 * 10 * 11 floats per step: steps 1 and 2 start off 16-byte alignment
    traj, truth = row_inputs(row)
    mask = make_mask(130, 3)
    base = _np(eng.calibration_stats(traj, truth, mask, E=5))
    assert_matches_reference(base, traj, truth, mask, 5, 16, "m = 130")
    assert_identical(_np(eng.calibration_stats(traj, truth, mask, E=5)), base, "second run")
    assert_identical(_np(eng.calibration_stats(traj, truth, mask, calls=[64, 64, 2], E=5)), base, "launches [64, 64, 2]")
    wide = np.full((130, 3 * 11 + 7), FILL, np.float32)
    wide[:, :33] = truth.reshape(130, 33)
    assert_identical(_np(eng.calibration_stats(traj, wide, mask, E=5, truth_ld=40)), base, "truth_ld = F D + 7")
    for k in range(4):
        assert_identical(_np(eng.calibration_stats(at_offset(eng, traj, k), truth, mask, E=5)), base, "buffer offset %d floats" % k)


# ---------------------------------------------------------------------------------------------------------------------- 4
E4, P4, F4, N4 = 5, 10, 3, 130


@pytest.fixture(scope="module")
def comp(gpu):
    prob = synth.make_problem(env="halfcheetah", context=True, E=E4, m=N4, H=F4, seed=61, trained_like=True)
    D, A = prob["D"], prob["A"]
    rng = np.random.default_rng(62)
    acts = rng.uniform(-1, 1, (N4, 1, F4, A)).astype(np.float32)
    obs = rng.standard_normal((N4, F4, D)).astype(np.float32)
    obs[:, 0] = prob["obs"].astype(np.float32)
    truth = (obs[:, :1] + rng.standard_normal((N4, F4, D))).astype(np.float32)
    mask = make_mask(N4, F4)
    ds = dict(obs=obs.reshape(N4, F4 * D), act=acts[:, 0].reshape(N4, F4 * A).copy(), obs_next=truth.reshape(N4, F4 * D), cp_obs=prob["cp_obs"],
              cp_act=prob["cp_act"], future_bool=mask)
    e = make_engine(prob, p=P4)
    c = dict(prob=prob, acts=acts, truth=truth, mask=mask, eng=e, dev={k: e._t(v) for k, v in ds.items()},
             eps=rng.standard_normal((F4, N4, 1, P4, D)).astype(np.float32))
    yield c
    e.close()


def test_composite_is_rollout_plus_statistics_chunk_by_chunk(comp):
    eng, prob = comp["eng"], comp["prob"]
    got = _np(eng.eval_calibration(comp["dev"], N4, F4, chunk=64, seed=7, call=3))
    ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"])                       # [E, N, C]: the batched encoder, as the composite forces it
    parts = []
    for ci, w0 in enumerate(range(0, N4, 64)):
        w1 = min(w0 + 64, N4)
        _, t = eng.rollout_returns(prob["obs"][w0:w1], ctx[:, w0:w1].contiguous(), comp["acts"][w0:w1], seed=7, call=3, it=2 * ci, want_traj=True)
        parts.append(t)
    assert len(parts) == 3
    traj = torch.cat(parts, dim=1)
    assert tuple(traj.shape) == (F4, N4, 1, P4, prob["D"])
    iso = _np(eng.calibration_stats(traj, comp["truth"], comp["mask"]))
    assert_identical(got, iso, "composite vs rollout_returns + calibration_stats")
    assert got["count"].min() > 0 and got["diverged"].sum() == 0 and got["degenerate"].sum() == 0
    assert (got["rank_hist"].sum(-1) == got["count"][:, None]).all()
    assert_matches_reference(got, traj.cpu().numpy().reshape(F4, N4, P4, -1), comp["truth"], comp["mask"], E4, 16, "model trajectory")
    # the same (seed, call): cadm_eval_horizon sees the same trajectories
    hor = _np(eng.eval_horizon(comp["dev"], N4, F4, chunk=64, seed=7, call=3))
    np.testing.assert_array_equal(got["count"], hor["count"])
    np.testing.assert_array_equal(got["diverged"], hor["diverged"])
    iso_h = _np(eng.horizon_error(traj, comp["truth"], comp["mask"]))
    assert np.array_equal(hor["spread"].view(np.uint32), iso_h["spread"].view(np.uint32))
    assert_identical(_np(eng.eval_calibration(comp["dev"], N4, F4, chunk=64, seed=7, call=3)), got, "second run")
    other = _np(eng.eval_calibration(comp["dev"], N4, F4, chunk=64, seed=7, call=4))
    assert not np.array_equal(other["crps"], got["crps"])
    np.testing.assert_array_equal(other["count"], got["count"])


def test_composite_is_invariant_to_the_chunk(comp):
    eng = comp["eng"]
    a = _np(eng.eval_calibration(comp["dev"], N4, F4, chunk=64, eps=comp["eps"].copy()))
    b = _np(eng.eval_calibration(comp["dev"], N4, F4, chunk=128, eps=comp["eps"].copy()))
    assert_identical(a, b, "chunk 64 vs 128")
    assert_identical(_np(eng.eval_calibration(comp["dev"], N4, F4, eps=comp["eps"].copy())), a, "chunk 64 vs one chunk")
    assert eng.lib.cadm_eval_calibration_workspace_bytes(eng._ctx, N4, F4, 64) > 0
    assert eng.lib.cadm_eval_calibration_workspace_bytes(eng._ctx, N4, F4, 100) == 0
    with pytest.raises(ValueError, match="multiple of 64"):
        eng.eval_calibration(comp["dev"], N4, F4, chunk=100)
    with pytest.raises(_lib.CadmError, match="n_forwards"):
        eng.eval_calibration(comp["dev"], N4, F4 + 1)


# ---------------------------------------------------------------------------------------------------------------------- 5
RESULT_KEYS = sorted(("rank_hist", "rank_hist_member", "ties", "degenerate", "count", "diverged", "crps", "z2", "nll", "z2_ideal", "coverage",
                      "nominal", "calibration_error"))


def _windows(rng, n, D, A, Hh, f):
    obs = rng.standard_normal((n, f * D))
    fb = np.ones((n, f))
    for i in range(0, n, 4):
        fb[i, (i // 4) % f + 1:] = 0.0
    fb[2] = 0.0
    return dict(obs=obs, act=rng.uniform(-1, 1, (n, f * A)), obs_next=obs + 0.1 * rng.standard_normal((n, f * D)),
                cp_obs=0.1 * rng.standard_normal((n, D * Hh)), cp_act=rng.uniform(-1, 1, (n, A * Hh)), future_bool=fb)


def check_result(res, f, d, p, e, count):
    assert sorted(res) == RESULT_KEYS
    k = p // 2
    assert res["rank_hist"].shape == (f, d, p + 1) and res["rank_hist_member"].shape == (e, f, d, p // e + 1)
    assert res["ties"].shape == res["degenerate"].shape == res["crps"].shape == res["z2"].shape == res["nll"].shape == (f, d)
    assert res["count"].shape == res["diverged"].shape == res["calibration_error"].shape == (f,)
    assert res["coverage"].shape == (f, d, k) and res["nominal"].shape == (k,)
    assert all(res[n].dtype == np.int64 for n in INTS) and all(res[n].dtype == np.float64 for n in SUMS + ("coverage", "nominal", "calibration_error"))
    np.testing.assert_array_equal(res["count"], count)
    assert (res["rank_hist"].sum(-1) == res["count"][:, None]).all() and (res["rank_hist_member"].sum(-1) == res["count"][None, :, None]).all()
    assert (np.diff(res["coverage"], axis=-1) <= 0).all() and (np.diff(res["nominal"]) < 0).all()
    assert p > 3 and res["z2_ideal"] == (p + 1.0) / (p - 3.0)
    assert res["diverged"].sum() == 0 and np.isfinite(res["crps"]).all() and (res["crps"] > 0).all()
    assert (res["calibration_error"] >= 0).all() and (res["calibration_error"] <= 1).all()


def test_class_api(gpu):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDM
    from cadm_amd.envs import EnvSpec
    D, A, Hh, f, H, e, p = 18, 6, 10, 4, 8, 5, 10
    kw = dict(hidden_nonlinearity="swish", n_forwards=H, n_candidates=64, ensemble_size=e, n_particles=p, use_cem=True, batch_size=64,
              history_length=Hh, future_length=f, seed=3)
    rng = np.random.default_rng(0)
    w = _windows(rng, 200, D, A, Hh, f)
    args = (w["obs"], w["act"], w["obs_next"], w["cp_obs"], w["cp_act"], w["future_bool"])
    models = [CaDM("dyn", EnvSpec("halfcheetah"), **kw) for _ in range(2)]
    with pytest.raises(RuntimeError, match="statistics"):
        models[0].evaluate_calibration(*args)
    for mdl in models:
        mdl.fit(*args, epochs=2)
    model, twin = models
    held = _windows(rng, 150, D, A, Hh, f)
    hargs = (held["obs"], held["act"], held["obs_next"], held["cp_obs"], held["cp_act"], held["future_bool"])
    n_ds, call, ecall = model._dataset["obs"].shape[0], model._call, model._eval_call
    res = model.evaluate_calibration(*hargs)
    check_result(res, f, D, p, e, (np.cumprod(held["future_bool"], axis=1) > 0).sum(0))
    assert np.isfinite(res["z2"]).all() and np.isfinite(res["nll"]).all() and res["degenerate"].sum() == 0
    assert model._dataset["obs"].shape[0] == n_ds and model._call == call and model._eval_call == ecall + 1
    # the counter is evaluate_horizon's: the two draw under different call words, and a repeat moves on
    res2 = model.evaluate_calibration(*hargs, chunk=64)
    assert not np.array_equal(res["crps"], res2["crps"])
    hor = model.evaluate_horizon(*hargs)
    np.testing.assert_array_equal(hor["count"], res["count"])
    assert model._eval_call == ecall + 3
    # count == 0 -> NaN
    r0 = model.evaluate_calibration(*hargs[:5], np.zeros_like(held["future_bool"]))
    assert (r0["count"] == 0).all() and r0["rank_hist"].sum() == 0
    assert all(np.isnan(r0[k]).all() for k in ("crps", "z2", "nll", "coverage", "calibration_error"))
    # planning is the same with or without evaluations in between
    o, cpo, cpa = rng.standard_normal((2, D)), 0.1 * rng.standard_normal((2, D * Hh)), rng.uniform(-1, 1, (2, A * Hh))
    mean, var = np.zeros((2, H, A)), np.full((2, H, A), 0.25)
    np.testing.assert_array_equal(model.get_action(o, cpo, cpa, mean, var), twin.get_action(o, cpo, cpa, mean, var))
    with pytest.raises(ValueError, match="no windows"):
        model.evaluate_calibration(*(a[:0] for a in hargs))
    # windows longer than the planning horizon
    long = CaDM("dyn", EnvSpec("halfcheetah"), **dict(kw, future_length=9))
    long.set_normalization(model.normalization)
    lw = _windows(rng, 70, D, A, Hh, 9)
    with pytest.raises(ValueError, match="n_forwards"):
        long.evaluate_calibration(lw["obs"], lw["act"], lw["obs_next"], lw["cp_obs"], lw["cp_act"], lw["future_bool"])


def test_vanilla_class_on_a_declared_env(gpu):
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Vanilla
    from cadm_amd.env_spec import EnvDecl
    spec = EnvDecl(7, 1, preproc=["id", "id", "sincos", "id", "drop", "id", "id"],          # tests/test_gpu_horizon.py's small_vanilla
                   reward=[dict(kind="linear", dim=0, when="next_obs"), dict(kind="square", dim=2, w=-0.1, when="next_obs"),
                           dict(kind="outside", dim=1, w=-1.0, lo=-1.5, hi=1.5, when="next_obs")], ctrl_cost=0.01)
    D, A = 7, 1
    model = Vanilla("dyn", spec, hidden_nonlinearity="swish", n_forwards=5, n_candidates=64, ensemble_size=5, n_particles=5, use_cem=True,
                    batch_size=32, normalize_input=True, deterministic=True)
    rng = np.random.default_rng(1)
    obs = rng.standard_normal((200, D))
    act, nxt = rng.uniform(-1, 1, (200, A)), obs + 0.1 * rng.standard_normal((200, D))
    model.fit(obs, act, nxt, epochs=2)
    res = model.evaluate_calibration(obs[:130], act[:130], nxt[:130])
    check_result(res, 1, D, 5, 5, [130])
    assert np.array_equal(res["rank_hist_member"].sum(-1), np.full((5, 1, D), 130))
    with pytest.raises(ValueError, match="no windows"):
        model.evaluate_calibration(obs[:0], act[:0], nxt[:0])


# ---------------------------------------------------------------------------------------------------------------------- 6
def _filled_out(dev, f, d, p, e):
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device=dev)
    z = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device=dev)
    out = dict(rank_hist=i(f, d, p + 1), rank_hist_member=i(e, f, d, p // e + 1), ties=i(f, d), degenerate=i(f, d), crps=z(f, d), z2=z(f, d), nll=z(f, d),
               count=i(f), diverged=i(f))
    c = _lib.CalibrationOut()
    for k, v in out.items():
        setattr(c, k, v.data_ptr())
    return out, c


REFUSALS = [   # id, p, E, D, m, window0, partials_blocks, null, what the message names
    ("null-traj", 10, 5, 18, 3, 0, 1, "traj", ("traj is null",)),
    ("null-out-member", 10, 5, 18, 3, 0, 1, "crps", ("out or one of its pointers",)),
    ("null-out", 10, 5, 18, 3, 0, 1, "out", ("out or one of its pointers",)),
    ("p-not-multiple-of-E", 10, 3, 18, 3, 0, 1, None, ("p (10)", "E (3)")),
    ("window0-32", 10, 5, 18, 3, 32, 2, None, ("window0 (32)",)),
    ("D65", 10, 5, 65, 3, 0, 1, None, ("D (65)",)),
    ("too-few-partials-blocks", 10, 5, 18, 70, 0, 1, None, ("partials_blocks (1)",)),
    ("p185-D64", 185, 5, 64, 3, 0, 1, None, ("does not fit", "p (185)")),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_statistics_refusals_leave_the_outputs_alone(eng, case):
    _, p, e, d, m, window0, blocks, null, names = case
    f, dev = 2, eng.device
    traj, truth, mask = (torch.zeros(n, dtype=torch.float32, device=dev) for n in (f * m * p * d, m * f * d, m * f))
    partials = torch.zeros(2 * f * 3 * d, dtype=torch.float32, device=dev)
    out, c = _filled_out(dev, f, d, p, max(e, 1))
    if null in out:
        setattr(c, null, None)
    rc = eng.lib.cadm_calibration_stats(None if null == "traj" else ptr(traj), ptr(truth), f * d, ptr(mask), m, f, p, e, d, window0, ptr(partials),
                                        blocks, None if null == "out" else ct.byref(c), 1, eng.stream)
    msg = eng.lib.cadm_last_error().decode()
    assert rc == -1 and msg.startswith("cadm_calibration_stats:") and all(n in msg for n in names), "rc %d: %r" % (rc, msg)
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())


@pytest.mark.parametrize("chunk,f,name", [(100, F4, "chunk (100)"), (64, F4 + 1, "n_forwards")], ids=["chunk-100", "F-above-H"])
def test_composite_refusals_leave_the_outputs_alone(comp, chunk, f, name):
    eng, dev = comp["eng"], comp["dev"]
    out, c = _filled_out(eng.device, f, eng.D, P4, E4)
    ws = torch.empty((1 << 24,), dtype=torch.uint8, device=eng.device)
    rc = eng.lib.cadm_eval_calibration(eng._ctx, ptr(dev["obs"]), ptr(dev["act"]), ptr(dev["obs_next"]), ptr(dev["cp_obs"]), ptr(dev["cp_act"]),
                                       ptr(dev["future_bool"]), N4, f, chunk, 0, 0, None, ptr(ws), ct.byref(c), eng.stream)
    msg = eng.lib.cadm_last_error().decode()
    assert rc == -1 and msg.startswith("cadm_eval_calibration:") and name in msg, "rc %d: %r" % (rc, msg)
    rc = eng.lib.cadm_eval_calibration(eng._ctx, ptr(dev["obs"]), ptr(dev["act"]), ptr(dev["obs_next"]), ptr(dev["cp_obs"]), ptr(dev["cp_act"]),
                                       ptr(dev["future_bool"]), N4, F4, 64, 0, 0, None, ptr(ws), None, eng.stream)
    assert rc == -1 and "null argument" in eng.lib.cadm_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())
