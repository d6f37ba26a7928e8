"""CPU: the numpy restatement of the risk-aware candidate scores (tests/risk_ref.py) held to known answers, the tail-fraction rule of the
model classes, what their constructors refuse before an engine is built, and the new exports as far as they go without a ctx."""
import ctypes

import numpy as np
import pytest

import risk_ref

M, N, P, E = 2, 37, 20, 5


def _rows(seed=0, p=P):
    return np.random.default_rng(seed).uniform(-30.0, 30.0, (M, N, p))


def test_kappa_zero_gives_the_mean():
    r = _rows()
    mean = risk_ref.score(r, "mean")
    np.testing.assert_allclose(mean, r.mean(axis=-1), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(risk_ref.score(r, "mean_std", kappa=0.0), mean)
    np.testing.assert_array_equal(risk_ref.score(r, "member_std", kappa=0.0, E=E), mean)


def test_std_modes_by_hand():
    r = np.array([[1.0, 3.0, 5.0, 7.0]])                              # mu 4, deviations -3 -1 1 3: sigma = sqrt(5)
    assert abs(risk_ref.score(r, "mean_std", kappa=2.0)[0] - (4.0 - 2.0 * np.sqrt(5.0))) <= 1e-15
    assert abs(risk_ref.score(r, "mean_std", kappa=-1.0)[0] - (4.0 + np.sqrt(5.0))) <= 1e-15
    # two members (1, 3) and (5, 7): member means 2 and 6, sigma_E = 2
    assert abs(risk_ref.score(r, "member_std", kappa=0.5, E=2)[0] - 3.0) <= 1e-15
    # every particle its own member: the member spread is the particle spread
    rr = _rows(1)
    np.testing.assert_allclose(risk_ref.score(rr, "member_std", kappa=1.5, E=P), risk_ref.score(rr, "mean_std", kappa=1.5), rtol=0, atol=1e-12)
    np.testing.assert_allclose(risk_ref.score(rr, "mean_std", kappa=1.0), rr.mean(-1) - rr.std(-1), rtol=0, atol=1e-12)


def test_cvar_ends_and_ties():
    r = _rows(2)
    np.testing.assert_allclose(risk_ref.score(r, "cvar", k=P), r.mean(axis=-1), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(risk_ref.score(r, "cvar", k=1), r.min(axis=-1))
    np.testing.assert_allclose(risk_ref.score(r, "cvar", k=3), np.sort(r, axis=-1)[..., :3].mean(axis=-1), rtol=0, atol=1e-13)
    t = np.array([[2.0, -1.0, 2.0, -1.0, 0.0, -0.0]])
    np.testing.assert_array_equal(risk_ref.ranks(t), [[4, 0, 5, 1, 2, 3]])      # ties (-0.0 against 0.0 included) to the lower index
    assert risk_ref.score(t, "cvar", k=2)[0] == -1.0 and risk_ref.score(t, "cvar", k=3)[0] == -2.0 / 3.0
    assert risk_ref.score(t, "cvar", k=5)[0] == 0.0                   # one of the two 2.0 counts
    c = np.full((1, 7), 3.25)
    for k in (1, 4, 7):
        assert risk_ref.score(c, "cvar", k=k)[0] == 3.25


def test_positive_affine_maps_commute_with_every_score():
    """S(a r + b) = a S(r) + b for a > 0"""
    r = _rows(3)
    for a, b in ((2.0, -7.0), (0.125, 100.0), (3.7, 0.3)):
        for mode, kw in (("mean", {}), ("mean_std", dict(kappa=2.0)), ("mean_std", dict(kappa=-1.0)), ("member_std", dict(kappa=0.5, E=E)),
                         ("cvar", dict(k=2)), ("cvar", dict(k=P - 1))):
            np.testing.assert_allclose(risk_ref.score(a * r + b, mode, **kw), a * risk_ref.score(r, mode, **kw) + b, rtol=0, atol=1e-11)
    # not for a < 0: the pessimistic score of -r is not minus the pessimistic score of r
    assert np.abs(risk_ref.score(-r, "mean_std", kappa=2.0) + risk_ref.score(r, "mean_std", kappa=2.0)).max() > 1.0


def test_member_std_vanishes_when_the_member_means_coincide():
    rng = np.random.default_rng(4)
    q = P // E
    d = rng.uniform(-5.0, 5.0, (M, N, E, q))
    d -= d.mean(axis=-1, keepdims=True)                               # every member: mean 0 ...
    r = (d + 12.5).reshape(M, N, P)                                   # ... then the same mean for all
    s = risk_ref.score(r, "member_std", kappa=2.0, E=E)
    np.testing.assert_allclose(s, 12.5, rtol=0, atol=1e-12)
    assert np.abs(risk_ref.score(r, "mean_std", kappa=2.0) - 12.5).min() > 1.0      # the particles themselves do spread


def test_non_finite_rows_score_the_plain_mean():
    r = _rows(5)
    bad = r.copy()
    bad[0, 1, 3], bad[0, 5, 0], bad[1, 2, 19], bad[1, 7, 4], bad[1, 7, 9] = np.nan, np.inf, -np.inf, np.inf, -np.inf
    hit = np.zeros((M, N), bool)
    hit[0, 1] = hit[0, 5] = hit[1, 2] = hit[1, 7] = True
    with np.errstate(invalid="ignore"):
        plain = bad.sum(axis=-1) / P
    assert np.isnan(plain[0, 1]) and plain[0, 5] == np.inf and plain[1, 2] == -np.inf and np.isnan(plain[1, 7])
    for mode, kw in (("mean", {}), ("mean_std", dict(kappa=2.0)), ("member_std", dict(kappa=-1.0, E=E)), ("cvar", dict(k=1)), ("cvar", dict(k=P))):
        got = risk_ref.score(bad, mode, **kw)
        np.testing.assert_array_equal(got[hit], plain[hit])
        np.testing.assert_array_equal(got[~hit], risk_ref.score(r, mode, **kw)[~hit])      # the finite neighbours are unaffected


def test_generic_over_dtype():
    r32 = _rows(6).astype(np.float32)
    for mode, kw in (("mean_std", dict(kappa=2.0)), ("member_std", dict(kappa=0.5, E=E)), ("cvar", dict(k=2))):
        got = risk_ref.score(r32, mode, **kw)
        assert got.dtype == np.float32
        assert np.abs(got - risk_ref.score(r32.astype(np.float64), mode, **kw)).max() <= 1e-5 * 30.0


@pytest.mark.parametrize("alpha,p,k", [(0.1, 20, 2), (0.05, 20, 1), (0.01, 20, 1), (0.15, 20, 3), (0.25, 20, 5), (0.26, 20, 6), (0.5, 5, 3),
                                       (0.2, 5, 1), (0.3, 10, 3), (0.7, 10, 7), (0.35, 20, 7), (1.0, 20, 20), (1.0, 5, 5), (1e-9, 20, 1),
                                       (0.999, 20, 20), (0.95, 20, 19), (0.6, 5, 3), (1.0 / 3.0, 30, 10)])
def test_tail_fraction_to_particle_count(alpha, p, k):
    """k = min(p, max(1, ceil(round(alpha p, 6)))): 0.1 * 20, 0.15 * 20, 0.35 * 20 and 0.7 * 10 sit a rounding above an integer in
    binary and must not take one more particle."""
    from cadm_amd.engine import HipEngine
    assert HipEngine.cvar_k(alpha, p) == k == risk_ref.cvar_k(alpha, p)


def test_constructors_refuse_bad_score_kwargs_before_an_engine_is_built(monkeypatch):
    from cadm_amd import engine as engine_mod
    from cadm_amd.dynamics import mlp_cadm_ensemble_cem_dynamics as cadm_mod
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as VanillaModel
    from cadm_amd.envs import make_env_spec

    def no_engine(*a, **kw):
        raise AssertionError("the engine was built before the kwargs were refused")
    monkeypatch.setattr(engine_mod.HipEngine, "__init__", no_engine)
    env = make_env_spec("halfcheetah")
    base = dict(name="dyn", env=env, hidden_sizes=(32,) * 4, n_forwards=5, n_candidates=64, ensemble_size=5, n_particles=20, use_cem=True)
    cases = ((dict(cem_score="variance", cem_risk=1.0), "cem_score must be"),
             (dict(cem_score="mean", cem_risk=1.0), "cem_risk configures a risk-aware score"),
             (dict(cem_risk=0.0), "cem_risk configures a risk-aware score"),
             (dict(cem_score="mean_std"), "needs a finite cem_risk"),
             (dict(cem_score="member_std"), "needs a finite cem_risk"),
             (dict(cem_score="cvar"), "needs a finite cem_risk"),
             (dict(cem_score="mean_std", cem_risk=float("nan")), "needs a finite cem_risk"),
             (dict(cem_score="member_std", cem_risk=float("inf")), "needs a finite cem_risk"),
             (dict(cem_score="cvar", cem_risk=float("nan")), "needs a finite cem_risk"),
             (dict(cem_score="cvar", cem_risk=0.0), "tail fraction"),
             (dict(cem_score="cvar", cem_risk=-0.1), "tail fraction"),
             (dict(cem_score="cvar", cem_risk=1.5), "tail fraction"),
             (dict(use_cem=False, cem_score="mean_std", cem_risk=1.0), "need use_cem=True"),
             (dict(use_cem=False, cem_score="cvar", cem_risk=0.1), "need use_cem=True"))
    for cls in (cadm_mod.MLPEnsembleCEMDynamicsModel, VanillaModel):
        for bad, msg in cases:
            with pytest.raises(ValueError, match=msg):
                cls(**dict(base, **bad))
        with pytest.raises(NotImplementedError, match="continuous actions only"):
            cls(**dict(base, env=make_env_spec("cartpole"), cem_score="cvar", cem_risk=0.1))
        import torch.distributed as dist
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
        with pytest.raises(NotImplementedError, match="more than one rank"):
            cls(**dict(base, process_group=object(), cem_score="mean_std", cem_risk=0.0))
        # legal kwargs get as far as the engine: kappa = 0 and a negative kappa with the std modes, alpha = 1 with cvar
        for ok in (dict(cem_score="mean_std", cem_risk=0.0), dict(cem_score="member_std", cem_risk=-1.0), dict(cem_score="cvar", cem_risk=1.0)):
            with pytest.raises(AssertionError, match="the engine was built"):
                cls(**dict(base, **ok))


def test_new_exports_are_bound_and_refuse_null_arguments_without_a_gpu():
    import os
    from cadm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("cadm_particle_score", "cadm_scored_plan"):
        assert hasattr(raw, name), "%s is not exported" % name
        assert name in _lib.SIGNATURES, "%s is not bound" % name
    assert [f[0] for f in _lib.ScoreParams._fields_] == ["mode", "kappa", "k"] and ctypes.sizeof(_lib.ScoreParams) == 12
    assert _lib.SCORE_MODES == {"mean": 0, "mean_std": 1, "member_std": 2, "cvar": 3}
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    P_ = ctypes.c_void_p(ctypes.addressof(buf))
    sc, prm = _lib.ScoreParams(), _lib.MppiParams()
    prm.temperature = 1.0
    assert lib.cadm_particle_score(None, P_, 1, 1, ctypes.byref(sc), P_, None) == -1
    assert lib.cadm_last_error().decode().startswith("cadm_particle_score:")
    assert lib.cadm_scored_plan(None, ctypes.byref(sc), 0, ctypes.byref(prm), P_, None, None, P_, P_, None, None, 1, 1, 0, 0, P_, P_, None, None) == -1
    assert lib.cadm_last_error().decode().startswith("cadm_scored_plan:")
    assert lib.cadm_scored_plan(None, None, 0, None, P_, None, None, P_, P_, None, None, 1, 1, 0, 0, P_, P_, None, None) == -1
    assert lib.cadm_scored_plan(None, None, 2, ctypes.byref(prm), P_, None, None, P_, P_, None, None, 1, 1, 0, 0, P_, P_, None, None) == -1
    assert "update 2" in lib.cadm_last_error().decode()
