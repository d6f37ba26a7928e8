"""CPU: the numpy restatement of the value-expansion targets (tests/targets_ref.py, the twin of csrc/imagine_targets.hip) -- hand-worked
cases, identities of the float64 form, the float32 form's distance from it, and the refusals of `planner.imagine_targets_args`."""
import numpy as np
import pytest

import targets_ref as tref
from cadm_amd import planner as hplanner

F = np.float32
INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------- 1: by hand
def _hand():
    """m = 1, n = 4, k = 3; gamma = lambda = 0.5 and values that are exact in binary.  Branch 0: a full row; 1: terminated at step 1;
    2: diverged at step 1; 3: cut by max_disagreement = 1 at step 2."""
    rew = np.array([[1, 2, 4], [1, 10, 0], [1, 0, 0], [1, 2, 4]], F).T.reshape(3, 1, 4)
    valid = np.array([[1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 1, 1]], np.uint8).T.reshape(3, 1, 4)
    done = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0]], np.uint8).T.reshape(3, 1, 4)
    dis = np.array([[.5, .25, .125], [.5, .25, 0], [.5, 0, 0], [.5, .25, 5]], F).T.reshape(3, 1, 4)
    boot = np.array([[10, 20, 40, 24], [10, 20, 40, 80], [10, 20, 40, 80], [10, 20, 40, 80]], F).T.reshape(4, 1, 4)
    return dict(rew=rew, valid=valid, done=done, disagreement=dis, boot=boot)


def _rows(x):
    return np.asarray(x)[:, 0, :].T.tolist()      # [branch][t]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_worked_rows(dtype):
    out = tref.targets(**_hand(), gamma=0.5, lam=0.5, max_disagreement=1.0, var_floor=8.0, dtype=dtype)
    assert out["lambda_return"].dtype == dtype and out["nstep"].dtype == dtype
    # full: G_2 = 4 + .5 * 24 = 16;  G_1 = 2 + .5 * (.5 * 40 + .5 * 16) = 16;  G_0 = 1 + .5 * (.5 * 20 + .5 * 16) = 10
    # terminated: G_1 = 10 (no bootstrap);  G_0 = 1 + .5 * (.5 * 20 + .5 * 10) = 8.5
    # diverged: G_0 = 1 + .5 * 20, the value of the last finite state;   cut: G_1 = 2 + .5 * 40 = 22;  G_0 = 1 + .5 * (10 + 11) = 11.5
    assert _rows(out["lambda_return"]) == [[10.0, 16.0, 16.0], [8.5, 10.0, 0.0], [11.0, 0.0, 0.0], [11.5, 22.0, 0.0]]
    # full: 1 + .5 * 20;  1 + .5 * 2 + .25 * 40;  1 + 1 + .25 * 4 + .125 * 24.   terminated: 11;  1 + .5 * 10 = 6, and 6 at every longer horizon
    assert _rows(out["nstep"]) == [[11.0, 12.0, 6.0], [11.0, 6.0, 6.0], [11.0, 0.0, 0.0], [11.0, 12.0, 0.0]]
    assert _rows(out["nstep_ok"]) == [[1, 1, 1], [1, 1, 1], [1, 0, 0], [1, 1, 0]]
    assert _rows(out["used"]) == [[1, 1, 1], [1, 1, 0], [1, 0, 0], [1, 1, 0]]
    assert out["L"].tolist() == [[3, 2, 1, 2]] and out["term"].tolist() == [[False, True, False, False]]
    # STEVE: h = 1: 11 x 4, var 0;  h = 2: 12, 6, 12: mean 10, var (4 + 16 + 4) / 3 = 8;  h = 3: 6, 6: var 0.   w = 1 / (var + 8)
    assert out["steve_count"][:, 0].tolist() == [4, 3, 2]
    assert out["steve_mean"][:, 0].tolist() == [11.0, 10.0, 6.0] and out["steve_var"][:, 0].tolist() == [0.0, 8.0, 0.0]
    # W = .125 + .0625 + .125 = .3125;  S = 1.375 + .625 + .75 = 2.75: one correctly rounded division of exact operands each
    assert out["steve"].tolist() == [dtype(8.8)] and out["steve_weight"][:, 0].tolist() == [dtype(0.4), dtype(0.2), dtype(0.4)]
    assert out["steve_fallback"].tolist() == [0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_worked_penalty(dtype):
    """the full row under penalty 2: r~ = rew - 2 * disagreement = 0, 1.5, 3.75"""
    h = {key: v[:, :, :1] for key, v in _hand().items()}
    out = tref.targets(**h, gamma=0.5, lam=0.5, penalty=2.0, dtype=dtype)
    # G_2 = 3.75 + 12 = 15.75;  G_1 = 1.5 + .5 * (20 + 7.875) = 15.4375;  G_0 = 0 + .5 * (10 + 7.71875) = 8.859375
    assert _rows(out["lambda_return"]) == [[8.859375, 15.4375, 15.75]]
    # 0 + .5 * 20;  .5 * 1.5 + .25 * 40;  .75 + .25 * 3.75 + .125 * 24
    assert _rows(out["nstep"]) == [[10.0, 10.75, 4.6875]]


# ---------------------------------------------------------------------------------------------------------------------- 2: identities
def _draw(seed, m=6, n=4, k=None):
    rng = np.random.default_rng(1000 + seed)
    k = int(rng.integers(1, 16)) if k is None else k
    return tref.make_inputs(m, n, k, seed), k, rng


def test_identities_of_the_float64_form():
    tol = dict(rtol=1e-12, atol=1e-12)
    for seed in range(20):
        x, k, rng = _draw(seed)
        beta, gamma = float(rng.choice([0.0, 0.7])), float(rng.uniform(0.9, 1.0))
        kw = dict(penalty=beta, max_disagreement=[None, 1.5][seed % 2], dtype=np.float64)
        rt = x["rew"].astype(np.float64) - float(F(beta)) * x["disagreement"].astype(np.float64)
        b, g = x["boot"].astype(np.float64), float(F(gamma))
        # lambda = 0: the one-step target of every used step (the last step of a terminated row: its reward alone)
        o = tref.targets(**x, gamma=gamma, lam=0.0, **kw)
        L, term = o["L"], o["term"]
        t = np.arange(k)[:, None, None]
        one = np.where((t == L[None] - 1) & term[None], rt, rt + g * b[1:])
        np.testing.assert_allclose(o["lambda_return"], np.where(t < L[None], one, 0.0), **tol)
        assert ((o["used"] > 0) == (t < L[None])).all()
        # lambda = 1: the lambda-return of the start state is its longest n-step target
        o = tref.targets(**x, gamma=gamma, lam=1.0, **kw)
        has = L >= 1
        ii, jj = np.nonzero(has)
        np.testing.assert_allclose(o["lambda_return"][0][has], o["nstep"][L[has] - 1, ii, jj], **tol)
        assert (o["nstep_ok"][L[has] - 1, ii, jj] == 1).all() and (o["nstep_ok"][:, ~has] == 0).all()
        # gamma = 1, no penalty, nothing to bootstrap from: the plain reward sum
        o = tref.targets(x["rew"], x["valid"], x["done"], x["disagreement"], np.zeros_like(x["boot"]), 1.0, lam=1.0,
                         max_disagreement=kw["max_disagreement"], dtype=np.float64)
        total = np.where(t < L[None], x["rew"].astype(np.float64), 0.0).sum(axis=0)
        np.testing.assert_allclose(o["lambda_return"][0], total, **tol)
        np.testing.assert_allclose(o["nstep"][L[has] - 1, ii, jj], total[has], **tol)


def test_steve_is_a_convex_combination_or_the_fallback():
    seen = 0
    for seed in range(20):
        x, k, _ = _draw(seed)
        o = tref.targets(**x, gamma=0.97, var_floor=1e-2, dtype=np.float64)
        w, mean = o["steve_weight"], o["steve_mean"]
        for i in range(w.shape[1]):
            on = w[:, i] > 0
            if on.any():
                assert mean[on, i].min() - 1e-12 <= o["steve"][i] <= mean[on, i].max() + 1e-12
                np.testing.assert_allclose(w[:, i].sum(), 1.0, rtol=1e-12)
                assert (o["steve_count"][on, i] >= 2).all() and o["steve_fallback"][i] == 0
                seen += 1
        # no horizon with two valid branches: one branch alone stays alive
        y = {key: v.copy() for key, v in x.items()}
        y["valid"][:, :, 1:] = 0
        o = tref.targets(**y, gamma=0.97, var_floor=1e-2, dtype=np.float64)
        assert (o["steve_count"] <= 1).all() and (o["steve_fallback"] == 1).all() and (o["steve_weight"] == 0).all()
        np.testing.assert_array_equal(o["steve"], y["boot"][0, :, 0].astype(np.float64))
    assert seen >= 60


# ---------------------------------------------------------------------------------------------------------------------- 3: float32 against float64
def test_float32_chain_stays_within_its_operation_count():
    """lambda_return and nstep of the float32 form lie within 2 (k + 3) 2^-24 (sum_t |rew| + penalty sum_t |disagreement| + max_t |boot|)
    of the float64 form, per row: the operation count of the chain times the sum of the magnitudes of its terms."""
    worst = 0.0
    for seed in range(200):
        x, k, rng = _draw(seed)
        beta = float(rng.choice([0.0, 0.7]))
        kw = dict(gamma=float(rng.uniform(0.9, 1.0)), lam=float(rng.uniform()), penalty=beta, max_disagreement=[None, 1.5][seed % 2])
        a, b = tref.targets(**x, **kw, dtype=np.float32), tref.targets(**x, **kw, dtype=np.float64)
        for key in ("nstep_ok", "used", "L", "term"):
            np.testing.assert_array_equal(a[key], b[key])
        mag = (np.abs(x["rew"].astype(np.float64)).sum(axis=0) + float(F(beta)) * np.abs(x["disagreement"].astype(np.float64)).sum(axis=0)
               + np.abs(x["boot"].astype(np.float64)).max(axis=0))
        bound = 2.0 * (k + 3) * 2.0 ** -24 * mag
        for key in ("lambda_return", "nstep"):
            err = np.abs(a[key].astype(np.float64) - b[key]).max(axis=0)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), "%s, seed %d: worst ratio to the bound %.3f" % (key, seed, float((err / bound).max()))
    print("\nworst |float32 - float64| relative to the bound: %.3f" % worst)


STEVE_MEASURED = 4.04e-7      # the worst distance `_steve_distance` measures on its own seeded inputs (float32 against float64)


def _steve_distance():
    worst = 0.0
    for seed in range(200):
        x, _, rng = _draw(seed)
        kw = dict(gamma=float(rng.uniform(0.9, 1.0)), var_floor=1e-2)
        a, b = tref.targets(**x, **kw, dtype=np.float32), tref.targets(**x, **kw, dtype=np.float64)
        np.testing.assert_array_equal(a["steve_count"], b["steve_count"])
        np.testing.assert_array_equal(a["steve_fallback"], b["steve_fallback"])
        scale = np.abs(b["nstep"]).max()
        if scale > 0:
            worst = max(worst, float(np.abs(a["steve"].astype(np.float64) - b["steve"]).max() / scale))
    return worst


def test_float32_steve_against_float64():
    """No closed bound: the inverse-variance weights amplify the rounding of a small variance.  Measured on these 200 seeded draws
    (var_floor = 1e-2) the worst |float32 - float64| of `steve` relative to max |nstep| is 4.04e-7 (STEVE_MEASURED); four times that is
    asserted."""
    worst = _steve_distance()
    print("\nworst |steve32 - steve64| / max |nstep|: %.3e" % worst)
    assert worst <= 4.0 * STEVE_MEASURED


# ---------------------------------------------------------------------------------------------------------------------- 4: the GPU test's shapes
def test_group_rule():
    """`targets_ref.group` / `lds_bytes`, the restated `tgt_group` / `tgt_lds_bytes` of csrc/imagine_targets.hip, on the shapes
    tests/test_gpu_imagine_targets.py launches: the three whose group the 48 KiB budget or m cuts, the shapes it leaves alone, and
    the refusal"""
    assert tref.lds_bytes(8, 16, 64) == 8 * 5632 <= 48 * 1024 < tref.lds_bytes(9, 16, 64)
    for (m, n, k), (G, owned) in tref.GROUPS.items():
        assert tref.group(m, n, k) == G and [min(G, m - i) for i in range(0, m, G)] == owned and sum(owned) == m
    assert tref.group(20, 16, 64) < 256 // 16 and tref.group(9, 100, 20) == 256 // 100 and tref.group(3, 300, 4) == 1 and 300 > tref.THREADS
    # the shapes from before: none is cut by the budget
    for m, n, k, steve in tref.SHAPES:
        if steve and (m, n, k) not in tref.GROUPS:
            assert tref.group(m, n, k) == min(max(256 // n, 1), m), (m, n, k)
    assert tref.group(1, 700, 20) == 0 and tref.group(2, 700, 14) == 1 and tref.lds_bytes(1, 700, 14) == 5 * 9800 + 8 * 14


@pytest.mark.parametrize("m,n,k,steve", tref.SHAPES, ids=["m%d-n%d-k%d" % s[:3] for s in tref.SHAPES])
def test_every_branch_occurs_at_every_shape(m, n, k, steve):
    """over the 9 variants and 3 parameter sets tests/test_gpu_imagine_targets.py::test_against_restatement runs at a shape, the
    restatement reaches every branch of the arithmetic the shape admits -- what a bit-equal kernel is then known to have computed"""
    seen = set()
    for v in range(9):
        x = tref.variant(m, n, k, v)
        for cfg in tref.CONFIGS:
            gamma, lam, beta, maxd = cfg
            want = tref.targets(**x, gamma=gamma, lam=lam, penalty=beta, max_disagreement=maxd, var_floor=tref.FLOOR if steve else None)
            seen |= tref.branches(x, cfg, want, steve)
    need = tref.needed(k, steve)
    assert seen >= need, "never occurred: %s" % sorted(need - seen)


# ---------------------------------------------------------------------------------------------------------------------- 5: the parser
def _batch(k=3, m=2, n=2, D=5):
    z = np.zeros((k, m, n), F)
    return dict(rew=z, valid=np.ones((k, m, n), np.uint8), done=np.zeros((k, m, n), np.uint8), disagreement=z, states=np.zeros((k + 1, m, n, D), F))


def test_parser_accepts_and_resolves():
    a = hplanner.imagine_targets_args(_batch(), 0.99, has_value=True)
    assert (a.m, a.n, a.k) == (2, 2, 3) and a.bootstrap == "value" and a.var_floor is None and a.max_disagreement == INF
    assert a.gamma == float(F(0.99)) and a.lam == float(F(0.95)) and a.penalty == 0.0
    assert hplanner.imagine_targets_args(_batch(), 1.0, bootstrap="auto", has_q=True).bootstrap == "q"
    assert hplanner.imagine_targets_args(_batch(), 1.0, has_value=True, has_q=True).bootstrap == "value"
    assert hplanner.imagine_targets_args(_batch(), 1.0, bootstrap="q", has_value=True, has_q=True).bootstrap == "q"
    a = hplanner.imagine_targets_args(_batch(), 0.5, 0.0, np.zeros((4, 2, 2), F), penalty=1.5, max_disagreement=2.0, steve=dict(var_floor=0.1))
    assert a.bootstrap == "given" and a.var_floor == float(F(0.1)) and a.max_disagreement == 2.0 and a.penalty == 1.5 and a.lam == 0.0
    import torch
    tb = {key: torch.as_tensor(v) for key, v in _batch().items()}
    assert hplanner.imagine_targets_args(tb, 0.9, bootstrap=torch.zeros(4, 2, 2)).bootstrap == "given"


def test_parser_refusals():
    ok = np.zeros((4, 2, 2), F)
    f = hplanner.imagine_targets_args
    for drop in ("rew", "valid", "done", "disagreement", "states"):
        b = _batch()
        del b[drop]
        with pytest.raises(ValueError, match="lacks %s" % drop):
            f(b, 0.9, bootstrap=ok)
    with pytest.raises(ValueError, match="must be the dict"):
        f(None, 0.9, bootstrap=ok)
    for key in ("valid", "done", "disagreement"):
        b = _batch()
        b[key] = b[key][:, :1]
        with pytest.raises(ValueError, match=r"batch\['%s'\]" % key):
            f(b, 0.9, bootstrap=ok)
    b = _batch()
    b["rew"] = b["rew"][0]
    with pytest.raises(ValueError, match=r"batch\['rew'\]"):
        f(b, 0.9, bootstrap=ok)
    b = _batch()
    b["states"] = b["states"][:-1]
    with pytest.raises(ValueError, match=r"batch\['states'\]"):
        f(b, 0.9, bootstrap=ok)
    for name, kw in (("gamma", dict(gamma=0.0)), ("gamma", dict(gamma=1.01)), ("gamma", dict(gamma=float("nan"))), ("gamma", dict(gamma="x")),
                     ("gamma", dict(gamma=True)), ("lam", dict(lam=-0.1)), ("lam", dict(lam=1.5)), ("lam", dict(lam=float("nan"))),
                     ("penalty", dict(penalty=-1.0)), ("penalty", dict(penalty=INF)), ("penalty", dict(penalty=float("nan"))),
                     ("max_disagreement", dict(max_disagreement=0.0)), ("max_disagreement", dict(max_disagreement=-2.0)),
                     ("max_disagreement", dict(max_disagreement=float("nan"))),
                     ("var_floor", dict(steve=dict(var_floor=0.0))), ("var_floor", dict(steve=dict(var_floor=INF))),
                     ("var_floor", dict(steve=dict(var_floor=float("nan")))), ("steve must be", dict(steve=dict(floor=1.0))),
                     ("steve must be", dict(steve=0.1))):
        args = dict(gamma=0.9, bootstrap=ok)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            f(_batch(), **args)
    assert f(_batch(), 0.9, bootstrap=ok, max_disagreement=INF).max_disagreement == INF
    with pytest.raises(ValueError, match="branches >= 2"):
        f(_batch(n=1), 0.9, bootstrap=np.zeros((4, 2, 1), F), steve=dict(var_floor=0.1))
    assert f(_batch(n=1), 0.9, bootstrap=np.zeros((4, 2, 1), F)).n == 1
    # the bootstrap: a model that declares neither is told all three choices
    with pytest.raises(ValueError, match=r"(?s)'value'.*'q'.*tensor or array"):
        f(_batch(), 0.9)
    with pytest.raises(ValueError, match="needs a model with cem_terminal_value"):
        f(_batch(), 0.9, bootstrap="value", has_q=True)
    with pytest.raises(ValueError, match="needs a model with cem_terminal_q"):
        f(_batch(), 0.9, bootstrap="q", has_value=True)
    with pytest.raises(ValueError, match="bootstrap must be"):
        f(_batch(), 0.9, bootstrap="v", has_value=True)
    for bad in (np.zeros((3, 2, 2), F), np.zeros((4, 2, 2, 1), F), None):
        with pytest.raises(ValueError, match="bootstrap"):
            f(_batch(), 0.9, bootstrap=bad, has_value=True)
