"""GPU: value-expansion targets (`cadm_imagine_targets`, csrc/imagine_targets.hip) against the float32 numpy restatement
(tests/targets_ref.py) bit for bit on synthetic arrays, positional independence, the input and workspace discipline, the refusals, the
class route and the absence of side effects.

The kernel reads no weights, so the kernel-level engine (pendulum, p = 5) is never rolled out.  Everything that rolls out runs on the
compiled-in halfcheetah 200 x 4 kernel with m = 3, branches = 3, horizon = 4.

Every output behind a division (steve, steve_mean, steve_var, steve_weight) is held to the restatement bit for bit as well: the
kernel's `__fdiv_rn` and numpy's float32 division are both correctly rounded.

The shapes, their planted variants and the bookkeeping of the branches are `targets_ref.SHAPES`, `variant` and `branches`:
tests/test_targets_ref.py runs them on the CPU and holds the restated `tgt_group` to the groups named here.  Three of the STEVE shapes
have a group the host cuts: (20, 16, 64) G = 8 of 16 by the 48 KiB budget (cap = G n under a cut G), (9, 100, 20) G = 2 with a partial
last group, (3, 300, 4) G = 1 with two passes of the row loop into the LDS tile."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import critic_ref as cref
import policy_ref as pref
import targets_ref as tref
import value_ref as vref
from cadm_amd import _lib
from cadm_amd import synth
from helpers import _np, make_engine, plan_act, plan_model

pytestmark = pytest.mark.gpu

F = np.float32
NAN = float("nan")
BIG = dict(hidden=(200,) * 4)
STEVE_KEYS = ("steve", "steve_weight", "steve_mean", "steve_var", "steve_count", "steve_fallback")
KEYS = ("lambda_return", "nstep", "nstep_ok", "used")
MAXD, FLOOR, CONFIGS = tref.MAXD, tref.FLOOR, tref.CONFIGS      # gamma, lam, penalty, max_disagreement of the three parameter sets


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %r %s against %r %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if got.dtype == np.float32:
        got, want = _bits(got), _bits(want)
    np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.fixture(scope="module")
def eng(gpu):
    prob = synth.make_problem(env="pendulum", context=False, E=5, m=2, H=3, seed=52)
    e = make_engine(prob, p=5)
    yield e
    assert not e._rollout_ready, "the kernel-level engine was rolled out"
    e.close()


def _dev(eng, x):
    return {key: torch.as_tensor(v).to(eng.device) for key, v in x.items()}


def _run(eng, x, cfg, floor=None):
    gamma, lam, beta, maxd = cfg
    d = _dev(eng, x)
    out = eng.imagine_targets(d["rew"], d["valid"], d["done"], d["disagreement"], d["boot"], gamma, lam, beta, maxd, floor)
    return {key: _np(v) for key, v in out.items()}


def _ref(x, cfg, floor=None):
    gamma, lam, beta, maxd = cfg
    return tref.targets(**x, gamma=gamma, lam=lam, penalty=beta, max_disagreement=maxd, var_floor=floor, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------- 1: bit for bit
_plant_row, _variant, SHAPES = tref.plant_row, tref.variant, tref.SHAPES      # (shared with tests/test_targets_ref.py, which runs them on the CPU)


@pytest.mark.parametrize("m,n,k,steve", SHAPES, ids=["m%d-n%d-k%d" % s[:3] for s in SHAPES])
def test_against_restatement(eng, m, n, k, steve):
    """Every output equals the float32 restatement bit for bit, on 9 planted variants of seeded inputs under 3 parameter sets, run to run;
    and the restatement shows that every branch of the arithmetic the shape admits occurred.  (130, 3, 2) is two workgroups of the STEVE
    form with a ragged second one; (300, 1, 3) two of the plain form.  (20, 16, 64): the 48 KiB budget cuts the group from 16 start
    states to 8, so the tile's stride is cap = 8 x 16 and the workgroups own 8, 8 and 4; (9, 100, 20): groups of 2 and a last one of 1;
    (3, 300, 4): one start state a workgroup, whose 300 rows take the row loop twice while it writes the tile -- the group is asserted
    against `targets_ref.group`, the restated `tgt_group`, before the launch."""
    floor = FLOOR if steve else None
    if (m, n, k) in tref.GROUPS:
        G, owned = tref.GROUPS[(m, n, k)]
        assert steve and tref.group(m, n, k) == G and [min(G, m - i) for i in range(0, m, G)] == owned
        assert G < min(max(256 // n, 1), m) or n > 256 or m % G, "the shape must cut the group, leave a partial one or take two row passes"
    seen = set()
    for v in range(9):
        x = _variant(m, n, k, v)
        for c, cfg in enumerate(CONFIGS):
            want = _ref(x, cfg, floor)
            got = _run(eng, x, cfg, floor)
            assert set(got) == set(KEYS + (STEVE_KEYS if steve else ()))
            for key in got:
                _same(got[key], want[key], "(%d, %d, %d) variant %d config %d: %s" % (m, n, k, v, c, key))
            if v == 0:
                again = _run(eng, x, cfg, floor)
                for key in got:
                    _same(again[key], got[key], "run to run: %s" % key)
            seen |= tref.branches(x, cfg, want, steve)
    need = tref.needed(k, steve)
    assert seen >= need, "never occurred: %s" % sorted(need - seen)


def test_lds_refusal_and_the_scan_without_steve(eng):
    """(1, 700, 20): one start state's 14000 targets do not fit the reduction's LDS tile, so the STEVE outputs are refused with a message
    that says so -- by the workspace query too -- and the scan without them runs (`test_against_restatement` holds its bits)."""
    x = _variant(1, 700, 20, 0)
    with pytest.raises(_lib.CadmError, match=r"cadm_imagine_targets: branches \(700\) x horizon \(20\) does not fit the STEVE reduction's LDS"):
        _run(eng, x, CONFIGS[0], FLOOR)
    assert eng.lib.cadm_imagine_targets_workspace_bytes(eng._ctx, 1, 700, 20, 1, None) == 0
    assert b"LDS" in eng.lib.cadm_last_error()
    assert eng.lib.cadm_imagine_targets_workspace_bytes(eng._ctx, 1, 700, 20, 0, None) > 0
    assert set(_run(eng, x, CONFIGS[0])) == set(KEYS)
    # the largest single start state that fits: 5 bytes a target and 8 k bytes
    assert eng.lib.cadm_imagine_targets_workspace_bytes(eng._ctx, 2, 700, 14, 1, None) > 0
    y = _variant(2, 700, 14, 8)
    want, got = _ref(y, CONFIGS[1], FLOOR), _run(eng, y, CONFIGS[1], FLOOR)
    for key in got:
        _same(got[key], want[key], "(2, 700, 14): %s" % key)


# ---------------------------------------------------------------------------------------------------------------------- 2: position
@pytest.mark.parametrize("m,n,k,shift", [(17, 3, 7, 5), (130, 3, 2, 50), (20, 16, 64, 3)])
def test_positional_independence(eng, m, n, k, shift):
    """the same start states at another position (rolled along m, across the workgroup boundary at (130, 3, 2); by 3 at (20, 16, 64),
    whose groups of 8 a start state then crosses) give the same bits"""
    x = _variant(m, n, k, 8)
    rolled = {key: np.ascontiguousarray(np.roll(v, shift, axis=1)) for key, v in x.items()}
    a, b = _run(eng, x, CONFIGS[1], FLOOR), _run(eng, rolled, CONFIGS[1], FLOOR)
    for key in a:
        axis = 0 if a[key].ndim == 1 else 1
        _same(b[key], np.roll(a[key], shift, axis=axis), "rolled by %d: %s" % (shift, key))


# ---------------------------------------------------------------------------------------------------------------------- 3: discipline
def _sizes(m, n, k, steve):
    s = [4 * k * m * n, 4 * k * m * n, k * m * n, k * m * n]
    return s + ([4 * m, 4 * k * m, 4 * k * m, 4 * k * m, 4 * k * m, m] if steve else [])


@pytest.mark.parametrize("steve", [False, True], ids=["plain", "steve"])
def test_inputs_and_workspace_discipline(eng, steve):
    """The inputs keep their bytes; of a buffer filled with a sentinel only the reported views change -- not the padding between them and
    nothing behind the reported size; the offsets are the 256-byte carve of the documented order."""
    m, n, k = 17, 3, 7
    x = _variant(m, n, k, 8)
    d = _dev(eng, x)
    lib, ctx = eng.lib, eng._ctx
    off = (ct.c_uint64 * _lib.TARGET_VIEWS)()
    need = lib.cadm_imagine_targets_workspace_bytes(ctx, m, n, k, int(steve), off)
    sizes = _sizes(m, n, k, steve)
    a256 = lambda v: (v + 255) // 256 * 256
    assert list(off)[:len(sizes)] == [int(v) for v in np.cumsum([0] + [a256(s) for s in sizes[:-1]])] and need == sum(a256(s) for s in sizes)
    assert all(o == 0 for o in list(off)[len(sizes):])
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=eng.device)
    prm = _lib.TargetParams(0.99, 0.5, 0.7, MAXD, FLOOR if steve else 0.0, int(steve))
    P = lambda t: ct.c_void_p(t.data_ptr())
    rc = lib.cadm_imagine_targets(ctx, P(d["rew"]), P(d["valid"]), P(d["done"]), P(d["disagreement"]), P(d["boot"]), m, n, k, ct.byref(prm),
                                  P(buf), None)
    assert rc == 0, lib.cadm_last_error()
    torch.cuda.synchronize()
    for key, v in x.items():
        _same(_np(d[key]), v, "input %s" % key)
    raw = _np(buf)
    inside = np.zeros(raw.shape, bool)
    want = _ref(x, CONFIGS[1], FLOOR if steve else None)
    for name, o, s in zip(KEYS + STEVE_KEYS, off, sizes):
        inside[int(o):int(o) + s] = True
        _same(raw[int(o):int(o) + s].view(want[name].dtype).reshape(want[name].shape), want[name], "view %s" % name)
    assert (raw[~inside] == 0xA5).all() and (~inside).sum() >= 512, "bytes outside the reported views were written"


def test_c_entry_refuses_bad_arguments(eng):
    """CADM_EINVAL and a message that names the call, before any HIP call: the buffer is never touched"""
    lib, ctx = eng.lib, eng._ctx
    src = torch.zeros(1 << 14, dtype=torch.float32, device=eng.device)
    buf = torch.zeros(1 << 14, dtype=torch.float32, device=eng.device)
    P, W = ct.c_void_p(src.data_ptr()), ct.c_void_p(buf.data_ptr())
    who = "cadm_imagine_targets"

    def run(c=ctx, arrays=(P,) * 5, m=2, n=2, k=2, ws=W, prm=True, **kw):
        q = dict(gamma=0.9, lam=0.5, penalty=0.0, max_disagreement=math.inf, var_floor=0.0, want_steve=0)
        q.update(kw)
        p = _lib.TargetParams(q["gamma"], q["lam"], q["penalty"], q["max_disagreement"], q["var_floor"], q["want_steve"])
        return lib.cadm_imagine_targets(c, *arrays, m, n, k, ct.byref(p) if prm else None, ws, None)

    def refused(rc, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1 and msg.startswith(who + ":") and frag in msg, (rc, msg)
    assert run() == 0
    assert run(var_floor=NAN) == 0, "var_floor is read only with want_steve"
    buf.fill_(7.0)
    torch.cuda.synchronize()
    for i in range(5):
        refused(run(arrays=tuple(None if j == i else P for j in range(5))), "null")
    refused(run(c=None), "null")
    refused(run(ws=None), "null")
    refused(run(prm=False), "null")
    for kw in (dict(m=0), dict(n=0), dict(k=0), dict(k=-2)):
        refused(run(**kw), "must be >= 1")
    refused(run(m=1 << 20, n=1 << 12), "too many")
    for g in (0.0, -0.5, 1.5, NAN):
        refused(run(gamma=g), "gamma")
    for v in (-0.1, 1.1, NAN):
        refused(run(lam=v), "lambda")
    for v in (-1.0, math.inf, NAN):
        refused(run(penalty=v), "penalty")
    for v in (0.0, -1.0, NAN):
        refused(run(max_disagreement=v), "max_disagreement")
    for v in (0.0, -1.0, math.inf, NAN):
        refused(run(want_steve=1, var_floor=v), "var_floor")
    refused(run(n=1, want_steve=1, var_floor=0.1), "branches >= 2")
    refused(run(m=1, n=700, k=20, want_steve=1, var_floor=0.1), "LDS")
    assert lib.cadm_imagine_targets_workspace_bytes(None, 2, 2, 2, 0, None) == 0
    assert lib.cadm_imagine_targets_workspace_bytes(ctx, 0, 2, 2, 0, None) == 0
    assert lib.cadm_imagine_targets_workspace_bytes(ctx, 2, 1, 2, 1, None) == 0
    torch.cuda.synchronize()
    assert (_np(buf) == 7.0).all() and (_np(src) == 0).all(), "a refused call wrote"
    # the engine's own checks of shapes and dtypes
    x = _dev(eng, _variant(3, 4, 5, 0))
    args = lambda **kw: [dict(x, **kw)[key] for key in ("rew", "valid", "done", "disagreement", "boot")]
    for bad, name in ((dict(valid=x["valid"].float()), "valid"), (dict(boot=x["boot"][:-1]), "boot"), (dict(done=x["done"][:, :2]), "done"),
                      (dict(disagreement=x["disagreement"].cpu()), "disagreement"), (dict(rew=x["rew"][0]), "rew"),
                      (dict(rew=x["rew"].transpose(1, 2)), "rew")):
        with pytest.raises(ValueError, match="imagine_targets: %s must be" % name):
            eng.imagine_targets(*args(**bad), 0.9)
    with pytest.raises(_lib.CadmError, match="gamma"):
        eng.imagine_targets(*args(), 1.5)


# ---------------------------------------------------------------------------------------------------------------------- 4: the class route
M, N, K, D, A = 3, 3, 4, 18, 6


def _actions(seed=3):
    return np.random.default_rng(seed).uniform(-1, 1, (M, N, K, A)).astype(F)


def _check_route(model, batch, boot, engine_boot, **kw):
    """model.imagine_targets(batch, bootstrap=boot) equals the engine call given `engine_boot`, bit for bit"""
    eng = model.engine
    out = model.imagine_targets(batch, 0.99, 0.9, bootstrap=boot, **kw)
    steve = kw.get("steve")
    direct = eng.imagine_targets(batch["rew"], batch["valid"], batch["done"], batch["disagreement"], engine_boot.contiguous(), 0.99, 0.9,
                                 kw.get("penalty", 0.0), kw.get("max_disagreement"), None if steve is None else steve["var_floor"])
    assert set(out) == set(direct) | {"boot"}
    for key in direct:
        assert isinstance(out[key], torch.Tensor) and out[key].is_cuda
        _same(_np(out[key]), _np(direct[key]), key)
    _same(_np(out["boot"]), _np(engine_boot), "boot")
    x = {key: _np(batch[key]) for key in ("rew", "valid", "done", "disagreement")}
    want = tref.targets(**x, boot=_np(engine_boot), gamma=0.99, lam=0.9, penalty=kw.get("penalty", 0.0),
                        max_disagreement=kw.get("max_disagreement"), var_floor=None if steve is None else steve["var_floor"])
    for key in direct:
        _same(_np(out[key]), want[key], "against the restatement: %s" % key)
    return {key: _np(v) for key, v in out.items()}


def test_class_route_value(gpu):
    """`imagine` then `imagine_targets` with bootstrap "value" (and "auto", which is value here) is the engine call given
    `value_eval(states)`; a caller tensor and a numpy array are taken as they are; numpy=True returns numpy copies; under terminate
    constraints whose bound some rows cross, those rows do not bootstrap."""
    tv = dict(hidden_sizes=(32,), activation="relu")
    model, prob = plan_model(False, K, m=M, cem_terminal_value=tv, **BIG)
    batch = model.imagine(prob["obs"], horizon=K, branches=N, actions=_actions())
    with pytest.raises(RuntimeError, match="no value net"):
        model.imagine_targets(batch, 0.99)
    with pytest.raises(ValueError, match="needs a model with cem_terminal_q"):
        model.imagine_targets(batch, 0.99, bootstrap="q")
    model.set_terminal_value(vref.he_net(D, (32,), 3))
    v = model.engine.value_eval(batch["states"])
    assert tuple(v.shape) == (K + 1, M, N)
    for boot in ("value", "auto"):
        out = _check_route(model, batch, boot, v, steve=dict(var_floor=FLOOR), penalty=0.5)
    assert (out["used"] == 1).all() and np.isfinite(out["steve"]).all() and (out["steve_count"] == N).all()
    own = torch.as_tensor(np.random.default_rng(1).standard_normal((K + 1, M, N)).astype(F)).cuda()
    _check_route(model, batch, own, own)
    _check_route(model, batch, _np(own), own, max_disagreement=float(np.median(_np(batch["disagreement"]))))
    # numpy in, numpy out
    nb = model.imagine(prob["obs"], horizon=K, branches=N, actions=_actions(), seed=model.seed, numpy=True)
    res = model.imagine_targets(nb, 0.99, 0.9, steve=dict(var_floor=FLOOR), numpy=True)
    assert all(isinstance(x, np.ndarray) for x in res.values()) and res["nstep_ok"].dtype == np.uint8 and res["steve_count"].dtype == np.int32
    want = tref.targets(nb["rew"], nb["valid"], nb["done"], nb["disagreement"], res["boot"], 0.99, 0.9, var_floor=FLOOR)
    for key in KEYS + STEVE_KEYS:
        _same(res[key], want[key], "numpy route: %s" % key)
    _same(res["boot"], model.terminal_value(nb["states"]).astype(F), "boot is terminal_value(states)")
    # terminate constraints: a bound half of the rows cross
    hi = float(np.median(_np(batch["states"])[1:, :, :, 0].max(axis=0)))      # (cons' first call repeats batch's rollouts)
    cons, _ = plan_model(False, K, m=M, cem_terminal_value=tv, cem_constraints=[dict(dim=0, hi=hi)], cem_constraint_mode="terminate",
                         cem_constraint_weight=1.0, **BIG)
    cons.set_terminal_value(vref.he_net(D, (32,), 3))
    cb = cons.imagine(prob["obs"], horizon=K, branches=N, actions=_actions())
    cv = cons.engine.value_eval(cb["states"])
    out = _check_route(cons, cb, "value", cv)
    done, valid, rew = _np(cb["done"]) > 0, _np(cb["valid"]) > 0, _np(cb["rew"])
    ended = done.any(axis=0)
    assert ended.any() and not ended.all()
    L = valid.sum(axis=0)
    _same(out["used"], valid.astype(np.uint8), "used is valid without a bound")
    ii, jj = np.nonzero(ended)
    _same(out["lambda_return"][L[ended] - 1, ii, jj], rew[L[ended] - 1, ii, jj], "a terminated row's last lambda-return is its reward alone")
    assert (out["nstep_ok"][:, ended] == 1).all(), "a terminated row has a target at every horizon"
    _same(out["nstep"][K - 1][ended], out["nstep"][L[ended] - 1, ii, jj], "... its terminal return")


def test_class_route_q_and_given(gpu):
    """bootstrap "q" (and "auto" on a model that declares only cem_terminal_q) is the engine call given `critic_eval(states)`; a model on
    the reference planner takes a caller's values and refuses "auto" naming the three choices."""
    tq = dict(hidden_sizes=(32,), activation="tanh", n_critics=2, reduce="min", policy=dict(hidden_sizes=(16,), activation="tanh"))
    model, prob = plan_model(False, K, m=M, cem_terminal_q=tq, **BIG)
    model.set_policy(pref.he_policy(D, (16,), A, 2, out_scale=0.5))
    batch = model.imagine(prob["obs"], horizon=K, branches=N, noise_std=0.1)
    with pytest.raises(RuntimeError, match="no critics"):
        model.imagine_targets(batch, 0.99)
    with pytest.raises(ValueError, match="needs a model with cem_terminal_value"):
        model.imagine_targets(batch, 0.99, bootstrap="value")
    model.set_critics(cref.he_critics(D, A, (32,), 2, 5))
    q = model.engine.critic_eval(batch["states"])
    assert tuple(q.shape) == (K + 1, M, N)
    for boot in ("q", "auto"):
        _check_route(model, batch, boot, q, steve=dict(var_floor=FLOOR))
    _same(_np(q), model.q_value(_np(batch["states"])).astype(F), "boot is q_value(states)")
    plain, _ = plan_model(False, K, m=M, **BIG)
    assert plain._opt is None
    pb = plain.imagine(prob["obs"], horizon=K, branches=N, actions=_actions())
    own = torch.zeros((K + 1, M, N), device="cuda")
    _check_route(plain, pb, own, own)
    with pytest.raises(ValueError, match=r"(?s)'value'.*'q'.*tensor or array"):
        plain.imagine_targets(pb, 0.99)
    with pytest.raises(ValueError, match="bootstrap"):
        plain.imagine_targets(pb, 0.99, bootstrap=own[:-1])
    one = plain.imagine(prob["obs"], horizon=K, branches=1, actions=_actions()[:, :1])
    with pytest.raises(ValueError, match="branches >= 2"):
        plain.imagine_targets(one, 0.99, bootstrap=own[:, :, :1], steve=dict(var_floor=FLOOR))


def test_no_side_effects(gpu):
    """A `get_action` before and after an `imagine_targets` returns the bits of two `get_action` calls without it; no counter moves."""
    tv = dict(hidden_sizes=(32,), activation="relu")
    a, prob = plan_model(False, K, m=M, cem_terminal_value=tv, **BIG)
    b, _ = plan_model(False, K, m=M, cem_terminal_value=tv, **BIG)
    for model in (a, b):
        model.set_terminal_value(vref.he_net(D, (32,), 3))
    mean, var = prob["init_mean"], prob["init_var"]
    p1, p2 = plan_act(a, prob, False, mean, var), plan_act(a, prob, False, mean, var)
    batch = b.imagine(prob["obs"], horizon=K, branches=N, actions=_actions())
    q1 = plan_act(b, prob, False, mean, var)
    counters = (b._call, b._imagine_call, b._eval_call)
    b.imagine_targets(batch, 0.99, steve=dict(var_floor=FLOOR))
    b.imagine_targets(batch, 0.99, bootstrap=torch.zeros((K + 1, M, N), device="cuda"), numpy=True)
    assert (b._call, b._imagine_call, b._eval_call) == counters
    q2 = plan_act(b, prob, False, mean, var)
    _same(q1, p1, "the first plan")
    _same(q2, p2, "the plan behind imagine_targets")
    assert not np.array_equal(p1, p2) and a._call == b._call == 2
