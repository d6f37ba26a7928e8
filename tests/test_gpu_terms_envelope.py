"""GPU: the planner terms behind the rollout -- the uncertainty cost (csrc/uncertainty.hip), the tracking targets (csrc/tracking.hip), the
actuator model (csrc/actuator.hip), the knots (csrc/knots.hip), the terminal value and the learned reward (csrc/mlp_chain.h, value.hip,
reward.hip) and the loop that carves a workspace for all of them (csrc/icem.hip) -- OFF the geometries their own files run on
(hopper_like and halfcheetah, D <= 18, A in {3, 6}, H <= 8, hidden widths that are multiples of 4).

Engines (tests/behind_rollout.py TERM_ENGINES, built when first asked for):
    pend    pendulum       D = 3   A = 1   E = 5  p = 5   H = 5       every kernel, and the loop
    ant     ant            D = 28  A = 8   E = 5  p = 10  H = 5       actuator, value and reward (K = 28, 36, 64)
    slim    slim_humanoid  D = 45  A = 17  E = 5  p = 15  H = 3       every kernel, and the loop
    slim35  slim_humanoid  D = 45  A = 17  E = 5  p = 35  H = 3       uncertainty with groups of 7
    wide    corner_spec("widest")  D = 48  A = 24  p = 10  H = 3      kernel level only, never rolled out: nothing is built on demand
    long    halfcheetah, vanilla   D = 18  A = 6   p = 5   H = 40     long chains
    one     halfcheetah, vanilla   H = 1                              reward and value at a one-step horizon
    p1      halfcheetah, E = 1, p = 1, deterministic, H = 5           tracking with 64 envs in one workgroup
The loop runs only on geometries the library carries (`cadm_rollout_builtin`: the built-in kinds at hidden 200 x 4, swish).

The checks are the ones the feature files define (imported, not restated), each at its own bar: the derived bounds of
tests/uncertainty_ref.py, tests/tracking_ref.py and tests/actuator_ref.py, bit equality and 2^-22 for the knots, `helpers.assert_close`
at 1e-5 of scale for the nets against tests/value_ref.py and tests/reward_ref.py.  Inputs: `behind_rollout.synth_traj`.  The nets are
`value_ref.ENVELOPE_NETS`; tests/test_value_ref.py and tests/test_reward_ref.py hold their float32 chains to the same bar on the CPU
and assert that they are live on these inputs (a dead net would pass anything).

Code no other test reaches -> the test here that does:
    uncertainty.hip  the second pass of the (candidate, dim) loop, G D = 360 > 256           test_uncertainty_kernel[slim-3-11], [wide-3-11]
                     a group of G = 7 (the LDS budget shrinks it): 7 + 7 + 1 candidates       test_uncertainty_kernel[slim35-3-5]
                     a span shorter than the workgroup (D = 3)                                test_uncertainty_kernel[pend-1-3]
                     the walking kernel over 40 steps under a `first` cut                     test_uncertainty_long_horizon_cut
    tracking.hip     a workgroup of 64 rows of 64 envs (ne = 64, n p = 1), and of 22 envs     test_tracking_kernel[p1-70-*], [p1-90-*]
                     tiles of 64 x 45 and 64 x 48 floats, and D = 3                           test_tracking_kernel[slim-150-*], [wide-100-*], [pend-135-*]
                     the early exit many steps before H                                       test_tracking_early_exit
    actuator.hip     A = 1 (256 candidates a workgroup, an empty dim sum), A = 8, 17, 24      test_actuator_kernel[pend-*], [ant-*], [slim-*], [wide-*]
                     H = 40 chains, a delay of 39                                             test_actuator_kernel[long-2-24]
    mlp_chain.h      widths off the multiples of 4 (units N .. N4 - 1 written as zeros), widths 1, 2, 3, a last 64-unit group of 1 or
                     2 units (65, 130), four hidden layers (the fourth swap of the LDS regions), a first layer of ONE k-step (K = 3, 4)
                     and of 16, 18, 27 and 30 k-steps (K = 62, 72, 107, 120)                  test_value_nets, test_reward_nets, test_nets_with_statistics
                     both row-tile variants at those widths                                   test_net_bits_in_a_large_batch
    reward.hip       reward_sum_kernel's second batch of 32 loads, a cut on either side of it test_reward_long_horizon
                     H = 1: every step reads `obs`, traj[t - 1] is never addressed            test_one_step_horizon
    knots.hip        A = 1, 17, 24; H = 40; spacings near and beyond a long H                 test_knots
    icem.hip         every optional region carved in one workspace; the terms on pendulum
                     and slim_humanoid                                                        test_everything_on, test_each_term_matters

Measured on an MI355X, worst |err| / bar (every kernel test prints its own; run with -s) -- every case passes, no kernel was changed:
    uncertainty      slim (3, 11) 0.011, (1, 3) 0.009; slim35 (3, 5) 0.006; wide 0.016; pend (3, 11) 0.025, (1, 3) 0.019; long with the cut 0.016
    tracking rows    K = 1: slim-150 0.666, wide-100 0.755, pend-135 0.762, p1-70 0.641, p1-90 0.727; K = 16: 0.035 .. 0.046; early exit 0.079
    tracking cost    K = 1: 0.155 .. 0.241; K = 16: 0.035 .. 0.046
    actuator cost    A = 1: 0.099 (3, 100), 0.140 (4, 1); A = 8: 0.089; A = 17: 0.076; A = 24: 0.055; H = 40: 0.034
    knots            interpolated steps at most 0.5 of 2^-22 (H = 40, r = 7, 39, 40), 0.25 at r = 2 and r = H = 3
    value nets       pend (K = 3) relu 0.214, tanh 0.073, swish 0.235; slim (45) 0.125, 0.126, 0.142; wide (48) 0.185, 0.094, 0.249;
                     ant (28) 0.073, 0.102, 0.104; H = 40: 0.078; H = 1: 0.046
    reward nets      pend K = 3: 0.565 (swish), K = 4: 0.166, K = 7: 0.105; slim K = 45: 0.182, 62: 0.240, 107: 0.218; wide K = 48: 0.250,
                     72: 0.162, 120: 0.174; ant K = 28: 0.164, 36: 0.090, 64: 0.086; H = 40 (K = 42): 0.107; H = 1: 0.081
    with statistics  reward 0.056 (pend), 0.133 (slim), 0.140 (wide), 0.084 (ant); value 0.117, 0.085, 0.065, 0.075
The float32 emulations of the restatements predict the same on the CPU: tracking 0.64 .. 0.76 at K = 1, uncertainty 0.006 .. 0.025."""
import ctypes as ct

import numpy as np
import pytest
import torch

import actuator_ref as aref
import behind_rollout as br
import reward_ref as rref
import tracking_ref as tref
import uncertainty_ref as uref
import value_ref as vref
from cadm_amd import planner as hplanner
from cadm_amd import synth
from cadm_amd.engine import HipEngine
from helpers import _np, corner_spec, floored_rel, make_engine, zero_carry
from test_gpu_actuator import _check_iterations as actuator_iterations
from test_gpu_actuator import _params as act_params
from test_gpu_actuator import _state as _act_state
from test_gpu_actuator import check_kernel as actuator_check
from test_gpu_constraints import binding_bounds, iteration0_traj
from test_gpu_knots import check_shape_actions
from test_gpu_reward import _check_iterations as reward_iterations
from test_gpu_reward import _set as set_reward
from test_gpu_reward import check_kernel_case as reward_check
from test_gpu_tracking import _tracking_inputs
from test_gpu_tracking import check_kernel_case as tracking_check
from test_gpu_uncertainty import _check as uncertainty_check
from test_gpu_uncertainty import _check_iterations as uncertainty_iterations
from test_gpu_uncertainty import _prm as unc_prm
from test_gpu_value import _check_iterations as value_iterations
from test_gpu_value import _set as set_value
from test_gpu_value import check_kernel_case as value_check

pytestmark = pytest.mark.gpu

F = np.float32
M, N, KE, ITERS = 2, 24, 8, 3
CONSTRAINED = {"slim": (1, 44), "pend": (2, 0)}      # the dims tests/test_gpu_constraints.py constrains on these kinds


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine) of `behind_rollout.TERM_ENGINES`, built when first asked for; 8 elites, 3 CEM iterations"""
    built = {}

    def get(name):
        if name not in built:
            kind, D, A, E, p, H = br.TERM_ENGINES[name]
            if name == "wide":
                prob = synth.make_problem(env=corner_spec(kind), context=True, E=E, m=M, H=H, seed=8)
            elif kind == "halfcheetah":
                prob = synth.make_problem(env=kind, context=False, E=E, m=M, H=H, seed=3, trained_like=True)
            else:
                prob = synth.make_problem(env=kind, context=True, E=E, m=M, H=H, seed=3, trained_like=True)
            eng = make_engine(prob, p=p, deterministic=name == "p1", num_elites=KE, num_cem_iters=ITERS)
            assert (eng.D, eng.A, eng.E, eng.p, eng.H) == (D, A, E, p, H)
            built[name] = (prob, eng)
        return built[name]
    yield get
    _, wide = built.get("wide", (None, None))
    assert wide is None or not wide._rollout_ready, "the envelope's corner was rolled out: a kernel-level test built a module on demand"
    for _, eng in built.values():
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------- 1: uncertainty
def _unc_lds_bytes(G, p, D):
    """csrc/uncertainty.hip unc_lds_bytes: the tile of G p D floats, G D variances and D weights, each padded to 4 floats"""
    pad4 = lambda v: (v + 3) & ~3
    return 4 * (pad4(G * p * D) + pad4(G * D) + pad4(D))


def _unc_group(p, D):
    return max(G for G in range(0, 9) if G == 0 or _unc_lds_bytes(G, p, D) <= 48 * 1024)


UNC = [("slim", 3, 11), ("slim", 1, 3), ("slim35", 3, 5), ("wide", 3, 11), ("pend", 3, 11), ("pend", 1, 3)]


@pytest.mark.parametrize("name,m,n", UNC, ids=["%s-%d-%d" % c for c in UNC])
def test_uncertainty_kernel(engines, name, m, n):
    """`cadm_uncertainty_cost`, both kernel forms (with and without step_out), both kinds x both forms x (broadcast, per-dim with zeros,
    one-hot on dim 0, one-hot on dim D - 1) weights, within the undoubled bound of tests/uncertainty_ref.py.  slim and wide at (3, 11):
    33 candidates are four groups of 8 and one of 1, a group has 8 x 45 = 360 (8 x 48 = 384) (candidate, dim) pairs for 256 threads.
    slim35 at (3, 5): the tile of 8 candidates does not fit, 15 candidates go in groups of 7, 7 and 1.  pend: a group's span at (1, 3)
    is 3 x 5 x 3 = 45 floats."""
    _, eng = engines(name)
    D, p = eng.D, eng.p
    G = _unc_group(p, D)
    assert G == (7 if name == "slim35" else 8)
    if name == "slim35":
        assert _unc_lds_bytes(7, p, D) <= 48 * 1024 < _unc_lds_bytes(8, p, D) and (m * n) % G == 1
    if name in ("slim", "wide") and n == 11:
        assert G * D > 256 and (m * n) % G == 1
    traj, _, _ = br.term_traj(name, m, n, 7 + n)
    worst = 0.0
    for kind in uref.KINDS:
        for form in uref.FORMS:
            for style in ("broadcast", "per-dim", "one-hot-0", "one-hot-%d" % (D - 1)):
                w = uref.make_w(style, D, seed=n)
                assert style[0] != "o" or (w[0 if style == "one-hot-0" else D - 1] == 1 and w.sum() == 1)
                r, step, cost = uncertainty_check(eng, traj, kind, w, form, None, None, "%s m=%d n=%d %s %s %s" % (name, m, n, kind, form, style))
                assert (cost > 0).all()
                worst = max(worst, r)
    print("\n[uncertainty %s m=%d n=%d, G = %d] worst |err| / bound %.3f" % (name, m, n, G, worst))
    assert worst > 0


def test_uncertainty_long_horizon_cut(engines):
    """H = 40 at (2, 9): `first` drawn over 0 .. 40 with 0 and 40 planted -- the stepwise form (a grid of 40 steps) and the walking form
    (one workgroup walks 40 steps) against the restatement with the same cut, and without a cut."""
    _, eng = engines("long")
    H, m, n = eng.H, 2, 9
    traj, _, _ = br.term_traj("long", m, n, 16)
    first = np.random.default_rng(17).integers(0, H + 1, (m, n, eng.p)).astype(np.int32)
    first[0, 0], first[1, 8], first[1, 3] = 0, H, H
    first[1, 3, 2] = 32
    cut = first.min(axis=2)
    assert cut[0, 0] == 0 and cut[1, 8] == H and cut[1, 3] == 32 and len(set(cut.ravel().tolist())) > 6
    worst = 0.0
    w = uref.make_w("per-dim", eng.D, seed=4)
    for kind in uref.KINDS:
        for form in uref.FORMS:
            for f in (first, None):
                r, step, cost = uncertainty_check(eng, traj, kind, w, form, None, f, "long %s %s cut=%s" % (kind, form, f is not None))
                assert (cost > 0).all()
                worst = max(worst, r)
    print("\n[uncertainty long (2, 9), H = 40] worst |err| / bound %.3f" % worst)


# ---------------------------------------------------------------------------------------------------------------------- 2: tracking
TRACK = [(s, K) for s in ("slim-150", "wide-100", "pend-135", "p1-70", "p1-90") for K in (1, 16)]
TRACK_ENGINE = {"slim-150": "slim", "wide-100": "wide", "pend-135": "pend", "p1-70": "p1", "p1-90": "p1", "long-130": "long"}
TRACK_DIMS = {"slim-150": (0, 44), "wide-100": (0, 47)}      # the first and the last dim of the widest tiles


@pytest.mark.parametrize("shape,K", TRACK, ids=["%s-K%d" % c for c in TRACK])
def test_tracking_kernel(engines, shape, K):
    """`cadm_tracking_returns` within the derived bound of tests/tracking_ref.py for T in {1, H, H + 3}, K = 1 (each kind alone) and
    K = 16, with `make_case`'s offsets and NaN targets.  slim-150 and wide-100: 64 + 64 + 22 (64 + 36) rows in tiles of 64 x 45 (48)
    floats, terms on dim 0 and on the last dim.  p1-70: one row per env, so workgroup 0 stages the offsets and the target rows of 64
    envs and workgroup 1 those of 6; p1-90: three rows per env, the first workgroup ends inside env 21.  There every env has its own
    offset (negative ones and ones beyond T among them) and its own target rows: no two envs of a workgroup share both, and a row held
    against its neighbour env's targets, or at its neighbour's offset, is off by more than the bound."""
    _, eng = engines(TRACK_ENGINE[shape])
    H, m, n, p, D = tref.SHAPES[shape][:5]
    assert (eng.H, eng.p, eng.D) == (H, p, D)
    worst = worst_cost = 0.0
    for T in (1, H, H + 3):
        for ki, kinds in enumerate([(k,) for k in tref.KINDS] if K == 1 else [tref.KINDS]):
            dims = TRACK_DIMS.get(shape)
            if dims is not None and K == 1:
                dims = dims[(ki + T) % 2:][:1]
            case = tref.make_case(shape, K, T, kinds=kinds, seed=len(kinds[0]), dims=dims)
            traj, rows, terms, targets, offset = case
            if dims is not None:
                assert [c["dim"] for c in terms[:len(dims)]] == list(dims)
            what = "%s K=%d T=%d %s" % (shape, K, T, "/".join(kinds))
            r, rc, _, out = tracking_check(eng, H, K, case, what)
            worst, worst_cost = max(worst, r), max(worst_cost, rc)
            if shape.startswith("p1"):
                for q0 in range(0, m * n * p, 64):      # the envs of one workgroup
                    envs = range(q0 // (n * p), (min(q0 + 64, m * n * p) - 1) // (n * p) + 1)
                    assert len({(int(offset[e]), targets[e].tobytes()) for e in envs}) == len(envs), what
                ref, _, S, counted = tref.tracking(traj, rows, terms, targets, offset)
                lim, some = tref.bound(S, ref, H, K), counted > 0
                other = tref.tracking(traj, rows, terms, np.roll(targets, 1, axis=0), offset)[0]
                assert (np.abs(other - ref) > lim)[some].all(), what + ": the neighbour env's targets would pass"
                assert (np.abs(out - other) > lim)[some].all()
                if T > 1 and K == 16:
                    moved = np.array([not np.array_equal(tref.target_rows(T, H, offset[e]), tref.target_rows(T, H, offset[e - 1])) for e in range(m)])
                    other = tref.tracking(traj, rows, terms, targets, np.roll(offset, 1))[0]
                    assert moved.sum() > m // 2 and (np.abs(other - ref) > lim)[moved].all(), what + ": the neighbour env's offset would pass"
    if shape == "p1-70":
        assert n * p == 1 and m == 64 + 6
    print("\n[tracking %s K=%d] worst |err| / bound: rows %.3f, cost %.3f" % (shape, K, worst, worst_cost))


def test_tracking_early_exit(engines):
    """H = 40, 130 rows in workgroups of 64, 64 and 2.  (a) every row of the first workgroup is cut at step 0 -- it leaves the step loop
    39 steps early --, no row of the second is cut, the third is mixed; (b) the first workgroup's cuts are drawn over 0 .. 5.  NaN planted
    in every tracked dim behind each cut reaches no row, and the rows are the restatement's with the same cut within the bound."""
    shape = "long-130"
    _, eng = engines("long")
    H, m, n, p, D = tref.SHAPES[shape][:5]
    assert (eng.H, eng.p, eng.D) == (H, p, D) and m * n * p == 130
    K = 3
    traj, rows, terms, _, _ = tref.make_case(shape, K, 1)
    tracked = sorted({c["dim"] for c in terms})
    targets = np.full((m, 1, K), 0.5, np.float32)
    worst = 0.0
    for variant in ("a", "b"):
        first = np.full((m * n * p,), H, np.int32)
        first[:64] = 0 if variant == "a" else np.random.default_rng(5).integers(0, 6, 64)
        first[128:] = (3, H)
        first = first.reshape(m, n, p)
        ref, _, S, counted = tref.tracking(traj, rows, terms, targets, None, first)
        assert (counted == K * np.minimum(first + 1, H)).all()
        bad = traj.copy()
        behind = np.arange(H)[:, None, None, None] > first[None]
        for d in tracked:
            bad[..., d][behind] = np.nan
        by_row = bad.reshape(H, m * n * p, D)
        assert np.isnan(by_row[6:, :64][:, :, tracked]).all() and np.isfinite(by_row[:, 64:128]).all() and np.isnan(by_row[4:, 128, tracked]).all()
        out = _np(eng.tracking_returns(bad, rows, terms, targets, first=first))
        assert np.isfinite(out).all(), "a NaN behind the cut reached a row"
        lim, err = tref.bound(S, ref, H, K), np.abs(out - ref)
        assert (err <= lim).all(), "variant %s: worst |err| / bound %.3f" % (variant, (err / lim).max())
        worst = max(worst, float((err / lim).max()))
        np.testing.assert_array_equal(_bits(_np(eng.tracking_returns(traj, rows, terms, targets, first=first))), _bits(out))
    print("\n[tracking long-130, early exit] worst |err| / bound %.3f" % worst)


# ---------------------------------------------------------------------------------------------------------------------- 3: actuator
def _weighted_case(*args, **kw):
    """`actuator_ref.make_case` with a rate cost on every dim (its own weights are zero on every third dim: all of A = 1)"""
    seqs, dl, w, prev, prefix = aref.make_case(*args, **kw)
    return seqs, dl, np.linspace(1.7, 0.4, w.size).astype(F), prev, prefix


ACT = [("pend", 3, 100), ("pend", 4, 1), ("ant", 3, 24), ("slim", 4, 7), ("wide", 4, 7), ("long", 2, 24)]


@pytest.mark.parametrize("name,m,n", ACT, ids=["%s-%d-%d" % c for c in ACT])
def test_actuator_kernel(engines, name, m, n):
    """`cadm_actuate_actions` for d in {0, 1, H - 1}: the sequences bit for bit, the cost within `actuator_ref.bound` -- the body of
    tests/test_gpu_actuator.py's kernel test.  A = 1: 300 chains in workgroups of 256 and 44 candidates, the dim sum adds nothing;
    A = 8: 72 candidates in workgroups of 32, 32 and 8, no idle thread; A = 17: 28 candidates in workgroups of 15 and 13, one idle
    thread, the dim sum reads up to index 254; A = 24: workgroups of 10, 10 and 8 candidates, 16 idle threads; H = 40: a delay of 39."""
    _, eng = engines(name)
    cpb = 256 // eng.A
    assert {"pend": (256, 0), "ant": (32, 0), "slim": (15, 1), "wide": (10, 16), "long": (42, 4)}[name] == (cpb, 256 - cpb * eng.A)
    worst = actuator_check(eng, name, m, n, _weighted_case if eng.A == 1 else aref.make_case)
    print("\n[actuator %s A=%d H=%d m=%d n=%d] cost: worst |err| / bound %.3f" % (name, eng.A, eng.H, m, n, worst))


# ---------------------------------------------------------------------------------------------------------------------- 4: knots
KNOTS = [(e, r) for e in ("pend", "slim", "wide") for r in ("2", "H", "H+3")] + [("long", r) for r in ("2", "7", "39", "40", "64")]


@pytest.mark.parametrize("interp", ["hold", "linear"])
@pytest.mark.parametrize("name,r", KNOTS, ids=["%s-r%s" % c for c in KNOTS])
def test_knots(engines, name, r, interp):
    """`cadm_shape_actions` at A = 1, 17 and 24 and at H = 40 with spacings 2, H and H + 3 (one knot: everything is held), and at H = 40
    near and beyond the horizon (39, 40, 64) -- the body of tests/test_gpu_knots.py's primitive test: phases (0, 1, r - 1), phases
    outside [0, r) and none, n in {1, 37}; HOLD bit-equal, LINEAR bit-equal at knots and in held tails and within 2^-22 elsewhere."""
    _, eng = engines(name)
    r = {"H": eng.H, "H+3": eng.H + 3}.get(r) or int(r)
    worst = check_shape_actions(eng, r, interp, ns=(1, 37))
    print("\n[knots %s A=%d H=%d r=%d %s] interpolated steps vs float64: %.3f of 2^-22" % (name, eng.A, eng.H, r, interp, worst / 2.0 ** -22))


# ---------------------------------------------------------------------------------------------------------------------- 5: value and reward nets
def _live(x, layers, act, what, mean=None, std=None):
    share, spread = vref.liveness(x, layers, act, mean, std)
    assert share >= 0.5 and spread > 1e-3, "%s: live share %.2f, output spread %.2e: the net checks nothing" % (what, share, spread)


def _nets_of(name):
    return [(130, 66)] if name == "ant" else vref.ENVELOPE_NETS


NET_ENGINES = [(e, a) for e in ("pend", "slim", "wide", "ant") for a in vref.ACTS]


@pytest.mark.parametrize("name,act", NET_ENGINES, ids=["%s-%s" % c for c in NET_ENGINES])
def test_value_nets(engines, name, act):
    """`cadm_value_eval` / `cadm_value_returns` with `value_ref.ENVELOPE_NETS` at input widths 3, 45, 48 (and 28 with (130, 66)) against
    the float64 restatement at 1e-5 of scale, at (3, 11) and (3, 1); v_out has `cadm_value_eval`'s bits, the rows are the row update
    from them."""
    _, eng = engines(name)
    worst = 0.0
    for hidden in _nets_of(name):
        layers = vref.envelope_net(eng.D, hidden)
        prm = HipEngine.value_params(hidden, act, 0.5)
        eng.set_value_net(prm, layers)
        for m, n in ((3, 11), (3, 1)):
            traj = br.term_traj(name, m, n, 80 + n)[0]
            what = "value %s %r %s m=%d n=%d" % (name, hidden, act, m, n)
            if n == 11:
                _live(traj[-1], layers, act, what)
            rows = np.random.default_rng(n).standard_normal((m, n, eng.p)).astype(F)
            worst = max(worst, value_check(eng, prm, layers, act, traj, rows, 0.5, what)[0])
    print("\n[value %s %s, K = %d] worst |err| / (1e-5 of scale): %.3f" % (name, act, eng.D, worst))


@pytest.mark.parametrize("name,act", NET_ENGINES, ids=["%s-%s" % c for c in NET_ENGINES])
def test_reward_nets(engines, name, act):
    """`cadm_reward_returns` / `cadm_reward_eval` with `value_ref.ENVELOPE_NETS` and every `inputs` kind -- K = 3, 4, 7 on pend (a first
    layer of one k-step), 45, 62, 107 on slim at (3, 11) and (3, 1), 48, 72, 120 on wide, 28, 36, 64 on ant with (130, 66) -- against
    the float64 restatement at 1e-5 of scale; `cadm_reward_eval` gives step_out's bits, the sum and the rows are the restatement's from
    them."""
    _, eng = engines(name)
    worst = {}
    for inputs in rref.INPUTS:
        K = rref.input_dims(inputs, eng.D, eng.A)
        for hidden in _nets_of(name):
            layers = vref.envelope_net(K, hidden)
            prm = HipEngine.reward_params(inputs, hidden, act, 0.5)
            eng.set_reward_net(prm, layers)
            for m, n in ((3, 11), (3, 1)) if name in ("slim", "pend") else ((3, 11),):
                traj, obs, actions = br.term_traj(name, m, n, 80 + n)
                what = "reward %s %s %r %s m=%d n=%d" % (name, inputs, hidden, act, m, n)
                if n == 11:
                    _live(rref.gather_inputs(traj, obs, actions, inputs), layers, act, what)
                rows = np.random.default_rng(n).standard_normal((m, n, eng.p)).astype(F)
                r = reward_check(eng, prm, layers, act, inputs, traj, obs, actions, rows, 0.5, what)[0]
                worst[K] = max(worst.get(K, 0.0), r)
    print("\n[reward %s %s] worst |err| / (1e-5 of scale) by K: %s" % (name, act, ", ".join("%d: %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("name", ["pend", "slim", "wide", "ant"])
def test_nets_with_statistics(engines, name):
    """One net per engine -- (130, 66) on the widest input, tanh -- with in_mean / in_std that are not 0 / 1 over the whole concatenated
    input, for the reward and for the value: the restatement with the statistics at 1e-5 of scale, and the one without them off by
    more than 1e-3 (the statistics matter)."""
    _, eng = engines(name)
    hidden, act, inputs, m, n = (130, 66), "tanh", "obs_act_next_obs", 3, 11
    traj, obs, actions = br.term_traj(name, m, n, 80 + n)
    rows = np.zeros((m, n, eng.p), F)
    rng = np.random.default_rng(8)
    K = rref.input_dims(inputs, eng.D, eng.A)
    mean, std = rng.standard_normal(K).astype(F), rng.uniform(0.3, 4.0, K).astype(F)
    layers = vref.envelope_net(K, hidden)
    prm = HipEngine.reward_params(inputs, hidden, act, 1.0)
    eng.set_reward_net(prm, layers, in_mean=mean, in_std=std)
    x = rref.gather_inputs(traj, obs, actions, inputs)
    _live(x, layers, act, "reward %s with statistics" % name, mean, std)
    r, steps, _ = reward_check(eng, prm, layers, act, inputs, traj, obs, actions, rows, 1.0, "reward %s with statistics" % name, mean, std)
    assert floored_rel(steps, rref.reward64(x, layers, act)) > 1e-3, "the statistics must matter"
    layers = vref.envelope_net(eng.D, hidden)
    prm = HipEngine.value_params(hidden, act, 1.0)
    eng.set_value_net(prm, layers, obs_mean=mean[:eng.D], obs_std=std[:eng.D])
    _live(traj[-1], layers, act, "value %s with statistics" % name, mean[:eng.D], std[:eng.D])
    rv, v, _ = value_check(eng, prm, layers, act, traj, rows, 1.0, "value %s with statistics" % name, mean[:eng.D], std[:eng.D])
    assert floored_rel(v, vref.value(traj[-1].reshape(-1, eng.D), layers, act)) > 1e-3, "the statistics must matter"
    print("\n[statistics %s] worst |err| / (1e-5 of scale): reward (K = %d) %.3f, value %.3f" % (name, K, r, rv))


BATCH = [((5, 7), "relu"), ((130, 66), "tanh"), ((37, 37, 37, 37), "swish")]


@pytest.mark.parametrize("hidden,act", BATCH, ids=["x".join(map(str, h)) for h, _ in BATCH])
def test_net_bits_in_a_large_batch(engines, hidden, act):
    """slim, K = 107 and 45: the small batch's step rewards (values) recur with the same bits inside a batch of more than 2 sixteen-row
    tiles per CU (the CU count is the device's) and 16 rows, where the launcher may take its other row-tile variant and the small
    batch's candidates sit at other row positions -- tests/test_gpu_reward.py's and tests/test_gpu_value.py's large-batch comparison at
    widths off the multiples of 4."""
    _, eng = engines("slim")
    H, p, D = eng.H, eng.p, eng.D
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    need = 2 * 16 * cus + 16
    m, n, inputs = 2, 11, "obs_act_next_obs"
    traj, obs, actions = br.term_traj("slim", m, n, 41)
    prm, _ = set_reward(eng, inputs, hidden, act, seed=21)
    rows = np.zeros((m, n, p), F)
    _, steps, _ = eng.reward_returns(traj, obs, actions, rows, prm, want_steps=True)
    steps = _np(steps)
    reps = need // (H * m * n * p) + 2
    assert H * m * n * reps * p > need
    big = eng.reward_returns(np.tile(traj, (1, 1, reps, 1, 1)), obs, np.tile(actions, (1, reps, 1, 1)), np.zeros((m, n * reps, p), F), prm,
                             want_steps=True)[1]
    big = _np(big).reshape(H, m, reps, n, p)
    for r in (0, 1, reps - 1):
        np.testing.assert_array_equal(_bits(big[:, :, r]), _bits(steps), err_msg="reward %r: copy %d of the candidates" % (hidden, r))
    flat = rref.gather_inputs(traj, obs, actions, inputs).reshape(-1, 2 * D + eng.A)
    full = steps.reshape(-1)
    ev = _np(eng.reward_eval(np.concatenate([flat[3:]] + [flat] * (need // flat.shape[0] + 2), axis=0)))
    assert ev.shape[0] > need
    np.testing.assert_array_equal(_bits(ev[:flat.shape[0] - 3]), _bits(full[3:]), err_msg="reward_eval, head")
    np.testing.assert_array_equal(_bits(ev[-flat.shape[0]:]), _bits(full), err_msg="reward_eval, tail")
    # the value net on the last states
    set_value(eng, hidden, act, seed=21)
    states = traj[-1].reshape(-1, D)
    small = _np(eng.value_eval(states))
    ev = _np(eng.value_eval(np.concatenate([states[3:]] + [states] * (need // states.shape[0] + 2), axis=0)))
    assert ev.shape[0] > need
    np.testing.assert_array_equal(_bits(ev[:states.shape[0] - 3]), _bits(small[3:]), err_msg="value_eval, head")
    np.testing.assert_array_equal(_bits(ev[-states.shape[0]:]), _bits(small), err_msg="value_eval, tail")


def test_reward_long_horizon(engines):
    """H = 40 at (2, 9), (37, 5) tanh, K = 42: the step sum's second batch of 32 loads.  `first` drawn over 0 .. 40 with 0, 31, 32, 33, 39
    and 40 planted: S is `reward_ref.step_sum` of the kernel's own step rewards bit for bit, the steps behind the cut read NaN, and NaN
    planted only in steps that are not counted changes no row; without `first` all 40 steps count.  The value net reads traj[39]: a NaN
    planted in traj[38] changes nothing."""
    _, eng = engines("long")
    H, p, m, n, inputs = eng.H, eng.p, 2, 9, "obs_act_next_obs"
    traj, obs, actions = br.term_traj("long", m, n, 12)
    K = rref.input_dims(inputs, eng.D, eng.A)
    layers = rref.he_net(K, (37, 5), seed=6)
    prm = HipEngine.reward_params(inputs, (37, 5), "tanh", 2.0)
    eng.set_reward_net(prm, layers)
    _live(rref.gather_inputs(traj, obs, actions, inputs), layers, "tanh", "reward long")
    rows = np.random.default_rng(4).standard_normal((m, n, p)).astype(F)
    r, ref_steps, _ = reward_check(eng, prm, layers, "tanh", inputs, traj, obs, actions, rows, 2.0, "reward long, no cut")
    first = np.random.default_rng(13).integers(0, H + 1, (m, n, p)).astype(np.int32)
    first.reshape(-1)[:6] = (0, 31, 32, 33, 39, 40)
    live = rref.counted(H, (m, n, p), first)
    out, steps, S = (_np(t) for t in eng.reward_returns(traj, obs, actions, rows, prm, first=first, want_steps=True))
    assert np.isnan(steps[~live]).all() and (~live).any()
    np.testing.assert_array_equal(_bits(steps[live]), _bits(ref_steps[live]))
    np.testing.assert_array_equal(_bits(S), _bits(rref.step_sum(ref_steps, first)))
    np.testing.assert_array_equal(_bits(out), _bits(rref.update(rows, rref.step_sum(ref_steps, first), 2.0)))
    only = traj.copy()
    only[~live] = np.nan                               # s_{t+1} of every step that is not counted: no counted step reads it
    out2, steps2, S2 = (_np(t) for t in eng.reward_returns(only, obs, actions, rows, prm, first=first, want_steps=True))
    assert np.isnan(only).any()
    np.testing.assert_array_equal(_bits(out2), _bits(out), err_msg="NaN in steps that are not counted reached a row")
    np.testing.assert_array_equal(_bits(S2), _bits(S))
    np.testing.assert_array_equal(_bits(steps2), _bits(steps))
    print("\n[reward long (2, 9), H = 40, K = %d] worst |err| / (1e-5 of scale): %.3f" % (K, r))
    # the value: V of traj[H - 1]
    vlayers = vref.envelope_net(eng.D, (37, 37, 37, 37))
    vprm = HipEngine.value_params((37, 37, 37, 37), "swish", 2.0)
    eng.set_value_net(vprm, vlayers)
    _live(traj[-1], vlayers, "swish", "value long")
    rv, v, _ = value_check(eng, vprm, vlayers, "swish", traj, rows, 2.0, "value long")
    bad = traj.copy()
    bad[H - 2] = np.nan
    out_b, v_b = (_np(t) for t in eng.value_returns(bad, rows, vprm, want_v=True))
    np.testing.assert_array_equal(_bits(v_b).reshape(-1), _bits(v), err_msg="a NaN in traj[H - 2] reached V")
    np.testing.assert_array_equal(_bits(out_b), _bits(vref.update(rows, v_b, 2.0)))
    print("[value long (2, 9), H = 40] worst |err| / (1e-5 of scale): %.3f" % rv)


def test_one_step_horizon(engines):
    """H = 1: every step's s_t is `obs` (traj[t - 1] is never addressed) -- every `inputs` kind against the restatement; `first` in {0, 1}
    cuts nothing off the reward (step 0 always counts), while for the value first = 0 < H is a cut: the row keeps its bits, V reads NaN."""
    _, eng = engines("one")
    assert eng.H == 1
    m, n, p = 3, 11, eng.p
    traj, obs, actions = br.term_traj("one", m, n, 91)
    rows = np.random.default_rng(2).standard_normal((m, n, p)).astype(F)
    first = np.random.default_rng(3).integers(0, 2, (m, n, p)).astype(np.int32)
    assert (first == 0).any() and (first == 1).any()
    worst = 0.0
    for inputs in rref.INPUTS:
        K = rref.input_dims(inputs, eng.D, eng.A)
        layers = vref.envelope_net(K, (5, 7))
        prm = HipEngine.reward_params(inputs, (5, 7), "swish", 0.5)
        eng.set_reward_net(prm, layers)
        _live(rref.gather_inputs(traj, obs, actions, inputs), layers, "swish", "reward one " + inputs)
        r, steps, _ = reward_check(eng, prm, layers, "swish", inputs, traj, obs, actions, rows, 0.5, "reward H=1 " + inputs)
        worst = max(worst, r)
        out, s2, S = (_np(t) for t in eng.reward_returns(traj, obs, actions, rows, prm, first=first, want_steps=True))
        np.testing.assert_array_equal(_bits(s2), _bits(steps), err_msg="first in {0, 1} is no cut at H = 1")
        np.testing.assert_array_equal(_bits(out), _bits(rref.update(rows, rref.step_sum(steps), 0.5)))
    layers = vref.envelope_net(eng.D, (5, 7))
    prm = HipEngine.value_params((5, 7), "swish", 0.5)
    eng.set_value_net(prm, layers)
    rv, v, _ = value_check(eng, prm, layers, "swish", traj, rows, 0.5, "value H=1")
    out, v2 = (_np(t) for t in eng.value_returns(traj, rows, prm, first=first, want_v=True))
    cut = first < 1
    np.testing.assert_array_equal(_bits(out[cut]), _bits(rows[cut]), err_msg="a row with first = 0 < H must keep its bits")
    assert np.isnan(v2[cut]).all()
    np.testing.assert_array_equal(_bits(v2[~cut]), _bits(v.reshape(m, n, p)[~cut]))
    np.testing.assert_array_equal(_bits(out[~cut]), _bits(vref.update(rows, v.reshape(m, n, p), 0.5)[~cut]))
    print("\n[H = 1] worst |err| / (1e-5 of scale): reward %.3f, value %.3f" % (worst, rv))


# ---------------------------------------------------------------------------------------------------------------------- 6: the loop
def act_state(eng, d, seed):
    """tests/test_gpu_actuator.py's (prev, prefix): env 0 known with one free committed element, env 1's prev unknown.  It frees
    element [0, 0, 1] of the prefix, which A = 1 does not have: there element [0, 0, 0]."""
    if eng.A > 1:
        return _act_state(eng, d, seed)
    rng = np.random.default_rng(seed)
    prev = rng.uniform(-0.8, 0.8, (M, 1)).astype(F)
    prev[1] = np.nan
    prefix = rng.uniform(-1, 1, (M, d, 1)).astype(F)
    prefix[0, 0, 0] = np.nan
    return eng._t(prev).clone(), eng._t(prefix).clone()


def _everything(eng, prob, name, mppi):
    """every optional stage of the loop on one engine: a dict of the parameter objects and what the checks need to restate them"""
    H, A, D = eng.H, eng.A, eng.D
    assert eng.lib.cadm_rollout_builtin(eng._ctx), "%s: the loop tests run on geometries the library carries" % name
    e = dict(inputs="obs_act_next_obs")
    e["track"], e["targets"], e["offset"], e["terms"] = _tracking_inputs(eng, prob, 3, H, 13)
    traj0 = iteration0_traj(eng, prob, 1.0 if mppi else 0.0, 4, 1)
    e["cons"] = HipEngine.constraint_params(binding_bounds(traj0, CONSTRAINED[name], H, "%s, everything on" % name), "terminate", 4.0)
    e["reward"], _ = set_reward(eng, e["inputs"], (37, 5), "tanh", seed=31, weight=1.5)
    e["value"], _ = set_value(eng, (3,), "swish", seed=33, weight=3.0)
    e["w"] = uref.make_w("per-dim", D, seed=8)
    e["unc"] = unc_prm(eng, "total", 0.3, e["w"], "std", None)
    rng = np.random.default_rng(3)
    e["dl"] = np.where(np.arange(A) % 2 == 0, 0.3, np.inf).astype(F)
    e["rate_w"] = np.where(np.arange(A) % 3 == 2, 0.0, rng.uniform(0.5, 4.0, A)).astype(F)      # costs on two of every three dims
    e["act"] = act_params(eng, 1, e["dl"], e["rate_w"])
    e["knots"] = HipEngine.knot_params(2, "linear")
    e["phase"] = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    e["score"] = HipEngine.score_params("cvar", k=2)
    e["icem"] = dict(noise_beta=1.0 if mppi else 0.0, keep_elites=2, decay=1.25, return_best=not mppi, add_mean_last=True)
    e["prm"] = HipEngine.mppi_params(temperature=0.5, relative=True, **e["icem"]) if mppi else HipEngine.icem_params(**e["icem"])
    return e


def _fused(eng, e, args, state, carry, call, off=(), policy=None, critic=None, **kw):
    """`cadm_rewarded_plan` with everything of `e` on but the terms named in `off`; policy: a `policy_params` of the engine's registered
    policy net -- then `cadm_guided_plan` with its proposals next to them (tests/test_gpu_policy_envelope.py); critic: a `critic_params`
    of the registered critics -- then `cadm_critic_plan` (tests/test_gpu_critic_envelope.py; "value" must be in `off`: one terminal term)"""
    g = lambda k: None if k in off else e[k]
    prev, prefix = (None, None) if "act" in off else state
    plan = eng.rewarded_plan if policy is None else (lambda *a, **k: eng.guided_plan(policy, *a, **k))
    if critic is not None:
        plan = lambda *a, **k: eng.critic_plan(critic, policy, *a, **k)
    return plan(g("reward"), g("value"), g("unc"), g("act"), prev, prefix, True, g("track"), e["targets"], e["offset"], g("knots"),
                None if "knots" in off else e["phase"], e["cons"], e["score"], e["prm"], *args, N, carry=carry[0],
                carry_valid=carry[1], seed=4, call=call, **kw)


def _stepwise(eng, e, args, state, carry, call, mppi, off=(), policy=None, critic=None, **kw):
    """the same loop one launch at a time"""
    g = lambda k: None if k in off else e[k]
    return hplanner.icem_plan(eng, *args, N, carry=carry[0], carry_valid=carry[1], seed=4, call=call, update="mppi" if mppi else "cem",
                              temperature=0.5, relative=True, score=e["score"], constraints=e["cons"], knots=g("knots"),
                              phase=None if "knots" in off else e["phase"], tracking=None if "track" in off else (e["track"], e["targets"], e["offset"]),
                              actuator=None if "act" in off else (e["act"], state[0], state[1]), action_advance=True, uncertainty=g("unc"),
                              value=g("value"), reward=g("reward"), policy=policy, critic=critic, **e["icem"], **kw)


LOOP = [(e, u) for e in ("slim", "pend") for u in ("mppi", "cem")]


@pytest.mark.parametrize("name,update", LOOP, ids=["%s-%s" % c for c in LOOP])
def test_everything_on(engines, name, update):
    """TERMINATE constraints, three tracking terms, a reward net (obs_act_next_obs, (37, 5), tanh), a value net ((3,), swish), an
    uncertainty term (total, std), an actuator (delay 1, limits on even dims, costs on two of every three), knots (2, linear), a CVaR
    score, two kept elites, decay 1.25, the mean added last -- under the MPPI update with coloured noise, and under the elite refit
    returning the best plan.  `cadm_rewarded_plan` == the stepwise loop bit for bit over two calls: the plan, the best return, the
    carry, the actuator's prev and prefix; every stepwise iteration passes the feature files' own checks.  Then the C entry with a
    workspace of exactly `cadm_rewarded_workspace_bytes` bytes and 4 KiB of a bit pattern behind it: call 2's plan again, the pattern
    intact."""
    prob, eng = engines(name)
    H, A, mppi = eng.H, eng.A, update == "mppi"
    e = _everything(eng, prob, name, mppi)
    obs3 = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    ca, cb = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    sa, sb = act_state(eng, 1, 8), act_state(eng, 1, 8)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        before = (_np(sa[0]).copy(), _np(sa[1]).copy())
        kept = [t.clone() for t in (*ca, *sa)] + [eng._t(mean).clone()]
        a, ra = _fused(eng, e, (*obs3, mean, var), sa, ca, call, want_best_return=True)
        b, info, extra = _stepwise(eng, e, (*obs3, mean, var), sb, cb, call, mppi, return_info=True)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max()
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        for x, y, what in ((ca[0], cb[0], "carry"), (sa[0], sb[0], "prev"), (sa[1], sb[1], "prefix")):
            np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)), err_msg="%s after call %d" % (what, call))
        reward_iterations(eng, info, prob, e["reward"], e["inputs"], True)
        value_iterations(eng, info, e["value"], True)
        uncertainty_iterations(eng, info, e["unc"], "total", e["w"], "std", None, terminate=True)
        actuator_iterations(eng, info, 1, e["dl"], e["rate_w"], before)
        for x in info:
            first = _np(x["first_violation"])
            _, cost_ref, S, _ = tref.tracking(_np(x["traj"]), _np(x["rows_untracked"]), e["terms"], _np(e["targets"]), _np(e["offset"]), first)
            assert (np.abs(_np(x["track_cost"]) - cost_ref) <= tref.bound(S, None, H, 3)).all()
        assert len({int(x["rows"].shape[1]) for x in info}) > 1, "decay must change the packed candidate count"
        if call == 1:
            share = float((_np(info[0]["first_violation"]) < H).mean())
            assert 0.1 <= share <= 0.9, "%.2f of the rows are cut" % share
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    assert (mppi, "rew", True, True, True) in eng._loop_ws
    # the C entry on call 2's inputs, in a workspace of exactly the size it asks for
    lib = eng.lib
    _, full = eng._as_mppi_params(e["prm"])
    nbytes = lib.cadm_rewarded_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, 1, 1)
    assert nbytes > 0
    ws = torch.empty((nbytes + 4096,), dtype=torch.uint8, device=eng.device)
    ws[nbytes:] = 0xA5
    assert ws.data_ptr() % 256 == 0
    carry2, valid2, prev2, prefix2, mean2 = kept
    targets, T, offset = eng._targets(e["targets"], e["offset"], M, 3, "test")
    t = [eng._t(x) for x in obs3] + [mean2, eng._t(var)]
    out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
    best = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = lib.cadm_rewarded_plan(eng._ctx, ct.byref(e["reward"]), ct.byref(e["value"]), ct.byref(e["unc"]), ct.byref(e["act"]), P(prev2), P(prefix2),
                                1, ct.byref(e["track"]), P(targets), T, P(offset), ct.byref(e["knots"]), P(e["phase"]), ct.byref(e["cons"]),
                                ct.byref(e["score"]), int(mppi), ct.byref(full), *[P(x) for x in t], P(carry2), P(valid2), M, N, 4, 2, P(ws),
                                P(out), P(best), eng.stream)
    assert rc == 0, lib.cadm_last_error().decode()
    np.testing.assert_array_equal(_bits(_np(out)), _bits(a), err_msg="the C entry in an exact workspace")
    np.testing.assert_array_equal(_bits(_np(best)), _bits(_np(ra)))
    np.testing.assert_array_equal(_bits(_np(carry2)), _bits(_np(ca[0])))
    assert (_np(ws[nbytes:]) == 0xA5).all(), "the loop wrote behind the workspace it asked for"


TERMS = ["reward", "value", "unc", "act", "track", "knots"]


@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("name", ["slim", "pend"])
def test_each_term_matters(engines, name, term):
    """Everything on under MPPI, then one of the six terms NULL and the other five on: another plan than with all six, and bit for bit
    the plan, the best return and the carry of the stepwise loop without that term.  reward = NULL is `cadm_valued_plan`'s loop: the C
    entry with NULL in that place and the valued loop's workspace gives `valued_plan`'s bits."""
    prob, eng = engines(name)
    H, A = eng.H, eng.A
    e = _everything(eng, prob, name, True)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"])
    full = _np(_fused(eng, e, args, act_state(eng, 1, 8), zero_carry(eng, M, 2, H), 1))
    ca, cb = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    sa, sb = act_state(eng, 1, 8), act_state(eng, 1, 8)
    a, ra = _fused(eng, e, args, sa, ca, 1, off=(term,), want_best_return=True)
    b, _, extra = _stepwise(eng, e, args, sb, cb, 1, True, off=(term,), return_info=True)
    a = _np(a)
    assert np.isfinite(a).all() and not np.array_equal(_bits(a), _bits(full)), "%s does not change the plan" % term
    np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="without %s: the plan" % term)
    np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])))
    np.testing.assert_array_equal(_bits(_np(ca[0])), _bits(_np(cb[0])))
    if term != "act":
        np.testing.assert_array_equal(_bits(_np(sa[0])), _bits(_np(sb[0])))
        np.testing.assert_array_equal(_bits(_np(sa[1])), _bits(_np(sb[1])))
    if term == "reward":
        lib = eng.lib
        _, prm = eng._as_mppi_params(e["prm"])
        ws = eng._loop_workspace(True, M, N, 2, val=(True, True, True))
        carry, valid = zero_carry(eng, M, 2, H)
        prev, prefix = act_state(eng, 1, 8)
        targets, T, offset = eng._targets(e["targets"], e["offset"], M, 3, "test")
        t = [eng._t(x) for x in args]
        out = torch.empty((M, H, A), dtype=torch.float32, device=eng.device)
        P = lambda x: ct.c_void_p(x.data_ptr())
        rc = lib.cadm_rewarded_plan(eng._ctx, None, ct.byref(e["value"]), ct.byref(e["unc"]), ct.byref(e["act"]), P(prev), P(prefix), 1,
                                    ct.byref(e["track"]), P(targets), T, P(offset), ct.byref(e["knots"]), P(e["phase"]), ct.byref(e["cons"]),
                                    ct.byref(e["score"]), 1, ct.byref(prm), *[P(x) for x in t], P(carry), P(valid), M, N, 4, 1, P(ws), P(out),
                                    None, eng.stream)
        assert rc == 0, lib.cadm_last_error().decode()
        np.testing.assert_array_equal(_bits(_np(out)), _bits(a), err_msg="cadm_rewarded_plan(reward = NULL) in the valued loop's workspace")
