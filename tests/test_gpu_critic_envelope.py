"""GPU: the terminal value from Q critics (`cadm_critic_eval`, `cadm_critic_returns`, `cadm_critic_plan`; csrc/critic.hip) OFF the
geometry tests/test_gpu_critic.py runs its kernel on (hopper_like: D = 11, A = 3, K = 14, p = 5, H = 3; hidden widths that are multiples
of 4; C <= 3; actors of at most three dense layers; the loop on halfcheetah only).

Engines (tests/behind_rollout.py TERM_ENGINES, built when first asked for; kernel level, nothing is rolled out and nothing is built on
demand; rows of the two launches from behind_rollout.CRITIC_ROWS):
    pend    pendulum       D = 3   A = 1   K = 4   K4 = 4   D4 = 4    135 and 5 rows    W = K4 - D = 1: line 3 is the action loop's alone
    ant     ant            D = 28  A = 8   K = 36  K4 = 36  D4 = 28   210 and 10 rows   D = D4 and K = K4: neither loop pads
    slim    slim_humanoid  D = 45  A = 17  K = 62  K4 = 64  D4 = 48   150 and 15 rows   three padding lines behind D, two behind K
    wide    corner_spec("widest")  D = 48  A = 24  K = 72             330 and 10 rows   the widest declarable env
    long    halfcheetah, H = 40    D = 18  A = 6   K = 24             165 and 5 rows    traj + 39 total D; weight * disc[40] (gamma 0.97)
    one     halfcheetah, H = 1                                        165 and 5 rows    the terminal state is traj[0]
    p1      halfcheetah, E = 1, p = 1                                 33 and 1 rows     total = m n
The loop runs on the built-in geometries pendulum and slim_humanoid (tests/test_gpu_terms_envelope.py's engines and problems).

The checks are tests/test_gpu_critic.py's own, imported: `check_kernel_cases` (the body of its `test_kernel_against_restatement`),
`check_bits_in_any_batch`, `check_non_finite_and_first`, `check_fused_equals_stepwise`, and tests/test_gpu_terms_envelope.py's
`_everything` / `_fused` / `_stepwise` with a `critic=`.  No bar of its own: `helpers.assert_close` at 1e-5 of scale against the float64
restatement (tests/critic_ref.py), bit equality everywhere else.  The cases are `critic_ref.ENVELOPE_CASES` -- critics (1,), (3,),
(65,), (130, 66), (50, 30, 70, 18), (37,) * 4 behind actors (), (50, 30, 70, 18), (37,) * 4; C in (1, 4, 5), both reduces, both
squashes, every activation --; tests/test_critic_ref.py holds every one of them, on every engine, to the liveness conditions and holds
the float32 chain of the restatement to the same bar on the CPU (worst 0.35 of it).

Code no other test reaches -> the test here that does:
    critic.hip  the state loop without padding lines (D = D4), the action loop without zero lines (K = K4)      test_kernel[ant-*]
                W = K4 - D = 1, line 3 written by the action loop only; A = 1                                   test_kernel[pend-*]
                three zero lines behind D in the actor's tile, two behind K in the critics'; A = 17             test_kernel[slim-*]
                A = 8, 24; K4 = 36, 64, 72 (`critic_kernel<1>` and `<2>`: the swizzle on odd k beyond K4 = 16)   test_kernel[*], test_two_row_tiles
                hidden widths off the multiples of 4, four hidden layers (the fourth region swap) under an
                actor of five dense layers; `critic_lds_bytes` where the actor's regions are the wider ones     test_kernel[*]
                C = 4 and C = 5: vres[C][R] and the flags behind it                                             test_kernel[*]
                `traj + (H - 1) total D` at H = 40 and H = 1; weight * disc[40]                                 test_kernel[long-*], [one-*]
                p = 1, E = 1                                                                                    test_kernel[p1-*]
                the regions sized without the actor (given actions) at D = 3, 45, 48                            test_given_actions
                poison in the last real dim (44) next to the padding lines 45 .. 47; `first` over 0 .. 40       test_non_finite_and_first
    icem.hip    the critic stage on pendulum and slim_humanoid, beside every other term                         test_loop, test_critics_beside_every_term

Measured on an MI355X, worst |err| / (1e-5 x max(|ref|, rms)) over q and every critic's q (run with -s) -- every case passes, no kernel
was changed:
                relu   tanh   swish
    pend  K = 4   0.144  0.164  0.492
    ant   K = 36  0.243  0.128  0.208
    slim  K = 62  0.123  0.137  0.216
    wide  K = 72  0.177  0.190  0.338
    long  K = 24  0.102  0.102  0.184
    one   K = 24  0.128  0.107  0.256
    p1    K = 24  0.112  0.090  0.254
The float32 chain of the restatement alone gives 0.085 .. 0.352 on the same cases (tests/test_critic_ref.py prints them; its worst is
pend under swish as well, 0.352): no GPU figure is as much as twice the CPU's.  Given actions, two row tiles, the non-finite rows and
the loop are bit equality.  The whole file runs in 5 s; the slowest case (18 cases x 2 launches on pend) in 0.2 s."""
import numpy as np
import pytest

import behind_rollout as br
import critic_ref as cref
import discount_ref as dref
from cadm_amd.engine import HipEngine
from helpers import _np, zero_carry
from test_gpu_critic import (_bits, _register, check_bits_in_any_batch, check_fused_equals_stepwise, check_kernel_cases,
                             check_non_finite_and_first)
from test_gpu_policy_envelope import _loop_policy
from test_gpu_terms_envelope import CONSTRAINED, _everything, _fused, _stepwise, act_state
from test_gpu_terms_envelope import engines      # noqa: F401  (the module-scoped fixture: TERM_ENGINES, built when first asked for)

pytestmark = pytest.mark.gpu

F = np.float32
M = 2
GEOMETRY = {"pend": (3, 1), "ant": (28, 8), "slim": (45, 17), "wide": (48, 24), "long": (18, 6), "one": (18, 6), "p1": (18, 6)}


# ---------------------------------------------------------------------------------------------------------------------- 1: the kernel
KERNEL = [(name, act) for name in br.CRITIC_ROWS for act in cref.ACTS]


@pytest.mark.parametrize("name,act", KERNEL, ids=["%s-%s" % c for c in KERNEL])
def test_kernel(engines, name, act):
    """tests/test_gpu_critic.py's `test_kernel_against_restatement`, as it stands, on every `critic_ref.ENVELOPE_CASES` entry: q, every
    critic's q and the action used against the float64 restatement at 1e-5 of scale; q against `reduce32` of the critics' bit for bit;
    `critic_returns`' q_out against `critic_eval` and its rows against the row update bit for bit -- at a launch that ends in a partial
    tile and at one of fewer than 16 rows.  "long" carries a discount: the update multiplies by float32(0.5 disc[40])."""
    _, eng = engines(name)
    assert (eng.D, eng.A) == GEOMETRY[name]
    rows_of = br.CRITIC_ROWS[name]
    assert all((m * n * eng.p) % 16 != 0 for m, n in rows_of) and rows_of[0][0] * rows_of[0][1] * eng.p > 16 > rows_of[1][0] * rows_of[1][1] * eng.p
    states_of = lambda m, n, seed: cref.kernel_states(m, n, seed, name=name)
    weight = 0.5
    try:
        if name == "long":
            eng.set_discount(br.CRITIC_GAMMA)
            disc = eng.discount_weights()
            np.testing.assert_array_equal(_bits(disc), _bits(dref.weights(br.CRITIC_GAMMA, eng.H)))
            weight = dref.terminal_weight(0.5, disc)
            assert eng.H == 40 and 0 < weight < 0.2
        worst = check_kernel_cases(eng, act, cref.ENVELOPE_CASES, rows_of, states_of, weight)
    finally:
        if name == "long":
            eng.set_discount(1.0)
    print("\n[critic %s %s, K = %d] worst |err| / (1e-5 of scale): %.3f" % (name, act, eng.D + eng.A, worst))


# ---------------------------------------------------------------------------------------------------------------------- 2: given actions
@pytest.mark.parametrize("name", ["pend", "slim", "wide"])
def test_given_actions(engines, name):
    """`critic_eval(states, actions=policy_eval(states))` -- a launch whose regions are sized without the actor -- has the fused path's
    bits: q, every critic's q and act_out; under the widest critic net behind the deepest actor and under the narrowest behind none."""
    _, eng = engines(name)
    m, n = br.CRITIC_ROWS[name][0]
    states = cref.kernel_states(m, n, 51, name=name)[1]
    for hidden, phidden, act, C, reduce in (((130, 66), (37, 37, 37, 37), "swish", 5, "mean"), ((3,), (), "relu", 4, "min")):
        actor, critics, mean, std = cref.kernel_case(states, eng.A, hidden, phidden, C, act, "tanh", 23)
        _register(eng, actor, critics, hidden, phidden, act, reduce, 1.0, mean, std)
        full, each, a = (_np(x) for x in eng.critic_eval(states, want_each=True, want_actions=True))
        assert np.isfinite(full).all() and full.std() > 0
        pa = _np(eng.policy_eval(states))
        np.testing.assert_array_equal(_bits(a), _bits(pa), err_msg="act_out against policy_eval")
        g, geach, ga = (_np(x) for x in eng.critic_eval(states, actions=pa, want_each=True, want_actions=True))
        np.testing.assert_array_equal(_bits(g), _bits(full), err_msg="%s %r: given the actor's action" % (name, hidden))
        np.testing.assert_array_equal(_bits(geach), _bits(each))
        np.testing.assert_array_equal(_bits(ga), _bits(pa), err_msg="act_out of given actions")


# ---------------------------------------------------------------------------------------------------------------------- 3: two row tiles
TILES = [(name, hidden) for name in ("slim", "wide") for hidden in ((130, 66), (50, 30, 70, 18))]


@pytest.mark.parametrize("name,hidden", TILES, ids=["%s-%s" % (n_, "x".join(map(str, h))) for n_, h in TILES])
def test_two_row_tiles(engines, name, hidden):
    """tests/test_gpu_critic.py's `test_a_state_has_the_same_bits_in_any_batch` at K4 = 64 and 72: 165 states at the head and the tail
    of more than 2 x 16 x the CU count rows (`critic_kernel<2>`) have the bits of the one-tile launch; and at R = 1, 5, 16, rolled by 7,
    given the actor's actions, run to run.  slim: the 165 states are the last states of an (1, 11) trajectory, so `critic_returns`' q_out
    and the call with leading dims are held too."""
    _, eng = engines(name)
    traj = None
    if name == "slim":
        traj, states = cref.kernel_states(1, 11, 41, name=name)
    else:
        states = cref.kernel_states(2, 11, 41, name=name)[1][:165]
    assert states.shape == (165, eng.D)
    phidden, act, C, reduce = ((50, 30, 70, 18), "tanh", 4, "mean") if hidden == (130, 66) else ((37, 37, 37, 37), "swish", 5, "min")
    check_bits_in_any_batch(eng, states, hidden, phidden, act, C, reduce, traj)


# ---------------------------------------------------------------------------------------------------------------------- 4: non-finite rows, the first cut
@pytest.mark.parametrize("name,act", [("slim", "relu"), ("slim", "tanh"), ("long", "relu")], ids=["slim-relu", "slim-tanh", "long-relu"])
def test_non_finite_and_first(engines, name, act):
    """tests/test_gpu_critic.py's `test_non_finite_terminal_states_and_the_first_cut`.  slim: the poison sits in dim 44, the last line in
    front of the padding lines 45 .. 47 of the actor's tile (nothing can be planted there: every row that is not poisoned keeps its
    bits, so nothing leaks out of them), and in dim 0.  long: H = 40, `first` drawn over 0 .. 40, the terminal state at traj + 39 total
    D; `behind_rollout`'s seed for it is one under which a poisoned row stays uncut."""
    _, eng = engines(name)
    m, n = (2, 5) if name == "slim" else (3, 11)
    clean = cref.kernel_states(m, n, 12, name=name)[0]
    if name == "slim":
        check_non_finite_and_first(eng, act, clean, dims=(44, 0), hidden=(50, 30, 70, 18), phidden=(37, 37, 37, 37))
    else:
        check_non_finite_and_first(eng, act, clean, hidden=(130, 66), phidden=(50, 30, 70, 18), seed=br.CRITIC_LONG_SEED)


# ---------------------------------------------------------------------------------------------------------------------- 5: the loop
LOOP = [(name, combo) for name in ("pend", "slim") for combo in ("cem", "mppi-terminate", "cem-prior")]


@pytest.mark.parametrize("name,combo", LOOP, ids=["%s-%s" % c for c in LOOP])
def test_loop(engines, name, combo):
    """tests/test_gpu_critic.py's `test_fused_equals_stepwise` on pendulum and slim_humanoid: `cadm_critic_plan` == the stepwise loop
    (`planner.icem_plan(critic=...)`) bit for bit over two calls, under the elite refit, under MPPI with TERMINATE constraints on the
    dims tests/test_gpu_constraints.py constrains on these kinds, and with a policy prior in the same call; critics (37,) * 4 behind an
    actor (50, 30)."""
    prob, eng = engines(name)
    assert eng.lib.cadm_rollout_builtin(eng._ctx), "%s: the loop tests run on geometries the library carries" % name
    check_fused_equals_stepwise(prob, eng, combo, CONSTRAINED[name], hidden=(37, 37, 37, 37), phidden=(50, 30))


BESIDE = [("slim", "mppi"), ("pend", "cem")]


@pytest.mark.parametrize("name,update", BESIDE, ids=["%s-%s" % c for c in BESIDE])
def test_critics_beside_every_term(engines, name, update):
    """tests/test_gpu_terms_envelope.py's `_everything` without the value net (one terminal term) -- TERMINATE constraints, tracking, a
    reward net, an uncertainty term, an actuator, knots, a CVaR score -- plus a policy prior of 6 proposals and two critics (65,) at the
    actor's action: `cadm_critic_plan` == the stepwise loop bit for bit over two calls: the plan, the best return, the carry, the
    actuator's prev and prefix.  Without the critics the plan is another."""
    prob, eng = engines(name)
    H, A, mppi = eng.H, eng.A, update == "mppi"
    e = _everything(eng, prob, name, mppi)
    pol = _loop_policy(eng)
    crt = HipEngine.critic_params((65,), "swish", 2, "min", 2.0)
    eng.set_critic_nets(crt, cref.he_critics(eng.D, eng.A, (65,), 2, 35))
    obs3 = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    ca, cb = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    sa, sb = act_state(eng, 1, 8), act_state(eng, 1, 8)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = _fused(eng, e, (*obs3, mean, var), sa, ca, call, off=("value",), policy=pol, critic=crt, want_best_return=True)
        b, info, extra = _stepwise(eng, e, (*obs3, mean, var), sb, cb, call, mppi, off=("value",), policy=pol, critic=crt, return_info=True)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max()
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        for x, y, what in ((ca[0], cb[0], "carry"), (sa[0], sb[0], "prev"), (sa[1], sb[1], "prefix")):
            np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)), err_msg="%s after call %d" % (what, call))
        for x in info:
            q, before, rows, first = _np(x["q"]), _np(x["q_rows"]), _np(x["rows"]), _np(x["first_violation"])
            np.testing.assert_array_equal(_bits(rows), _bits(cref.update(before, q, crt.weight, first, H)))
            assert np.isnan(q[first < H]).all() and np.isfinite(q[first >= H]).all() and (first >= H).any()
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    other = _np(_fused(eng, e, (*obs3, prob["init_mean"], var), act_state(eng, 1, 8), zero_carry(eng, M, 2, H), 1, off=("value",), policy=pol))
    first_call = _np(_fused(eng, e, (*obs3, prob["init_mean"], var), act_state(eng, 1, 8), zero_carry(eng, M, 2, H), 1, off=("value",), policy=pol,
                            critic=crt))
    assert np.isfinite(other).all() and not np.array_equal(_bits(other), _bits(first_call)), "the critics do not change the plan"
