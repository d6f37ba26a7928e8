"""GPU: the policy prior's proposal roll (`cadm_policy_propose`, csrc/policy.hip) and the guided loop (`cadm_guided_plan`, csrc/icem.hip)
OFF the one geometry tests/test_gpu_policy.py rolls on (halfcheetah: D = 18, A = 6, p in {5, 20}, H <= 5, at most 51 rows a launch,
bounds -1, 1, no other planner term next to the proposals).

Engines (tests/behind_rollout.py POLICY_ENGINES, built when first asked for, each with an H = 1 twin of the same weights; every one a
geometry the library carries -- `cadm_rollout_builtin` -- but "wide", which is never rolled out):
    pend    pendulum, context        D = 3   A = 1   p = 5   H = 5     A = 1, D4 = 4
    ant     ant, context             D = 28  A = 8   p = 10  H = 3     two full noise groups, p = 10
    slim    slim_humanoid, context   D = 45  A = 17  p = 15  H = 3     odd D, noise groups 0 .. 4 with one dim in the last, p = 15
    long    halfcheetah, vanilla     D = 18  A = 6   p = 5   H = 40    the long roll
    big     halfcheetah, vanilla     "long"'s weights, H = 2           8255 rows: two row tiles per workgroup
    bnd     halfcheetah, context     bounds -0.5, 2.0, H = 3           mid, half and the clip in the roll
    fit     halfcheetah, vanilla     H = 5                             tests/test_gpu_policy.py's "hc5-vanilla": the exact fit of the slots
    wide    corner_spec("widest")    D = 48  A = 24  p = 10  H = 1     noise at A = 24 through the C entry: at H = 1 the roll launches no
                                                                       rollout, and `cadm_policy_propose` asks for none to be registered
The problems are tests/test_gpu_terms_envelope.py's (m = 2, seed 3, `trained_like`), grown to more envs by `behind_rollout.with_rows`.

No tolerance of its own.  An action of a step: `policy_ref.emulate32` on `particle_mean32` of the states the step read, at 1e-5 of the
action range; a recovered draw: (1e-5 of the range) / noise_std + 4e-6 max(1, radius / 2); everything else bit equality -- the checks
are `test_gpu_policy.check_roll` and tests/test_gpu_terms_envelope.py's `_everything`, `_fused`, `_stepwise` and `act_state`,
imported.  tests/test_policy_ref.py shows on the CPU that the restatement alone meets what the tests ask of their inputs: the nets hold
the bar and are live on these D, more than half of the draws (0.98 with the bias-only net) stay unclipped at step 0 of every geometry,
and the roll of engine "long" stays finite and below 1e4 over all 40 steps (the synthetic model doubles its states every five steps:
the first layer of that net is scaled by 2^-7, `behind_rollout.policy_layers`, so that the tanh squash stays open).

Code no other test reaches -> the test here that does:
    policy.hip  noise groups g = d >> 2 of 1 (full), 2, 3 and a last group of one dim (A = 8, 17)        test_roll_per_kind[ant-*], [slim-*]
                A = 1: z0 of words (0, 1) alone; D4 = 4                                                  test_roll_per_kind[pend-*]
                six full groups (A = 24), every one against Philox                                       test_noise_at_24_actions
                the particle sum at p = 10 and 15 (the division is inexact), D = 45 (D4 = 48), D = 28    test_roll_per_kind
                policy_step_kernel<2> with obs, p > 1, `states` stores and the q % P noise gate          test_two_row_tile_roll_*
                nf = nf || mlp_nonfinite(v) over particles j >= 1: a row that is partly non-finite        test_partly_non_finite_row
                a non-finite context of one member of one env next to clean envs in the tile             test_non_finite_context_of_one_member
                cur / next beyond two swaps, seqs[(q H + t) A + d] at H = 40, words POLICY_IT + 2 t, t > 1  test_long_roll
                mid, half, clip, noise and the rollout's own normalisation at bounds -0.5, 2.0           test_bounds_in_the_roll
    rollout     cadm_launch_rollout(horizon = 1) from obs_rows with 41275 rows: the launcher's flavours   test_two_row_tile_roll_with_noise
    icem.hip    the proposals next to TERMINATE constraints, tracking, uncertainty, actuator, knots, a
                value and a reward net and a CVaR score, on slim_humanoid and pendulum                    test_guided_everything_on
                `pseqs` / `pws` behind everything else in exactly cadm_guided_workspace_bytes bytes       test_guided_everything_on
                the policy as a seventh term; each of the six others NULL beside it                      test_policy_matters, test_each_term_off_beside_the_policy
                K + 1 + P == n_min accepted, the slots 2 .. 14 and 3 .. 15                               test_exact_fit

Two checks are not the ones the issue wrote down; neither exposed a fault, and no kernel was changed.
(1) It asked that envs 0, 31 and 64 of the 65-env batch, proposed alone, give their rows' bits "at both steps".  The one-step rollout
draws its head noise by GLOBAL row id ((mi n + ni) p + j, oracle/philox.py eps_normals): env 31 alone sits at mi = 0 and reads env 0's
noise, so only env 0 can agree at step 1 -- by the library's contract.  test_two_row_tile_roll_without_noise holds instead: env 0 alone
at both steps; envs 31 and 64 alone at step 0; envs 0 and 31 at both steps inside the first 32 envs proposed together (4064 rows: one
row tile per workgroup, the same row ids); and at step 1 the rows of envs 0, 31 and 64 against `policy_eval` (a one-tile launch, p = 1)
of `particle_mean32` of the states the big roll itself read, bit for bit -- what the issue's check was after: the two-tile kernel's
particle sum, obs path and stores against the one-tile kernel.
(2) It built the partly non-finite row from ctx_vec[2, 1, :] = NaN (+inf).  That makes none: the rollout kernel gives a particle that
read a non-finite context a NaN RETURN and keeps its trajectory finite (csrc/rollout_xdl.h, "Non-finite inputs"; measured: particles
2, 7 and 12 of env 1 read the row, 0 of them are non-finite at step 1), and the roll reads trajectories.  A non-finite weight makes none
either: `cadm_repack` refuses it (test_no_weight_makes_a_partly_non_finite_row).  The issue's inputs keep every assertion that does not
rest on that premise -- step 0 of env 1 is the clean run's, envs 0 and 2 keep their bits in `seqs` and `states`, the sequences are
finite -- in test_non_finite_context_of_one_member; and the partly non-finite row, with both of its assertions (some, not all), the
finite particle 0 and the fallback from step 1 on, is made by a model that overflows: member 2's mean-head bias +-3e38 in the dim
whose delta_std is 1.93 gives its particles (6, 7, 8 of 15) +-inf in that dim in EVERY row (test_partly_non_finite_row).  NaN cannot
be put into a particle without putting it into `obs`.

Measured on an MI355X, worst |err| / bar (every test prints its own; run with -s) -- every case passes, no kernel was changed:
    roll per kind    action err / (1e-5 of the range), noise err / bound, unclipped share over all steps:
                     pend (3, 6) 0.012, 0.012, 0.973; (1, 17) 0.019, 0.017, 0.963;  ant (3, 6) 0.019, 0.019, 0.881; (1, 17) 0.018, 0.017, 0.852;
                     slim (3, 6) 0.021, 0.021, 0.952; (1, 17) 0.022, 0.021, 0.953
    noise at A = 24  |draw - Philox| / bound 0.180; by group 0.143 0.133 0.180 0.160 0.146 0.155; every draw unclipped
    two row tiles    (65, 127): action 0.033, noise 0.029; everything else bit for bit
    long roll        H = 40, (2, 6): action 0.018, noise 0.017; the largest |state| 3.15e3 (the CPU roll of tests/test_policy_ref.py: 3.15e3)
    bounds -0.5, 2   tanh: action 0.029, noise 0.026, 34 elements on lb and 14 on ub of 324; none: 0.026, 0.024, 125 on lb, 3 on ub
    the guided loop, the seventh term, the exact fit, the non-finite rows: bit equality throughout
The whole file runs in 4 s, the slowest case (8255 rows with noise) in 0.3 s."""
import ctypes as ct
import math

import numpy as np
import pytest
import torch

import behind_rollout as br
import policy_ref as pref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd.engine import HipEngine
from helpers import _np, corner_spec, make_engine, zero_carry
from test_gpu_policy import check_roll
from test_gpu_terms_envelope import _everything, _fused, _stepwise, act_state

pytestmark = pytest.mark.gpu

F = np.float32
M, N, KE, ITERS = 2, 24, 8, 3
SEED, CALL = br.POLICY_SEED, br.POLICY_CALL
TWIN_OF = {"big": "long"}      # engines of one family share their weights, hence their H = 1 twin


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def engines(gpu):
    """name -> (problem, engine) of `behind_rollout.POLICY_ENGINES`, built when first asked for; "<name>-h1": the twin with n_forwards = 1,
    the same weights and the same bounds; 8 elites, 3 CEM iterations"""
    built, probs = {}, {}

    def get(name):
        base, _, twin = name.partition("-")
        if twin:
            base = TWIN_OF.get(base, base)
            name = base + "-h1"
        if name not in built:
            kind, D, A, E, p, H, context, bounds = br.POLICY_ENGINES[base]
            if base not in probs:
                probs[base] = br.policy_problem(base, corner_spec(kind) if base == "wide" else None)
            kw = {} if bounds is None else dict(lower_bound=bounds[0], upper_bound=bounds[1])
            eng = make_engine(probs[base], p=p, H=1 if twin else H, num_elites=KE, num_cem_iters=ITERS, **kw)
            assert (eng.D, eng.A, eng.E, eng.p, eng.C > 0) == (D, A, E, p, context)
            assert base == "wide" or eng.lib.cadm_rollout_builtin(eng._ctx), "%s: nothing may be built on demand" % base
            built[name] = (probs[base], eng)
        return built[name]
    yield get
    for n_, (_, eng) in built.items():
        assert not n_.startswith("wide") or not eng._rollout_ready, "the envelope's corner was rolled out: a module was built on demand"
        eng.close()


def _net(eng, name, P, noise, squash="tanh"):
    """registers `behind_rollout.policy_layers(name)`: (policy_params, layers, act, squash)"""
    layers, act, squash = br.policy_layers(name, squash)
    prm = HipEngine.policy_params(tuple(W.shape[1] for W, _ in layers[:-1]), act, squash, P, noise)
    eng.set_policy_net(prm, layers)
    return prm, layers, act, squash


def _loop_policy(eng, P=6, noise=0.3):
    hidden, act, squash, seed = br.POLICY_LOOP_NET
    prm = HipEngine.policy_params(hidden, act, squash, P, noise)
    eng.set_policy_net(prm, pref.he_policy(eng.D, hidden, eng.A, seed, 0.5))
    return prm


# ---------------------------------------------------------------------------------------------------------------------- 1: the roll per kind
KIND_ROLLS = [(n, m, P) for n in ("pend", "ant", "slim") for m, P in br.POLICY_ROLLS[n][1]]


@pytest.mark.parametrize("name,m,P", KIND_ROLLS, ids=["%s-m%d-P%d" % r for r in KIND_ROLLS])
def test_roll_per_kind(engines, name, m, P):
    """`check_roll` -- the action of every step against the restatement, the recovered noise against Philox, the next states bit for bit
    against the twin's one-step `rollout_returns` under POLICY_IT + 2 t -- on pendulum (A = 1: the draw is z0 of words (0, 1) of group
    0), ant (groups 0 and 1 full, p = 10) and slim_humanoid (D = 45, groups 0 .. 4, dim 16 alone in the last, p = 15); m = 3, P = 6: the
    envs share a 16-row tile; m = 1, P = 17 crosses one.  No two unclipped elements of the noisy sequences are equal: every (sequence,
    step, dim) has a draw of its own."""
    prob, eng = engines(name)
    _, twin = engines(name + "-h1")
    noise = br.POLICY_ROLLS[name][0]
    prm, layers, act, squash = _net(eng, name, P, noise)
    assert (50, 30, 70, 18) == tuple(prm.hidden)[:prm.n_hidden] and (act, squash) == ("swish", "tanh")
    seqs, states, worst_a, worst_z = check_roll(eng, twin, br.with_rows(prob, m), prm, layers, act, squash, m, SEED, CALL, noise, -1.0, 1.0)
    noisy = seqs[:, 1:]
    free = np.abs(noisy) < 1.0
    assert len(np.unique(noisy[free])) == int(free.sum()), "two draws gave the same action"
    if name == "slim":
        assert eng.A == 17 and free[..., 16].any(), "no unclipped draw of noise group 4 was checked"
    if name == "pend":
        assert eng.A == 1 and free.all(axis=-1).any()      # (`check_roll` held it to xi(..., A = 1), which is xi[..., 0] of any wider A)
    if name == "ant":
        assert free[..., 4:8].any()
    print("\n[%s m=%d P=%d] worst action err / (1e-5 of range) %.3f, worst noise err / bound %.3f, unclipped %.3f"
          % (name, m, P, worst_a, worst_z, free.mean()))


# ---------------------------------------------------------------------------------------------------------------------- 2: noise at A = 24
def test_noise_at_24_actions(engines):
    """The widest declarable env, H = 1, through `cadm_policy_propose` itself with a workspace of exactly `cadm_policy_workspace_bytes`
    bytes (`engine.policy_propose` would build a rollout module for the declaration first; at H = 1 the roll launches no rollout, and
    the C entry asks for none -- ctx_vec is never read either).  tests/test_gpu_policy.py's bias-only net: zero weights, the bias
    linspace(-0.3, 0.3, 24), squash "none", so sequence 0 is the bias bit for bit and every other element is b + noise_std * xi up to
    two roundings -- six full Philox groups against `policy_ref.xi` at test_noise_against_philox's bound."""
    prob, eng = engines("wide")
    assert eng.H == 1 and eng.A == 24 and not eng.lib.cadm_rollout_builtin(eng._ctx)
    noise, ((m, P),) = br.POLICY_ROLLS["wide"]
    prm, layers, _, _ = _net(eng, "wide", P, noise)
    b = layers[0][1]
    lib, A = eng.lib, eng.A
    obs = eng._t(np.asarray(br.with_rows(prob, m)["obs"], F))
    ctx_vec = torch.zeros((eng.E, m, eng.C), dtype=torch.float32, device=eng.device)
    need = lib.cadm_policy_workspace_bytes(eng._ctx, m, P)
    assert need > 0
    ws = torch.empty((need + 4096,), dtype=torch.uint8, device=eng.device)
    ws[need:] = 0xA5
    seqs = torch.full((m, P, 1, A), float("nan"), dtype=torch.float32, device=eng.device)
    Pt = lambda x: ct.c_void_p(x.data_ptr())
    rc = lib.cadm_policy_propose(eng._ctx, ct.byref(prm), Pt(obs), Pt(ctx_vec), m, 77, 4, Pt(seqs), None, Pt(ws), eng.stream)
    assert rc == 0, lib.cadm_last_error().decode()
    seqs = _np(seqs)
    assert (_np(ws[need:]) == 0xA5).all(), "the roll wrote behind the workspace it asked for"
    np.testing.assert_array_equal(_bits(seqs[:, 0, 0]), _bits(np.broadcast_to(b, (m, A))), err_msg="sequence 0")
    z = pref.xi(77, 4, m, P, 0, A)[:, 1:]
    a = seqs[:, 1:, 0]
    free = np.abs(a) < 1.0
    assert free.mean() > 0.98 and (np.abs(b + F(noise) * z)[~free] >= 1.0 - 1e-5).all()
    rec = (a.astype(np.float64) - b.astype(np.float64)) / float(F(noise))
    bound = 4e-6 * np.maximum(1.0, pref.xi_radius(77, 4, m, P, 0, A)[:, 1:] / 2.0) + 2.0 ** -23 / noise
    ratio = np.abs(rec - z) / bound
    assert (ratio[free] <= 1.0).all(), "worst %.3f of the bound" % ratio[free].max()
    for g in range(6):
        assert free[..., 4 * g:4 * g + 4].mean() > 0.9, "group %d is hardly checked" % g
    assert len(np.unique(a[free])) == int(free.sum())
    print("\n[noise at A = 24, m=%d P=%d] worst |draw - Philox| / bound %.3f, by group %s, unclipped %.4f"
          % (m, P, ratio[free].max(), " ".join("%.3f" % np.where(free, ratio, 0.0)[..., 4 * g:4 * g + 4].max() for g in range(6)), free.mean()))


# ---------------------------------------------------------------------------------------------------------------------- 3: two row tiles
BIG_M, BIG_P = br.POLICY_ROLLS["big"][1][0]


def _big(engines):
    prob, eng = engines("big")
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    total = BIG_M * BIG_P
    assert total == 8255 and total > 2 * 16 * 256 and (total + 15) // 16 > 2 * cus, "%d rows on %d CUs: one row tile per workgroup" % (total, cus)
    assert (32 * BIG_P + 15) // 16 <= 2 * cus, "32 envs must still take one row tile per workgroup"
    return br.with_rows(prob, BIG_M), eng


def test_two_row_tile_roll_without_noise(engines):
    """Engine big, m = 65, P = 127: 8255 rows are more than two 16-row tiles per CU, the roll's steps run `policy_step_kernel<2>` --
    from `obs` at step 0, over p = 5 particles at step 1.  noise_std = 0.  Every sequence of an env equals its sequence 0 at step 0.
    Env 0 proposed alone has its rows' bits at both steps; envs 31 and 64 alone at step 0 (alone they sit at mi = 0 and their one-step
    rollout reads env 0's head noise: see the module docstring); envs 0 and 31 at both steps inside the first 32 envs proposed together
    (4064 rows: one row tile); and step 1 of envs 0, 31 and 64 is `policy_eval` -- one row tile, p = 1 -- of `particle_mean32` of the
    states the big roll read, bit for bit."""
    prob, eng = _big(engines)
    hidden, act, squash, _ = br.POLICY_BIG_NET
    prm, layers, _, _ = _net(eng, "big", BIG_P, 0.0)
    obs = np.asarray(prob["obs"], F)
    seqs, states = (_np(x) for x in eng.policy_propose(prm, obs, None, seed=SEED, call=CALL, want_states=True))
    assert seqs.shape == (BIG_M, BIG_P, 2, eng.A) and np.isfinite(seqs).all() and np.isfinite(states).all()
    np.testing.assert_array_equal(_bits(seqs[:, :, 0]), _bits(np.repeat(seqs[:, :1, 0], BIG_P, axis=1)), err_msg="step 0: every sequence is sequence 0")
    assert not np.array_equal(seqs[:, 1, 1], seqs[:, 0, 1]), "step 1: the sequences' particles differ by their head noise"
    assert len({seqs[e, 0, 0].tobytes() for e in range(BIG_M)}) == BIG_M
    for e in (0, 31, 64):
        alone = _np(eng.policy_propose(prm, obs[e:e + 1], None, seed=SEED, call=CALL))
        np.testing.assert_array_equal(_bits(alone[0, :, 0]), _bits(seqs[e, :, 0]), err_msg="env %d alone, step 0" % e)
        if e == 0:
            np.testing.assert_array_equal(_bits(alone[0]), _bits(seqs[0]), err_msg="env 0 alone, both steps")
        est = pref.particle_mean32(states[1][e])
        np.testing.assert_array_equal(_bits(_np(eng.policy_eval(est))), _bits(seqs[e, :, 1]), err_msg="env %d, step 1 against policy_eval" % e)
    part = _np(eng.policy_propose(prm, obs[:32], None, seed=SEED, call=CALL))
    for e in (0, 31):
        np.testing.assert_array_equal(_bits(part[e]), _bits(seqs[e]), err_msg="env %d inside a one-tile launch of 32 envs, both steps" % e)


def test_two_row_tile_roll_with_noise(engines):
    """The same 8255 rows with noise_std = 0.3 and states_out, through `check_roll`: the actions of both steps against the restatement,
    the q % P noise gate and the draws against Philox, states[0] is `obs` broadcast, states[1] is the twin's one-step `rollout_returns`
    on all 8255 x 5 rows bit for bit (41275 rows from obs_rows at horizon 1: the launcher mixes its flavours), the same bits run to run,
    with and without states_out; and env 0 proposed alone has the big batch's env-0 bits at both steps."""
    prob, eng = _big(engines)
    _, twin = engines("big-h1")
    noise = br.POLICY_ROLLS["big"][0]
    prm, layers, act, squash = _net(eng, "big", BIG_P, noise)
    seqs, states, worst_a, worst_z = check_roll(eng, twin, prob, prm, layers, act, squash, BIG_M, SEED, CALL, noise, -1.0, 1.0)
    alone, st = (_np(x) for x in eng.policy_propose(prm, np.asarray(prob["obs"], F)[:1], None, seed=SEED, call=CALL, want_states=True))
    np.testing.assert_array_equal(_bits(alone[0]), _bits(seqs[0]), err_msg="env 0 alone, both steps")
    np.testing.assert_array_equal(_bits(st[:, 0]), _bits(states[:, 0]))
    np.testing.assert_array_equal(_bits(seqs[:, 0, 0]), _bits(_np(eng.policy_eval(np.asarray(prob["obs"], F)))), err_msg="sequence 0 has no noise")
    print("\n[two row tiles, m=%d P=%d] worst action err / (1e-5 of range) %.3f, worst noise err / bound %.3f" % (BIG_M, BIG_P, worst_a, worst_z))


# ---------------------------------------------------------------------------------------------------------------------- 4: partly non-finite
POISON = [float("nan"), math.inf]


@pytest.mark.parametrize("poison", POISON, ids=["nan", "inf"])
def test_non_finite_context_of_one_member(engines, poison):
    """slim_humanoid, m = 3, P = 6: member 2's context of env 1 is non-finite.  Step 0 of env 1 (it reads `obs`) is the clean run's bit
    for bit, the sequences stay finite, and envs 0 and 2 -- rows of the same tile, particles of the same rollout workgroups -- keep
    their bits in `seqs` and `states` at every step.  The rollout kernel gives such particles a NaN RETURN and keeps their trajectory
    finite (csrc/rollout_xdl.h, "Non-finite inputs"), so the roll, which reads trajectories, sees no non-finite particle here and takes
    no fallback: the module docstring says what that means for the issue's check."""
    prob, eng = engines("slim")
    prob = br.with_rows(prob, 3)
    prm = HipEngine.policy_params((5, 7), "relu", "tanh", 6, 0.3)
    eng.set_policy_net(prm, pref.envelope_policy(eng.D, (5, 7), eng.A))
    obs = np.asarray(prob["obs"], F)
    ctx_vec = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    assert tuple(ctx_vec.shape) == (eng.E, 3, eng.C)
    clean, cs = (_np(x) for x in eng.policy_propose(prm, obs, ctx_vec, seed=2, call=3, want_states=True))
    assert np.isfinite(cs).all()
    bad = ctx_vec.clone()
    bad[2, 1, :] = poison
    seqs, st = (_np(x) for x in eng.policy_propose(prm, obs, bad, seed=2, call=3, want_states=True))
    assert np.isfinite(seqs).all()
    np.testing.assert_array_equal(_bits(seqs[1, :, 0]), _bits(clean[1, :, 0]), err_msg="step 0 of the poisoned env reads obs")
    np.testing.assert_array_equal(_bits(st[0]), _bits(cs[0]))
    for e in (0, 2):
        np.testing.assert_array_equal(_bits(seqs[e]), _bits(clean[e]), err_msg="env %d met its neighbour's poison" % e)
        np.testing.assert_array_equal(_bits(st[:, e]), _bits(cs[:, e]))
    moved = (st[1][1] != cs[1][1]).any(axis=-1)                    # [P, p]: the particles that read the poisoned context
    assert moved.any(axis=1).all() and (~moved).any(axis=1).all() and not moved[:, 0].any()
    nf = ~np.isfinite(st[1][1]).all(axis=-1)
    print("\n[non-finite context, %r] particles of env 1 that read it: %s of %d; non-finite among them at step 1: %d"
          % (poison, sorted(set(np.nonzero(moved)[1].tolist())), eng.p, int(nf.sum())))


def test_no_weight_makes_a_partly_non_finite_row(engines):
    """The other way to a row whose particles are partly non-finite -- one member's weights -- is closed before any kernel runs: the
    library refuses a non-finite dynamics weight or bias when it packs them.  With the test above: through the entry points a particle
    state is non-finite behind a non-finite `obs`, which every particle of the row reads (tests/test_gpu_policy.py's
    test_non_finite_start_state_of_one_env), or where the model itself overflows: the next test."""
    prob, eng = engines("slim")
    for poison in POISON:
        ff = type(prob["ff"])(prob["ff"])
        ff["output_mu_bias"] = prob["ff"]["output_mu_bias"].copy()
        ff["output_mu_bias"][2, 0, 0] = poison
        with pytest.raises(_lib.CadmError, match="non-finite"):
            make_engine(dict(prob, ff=ff), p=eng.p, num_elites=KE, num_cem_iters=ITERS)


@pytest.mark.parametrize("sign", [1.0, -1.0], ids=["plus-inf", "minus-inf"])
def test_partly_non_finite_row(engines, sign):
    """What does make one: a second slim_humanoid engine whose member 2 has the finite bias +-3e38 in its mean head, in the dim with the
    largest delta_std (> 1.14), so that the denormalised delta of member 2's particles overflows to +-inf.  After the first one-step
    rollout SOME particles of every row -- member 2's -- are non-finite and the others are not, particle 0 among the finite ones: the
    flag comes from the `nf = nf || mlp_nonfinite(v)` chain over j >= 1.  Step 0 (it reads `obs`) is the clean engine's bit for bit,
    the finite particles of step 1 have the clean engine's bits, and from step 1 on every action is the fallback, finite."""
    prob, clean_eng = engines("slim")
    prob = br.with_rows(prob, 3)
    dstd = np.asarray(prob["stats"]["delta_std"], F)
    d = int(dstd.argmax())
    assert float(dstd[d]) * 3.0e38 > 1.05 * float(np.finfo(F).max)
    ff = type(prob["ff"])(prob["ff"])
    ff["output_mu_bias"] = prob["ff"]["output_mu_bias"].copy()
    ff["output_mu_bias"][2, 0, d] = sign * 3.0e38
    eng = make_engine(dict(prob, ff=ff), p=clean_eng.p, num_elites=KE, num_cem_iters=ITERS)
    assert eng.lib.cadm_rollout_builtin(eng._ctx) and eng.H == 3
    prm = HipEngine.policy_params((5, 7), "relu", "tanh", 6, 0.3)
    for e_ in (eng, clean_eng):
        e_.set_policy_net(prm, pref.envelope_policy(eng.D, (5, 7), eng.A))
    obs = np.asarray(prob["obs"], F)
    clean, cs = (_np(x) for x in clean_eng.policy_propose(prm, obs, clean_eng.context_forward(prob["cp_obs"], prob["cp_act"]), seed=2, call=3,
                                                          want_states=True))
    seqs, st = (_np(x) for x in eng.policy_propose(prm, obs, eng.context_forward(prob["cp_obs"], prob["cp_act"]), seed=2, call=3, want_states=True))
    eng.close()
    assert np.isfinite(seqs).all() and np.isfinite(cs).all()
    np.testing.assert_array_equal(_bits(seqs[:, :, 0]), _bits(clean[:, :, 0]), err_msg="step 0 reads obs")
    np.testing.assert_array_equal(_bits(st[0]), _bits(cs[0]))
    nf = ~np.isfinite(st[1]).all(axis=-1)                          # [m, P, p]
    assert nf.any(axis=-1).all() and (~nf).any(axis=-1).all(), "every row must be partly non-finite:\n%r" % nf
    assert not nf[..., 0].any(), "particle 0 must stay finite: the flag has to come from a particle j >= 1"
    assert (st[1][nf][:, d] == sign * np.inf).all()
    np.testing.assert_array_equal(_bits(st[1][~nf]), _bits(cs[1][~nf]), err_msg="the other members' particles")
    fb = pref.fallback(-1.0, 1.0)
    assert (seqs[:, :, 1:] == fb).all() and (clean[:, :, 1:] != fb).all(axis=-1).any()
    print("\n[partly non-finite, dim %d = %+.0e * %.3f] non-finite particles of every row at step 1: %s of %d"
          % (d, sign * 3.0e38, dstd[d], sorted(set(np.nonzero(nf)[2].tolist())), eng.p))


# ---------------------------------------------------------------------------------------------------------------------- 5: the long roll
def test_long_roll(engines):
    """H = 40, m = 2, P = 6, noise 0.2: `check_roll` at every one of the 40 steps -- 39 swaps of `cur` / `next`, the stride
    seqs[(q H + t) A + d] at H = 40, the iteration words POLICY_IT + 2 t up to t = 38.  tests/test_policy_ref.py rolls the same policy
    through the oracle model on the CPU: the states stay finite and below 1e4."""
    prob, eng = engines("long")
    _, twin = engines("long-h1")
    noise, ((m, P),) = br.POLICY_ROLLS["long"]
    assert eng.H == 40 and hplanner.POLICY_IT + 2 * (eng.H - 2) < hplanner.FORECAST_IT
    prm, layers, act, squash = _net(eng, "long", P, noise)
    seqs, states, worst_a, worst_z = check_roll(eng, twin, prob, prm, layers, act, squash, m, SEED, CALL, noise, -1.0, 1.0)
    assert np.isfinite(states).all() and not np.array_equal(seqs[:, :, 38], seqs[:, :, 39])
    assert len({seqs[:, :, t].tobytes() for t in range(eng.H)}) == eng.H, "two steps wrote the same actions"
    print("\n[long roll H=40 m=%d P=%d] worst action err / (1e-5 of range) %.3f, worst noise err / bound %.3f, largest |state| %.3g"
          % (m, P, worst_a, worst_z, np.abs(states).max()))


# ---------------------------------------------------------------------------------------------------------------------- 6: bounds in the roll
@pytest.mark.parametrize("squash", pref.SQUASH)
def test_bounds_in_the_roll(engines, squash):
    """Engine bnd (lower_bound -0.5, upper_bound 2.0), m = 3, P = 6, noise 0.5, (37,) * 4 tanh with either squash: `check_roll` with
    these bounds -- mid + half * tanh, the noise, the clip; the twin's rollout, which normalises the clipped action the GPU wrote, gives
    the next states bit for bit.  The actions lie inside the bounds; without the squash some sit exactly on each."""
    prob, eng = engines("bnd")
    _, twin = engines("bnd-h1")
    lb, ub = br.POLICY_ENGINES["bnd"][7]
    assert (float(eng.cfg.lower_bound), float(eng.cfg.upper_bound)) == (lb, ub) == (float(twin.cfg.lower_bound), float(twin.cfg.upper_bound))
    noise, ((m, P),) = br.POLICY_ROLLS["bnd"]
    prm, layers, act, squash = _net(eng, "bnd", P, noise, squash)
    seqs, _, worst_a, worst_z = check_roll(eng, twin, br.with_rows(prob, m), prm, layers, act, squash, m, SEED, CALL, noise, lb, ub)
    assert seqs.min() >= F(lb) and seqs.max() <= F(ub) and seqs.max() > 1.0
    if squash == "none":
        assert (seqs == F(ub)).any() and (seqs == F(lb)).any()
    print("\n[bounds %s] worst action err / (1e-5 of range) %.3f, worst noise err / bound %.3f; on lb %d, on ub %d of %d"
          % (squash, worst_a, worst_z, (seqs == F(lb)).sum(), (seqs == F(ub)).sum(), seqs.size))


# ---------------------------------------------------------------------------------------------------------------------- 7: the guided loop
def _c_guided(eng, e, pol, mppi, obs3, mean, var, carry, valid, state, call, ws):
    """`cadm_guided_plan` itself with every term of `e`: (plan, best return)"""
    lib = eng.lib
    _, full = eng._as_mppi_params(e["prm"])
    targets, T, offset = eng._targets(e["targets"], e["offset"], M, 3, "test")
    t = [eng._t(x) for x in obs3] + [eng._t(mean), eng._t(var)]
    out = torch.empty((M, eng.H, eng.A), dtype=torch.float32, device=eng.device)
    best = torch.empty((M,), dtype=torch.float32, device=eng.device)
    P = lambda x: ct.c_void_p(x.data_ptr())
    rc = lib.cadm_guided_plan(eng._ctx, None if pol is None else ct.byref(pol), ct.byref(e["reward"]), ct.byref(e["value"]), ct.byref(e["unc"]),
                              ct.byref(e["act"]), P(state[0]), P(state[1]), 1, ct.byref(e["track"]), P(targets), T, P(offset), ct.byref(e["knots"]),
                              P(e["phase"]), ct.byref(e["cons"]), ct.byref(e["score"]), int(mppi), ct.byref(full), *[P(x) for x in t], P(carry),
                              P(valid), M, N, 4, call, P(ws), P(out), P(best), eng.stream)
    assert rc == 0, lib.cadm_last_error().decode()
    return out, best


def _exact_ws(eng, nbytes):
    ws = torch.empty((nbytes + 4096,), dtype=torch.uint8, device=eng.device)
    ws[nbytes:] = 0xA5
    assert nbytes > 0 and ws.data_ptr() % 256 == 0
    return ws


LOOP = [(e, u) for e in ("slim", "pend") for u in ("mppi", "cem")]


@pytest.mark.parametrize("name,update", LOOP, ids=["%s-%s" % c for c in LOOP])
def test_guided_everything_on(engines, name, update):
    """tests/test_gpu_terms_envelope.py's `_everything` -- TERMINATE constraints, three tracking terms, a reward and a value net, an
    uncertainty term, an actuator, knots, a CVaR score, two kept elites, decay 1.25, the mean added last -- plus a policy (50, 30) tanh /
    tanh with P = 6 proposals and noise 0.3, on slim_humanoid and pendulum, under the MPPI update and the elite refit.
    `cadm_guided_plan` == the stepwise loop (`icem_plan(..., policy=...)`) bit for bit over two calls: the plan, the best return, the
    carry, the actuator's prev and prefix, and the proposals against a stand-alone `policy_propose`.  Then the C entry on call 2's inputs
    in a workspace of exactly `cadm_guided_workspace_bytes` bytes with 4 KiB of a bit pattern behind it: call 2's bits, the pattern
    intact -- `pseqs` and the roll's workspace are the last views carved."""
    prob, eng = engines(name)
    H, A, mppi, P = eng.H, eng.A, update == "mppi", 6
    e = _everything(eng, prob, name, mppi)
    pol = _loop_policy(eng, P)
    obs3 = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    ca, cb = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    sa, sb = act_state(eng, 1, 8), act_state(eng, 1, 8)
    mean, var = prob["init_mean"], prob["init_var"]
    ctx_vec = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    for call in (1, 2):
        kept = [t.clone() for t in (*ca, *sa)] + [eng._t(mean).clone()]
        a, ra = _fused(eng, e, (*obs3, mean, var), sa, ca, call, policy=pol, want_best_return=True)
        b, info, extra = _stepwise(eng, e, (*obs3, mean, var), sb, cb, call, mppi, policy=pol, return_info=True)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max()
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        for x, y, what in ((ca[0], cb[0], "carry"), (sa[0], sb[0], "prev"), (sa[1], sb[1], "prefix")):
            np.testing.assert_array_equal(_bits(_np(x)), _bits(_np(y)), err_msg="%s after call %d" % (what, call))
        props = _np(extra["proposals"])
        assert props.shape == (M, P, H, A) and np.isfinite(props).all()
        np.testing.assert_array_equal(_bits(props), _bits(_np(eng.policy_propose(pol, prob["obs"], ctx_vec, seed=4, call=call))))
        assert len({int(x["rows"].shape[1]) for x in info}) > 1, "decay must change the packed candidate count"
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    assert (mppi, "pol", True, True, True, P) in eng._loop_ws
    nbytes = eng.lib.cadm_guided_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, 1, 1, P)
    under = eng.lib.cadm_rewarded_workspace_bytes(eng._ctx, M, N, 2, int(mppi), 1, 1, 1)
    assert nbytes > under > 0
    ws = _exact_ws(eng, nbytes)
    carry2, valid2, prev2, prefix2, mean2 = kept
    out, best = _c_guided(eng, e, pol, mppi, obs3, mean2, var, carry2, valid2, (prev2, prefix2), 2, ws)
    np.testing.assert_array_equal(_bits(_np(out)), _bits(a), err_msg="the C entry in an exact workspace")
    np.testing.assert_array_equal(_bits(_np(best)), _bits(_np(ra)))
    np.testing.assert_array_equal(_bits(_np(carry2)), _bits(_np(ca[0])))
    np.testing.assert_array_equal(_bits(_np(prev2)), _bits(_np(sa[0])))
    assert (_np(ws[nbytes:]) == 0xA5).all(), "the guided loop wrote behind the workspace it asked for"


# ---------------------------------------------------------------------------------------------------------------------- 8: a seventh term
@pytest.mark.parametrize("name", ["slim", "pend"])
def test_policy_matters(engines, name):
    """Everything on under MPPI: without the policy the plan is another one -- and that plan is `cadm_rewarded_plan`'s (`_fused`) bit
    for bit, from `cadm_guided_plan` itself with policy = NULL in the rewarded loop's workspace (what
    `cadm_guided_workspace_bytes(.., P = 0)` asks for)."""
    prob, eng = engines(name)
    H = eng.H
    e = _everything(eng, prob, name, True)
    pol = _loop_policy(eng)
    obs3 = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    args = (*obs3, prob["init_mean"], prob["init_var"])
    guided = _np(_fused(eng, e, args, act_state(eng, 1, 8), zero_carry(eng, M, 2, H), 1, policy=pol))
    ca = zero_carry(eng, M, 2, H)
    plain, rp = _fused(eng, e, args, act_state(eng, 1, 8), ca, 1, want_best_return=True)
    plain = _np(plain)
    assert np.isfinite(guided).all() and np.isfinite(plain).all()
    assert not np.array_equal(_bits(guided), _bits(plain)), "the proposals do not change the plan"
    nbytes = eng.lib.cadm_guided_workspace_bytes(eng._ctx, M, N, 2, 1, 1, 1, 1, 0)
    assert nbytes == eng.lib.cadm_rewarded_workspace_bytes(eng._ctx, M, N, 2, 1, 1, 1, 1)
    ws = _exact_ws(eng, nbytes)
    cc = zero_carry(eng, M, 2, H)
    out, best = _c_guided(eng, e, None, True, obs3, prob["init_mean"], prob["init_var"], cc[0], cc[1], act_state(eng, 1, 8), 1, ws)
    np.testing.assert_array_equal(_bits(_np(out)), _bits(plain), err_msg="cadm_guided_plan(policy = NULL) against cadm_rewarded_plan")
    np.testing.assert_array_equal(_bits(_np(best)), _bits(_np(rp)))
    np.testing.assert_array_equal(_bits(_np(cc[0])), _bits(_np(ca[0])))
    assert (_np(ws[nbytes:]) == 0xA5).all()


TERMS = ["reward", "value", "unc", "act", "track", "knots"]


@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("name", ["slim", "pend"])
def test_each_term_off_beside_the_policy(engines, name, term):
    """Everything on under MPPI with the policy, then one of the six other terms NULL: `cadm_guided_plan` == the stepwise loop without
    that term, bit for bit -- the plan, the best return, the carry, the actuator state: the proposals' slots and the workspace views
    behind a term that is absent."""
    prob, eng = engines(name)
    H = eng.H
    e = _everything(eng, prob, name, True)
    pol = _loop_policy(eng)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"], prob["init_mean"], prob["init_var"])
    ca, cb = zero_carry(eng, M, 2, H), zero_carry(eng, M, 2, H)
    sa, sb = act_state(eng, 1, 8), act_state(eng, 1, 8)
    a, ra = _fused(eng, e, args, sa, ca, 1, off=(term,), policy=pol, want_best_return=True)
    b, _, extra = _stepwise(eng, e, args, sb, cb, 1, True, off=(term,), policy=pol, return_info=True)
    a = _np(a)
    assert np.isfinite(a).all() and 0 < np.abs(a).max()
    np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="without %s: the plan" % term)
    np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])))
    np.testing.assert_array_equal(_bits(_np(ca[0])), _bits(_np(cb[0])))
    if term != "act":
        np.testing.assert_array_equal(_bits(_np(sa[0])), _bits(_np(sb[0])))
        np.testing.assert_array_equal(_bits(_np(sa[1])), _bits(_np(sb[1])))


# ---------------------------------------------------------------------------------------------------------------------- 9: the exact fit
@pytest.mark.parametrize("update", ["cem", "mppi"])
def test_exact_fit(engines, update):
    """24 candidates, 8 elites, 3 iterations, decay 2: the iterations have 24, 16 and 16 candidates.  Two kept elites, the mean added
    last and P = 13 proposals fill the last iteration exactly: K + 1 + P = 16 is accepted, `cadm_guided_plan` == the stepwise loop bit
    for bit over two calls, and the stepwise iterations' candidates hold the proposals in slots 2 .. 14 and, in the last, 3 .. 15 --
    behind the mean candidate in slot 2.  One proposal more is refused."""
    prob, eng = engines("fit")
    H, A, K, P, mppi = eng.H, eng.A, 2, 13, update == "mppi"
    assert (eng.num_elites, eng.num_cem_iters) == (KE, ITERS) and hplanner.policy_min_candidates(N, 2.0, KE, K, ITERS) == 16 == K + 1 + P
    pol = _loop_policy(eng, P)
    icem = dict(noise_beta=0.0, keep_elites=K, decay=2.0, return_best=False, add_mean_last=True)
    prm = HipEngine.mppi_params(temperature=0.5, relative=True, **icem) if mppi else HipEngine.icem_params(**icem)
    args = (prob["obs"], prob["cp_obs"], prob["cp_act"])
    none14 = (None, None, None, None, None, None, True, None, None, None, None, None, None, None)
    (ca, va), (cb, vb) = zero_carry(eng, M, K, H), zero_carry(eng, M, K, H)
    mean, var = prob["init_mean"], prob["init_var"]
    for call in (1, 2):
        a, ra = eng.guided_plan(pol, *none14, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=call, want_best_return=True)
        b, info, extra = hplanner.icem_plan(eng, *args, mean, var, N, carry=cb, carry_valid=vb, seed=4, call=call, return_info=True,
                                            update=update, temperature=0.5, relative=True, policy=pol, **icem)
        a = _np(a)
        assert a.shape == (M, H, A) and np.isfinite(a).all() and 0 < np.abs(a).max() <= 1.0
        np.testing.assert_array_equal(_bits(a), _bits(_np(b)), err_msg="plan of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ra)), _bits(_np(extra["best_ret"])), err_msg="best return of call %d" % call)
        np.testing.assert_array_equal(_bits(_np(ca)), _bits(_np(cb)))
        props = _np(extra["proposals"])
        assert props.shape == (M, P, H, A) and [int(x["actions"].shape[1]) for x in info] == [24, 16, 16]
        for it, x in enumerate(info):
            s = 3 if it + 1 == ITERS else 2
            assert s == hplanner.policy_slot(K, it + 1 == ITERS, True)
            np.testing.assert_array_equal(_bits(_np(x["actions"])[:, s:s + P]), _bits(props), err_msg="iteration %d" % it)
        last = _np(info[-1]["actions"])
        assert last.shape[1] == 3 + P, "the last iteration has no drawn candidate left"
        np.testing.assert_array_equal(_bits(last[:, 2]), _bits(np.clip(_np(info[-2]["mean"]), -1.0, 1.0)), err_msg="slot 2: the mean candidate")
        mean = np.concatenate([a[:, 1:], np.zeros((M, 1, A), F)], axis=1)
    one_more = HipEngine.policy_params(*br.POLICY_LOOP_NET[:3], P + 1, 0.3)
    with pytest.raises(_lib.CadmError, match="do not fit the 16"):
        eng.guided_plan(one_more, *none14, prm, *args, mean, var, N, carry=ca, carry_valid=va, seed=4, call=3)
