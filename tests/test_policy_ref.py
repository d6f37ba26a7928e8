"""CPU: the policy prior of the opt-in planner -- the float32 emulation of the kernel's chain against the float64 restatement
(tests/policy_ref.py), the noise, the fallback, the slot arithmetic, the struct and the signatures against the header, the options and
the host-side refusals; and, for the geometries of tests/test_gpu_policy_envelope.py (behind_rollout.py POLICY_ENGINES), that the
restatement alone meets what those tests ask of their inputs: the nets hold the bar and are live, more than half of the draws stay
unclipped, the 40-step roll stays finite.  The kernels themselves: tests/test_gpu_policy.py and tests/test_gpu_policy_envelope.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import behind_rollout as br
import policy_ref as pref
import value_ref as vref
from cadm_amd import _lib
from cadm_amd import planner as hplanner
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions
from helpers import assert_close, corner_spec, floored_rel, oracle_problem
from oracle import philox
from oracle import planner as oplanner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# (D, A) of the engines tests/test_gpu_policy.py evaluates on: pendulum, hopper_like, halfcheetah, the widest declarable env
SHAPES = [(3, 1), (11, 3), (18, 6), (48, 24)]
NETS = [()] + vref.ENVELOPE_NETS


def states_for(D, rows=37, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return rng.standard_normal((rows, D)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("act", pref.ACTS)
@pytest.mark.parametrize("squash", pref.SQUASH)
def test_float32_chain_against_float64(act, squash):
    """The kernel's chain in float32 stays within 1e-5 of the action range of the float64 restatement for every net of
    value_ref.ENVELOPE_NETS widened to A outputs, and the linear policy, on every (D, A) the GPU test uses; the nets meet the GPU test's
    liveness condition: a live hidden layer, outputs that differ between rows, and a tanh squash that is not saturated."""
    worst = 0.0
    for D, A in SHAPES:
        x = states_for(D)
        for hidden in NETS:
            layers = pref.envelope_policy(D, hidden, A)
            share, spread, open_ = pref.liveness(x, layers, act)
            assert share >= 0.5 and spread > 1e-3 and open_ >= 0.5, "D=%d A=%d %r %s: %.2f %.2e %.2f" % (D, A, hidden, act, share, spread, open_)
            ref = pref.action64(x, layers, act, squash, -1.0, 1.0)
            emu = pref.emulate32(x, layers, act, squash, -1.0, 1.0)
            assert emu.dtype == F and emu.shape == (37, A) and np.isfinite(ref).all()
            # the bar is 1e-5 of the action RANGE: ub - lb = 2 is the scale of every element
            assert np.abs(emu.astype(np.float64) - ref).max() <= 1e-5 * 2.0, (D, A, hidden)
            assert_close(emu, ref, what="D=%d A=%d %r %s %s" % (D, A, hidden, act, squash))
            worst = max(worst, floored_rel(emu, ref))
            assert np.abs(emu).max() <= 1.0
    print("\n[%s %s] float32 chain against float64: %.2e of scale" % (act, squash, worst))


def test_statistics_and_bounds():
    """obs_mean / obs_std and bounds that are not -1 / 1: (x - mean) * float32(1 / std), mid and half from the float32 bounds."""
    D, A = 18, 6
    rng = np.random.default_rng(2)
    x = states_for(D, seed=2)
    mean, std = rng.standard_normal(D).astype(F), rng.uniform(0.3, 4.0, D).astype(F)
    layers = pref.envelope_policy(D, (50, 30, 70, 18), A)
    ref = pref.action64(x, layers, "swish", "tanh", -0.5, 2.0, mean, std)
    emu = pref.emulate32(x, layers, "swish", "tanh", -0.5, 2.0, mean, std)
    assert np.abs(emu - ref).max() <= 1e-5 * 2.5
    assert emu.min() >= F(-0.5) and emu.max() <= F(2.0)
    assert np.abs(ref - pref.action64(x, layers, "swish", "tanh", -0.5, 2.0)).max() > 1e-3, "the statistics must matter"
    # no squash: the clip alone keeps the action inside the bounds
    raw = pref.emulate32(x, pref.he_policy(D, (16,), A, 1, out_scale=3.0), "relu", "none", -1.0, 1.0)
    assert (raw == 1.0).any() and (raw == -1.0).any() and (np.abs(raw) < 1.0).any()


def test_particle_mean_is_sequential():
    """The state estimate sums the particles in ascending order from particle 0 and divides once: an order a pairwise sum does not
    reproduce on values of mixed magnitude; p = 1 is the value itself."""
    x = np.array([[1.0e8], [1.0], [-1.0e8], [1.0]], F).reshape(1, 4, 1)
    got = pref.particle_mean32(x)
    assert got.dtype == F and got[0, 0] == F(F(F(F(1.0e8) + F(1.0)) + F(-1.0e8)) + F(1.0)) / F(4)
    assert got[0, 0] != F(np.float64(x.astype(np.float64).sum()) / 4)
    one = np.random.default_rng(0).standard_normal((5, 1, 7)).astype(F)
    np.testing.assert_array_equal(pref.particle_mean32(one).view(np.uint32), one[:, 0].view(np.uint32))
    rng = np.random.default_rng(1)
    many = rng.standard_normal((3, 20, 11)).astype(F)
    assert np.abs(pref.particle_mean32(many) - many.astype(np.float64).mean(axis=1)).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------- the noise
def test_noise_moments_and_counters():
    """xi is standard normal (mean, variance, fourth moment over 10^5 draws), differs between sequences, steps, dims, seeds and calls,
    and an action dim's draw does not depend on A, m or P beyond the row id mi * P + j."""
    z = pref.xi(3, 7, 8, 512, 0, 24).astype(np.float64)
    n = z.size
    assert abs(z.mean()) < 4.0 / np.sqrt(n) and abs(z.var() - 1.0) < 4.0 * np.sqrt(2.0 / n) and abs((z ** 4).mean() - 3.0) < 4.0 * np.sqrt(96.0 / n)
    assert abs(np.corrcoef(z[..., 0].ravel(), z[..., 1].ravel())[0, 1]) < 4.0 / np.sqrt(8 * 512)
    assert abs(np.corrcoef(z[..., 1].ravel(), z[..., 2].ravel())[0, 1]) < 4.0 / np.sqrt(8 * 512)
    a = pref.xi(3, 7, 2, 6, 1, 6)
    for other in (pref.xi(4, 7, 2, 6, 1, 6), pref.xi(3, 8, 2, 6, 1, 6), pref.xi(3, 7, 2, 6, 2, 6)):
        assert not np.array_equal(a, other)
    assert len(np.unique(a)) == a.size
    np.testing.assert_array_equal(pref.xi(3, 7, 2, 6, 1, 3), a[..., :3])                                  # fewer dims: the same draws
    np.testing.assert_array_equal(pref.xi(3, 7, 1, 12, 1, 6).reshape(2, 6, 6), a)                         # the row id is mi * P + j
    np.testing.assert_array_equal(pref.xi(3, 7, 4, 6, 1, 6)[:2], a)


def test_sequence_zero_stays_noiseless_and_the_fallback():
    """With noise, sequence 0 of every env has the bits it has without; the others move by noise_std * xi, one multiply and one add,
    before the clip.  A state with a non-finite value takes clip(0, lb, ub) in every dim, in both statements, whatever the bounds."""
    D, A, m, P = 11, 3, 3, 6
    layers = pref.envelope_policy(D, (5, 7), A)
    x = states_for(D, rows=m * P, seed=5).reshape(m, P, D)
    clean, raw = pref.emulate32(x, layers, "tanh", "tanh", -1.0, 1.0, want_raw=True)
    z = pref.xi(1, 2, m, P, 0, A)
    z[:, 0] = 0.0
    noisy = pref.emulate32(x, layers, "tanh", "tanh", -1.0, 1.0, xi=z, noise_std=0.3)
    np.testing.assert_array_equal(noisy[:, 0].view(np.uint32), clean[:, 0].view(np.uint32))
    want = np.minimum(np.maximum(raw + F(0.3) * z, F(-1)), F(1))
    np.testing.assert_array_equal(noisy[:, 1:].view(np.uint32), want[:, 1:].view(np.uint32))
    assert (noisy[:, 1:] != clean[:, 1:]).mean() > 0.9
    np.testing.assert_array_equal(pref.emulate32(x, layers, "tanh", "tanh", -1.0, 1.0, xi=z, noise_std=0.0).view(np.uint32), clean.view(np.uint32))
    bad = x.copy()
    bad[0, 1, 3], bad[1, 0, 0], bad[2, 5, 10] = np.nan, np.inf, -np.inf
    hit = np.zeros((m, P), bool)
    hit[0, 1] = hit[1, 0] = hit[2, 5] = True
    for lb, ub, fb in ((-1.0, 1.0, 0.0), (0.25, 2.0, 0.25), (-3.0, -0.5, -0.5)):
        assert pref.fallback(lb, ub) == F(fb)
        for fn in (pref.action64, pref.emulate32):
            a = fn(bad, layers, "tanh", "tanh", lb, ub)
            assert (a[hit] == fb).all() and np.isfinite(a).all()
        keep = pref.emulate32(x, layers, "tanh", "tanh", lb, ub)
        np.testing.assert_array_equal(pref.emulate32(bad, layers, "tanh", "tanh", lb, ub)[~hit].view(np.uint32), keep[~hit].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------- the slots
def test_slot_arithmetic_against_the_candidate_rule():
    """The proposals sit behind the kept elites and, in the last iteration with add_mean_last, the mean candidate; K + 1 + P must fit the
    smallest iteration's candidate count min(n, max(floor(n / decay^it), 2 num_elites, K + 1)) -- `planner.policy_min_candidates`
    against the engine's own statement of the rule and tests/policy_ref.py's."""
    assert hplanner.policy_slot(0, False, False) == 0 and hplanner.policy_slot(3, False, True) == 3
    assert hplanner.policy_slot(3, True, True) == 4 and hplanner.policy_slot(3, True, False) == 3
    for n, decay, KE, K, iters in ((200, 1.0, 50, 0, 5), (200, 1.25, 20, 5, 5), (64, 1.3, 8, 2, 3), (24, 2.0, 8, 8, 3), (500, 1.1, 10, 0, 7)):
        stub = types.SimpleNamespace(num_elites=KE)
        per_it = [HipEngine.icem_candidates(stub, n, decay, it, K) for it in range(iters)]
        assert per_it == [pref.n_it(n, decay, it, KE, K) for it in range(iters)]
        assert all(a >= b for a, b in zip(per_it, per_it[1:])), "the count never grows"
        least = hplanner.policy_min_candidates(n, decay, KE, K, iters)
        assert least == min(per_it) == per_it[-1]
        P = least - K - 1
        if P >= 1:      # the last proposal's slot is inside every iteration, with the mean candidate in front of it
            assert hplanner.policy_slot(K, True, True) + P <= least
    src = open(os.path.join(ROOT, "cadm_amd", "csrc", "icem.hip")).read()
    assert "K + (last && prm->add_mean_last ? 1 : 0)" in src and "(long long)K + 1 + P <= n_min" in src


# ---------------------------------------------------------------------------------------------------------------------- the envelope's inputs
# What tests/test_gpu_policy_envelope.py asks of its inputs, shown for the restatement alone: the engines, nets, seeds and noise levels
# are behind_rollout.py's POLICY_* tables, which both files read.
def envelope_problem(name):
    return br.policy_problem(name, corner_spec("widest") if name == "wide" else None)


envelope_layers = br.policy_layers


def test_nets_hold_the_bar_on_the_envelope_inputs():
    """The nets the envelope rolls, on D = 3, 28, 45 and 48 (and the halfcheetah nets that are new there): the float32 chain within 1e-5
    of the action range of the float64 restatement, and live -- on `states_for`'s rows and on the start states the roll reads."""
    worst = 0.0
    loop = br.POLICY_LOOP_NET
    cases = [(n, envelope_layers(n) + ((-1.0, 1.0),)) for n in ("pend", "ant", "slim", "big", "long")]
    cases += [("wide", (pref.envelope_policy(48, br.POLICY_NET[0], 24),) + br.POLICY_NET[1:] + ((-1.0, 1.0),))]
    cases += [("bnd", envelope_layers("bnd", sq) + ((-0.5, 2.0),)) for sq in pref.SQUASH]
    cases += [(n, (pref.he_policy(br.POLICY_ENGINES[n][1], loop[0], br.POLICY_ENGINES[n][2], loop[3], 0.5), loop[1], loop[2], (-1.0, 1.0)))
              for n in ("pend", "slim")]
    assert sorted({br.POLICY_ENGINES[n][1] for n, _ in cases}) == [3, 18, 28, 45, 48]
    for name, (layers, act, squash, (lb, ub)) in cases:
        D = br.POLICY_ENGINES[name][1]
        start = np.asarray(br.with_rows(envelope_problem(name), 3)["obs"], F)
        for x in (states_for(D), start):
            share, spread, open_ = pref.liveness(x, layers, act)
            assert share >= 0.5 and spread > 1e-3 and open_ >= 0.5, "%s %s: %.2f %.2e %.2f" % (name, squash, share, spread, open_)
            ref = pref.action64(x, layers, act, squash, lb, ub)
            emu = pref.emulate32(x, layers, act, squash, lb, ub)
            err = np.abs(emu.astype(np.float64) - ref).max()
            assert err <= 1e-5 * (ub - lb), (name, squash, err)
            assert emu.min() >= F(lb) and emu.max() <= F(ub)
            worst = max(worst, err / (1e-5 * (ub - lb)))
    print("\n[envelope nets] float32 chain against float64: %.3f of (1e-5 of the range)" % worst)


def test_noise_prefixes_and_counters_of_the_wide_groups():
    """An action dim's draw depends on (row, t, g = d >> 2) and its place in the group, never on A: the draws of a narrower env are the
    leading dims of a wider one's -- A = 1 uses z0 of words (0, 1) of group 0, A = 17 one dim of group 4, A = 24 six full groups -- and
    another group, step or row is another draw."""
    seed, call, m, P = br.POLICY_SEED, br.POLICY_CALL, 3, 17
    wide = pref.xi(seed, call, m, P, 1, 24)
    assert wide.shape == (m, P, 24) and len(np.unique(wide)) == wide.size
    for A in (1, 6, 8, 17):
        np.testing.assert_array_equal(pref.xi(seed, call, m, P, 1, A).view(np.uint32), wide[..., :A].view(np.uint32), err_msg="A = %d" % A)
    np.testing.assert_array_equal(pref.xi(seed, call, m, P, 1, 8)[..., :1], pref.xi(seed, call, m, P, 1, 1))
    # group g of one row is group 0 of no other counter: every (g, word pair) of a row differs, as do the steps and the rows
    for g in range(1, 6):
        assert not np.array_equal(wide[..., 4 * g:4 * g + 4], wide[..., :4]), "group %d repeats group 0" % g
    for t in (0, 2, 39):
        other = pref.xi(seed, call, m, P, t, 24)
        assert not (other == wide).any(), "step %d repeats step 1" % t
    assert not (np.roll(wide.reshape(m * P, 24), 1, axis=0) == wide.reshape(m * P, 24)).any()
    # the row id is mi * P + j: env 1 of (3, 17) is rows 17 .. 33 of one env with 51 sequences
    np.testing.assert_array_equal(pref.xi(seed, call, 1, m * P, 1, 17).reshape(m, P, 17), wide[..., :17])
    r = pref.xi_radius(seed, call, m, P, 1, 17)
    assert r.shape == (m, P, 17) and (r[..., 16] >= np.abs(wide[..., 16]) - 1e-6).all()


def test_share_of_unclipped_draws_at_step_zero():
    """The GPU tests recover the noise from the dims the clip left alone and ask that these are more than half (0.98 with the bias-only
    net of the A = 24 test): the restatement's own share at step 0 of every geometry, with the seeds, nets and noise levels of the
    GPU tests.  With bounds -0.5, 2 and squash "none", step 0 alone already has elements on either bound."""
    seed, call = br.POLICY_SEED, br.POLICY_CALL
    for name, (noise, shapes) in br.POLICY_ROLLS.items():
        _, D, A, _, _, _, _, bounds = br.POLICY_ENGINES[name]
        lb, ub = bounds or (-1.0, 1.0)
        prob = envelope_problem(name)
        for squash in (pref.SQUASH if name == "bnd" else ("tanh",)):
            layers, act, squash = envelope_layers(name, squash)
            for m, P in shapes:
                obs = np.asarray(br.with_rows(prob, m)["obs"], F)
                z = pref.xi(77 if name == "wide" else seed, 4 if name == "wide" else call, m, P, 0, A)      # (wide: test_noise_against_philox's)
                z[:, 0] = 0.0
                a = pref.emulate32(np.broadcast_to(obs[:, None], (m, P, D)), layers, act, squash, lb, ub, xi=z, noise_std=noise)
                free = ((a > F(lb)) & (a < F(ub)))[:, 1:]
                assert free.mean() > (0.98 if name == "wide" else 0.5), "%s %s m=%d P=%d: %.3f of the draws are unclipped" % (name, squash, m, P, free.mean())
                if name == "slim":
                    assert free[..., 16].any(), "no unclipped draw of group 4"
                if name == "bnd" and squash == "none":
                    assert (a == F(lb)).any() and (a == F(ub)).any()
                print("[%s %s m=%d P=%d noise %.2f] unclipped at step 0: %.3f" % (name, squash, m, P, noise, free.mean()))


def cpu_roll(prob, layers, act, squash, m, P, p, H, noise, seed, call):
    """the proposal roll of a vanilla problem restated on the CPU: `emulate32` on the particle mean, the oracle's one-step rollout from
    obs_rows under the Philox head noise of the iteration word POLICY_IT + 2 t -> (seqs [m,P,H,A], states [H,m,P,p,D])"""
    o = oracle_problem(br.with_rows(prob, m), F)
    E, D, A = prob["E"], prob["D"], prob["A"]
    states = np.broadcast_to(o["obs"][:, None, None, :], (m, P, p, D)).copy()
    seqs, read = np.empty((m, P, H, A), F), []
    for t in range(H):
        read.append(states)
        z = pref.xi(seed, call, m, P, t, A)
        z[:, 0] = 0.0
        a = pref.emulate32(pref.particle_mean32(states), layers, act, squash, xi=z, noise_std=noise)
        seqs[:, :, t] = a
        eps = philox.eps_normals(seed, call, hplanner.POLICY_IT + 2 * t, m, P, p, 1, D)
        _, traj = oplanner.rollout_indexed(o["env"], o["ff"], o["st"], o["obs"], None, np.ascontiguousarray(a[:, :, None, :]), eps, E, p, False,
                                           return_traj=True, obs_rows=states)
        states = traj[0].astype(F)
    return seqs, np.stack(read)


def test_the_long_roll_stays_finite():
    """Engine "long": the restated policy rolled through the oracle model for the H of POLICY_ENGINES -- every sequence, the noiseless
    one among them -- reads finite states below 1e4 in magnitude at every step, the last two steps' actions differ, and more than half
    of the draws stay unclipped at every step: the GPU test's checks along the 40 steps compare numbers, not NaN."""
    _, D, A, E, p, H = br.POLICY_ENGINES["long"][:6]
    noise, ((m, P),) = br.POLICY_ROLLS["long"]
    layers, act, squash = envelope_layers("long")
    seqs, states = cpu_roll(envelope_problem("long"), layers, act, squash, m, P, p, H, noise, br.POLICY_SEED, br.POLICY_CALL)
    assert H == 40 and states.shape == (H, m, P, p, D)
    assert np.isfinite(states).all() and np.abs(states).max() < 1e4, "the synthetic model leaves 1e4 within %d steps" % H
    assert np.isfinite(seqs).all() and not np.array_equal(seqs[:, :, H - 2], seqs[:, :, H - 1])
    free = np.abs(seqs[:, 1:]) < 1.0
    assert (free.mean(axis=(0, 1, 3)) > 0.5).all(), free.mean(axis=(0, 1, 3)).min()
    moved = np.abs(np.diff(states, axis=0)).max(axis=(1, 2, 3, 4))
    assert (moved > 0).all()
    print("\n[long roll on the CPU] largest |state| %.3g over %d steps, smallest unclipped share %.3f" % (np.abs(states).max(), H, free.mean(axis=(0, 1, 3)).min()))


def test_slot_arithmetic_of_the_exact_fit():
    """The GPU test of the exact fit: 24 candidates, 8 elites, 3 iterations, decay 2 -- 24, 16, 16 candidates --, 2 kept elites, the mean
    added last and 13 proposals: K + 1 + P = 16 = the smallest iteration, the proposals in slots 2 .. 14 and, last, 3 .. 15."""
    n, KE, iters, decay, K, P = 24, 8, 3, 2.0, 2, 13
    assert [pref.n_it(n, decay, it, KE, K) for it in range(iters)] == [24, 16, 16]
    assert hplanner.policy_min_candidates(n, decay, KE, K, iters) == 16 == K + 1 + P
    assert hplanner.policy_slot(K, False, True) == 2 and hplanner.policy_slot(K, True, True) == 3
    assert hplanner.policy_slot(K, True, True) + P == 16 and hplanner.policy_slot(K, False, True) + P == 15
    assert K + 1 + (P + 1) > hplanner.policy_min_candidates(n, decay, KE, K, iters)


# ---------------------------------------------------------------------------------------------------------------------- the header
def test_struct_constants_and_signatures_match_the_header():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    consts = {k: int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("CADM_MAX_POLICY_ACTIONS", "CADM_POLICY_NONE", "CADM_POLICY_TANH")}
    assert consts["CADM_MAX_POLICY_ACTIONS"] == _lib.MAX_POLICY_ACTIONS == 64
    assert _lib.POLICY_SQUASH == {"none": consts["CADM_POLICY_NONE"], "tanh": consts["CADM_POLICY_TANH"]}
    body = re.search(r"typedef struct cadm_policy_params \{(.*?)\} cadm_policy_params;", src, flags=re.S).group(1)
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[CADM_MAX_VALUE_LAYERS\])?;", body)
    want = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, want[t] * 4 if arr else want[t]) for t, n, arr in fields] == [(n, t) for n, t in _lib.PolicyParams._fields_]
    assert [n for n, _ in _lib.PolicyParams._fields_] == ["n_hidden", "hidden", "activation", "squash", "n_samples", "noise_std"]
    assert ctypes.sizeof(_lib.PolicyParams) == (1 + 4 + 1 + 1 + 1 + 1) * 4
    assert re.search(r"#define CADM_ABI_VERSION 2\b", src)
    kinds = {"cadm_ctx*": ctypes.c_void_p, "void*": ctypes.c_void_p, "float*": ctypes.c_void_p, "int32_t*": ctypes.c_void_p, "int": ctypes.c_int,
             "uint32_t": ctypes.c_uint32, "float**": ctypes.POINTER(ctypes.c_void_p)}
    structs = {"cadm_policy_params*": "PolicyParams", "cadm_reward_params*": "RewardParams", "cadm_value_params*": "ValueParams",
               "cadm_uncertainty_params*": "UncertaintyParams", "cadm_actuator_params*": "ActuatorParams", "cadm_track_params*": "TrackParams",
               "cadm_knot_params*": "KnotParams", "cadm_constraint_params*": "ConstraintParams", "cadm_score_params*": "ScoreParams",
               "cadm_mppi_params*": "MppiParams"}
    for name in ("cadm_set_policy_net", "cadm_policy_eval", "cadm_policy_workspace_bytes", "cadm_policy_propose", "cadm_guided_workspace_bytes",
                 "cadm_guided_plan"):
        ret, args = re.search(r"^(int|size_t) %s\((.*?)\);" % name, src, flags=re.S | re.M).groups()
        got = []
        for a in args.split(","):
            typ = re.sub(r"\bconst\b", "", a).strip().rsplit(" ", 1)[0].replace(" ", "")
            got.append(kinds[typ] if typ in kinds else ctypes.POINTER(getattr(_lib, structs[typ])))
        res, sig = _lib.SIGNATURES[name]
        assert res is (ctypes.c_int if ret == "int" else ctypes.c_size_t), name
        assert len(sig) == len(got) and all(x is y for x, y in zip(sig, got)), name
    # the loop entry is cadm_rewarded_plan's arguments behind the policy's one; the workspace query takes one count more
    assert _lib.SIGNATURES["cadm_guided_plan"][1][2:] == _lib.SIGNATURES["cadm_rewarded_plan"][1][1:]
    assert _lib.SIGNATURES["cadm_guided_workspace_bytes"][1][:-1] == _lib.SIGNATURES["cadm_rewarded_workspace_bytes"][1]
    # the roll's iteration words: even, above any planner iteration the library accepts next to it, below the forecast's word
    ph = open(os.path.join(ROOT, "cadm_amd", "csrc", "planner.h")).read()
    pit = int(re.search(r"#define CADM_POLICY_IT (0x[0-9A-Fa-f]+)", ph).group(1), 16)
    assert pit == _lib.POLICY_IT == hplanner.POLICY_IT and pit % 2 == 0 and pit < hplanner.FORECAST_IT < 1 << 24
    common = open(os.path.join(ROOT, "cadm_amd", "csrc", "common.h")).read()
    streams = dict(re.findall(r"#define (CADM_STREAM_\w+) (\d+)u", common))
    assert int(streams["CADM_STREAM_POLICY"]) == pref.STREAM_POLICY == 5
    assert len(set(streams.values())) == len(streams)
    assert "policy.hip" in open(os.path.join(ROOT, "cadm_amd", "csrc", "Makefile")).read()


# ---------------------------------------------------------------------------------------------------------------------- the options
def test_plan_options_accept_and_refuse():
    """`cem_policy_prior` alone takes the opt-in route and is folded into the struct the library reads; every default still gives None;
    the new fields sit in front of the reward ones, whose places existing tests pin; what is refused is refused without an engine."""
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_policy_prior=None) is None
    assert PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=None) is None
    assert PlanOptions._fields[-11:-9] == ("policy", "policy_params")
    assert PlanOptions(*range(18)).policy_params is None and PlanOptions(*range(18)).policy is None
    opt = PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=dict(), obs_dim=18, action_dim=6)
    assert opt.policy == ((256, 256), "relu", "tanh", 24, 0.0) and opt.update == "cem" and opt.value_params is None
    prm = opt.policy_params
    assert (prm.n_hidden, list(prm.hidden)[:2], prm.activation, prm.squash, prm.n_samples, prm.noise_std) == (2, [256, 256], 0, 1, 24, 0.0)
    opt = PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=dict(hidden_sizes=(), activation="swish", squash="none", n_samples=1, noise_std=0.25),
                                  cem_update="mppi")
    assert opt.policy == ((), "swish", "none", 1, 0.25) and opt.update == "mppi"
    with pytest.raises(ValueError, match="need use_cem=True"):
        PlanOptions.from_kwargs(cem_policy_prior=dict())
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_policy_prior=dict())
    for bad, frag in ((dict(hidden_sizes=(0,)), "hidden widths"), (dict(hidden_sizes=(513,)), "hidden widths"), (dict(hidden_sizes=(8,) * 5), "at most"),
                      (dict(activation="gelu"), "activation"), (dict(squash="sigmoid"), "squash"), (dict(squash=True), "squash"),
                      (dict(n_samples=0), "n_samples"), (dict(n_samples=2.5), "n_samples"), (dict(n_samples=True), "n_samples"),
                      (dict(noise_std=-0.1), "noise_std"), (dict(noise_std=float("nan")), "noise_std"), (dict(noise_std=float("inf")), "noise_std"),
                      (dict(noise_std="x"), "noise_std"), (dict(weight=1.0), "cem_policy_prior must be"), ("tanh", "cem_policy_prior must be")):
        with pytest.raises(ValueError, match=frag):
            PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=bad)
    with pytest.raises(ValueError, match="observation dims"):
        PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=dict(), obs_dim=129)
    with pytest.raises(ValueError, match="action dims"):
        PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=dict(), obs_dim=18, action_dim=65)


def test_opt_in_plan_routes_the_policy_first():
    """`HipEngine.opt_in_plan` hands a `PlanOptions` with a policy prior to `guided_plan`, with every other term's struct in its place."""
    seen = {}

    class Stub:
        def guided_plan(self, *a, **kw):
            seen["args"], seen["kw"] = a, kw
            return "plan"
    opt = PlanOptions.from_kwargs(use_cem=True, cem_policy_prior=dict(hidden_sizes=(8,)), cem_terminal_value=dict(hidden_sizes=(4,)),
                                  cem_keep_elites=2)
    assert HipEngine.opt_in_plan(Stub(), opt, "obs", None, None, "mean", "var", 64, seed=1) == "plan"
    a = seen["args"]
    assert a[0] is opt.policy_params and a[1] is None and a[2] is opt.value_params and a[15] is opt.params and a[16] == "obs"
    assert seen["kw"] == dict(seed=1)
