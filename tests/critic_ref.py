"""Numpy restatement of the terminal value from Q critics of the opt-in planner (csrc/critic.hip: cadm_critic_eval,
cadm_critic_returns) -- test infrastructure shared by tests/test_critic_ref.py (CPU) and tests/test_gpu_critic.py.

Built on tests/policy_ref.py (the actor: `action64` / `emulate32`) and tests/value_ref.py (a critic is a value net over [s ; a]).
`q64` states reduce_c Q_c(s, pi(s)) in float64: the float32 weights, statistics and 1 / std are the numbers the kernel reads, the
arithmetic is exact to float64.  `emulate32` walks the kernel's float32 chain (include/cadm_hip.h, "Terminal value from Q critics"): the
actor's action by policy_ref.emulate32 (squash as one multiply and one add, the clip), the critic input [s ; a] normalised with one
subtract and one multiply, every critic by value_ref.emulate32's chain, then the reduce orders: min as r = q_0, r = fmin(r, q_c) in
ascending c; mean as r = q_0, r = r + q_c in ascending c and, for C > 1, one division by float32(C).  `update` is the row update from q's
own bits (value_ref.update).  The two statements are held together at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5
of the output's scale."""
import numpy as np

import policy_ref as pref
import value_ref as vref

F = np.float32
ACTS = vref.ACTS
REDUCES = ("min", "mean")
update = vref.update


def he_critics(D, A, hidden, C, seed=0, out_scale=1.0):
    """C He-initialised critics, each [(W [in,out], b [out])] float32 of D + A -> hidden -> 1 (value_ref.he_net under seeds seed + 1000 c)"""
    return [vref.he_net(D + A, hidden, seed + 1000 * c, out_scale) for c in range(C)]


def _bad(states, actions=None):
    bad = ~np.isfinite(np.asarray(states, F)).all(axis=-1)
    if actions is not None:
        bad = bad | ~np.isfinite(np.asarray(actions, F)).all(axis=-1)
    return bad


def each64(states, actions, critics, act, mean=None, std=None):
    """every critic's Q [C, ...] in float64 at given actions [..., A] (float32 numbers, as the kernel holds them in LDS)"""
    u = np.concatenate([np.asarray(states, F), np.asarray(actions, F)], axis=-1)
    return np.stack([vref.value(u, layers, act, mean, std) for layers in critics])


def reduce64(each, reduce):
    with np.errstate(all="ignore"):
        return each.min(axis=0) if reduce == "min" else each.sum(axis=0) / float(each.shape[0]) if each.shape[0] > 1 else each[0]


def q64(states, critics, act, reduce, actor=None, actions=None, mean=None, std=None, lb=-1.0, ub=1.0, want_each=False):
    """reduce_c Q_c(s, a) [...] in float64.  a: `actions` [..., A] when given, else the actor's -- actor = dict(layers=, act=, squash=,
    mean=, std=) -- float64 action of s (policy_ref.action64).  A state (or given action) with a non-finite value has NaN.  want_each:
    (q, every critic's [C, ...])."""
    s = np.asarray(states, F)
    bad = _bad(s, actions)
    if actions is None:
        a = pref.action64(s, actor["layers"], actor["act"], actor.get("squash", "tanh"), lb, ub, actor.get("mean"), actor.get("std"))
    else:
        a = np.where(bad[..., None], 0.0, np.asarray(actions, F).astype(np.float64))
    x = np.concatenate([np.where(bad[..., None], 0.0, s.astype(np.float64)), a], axis=-1)
    K = x.shape[-1]
    mu = np.zeros((K,), F) if mean is None else np.asarray(mean, F)
    si = np.ones((K,), F) if std is None else vref.inv_std(std)
    each = []
    with np.errstate(all="ignore"):
        for layers in critics:
            h = (x - mu.astype(np.float64)) * si.astype(np.float64)
            for l, (W, b) in enumerate(layers):
                h = h @ np.asarray(W, F).astype(np.float64) + np.asarray(b, F).astype(np.float64)
                if l + 1 < len(layers):
                    h = vref.act64(h, act)
            each.append(np.where(bad, np.nan, h[..., 0]))
    each = np.stack(each)
    q = reduce64(each, reduce)
    return (q, each) if want_each else q


def reduce32(each, reduce):
    """the kernel's reduce over float32 q [C, ...]: min as fmin in ascending c (fminf: a NaN operand is ignored); mean as float32 adds in
    ascending c, then for C > 1 one float32 division by float32(C)"""
    each = np.asarray(each, F)
    C = each.shape[0]
    with np.errstate(all="ignore"):
        r = each[0]
        for c in range(1, C):
            r = np.fmin(r, each[c]) if reduce == "min" else r + each[c]
        if reduce == "mean" and C > 1:
            r = r / F(C)
    assert r.dtype == F
    return r


def emulate32(states, critics, act, reduce, actor=None, actions=None, mean=None, std=None, lb=-1.0, ub=1.0, want_each=False, want_action=False):
    """reduce_c Q_c(s, a) [...] float32 by the kernel's chain.  a: `actions` when given, else policy_ref.emulate32's noiseless action of
    s.  A row with a non-finite state (or given action) has q = NaN, set explicitly: the actor's fallback action is what `want_action`
    shows for it, not what a Q is computed from.  Returns q, or (q[, each [C, ...]][, the action used])."""
    s = np.asarray(states, F)
    bad = _bad(s, actions)
    if actions is None:
        a = pref.emulate32(s, actor["layers"], actor["act"], actor.get("squash", "tanh"), lb, ub, actor.get("mean"), actor.get("std"))
    else:
        a = np.asarray(actions, F)
    u = np.concatenate([np.where(bad[..., None], F(0), s), np.where(bad[..., None], F(0), a)], axis=-1).astype(F)
    each = np.stack([vref.emulate32(u, layers, act, mean, std) for layers in critics])
    each = np.where(bad, F(np.nan), each).astype(F)
    q = np.where(bad, F(np.nan), reduce32(each, reduce)).astype(F)
    res = (q,) + ((each,) if want_each else ()) + ((a,) if want_action else ())
    return res[0] if len(res) == 1 else res


def cut(q, first, H):
    """what q_out reads under `first`: NaN where first < H"""
    return np.where(np.asarray(first) < H, F(np.nan), np.asarray(q, F)).astype(F)


def critic_from_value(layers, D, A, seed=0):
    """a critic over [s ; a] whose action rows of W_0 are zero and whose state rows are the value net's: Q(s, a) = V(s) for every a"""
    W0, b0 = layers[0]
    W = np.zeros((D + A, W0.shape[1]), F)
    W[:D] = W0
    return [(W, b0.copy())] + [(w.copy(), b.copy()) for w, b in layers[1:]]


def liveness(states, critics, act, actor, mean=None, std=None, lb=-1.0, ub=1.0):
    """What makes a test of the fused kernel void, as a dict: `units` -- the smallest, over critics and actor, of value_ref / policy_ref's
    share of live hidden units; `unsaturated` -- the share of the actor's outputs with |z| < 2 (1.0 without a tanh squash); `action` --
    max |Q(s, pi(s)) - Q(s, 0)| over the rows and critics as a fraction of the largest |Q|: a critic that does not read its action lines
    checks nothing of the path between the two chains.  `check_live` asserts the three."""
    s = np.asarray(states, F).reshape(-1, np.shape(states)[-1])
    ps, _, unsat = pref.liveness((s - (0 if actor.get("mean") is None else np.asarray(actor["mean"], F)))
                                 * (1 if actor.get("std") is None else vref.inv_std(actor["std"])), actor["layers"], actor["act"])
    a = pref.action64(s, actor["layers"], actor["act"], actor.get("squash", "tanh"), lb, ub, actor.get("mean"), actor.get("std"))
    u = np.concatenate([s.astype(np.float64), a], axis=-1)
    units = min([ps] + [vref.liveness(u, layers, act, mean, std)[0] for layers in critics])
    at_pi = each64(s, a, critics, act, mean, std)
    at_0 = each64(s, np.zeros_like(a), critics, act, mean, std)
    move = float(np.abs(at_pi - at_0).max() / max(np.abs(at_pi).max(), 1e-300))
    return dict(units=units, unsaturated=1.0 if actor.get("squash", "tanh") != "tanh" else unsat, action=move)


def check_live(states, critics, act, actor, mean=None, std=None, lb=-1.0, ub=1.0, what=""):
    live = liveness(states, critics, act, actor, mean, std, lb, ub)
    assert live["units"] > 0.2, "%s: dead hidden units (%.2f live): the case checks nothing" % (what, live["units"])
    assert live["unsaturated"] > 0.5, "%s: the squash is saturated (%.2f of the outputs below 2)" % (what, live["unsaturated"])
    assert live["action"] > 1e-3, "%s: Q(s, pi(s)) and Q(s, 0) differ by %.2e of scale: the action lines are not read" % (what, live["action"])
    return live


# The kernel cases tests/test_gpu_critic.py runs on hopper_like (D = 11, A = 3: K = 14 is no multiple of 4) and tests/test_critic_ref.py
# holds to the liveness conditions on the CPU: every critic geometry behind every actor geometry, under every (C, reduce, squash).
KERNEL_CRITICS = [(), (48,), (64,), (200,), (64, 48, 200)]
KERNEL_ACTORS = [(), (64, 48)]
KERNEL_COMBOS = [(C, reduce, squash) for C in (1, 2, 3) for reduce in REDUCES for squash in pref.SQUASH]
KERNEL_ROWS = [(3, 11), (3, 1)]      # m, n at p = 5: 165 rows (ten full 16-row tiles and a tail of 5), 15 rows (less than a tile)


def kernel_states(m, n, seed, H=3, p=5, D=11, A=3, name=None):
    """(traj [H,m,n,p,D], its last states [m n p, D]) of behind_rollout.synth_traj; name: at the shape of that one of
    behind_rollout.TERM_ENGINES (`term_traj`) in the place of H, p, D, A"""
    from behind_rollout import synth_traj, term_traj
    traj = synth_traj(seed, H, m, n, p, D, A)[0] if name is None else term_traj(name, m, n, seed)[0]
    return traj, traj[-1].reshape(-1, traj.shape[-1])


def kernel_case(states, A, hidden, phidden, C, act, squash, seed):
    """(actor, critics, in_mean, in_std) of one kernel case: He-initialised nets, and input statistics that are not 0 / 1 -- near the
    states' own (offset by 0.1, widened by 1.1), as a learner's running statistics would be, and for the action dims 0.05 / 0.6"""
    s = np.asarray(states, F)
    D = s.shape[-1]
    smean, sstd = (s.mean(axis=0) + 0.1).astype(F), (1.1 * s.std(axis=0)).astype(F)
    actor = dict(layers=pref.he_policy(D, phidden, A, seed, out_scale=0.5), act=act, squash=squash, mean=smean, std=sstd)
    critics = he_critics(D, A, hidden, C, seed + 1)
    mean = np.concatenate([(smean - F(0.2)).astype(F), np.full((A,), 0.05, F)])
    std = np.concatenate([(F(0.9) * sstd).astype(F), np.full((A,), 0.6, F)])
    return actor, critics, mean, std


# The cases tests/test_gpu_critic_envelope.py runs on behind_rollout.CRITIC_ENGINES and tests/test_critic_ref.py holds to the liveness
# conditions on the CPU: hidden widths off the multiples of 4 (value_ref.ENVELOPE_NETS: widths 1 and 3, a last 64-unit group of 1 or 2
# units, four hidden layers) behind actors of one and of five dense layers; C cycles over (1, 4, 5) -- out of step with the actors,
# which cycle with the same period --, the reduce over (min, mean), the squash over (tanh, none).  Every activation runs every case.
ENVELOPE_CRITICS = [(1,), (3,), (65,), (130, 66), (50, 30, 70, 18), (37, 37, 37, 37)]
ENVELOPE_ACTORS = [(), (50, 30, 70, 18), (37, 37, 37, 37)]
ENVELOPE_CASES = [(hidden, phidden, (1, 4, 5)[(i + i // 3) % 3], REDUCES[i % 2], pref.SQUASH[(i // 2) % 2])
                  for i, (hidden, phidden) in enumerate((h, ph) for h in ENVELOPE_CRITICS for ph in ENVELOPE_ACTORS)]
assert all(tuple(h) in vref.ENVELOPE_NETS for h in ENVELOPE_CRITICS + ENVELOPE_ACTORS[1:])
