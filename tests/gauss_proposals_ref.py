"""Numpy restatement of one policy step of the proposal roll under proposals drawn from the head (csrc/policy_gauss.hip:
policy_gauss_roll_kernel behind cadm_set_policy_proposals) -- test infrastructure shared by tests/test_gauss_proposals_ref.py (CPU) and
tests/test_gpu_gauss_proposals.py, built on tests/policy_ref.py's particle mean and draws (stream word 5, the noise route's) and on
tests/gauss_policy_ref.py's sums of a SAC actor's last layer.

`step32` walks the arithmetic of include/cadm_hip.h ("Proposals of the policy prior drawn from the head") operation for operation in
float32 on the state estimates a step read, `step64` restates it in float64 on the same float32 weights and the same draws, `noise32`
is the noise route's step on the same estimates (policy_ref.emulate32: the anchor), and `bar` is tests/gauss_policy_ref.py's action
bar with sig replaced by std_scale * sig -- the project's 1e-5 of scale for an fp32 chain plus 4e-6 per unit of Box-Muller radius for
a device draw, propagated through the formulas; no number of its own."""
import numpy as np

import gauss_policy_ref as gref
import policy_ref as pref

F = np.float32
# (env name, D, A) of the two geometries, m envs, P sequences, H steps, p particles: A = 1 uses one dim of a Philox group, A = 6 the
# second group; P = 3 has a sequence without a draw and two with one
SHAPES = (("pendulum", 3, 1), ("halfcheetah", 18, 6))
M, P, H, NP = 2, 3, 4, 5
# tests/test_gpu_gauss_policy.py's widths, no multiple of 4 or 64; tanh units are bounded, so the un-squashed mean stays inside the action
# bounds while the synthetic model's states grow over the steps of a roll: with squash "none" a clipped action checks nothing
HIDDEN, ACT = (33, 70), "tanh"
LO, HI = -3.0, 0.5
SEED, CALL = 5, 9


def draws(seed, call, m, P, t, A, std_scale=1.0):
    """(xi [m, P, A] float32 with zeros where nothing is drawn -- sequence 0, or std_scale == 0 --, the Box-Muller radii [m, P, A]
    float64 with zeros there too)"""
    xi, r = pref.xi(seed, call, m, P, t, A), pref.xi_radius(seed, call, m, P, t, A)
    if not std_scale > 0.0:
        return np.zeros_like(xi), np.zeros_like(r)
    xi[:, 0], r[:, 0] = 0.0, 0.0
    return xi, r


def states(m, P, p, D, seed=0, spread=0.05):
    """particle states [m, P, p, D] float32 as a step t >= 1 reads them: one state per row, its particles scattered around it"""
    rng = np.random.default_rng(4000 + seed)
    return (rng.standard_normal((m, P, 1, D)) + spread * rng.standard_normal((m, P, p, D))).astype(F)


def _bounds(lo, hi, lb, ub):
    lo, hi, lb, ub = F(lo), F(hi), F(lb), F(ub)
    return lo, hi, lb, ub, F(0.5) * (ub + lb), F(0.5) * (ub - lb)


def step32(est, layers, act, squash, bound, lo, hi, xi, std_scale, lb=-1.0, ub=1.0, mean=None, std=None):
    """the actions [m, P, A] float32 of state estimates est [m, P, D] by the kernel's float32 arithmetic, every operation rounded on its
    own; layers: the SAC actor's (2 A outputs); xi [m, P, A] from `draws` (zeros where nothing is drawn: those rows take u = mu)"""
    est, e = np.asarray(est, F), np.asarray(xi, F)
    A = e.shape[-1]
    z = gref.z32(est, layers, act, mean, std)
    mu, l = z[..., :A], z[..., A:]
    lo, hi, lb, ub, mid, half = _bounds(lo, hi, lb, ub)
    drawn = np.zeros(e.shape, bool)
    if std_scale > 0.0:
        drawn[:, 1:] = True
    with np.errstate(all="ignore"):
        ls = np.minimum(np.maximum(l, lo), hi) if bound == "clamp" else lo + (F(0.5) * (hi - lo)) * (np.tanh(l) + F(1))
        sig = np.exp(ls)
        s = F(std_scale) * sig
        u = np.where(drawn, mu + s * e, mu)
        a = mid + half * np.tanh(u) if squash == "tanh" else u
        a = np.minimum(np.maximum(a, lb), ub)
    for v in (ls, sig, s, u, a):
        assert v.dtype == F
    bad = ~np.isfinite(est).all(axis=-1)
    return np.where(bad[..., None], pref.fallback(lb, ub), a).astype(F)


def step64(est, layers, act, squash, bound, lo, hi, xi, std_scale, lb=-1.0, ub=1.0, mean=None, std=None):
    """float64 restatement -> dict(act [m, P, A], sig = std_scale * exp(ls) (0 where nothing is drawn), z the 2 A sums): the bounds,
    std_scale, mid and half are the float32 numbers the kernel reads, the arithmetic is float64"""
    est, e = np.asarray(est, F), np.asarray(xi, np.float64)
    A = e.shape[-1]
    z = gref.z64(est, layers, act, mean, std)
    mu, l = z[..., :A], z[..., A:]
    lo, hi, lb, ub, mid, half = (float(v) for v in _bounds(lo, hi, lb, ub))
    ls = np.clip(l, lo, hi) if bound == "clamp" else lo + 0.5 * (hi - lo) * (np.tanh(l) + 1.0)
    s = float(F(std_scale)) * np.exp(ls)
    if std_scale > 0.0:
        s[:, 0] = 0.0
    else:
        s[:] = 0.0
    u = mu + s * e
    a = np.clip(mid + half * np.tanh(u) if squash == "tanh" else u, lb, ub)
    bad = ~np.isfinite(est).all(axis=-1)
    return dict(act=np.where(bad[..., None], float(pref.fallback(lb, ub)), a), sig=s, z=z, l=l)


def bar(ref, xi, radius, squash, bound, lo, hi, lb=-1.0, ub=1.0):
    """the bar on |act - ref["act"]| [m, P, A]: gauss_policy_ref.bars' action bar on the reference's own sums, with sig replaced by
    std_scale * sig (ref["sig"]; a row without a draw has sig = 0, |xi| = 0 and keeps the chain's share and the squash's rounding)"""
    sh = ref["act"].shape
    flat = dict(sig=ref["sig"].reshape(-1, sh[-1]), logp=np.zeros(int(np.prod(sh[:-1]))))
    act_bar, _ = gref.bars(ref["z"].reshape(-1, 2 * sh[-1]), flat, np.asarray(xi).reshape(-1, sh[-1]), np.asarray(radius).reshape(-1, sh[-1]),
                           squash, bound, lo, hi, lb, ub)
    return act_bar.reshape(sh)


def noise32(est, mean_layers, act, squash, xi, noise_std, lb=-1.0, ub=1.0, mean=None, std=None):
    """the noise route's step on the same estimates and draws (policy_ref.emulate32): the mode action plus noise_std * xi behind the squash"""
    return pref.emulate32(est, mean_layers, act, squash, lb, ub, mean, std, xi=xi, noise_std=noise_std)


def anchor_layers(D, hidden, A, seed=0):
    """a SAC actor whose log-std layer is all zeros (l = 0 exactly: the accumulator is seeded with the bias 0 and fma(0, x, 0) == 0), so
    that with lo < 0 < hi sig = exp(0) = 1 and the head route at std_scale = s is the noise route at noise_std = s"""
    layers = pref.he_policy(D, hidden, 2 * A, seed, 0.5)
    W, b = layers[-1]
    W, b = W.copy(), b.copy()
    W[:, A:], b[A:] = 0.0, 0.0
    return list(layers[:-1]) + [(W, b)]
