"""Numpy restatement of the policy prior of the opt-in planner (csrc/policy.hip: cadm_policy_eval, cadm_policy_propose) -- test
infrastructure shared by tests/test_policy_ref.py (CPU) and tests/test_gpu_policy.py.

`action64` states the action in float64; `emulate32` walks the kernel's float32 chain (include/cadm_hip.h, "Policy prior"): the input
normalised with one subtract and one multiply, every layer's accumulator seeded with the bias and then acc = fma(W[k][u], x_k, acc) for k
ascending (tests/value_ref.py's chain, with A outputs), the squash mid + half * tanh(z) as one multiply and one add, the noise
noise_std * xi as one multiply and one add, the clip.  `particle_mean32` is the state estimate: sequential float32 adds over the
particles, one division.  `xi` is the exploration noise from oracle/philox.py's generator under the kernel's counters.  The two
statements of the action are held together at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5 of the action range."""
import numpy as np

import value_ref as vref
from oracle import philox

F = np.float32
ACTS = vref.ACTS
SQUASH = ("tanh", "none")
STREAM_POLICY = 5      # csrc/common.h CADM_STREAM_POLICY


def he_policy(D, hidden, A, seed=0, out_scale=1.0):
    """He-initialised layers [(W [in,out], b [out])] float32 of D -> hidden -> A, with small non-zero biases"""
    rng = np.random.default_rng(seed)
    dims = [D] + list(hidden) + [A]
    layers = []
    for l in range(len(dims) - 1):
        W = (rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(F)
        b = (0.1 * rng.standard_normal(dims[l + 1])).astype(F)
        if l + 2 == len(dims):
            W, b = (W * F(out_scale)).astype(F), (b * F(out_scale)).astype(F)
        layers.append((W, b))
    return layers


def envelope_policy(D, hidden, A):
    """the net of value_ref.ENVELOPE_NETS widened to A outputs that the CPU and the GPU tests share; () is the linear policy"""
    hidden = tuple(hidden)
    return he_policy(D, hidden, A, seed=300 + (vref.ENVELOPE_NETS.index(hidden) if hidden else 99), out_scale=0.5)


def fallback(lb, ub):
    return F(min(max(F(0), F(lb)), F(ub)))


def _z64(x, layers, act, mean, std):
    D = x.shape[-1]
    mu = np.zeros((D,), F) if mean is None else np.asarray(mean, F)
    si = np.ones((D,), F) if std is None else vref.inv_std(std)
    with np.errstate(all="ignore"):
        h = (x - mu.astype(np.float64)) * si.astype(np.float64)
        for l, (W, b) in enumerate(layers):
            h = h @ np.asarray(W, F).astype(np.float64) + np.asarray(b, F).astype(np.float64)
            if l + 1 < len(layers):
                h = vref.act64(h, act)
    return h


def action64(states, layers, act, squash="tanh", lb=-1.0, ub=1.0, mean=None, std=None):
    """the noiseless action [..., A] in float64 of states [..., D]: the float32 weights, statistics, 1 / std, mid and half are the
    numbers the kernel reads, the arithmetic is exact to float64.  A state with a non-finite value has the fallback clip(0, lb, ub)."""
    x = np.asarray(states, F).astype(np.float64)
    bad = ~np.isfinite(x).all(axis=-1)
    z = _z64(np.where(bad[..., None], 0.0, x), layers, act, mean, std)
    mid, half = F(0.5) * (F(ub) + F(lb)), F(0.5) * (F(ub) - F(lb))
    a = float(mid) + float(half) * np.tanh(z) if squash == "tanh" else z
    a = np.minimum(np.maximum(a, float(F(lb))), float(F(ub)))
    return np.where(bad[..., None], float(fallback(lb, ub)), a)


def squash32(z, squash, lb, ub):
    """the float32 action before noise and clip: mid + half * tanh(z) (one multiply, one add), or z"""
    z = np.asarray(z, F)
    if squash != "tanh":
        return z
    mid, half = F(0.5) * (F(ub) + F(lb)), F(0.5) * (F(ub) - F(lb))
    out = mid + half * np.tanh(z)
    assert out.dtype == F
    return out


def emulate32(states, layers, act, squash="tanh", lb=-1.0, ub=1.0, mean=None, std=None, xi=None, noise_std=0.0, want_raw=False):
    """the action [..., A] float32 by the kernel's chain.  xi [..., A] (None: no noise) is added as noise_std * xi to the rows it is
    given for -- the caller passes zeros for sequence 0 -- before the clip.  want_raw: (action, the squashed action before noise and
    clip)."""
    x = np.asarray(states, F)
    D = x.shape[-1]
    mu = np.zeros((D,), F) if mean is None else np.asarray(mean, F)
    si = np.ones((D,), F) if std is None else vref.inv_std(std)
    bad = ~np.isfinite(x).all(axis=-1)
    with np.errstate(all="ignore"):
        h = (np.where(bad[..., None], F(0), x) - mu) * si
        assert h.dtype == F
        for l, (W, b) in enumerate(layers):
            W, b = np.asarray(W, F), np.asarray(b, F)
            acc = np.broadcast_to(b, h.shape[:-1] + b.shape).astype(F)
            for k in range(W.shape[0]):
                acc = (h[..., k:k + 1].astype(np.float64) * W[k].astype(np.float64) + acc.astype(np.float64)).astype(F)
            if l + 1 < len(layers):
                if act == "relu":
                    acc = np.maximum(acc, F(0))
                elif act == "tanh":
                    acc = np.tanh(acc)
                else:
                    acc = acc / (F(1) + np.exp(-acc))
            assert acc.dtype == F
            h = acc
        raw = squash32(h, squash, lb, ub)
        a = raw
        if xi is not None and noise_std > 0.0:
            a = raw + F(noise_std) * np.asarray(xi, F)
            assert a.dtype == F
        a = np.minimum(np.maximum(a, F(lb)), F(ub))
    a = np.where(bad[..., None], fallback(lb, ub), a).astype(F)
    return (a, raw) if want_raw else a


def particle_mean32(states):
    """the state estimate [..., D] float32 of particle states [..., p, D]: sequential float32 adds over the particles in ascending
    order, starting from particle 0's value, then one IEEE division by float32(p) (p = 1: the value itself)"""
    x = np.asarray(states, F)
    p = x.shape[-2]
    with np.errstate(all="ignore"):
        s = x[..., 0, :]
        for j in range(1, p):
            s = s + x[..., j, :]
        if p > 1:
            s = s / F(p)
    assert s.dtype == F
    return s


def xi(seed, call, m, P, t, A):
    """the exploration noise [m, P, A] float32 of step t: Philox4x32-10 keyed (seed, call), counter (mi * P + j, t, g, STREAM_POLICY);
    one call serves dims 4 g .. 4 g + 3, words (0, 1) through Box-Muller to dims 4 g and 4 g + 1, words (2, 3) to 4 g + 2 and 4 g + 3.
    Row j = 0 is drawn like the others here: the kernel never adds it."""
    row = np.arange(m * P, dtype=np.uint32).reshape(m, P)
    ng = (A + 3) // 4
    out = np.empty((m, P, 4 * ng), F)
    for g in range(ng):
        r = philox.philox4x32_10(philox._ctr(row, np.uint32(t), np.uint32(g), np.uint32(STREAM_POLICY)), philox._key(seed, call, row.shape))
        out[..., 4 * g], out[..., 4 * g + 1] = philox.box_muller(philox.u01(r[..., 0]), philox.u01(r[..., 1]))
        out[..., 4 * g + 2], out[..., 4 * g + 3] = philox.box_muller(philox.u01(r[..., 2]), philox.u01(r[..., 3]))
    return out[..., :A]


def xi_radius(seed, call, m, P, t, A):
    """the Box-Muller radius sqrt(-2 ln u1) [m, P, A] float64 behind every draw of `xi`: what the error of a device draw's sine or
    cosine is multiplied by"""
    z = xi(seed, call, m, P, t, 2 * ((A + 1) // 2)).astype(np.float64)
    r = np.hypot(z[..., 0::2], z[..., 1::2])
    return np.repeat(r, 2, axis=-1)[..., :A]


def liveness(x, layers, act):
    """(the smallest, over the hidden layers, of the largest share of non-zero units any row has; the smallest, over the action dims, of
    the standard deviation of the output z over the rows as a fraction of its largest magnitude; the share of outputs with |z| < 2, where
    tanh has not flattened a difference away) -- a net whose units are dead, whose output is constant or whose squash is saturated checks
    nothing"""
    x = np.asarray(x, F).astype(np.float64).reshape(-1, np.shape(x)[-1])
    h, share = x, 1.0
    for l, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, F).astype(np.float64) + np.asarray(b, F).astype(np.float64)
        if l + 1 < len(layers):
            h = vref.act64(h, act)
            share = min(share, float((h != 0).mean(axis=1).max()))
    spread = float((h.std(axis=0) / np.maximum(np.abs(h).max(axis=0), 1e-300)).min())
    return share, spread, float((np.abs(h) < 2.0).mean())


def n_it(n, decay, it, num_elites, K):
    """csrc/icem.hip icem_n_it: the candidates of iteration `it`, decay rounded to float32 as the library receives it"""
    v = int(np.floor(float(n) / float(np.float32(decay)) ** it))
    return min(n, max(v, 2 * num_elites, K + 1))
