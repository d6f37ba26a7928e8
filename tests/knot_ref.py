"""Numpy restatement of the knot grid of include/cadm_hip.h (cadm_shape_actions), written from the definition: per step, its segment, its
knot and the next knot.  LINEAR evaluates a[k] + (t - k) / (k' - k) * (a[k'] - a[k]) in float64 and rounds once to float32."""
import numpy as np

HOLD, LINEAR = 0, 1


def knot_steps(H, r, phi=0):
    """The knot steps of horizon H under spacing r and phase phi (any integer: taken modulo r, non-negative)."""
    phi = int(phi) % int(r)
    J = (H - 1 + phi) // r + 1
    return [max(0, j * r - phi) for j in range(J)]


def segment(t, H, r, phi):
    """(k_j, k_{j+1}) of step t: its segment's knot step and the next knot (which may lie beyond the horizon)."""
    phi = int(phi) % int(r)
    j = (t + phi) // r
    return max(0, j * r - phi), (j + 1) * r - phi


def exact_steps(H, r, interp, phi=0):
    """bool [H]: the steps whose shaped value is a copy (knot steps; every step under HOLD; the held tail under LINEAR)."""
    out = np.zeros(H, bool)
    for t in range(H):
        k, k1 = segment(t, H, r, phi)
        out[t] = t == k or interp == HOLD or k1 > H - 1
    return out


def shape_one(a, r, interp, phi=0):
    """a [H, A] float32 -> its shaped copy, float32"""
    a = np.asarray(a, np.float32)
    H = a.shape[0]
    out = a.copy()
    for t in range(H):
        k, k1 = segment(t, H, r, phi)
        if t == k:
            continue
        if interp == LINEAR and k1 <= H - 1:
            a0, a1 = a[k].astype(np.float64), a[k1].astype(np.float64)
            out[t] = (a0 + (float(t - k) / float(k1 - k)) * (a1 - a0)).astype(np.float32)
        else:
            out[t] = a[k]
    return out


def shape(seqs, r, interp, phase=None):
    """seqs [m, ..., H, A] -> shaped copy; phase [m] integers (None: 0)."""
    seqs = np.asarray(seqs, np.float32)
    m, (H, A) = seqs.shape[0], seqs.shape[-2:]
    out = np.empty_like(seqs)
    for mi in range(m):
        phi = 0 if phase is None else int(phase[mi])
        src, dst = seqs[mi].reshape(-1, H, A), out[mi].reshape(-1, H, A)
        for c in range(src.shape[0]):
            dst[c] = shape_one(src[c], r, interp, phi)
    return out


def linear_f32(a0, a1, t, k, k1):
    """The kernel's own expression, fmaf(w, a1 - a0, a0) with w = float32(t - k) / float32(k1 - k), for float32 a0 / a1 whose difference and
    product are exact in float64 (values on +-1, 0): the float64 sum then rounds once, as the fused multiply-add does."""
    a0, a1 = np.float32(a0), np.float32(a1)
    w = np.float32(t - k) / np.float32(k1 - k)
    d = np.float32(a1 - a0)
    return np.float32(np.float64(w) * np.float64(d) + np.float64(a0))


def breakpoints(plan):
    """The steps t >= 1 at which a plan [H, A] differs from its previous step in any action dim."""
    plan = np.asarray(plan)
    return [t for t in range(1, plan.shape[0]) if not np.array_equal(plan[t], plan[t - 1])]
