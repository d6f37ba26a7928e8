"""Numpy restatement of the terminal value of the opt-in planner (csrc/value.hip: cadm_value_eval, cadm_value_returns) -- test
infrastructure shared by tests/test_value_ref.py (CPU) and tests/test_gpu_value.py.

`value` states V in float64; `emulate32` walks the kernel's float32 chain (include/cadm_hip.h, "Terminal value"): the input normalised
with one subtract and one multiply, every layer's accumulator seeded with the bias and then acc = fma(W[k][u], x_k, acc) for k
ascending, the activation, the linear output.  (The kernel also walks the zero pads up to the next multiple of 4 of a layer's K:
fma(0, 0, acc) leaves every acc but -0.0 as it is, so the emulation does not.)  `update` is the row update from V's own bits: one float32
multiply, then one float32 add.  The two are held together at the project's bar for fp32 kernels, `helpers.assert_close` at 1e-5 of the
output's scale."""
import numpy as np

F = np.float32
ACTS = ("relu", "tanh", "swish")


def inv_std(std):
    """1 / std formed in float64 and rounded once to float32, as the host hands it to the library"""
    return (1.0 / np.asarray(std, np.float64)).astype(F)


def act64(z, act):
    with np.errstate(all="ignore"):
        if act == "relu":
            return np.maximum(z, 0.0)
        if act == "tanh":
            return np.tanh(z)
        return z / (1.0 + np.exp(-z))


def value(states, layers, act, mean=None, std=None):
    """V [...] in float64 of states [..., D]: layers a list of (W [in,out], b [out]); the float32 weights, statistics and 1 / std are the
    numbers the kernel reads, the arithmetic is exact to float64.  A state with a non-finite value has V = NaN."""
    x = np.asarray(states, F).astype(np.float64)
    D = x.shape[-1]
    mu = np.zeros((D,), F) if mean is None else np.asarray(mean, F)
    si = np.ones((D,), F) if std is None else inv_std(std)
    bad = ~np.isfinite(x).all(axis=-1)
    with np.errstate(all="ignore"):
        h = (np.where(bad[..., None], 0.0, x) - mu.astype(np.float64)) * si.astype(np.float64)
        for l, (W, b) in enumerate(layers):
            h = h @ np.asarray(W, F).astype(np.float64) + np.asarray(b, F).astype(np.float64)
            if l + 1 < len(layers):
                h = act64(h, act)
    return np.where(bad, np.nan, h[..., 0])


def emulate32(states, layers, act, mean=None, std=None):
    """V [...] float32 by the kernel's chain: bias-seeded accumulators, one fma per k in ascending order (the product of two float32
    numbers is exact in float64, the sum is rounded to float64 and then to float32: a double rounding that differs from the single one
    in about one sum in 2^29), float32 activations"""
    x = np.asarray(states, F)
    D = x.shape[-1]
    mu = np.zeros((D,), F) if mean is None else np.asarray(mean, F)
    si = np.ones((D,), F) if std is None else inv_std(std)
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
    return np.where(bad, F(np.nan), h[..., 0]).astype(F)


def update(rows, v, weight, first=None, H=None):
    """rows' float32 from V's float32 bits: float32(rows + float32(weight * v)), one multiply, then one add; with `first` a row with
    first < H keeps its input bits"""
    rows, v = np.asarray(rows, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        wv = F(weight) * v
        out = rows + wv
    assert wv.dtype == F and out.dtype == F
    if first is not None:
        out = np.where(np.asarray(first) < H, rows, out)
    return out


def he_net(D, hidden, seed=0, out_scale=1.0):
    """He-initialised layers [(W [in,out], b [out])] float32 of D -> hidden -> 1, with small non-zero biases"""
    rng = np.random.default_rng(seed)
    dims = [D] + list(hidden) + [1]
    layers = []
    for l in range(len(dims) - 1):
        W = (rng.standard_normal((dims[l], dims[l + 1])) * np.sqrt(2.0 / dims[l])).astype(F)
        b = (0.1 * rng.standard_normal(dims[l + 1])).astype(F)
        if l + 2 == len(dims):
            W, b = (W * F(out_scale)).astype(F), (b * F(out_scale)).astype(F)
        layers.append((W, b))
    return layers


# Hidden widths off the multiples of 4 and 64 (tests/test_gpu_terms_envelope.py): widths 1, 2, 3; units N .. N4 - 1 written as zeros
# (5, 7, 65, 66, 130, 50, 30, 70, 18, 37); a last 64-unit group of 1 or 2 units (65, 130); four hidden layers.
ENVELOPE_NETS = [(1,), (2,), (3,), (5, 7), (65,), (130, 66), (50, 30, 70, 18), (37, 37, 37, 37)]


def envelope_net(K, hidden):
    """the He-initialised net of ENVELOPE_NETS at input width K that the CPU and the GPU tests share"""
    return he_net(K, hidden, seed=100 + ENVELOPE_NETS.index(tuple(hidden)))


def liveness(x, layers, act, mean=None, std=None):
    """(the smallest, over the hidden layers, of the largest share of non-zero units any row has; the standard deviation of the float64
    output over the rows as a fraction of its largest magnitude) -- a net whose units are dead, or whose output is constant, checks
    nothing"""
    x = np.asarray(x, F).astype(np.float64).reshape(-1, np.shape(x)[-1])
    mu = 0.0 if mean is None else np.asarray(mean, F).astype(np.float64)
    si = 1.0 if std is None else inv_std(std).astype(np.float64)
    h, share = (x - mu) * si, 1.0
    for l, (W, b) in enumerate(layers):
        h = h @ np.asarray(W, F).astype(np.float64) + np.asarray(b, F).astype(np.float64)
        if l + 1 < len(layers):
            h = act64(h, act)
            share = min(share, float((h != 0).mean(axis=1).max()))
    out = h[:, 0]
    return share, float(out.std() / max(np.abs(out).max(), 1e-300))


def sequential(layers, act):
    """the same net as a torch.nn.Sequential (Linear.weight is [out,in])"""
    import torch
    mods = []
    cls = {"relu": torch.nn.ReLU, "tanh": torch.nn.Tanh, "swish": torch.nn.SiLU}[act]
    for l, (W, b) in enumerate(layers):
        lin = torch.nn.Linear(W.shape[0], W.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(np.ascontiguousarray(W.T)))
            lin.bias.copy_(torch.from_numpy(b))
        mods.append(lin)
        if l + 1 < len(layers):
            mods.append(cls())
    return torch.nn.Sequential(*mods)
