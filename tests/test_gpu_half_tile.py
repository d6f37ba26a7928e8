"""The half last hidden tile (cadm_amd/csrc/xdl_geo.h): at hidden 200 tile 12 holds units 192..199 only, and the cooperative kernel
(flavours 1 / 2) packs the low parts of those units' weights into the empty half of the tile's A operand -- two MFMAs per chunk into
one accumulator, a half-wave exchange in the epilogue, the tile moved to wave 4.  The wave-tile kernel (flavours 3 / 4) keeps three
MFMAs per chunk and is the reference the packed form must match BIT FOR BIT.

In a trained-like net the other 192 units hide a lane-mapping or exchange error of that tile in the 7th digit.  Here every consumer
of a hidden layer reads units 192..199 ONLY (the outgoing weights of units 0..191 are zero, those of the eight units scaled by
sqrt(200 / 8) so that the next layer's pre-activations keep their trained-like size): whatever the half tile gets wrong is the result.

Not tested, stated in xdl_geo.h: the zero rows of the second product add +-0 to LO, which can only change the sign of an exactly zero
LO; a NaN activation makes both forms NaN."""
import copy
import os

import numpy as np
import pytest
import torch

import precision
from cadm_amd import _lib, synth
from helpers import make_engine

pytestmark = pytest.mark.gpu

E, P_, N, H = 5, 20, 7, 4          # 28 rows per member: two row tiles, the second ragged
HALF0, HID = 192, 200              # units 192..199: the half tile
LOG2E = np.float32(1.4426950408889634)


def _only_half_tile(prob, first=HALF0):
    """Every consumer of a hidden layer reads the units from `first` on only; weights and biases INTO those units stay as drawn."""
    ff = prob["ff"]
    nh = len(prob["hidden_sizes"])
    gain = np.sqrt(prob["hidden_sizes"][0] / float(prob["hidden_sizes"][0] - first))
    for k in ["hidden_%d_weight" % l for l in range(1, nh)] + ["output_mu_weight", "output_logvar_weight"]:
        ff[k][:, :first, :] = 0.0
        ff[k][:, first:, :] *= gain
    for k in ff:                   # the engine's fp32 weights ARE the model: the oracles get the same numbers
        ff[k] = ff[k].astype(np.float32).astype(np.float64)
    return prob


def _as_packed(w, layer):
    """f16 high part of a weight as the packer splits it (layer 0 carries log2(e): xdl_geo.h), back in the model's units."""
    sc = LOG2E if layer == 0 else np.float32(1.0)
    return (w.astype(np.float32) * sc).astype(np.float16).astype(np.float32), sc


def _off_f16_grid(prob):
    """Weights into units 192..199 half an f16 ulp off the grid, all to the same side: w = f16(w) (1 + 2^-12), exact in fp32.  Their low
    part is then as large as a low part gets and carries the same sign in every product of a dot product."""
    for l in range(len(prob["hidden_sizes"])):
        w = prob["ff"]["hidden_%d_weight" % l]
        hi, sc = _as_packed(w[:, :, HALF0:], l)
        w[:, :, HALF0:] = ((hi * np.float32(1.0 + 2.0 ** -12)) / sc).astype(np.float32)
    return prob


def _without_lo(prob):
    """The same model with the low part of every weight into units 192..199 dropped (what a lost or misplaced w2 x1 product computes)."""
    q = copy.deepcopy(prob)
    for l in range(len(q["hidden_sizes"])):
        w = q["ff"]["hidden_%d_weight" % l]
        hi, sc = _as_packed(w[:, :, HALF0:], l)
        w[:, :, HALF0:] = hi / sc
    return q


def _run(eng, prob, ctx, acts, eps, flavour, **kw):
    eng.dev_set_rollout("xdl", row_tiles=int(flavour))
    try:
        rows, traj = eng.rollout_returns(prob["obs"], ctx, acts, eps=eps, want_traj=True, **kw)
        torch.cuda.synchronize()
        return rows.cpu().numpy(), traj.cpu().numpy()
    finally:
        eng.dev_set_rollout("xdl", row_tiles=0)


def _inputs(prob, seed, H_=H, n=N):
    rng = np.random.default_rng(seed)
    acts = rng.uniform(-1, 1, (1, n, H_, prob["A"])).astype(np.float32)
    eps = rng.standard_normal((H_, 1, n, P_, prob["D"])).astype(np.float32)
    return acts, eps


def _check(prob, acts, eps, lo_must_matter):
    """Flavours 1 and 2 against flavour 3, bit for bit, with injected noise and with device Philox; flavour 1 against the fp64 oracle
    at the trajectory bar of tests/test_gpu_precision.py (the fp32 oracle's own distance from fp64, x 4, floor 2e-6)."""
    R64, T64 = precision.oracle_rollout(prob, np.float64, acts, eps, P_, False)
    R32, T32 = precision.oracle_rollout(prob, np.float32, acts, eps, P_, False)
    o_t, o_r = precision.err_stats(T32, T64)["max_rel"], precision.err_stats(R32, R64)["max_rel"]
    bar_t, bar_r = max(4 * o_t, 2e-6), max(4 * o_r, 2e-6)
    if lo_must_matter:      # on the CPU first: these inputs do tell a kernel without the w2 x1 product from a correct one
        Rd, Td = precision.oracle_rollout(_without_lo(prob), np.float32, acts, eps, P_, False)
        d_t, d_r = precision.err_stats(Td, T64)["max_rel"], precision.err_stats(Rd, R64)["max_rel"]
        print("without LO: trajectory %.2e returns %.2e (bars %.2e / %.2e)" % (d_t, d_r, bar_t, bar_r))
        assert d_t > 1e-4 and d_t > 10 * bar_t and d_r > 10 * bar_r, (d_t, d_r, bar_t, bar_r)
    eng = make_engine(prob, p=P_, lib=_lib.load_dev())
    ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"]) if prob["cp"] is not None else None
    acts_d, eps_d = eng._t(acts), eng._t(eps)
    for kw, e in (({}, eps_d), ({"seed": 5, "call": 3, "it": 1}, None)):
        r3, t3 = _run(eng, prob, ctx, acts_d, e, 3, **kw)
        assert np.isfinite(r3).all() and np.isfinite(t3).all()
        for flavour in (1, 2):
            r, t = _run(eng, prob, ctx, acts_d, e, flavour, **kw)
            np.testing.assert_array_equal(r, r3, err_msg="returns, flavour %d" % flavour)
            np.testing.assert_array_equal(t, t3, err_msg="trajectory, flavour %d" % flavour)
            if e is not None and flavour == 1:
                x_t, x_r = precision.err_stats(t, T64)["max_rel"], precision.err_stats(r, R64)["max_rel"]
                print("flavour 1 vs fp64: trajectory %.2e (fp32 oracle %.2e) returns %.2e (%.2e)" % (x_t, o_t, x_r, o_r))
                assert x_t <= bar_t, (x_t, o_t)
                assert x_r <= bar_r, (x_r, o_r)
    eng.close()


@pytest.mark.parametrize("context", [True, False])      # with context: layer 0's invariant-chunk prologue runs for the half tile too
def test_only_the_half_tile_carries_the_signal(gpu, context):
    prob = _only_half_tile(synth.make_problem(env="halfcheetah", context=context, E=E, m=1, H=H, trained_like=True, seed=31))
    acts, eps = _inputs(prob, 3)
    _check(prob, acts, eps, lo_must_matter=False)


@pytest.mark.parametrize("context", [True, False])
def test_low_parts_of_the_half_tile_matter(gpu, context):
    prob = _off_f16_grid(_only_half_tile(synth.make_problem(env="halfcheetah", context=context, E=E, m=1, H=H, trained_like=True, seed=31)))
    acts, eps = _inputs(prob, 3)
    _check(prob, acts, eps, lo_must_matter=True)


@pytest.mark.parametrize("hidden,first", [
    ((196, 196), 192),      # 13 tiles, four real units in the half tile, which wave 4 owns as at 200
    ((120, 120), 112),      # 8 tiles, one per wave: the half tile stays with wave 7
])
def test_half_tile_in_jit_built_widths(gpu, hidden, first):
    """Built on demand from the same header: flavour 1 against the wave-tile kernel bit for bit, the last tile alone carrying the signal."""
    prob = _only_half_tile(synth.make_problem(env="halfcheetah", context=True, E=E, m=1, H=H, hidden_sizes=hidden, trained_like=True, seed=33), first)
    eng = make_engine(prob, p=P_, lib=_lib.load_dev())
    assert not eng.lib.cadm_rollout_builtin(eng._ctx)
    acts, eps = _inputs(prob, 4)
    ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    acts_d, eps_d = eng._t(acts), eng._t(eps)
    r3, t3 = _run(eng, prob, ctx, acts_d, eps_d, 3)
    r1, t1 = _run(eng, prob, ctx, acts_d, eps_d, 1)
    assert np.isfinite(r3).all() and np.abs(t3).max() > 0
    np.testing.assert_array_equal(r1, r3)
    np.testing.assert_array_equal(t1, t3)
    eng.close()


@pytest.mark.parametrize("hid", [128, 256])
def test_widths_without_a_half_tile_are_unchanged(gpu, hid):
    """128 and 256 are whole tiles: the three-MFMA path.  Flavours 1 / 2 against 3; and, where CADM_PARENT_DEV_LIB names a developer
    library built from the parent commit, a small plan and the rollout of both builds must be equal."""
    prob = synth.make_problem(env="halfcheetah", context=True, E=E, m=1, H=H, hidden_sizes=(hid,) * 4, trained_like=True, seed=35)
    acts, eps = _inputs(prob, 5)
    args = [prob[k] for k in ("obs", "cp_obs", "cp_act", "init_mean", "init_var")]
    out = {}
    libs = {"this": None}
    parent = os.environ.get("CADM_PARENT_DEV_LIB")
    if parent and os.path.exists(parent):
        libs["parent"] = parent
    for name, path in libs.items():
        eng = make_engine(prob, p=P_, lib=_lib.load_dev(path))
        assert eng.lib.cadm_rollout_builtin(eng._ctx)
        ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"])
        acts_d, eps_d = eng._t(acts), eng._t(eps)
        r3, t3 = _run(eng, prob, ctx, acts_d, eps_d, 3)
        for flavour in (1, 2):
            r, t = _run(eng, prob, ctx, acts_d, eps_d, flavour)
            np.testing.assert_array_equal(r, r3, err_msg="%s, flavour %d" % (name, flavour))
            np.testing.assert_array_equal(t, t3, err_msg="%s, flavour %d" % (name, flavour))
        plan = eng.cem_plan(*[eng._t(a) for a in args], 64, seed=2, call=1)
        out[name] = (r3, t3, plan.cpu().numpy())
        eng.close()
    assert np.isfinite(out["this"][2]).all()
    if "parent" in out:
        for a, b in zip(out["this"], out["parent"]):
            np.testing.assert_array_equal(a, b)
