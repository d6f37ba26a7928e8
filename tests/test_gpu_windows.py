"""SURVEY.md 8f-2 on the device: `cadm_build_windows` / the drop-in ModelSampleProcessor against golden vectors produced by
the reference's own `process_samples` (tests/golden/make_f2_golden.py) and against the (pinned) oracle restatement on a
larger ragged batch.  Index / byte work: bit-exact, for float64 (the reference's dtype) and float32."""
import os

import numpy as np
import pytest
import torch

from cadm_amd.samplers import ModelSampleProcessor
from oracle import windows as ow

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "f2_windows.npz"))
CASES = sorted({k.split("/")[0] for k in GOLD.files})
KEYS = ("concat_obs", "concat_act", "concat_next_obs", "concat_bool", "cp_observations", "cp_actions", "observations",
        "next_observations", "actions", "timesteps", "rewards")


def paths_of(case, dtype=np.float64):
    D, A, Hh, F = (int(v) for v in GOLD[case + "/meta"])
    lengths = GOLD[case + "/lengths"]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    return [{k: GOLD[case + "/in/" + k][offs[i]:offs[i + 1]].astype(dtype) for k in ("observations", "actions", "cp_obs", "cp_act", "rewards")}
            for i in range(len(lengths))], F


@pytest.mark.parametrize("case", CASES)
def test_device_windows_equal_the_reference_golden(gpu, case):
    paths, F = paths_of(case)
    got = ModelSampleProcessor(context=True, future_length=F).process_samples(paths)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], GOLD[case + "/out/" + k], err_msg="%s/%s" % (case, k))
    np.testing.assert_allclose(got["returns"], GOLD[case + "/out/returns"], rtol=1e-15, atol=0)
    # the reference leaves its zero padding in the caller's path dicts (:64-68)
    for p, L in zip(paths, GOLD[case + "/lengths"]):
        assert len(p["observations"]) == max(int(L), F + 1)


def test_device_windows_large_ragged_batch_float32_and_device_output(gpu):
    rng = np.random.default_rng(5)
    D, A, Hh, F = 18, 6, 10, 10
    lengths = list(rng.integers(1, 201, size=64)) + [1, 2, 11, 200]
    paths = [dict(observations=rng.standard_normal((L, D)).astype(np.float32), actions=rng.uniform(-1, 1, (L, A)).astype(np.float32),
                  rewards=rng.standard_normal(L), cp_obs=rng.standard_normal((L, D * Hh)).astype(np.float32),
                  cp_act=rng.uniform(-1, 1, (L, A * Hh)).astype(np.float32)) for L in lengths]
    ref = ow.process_samples([{k: np.asarray(v, np.float64) for k, v in p.items()} for p in paths], F)
    dev = ModelSampleProcessor(context=True, future_length=F).process_samples([dict(p) for p in paths], as_device=True)
    for k in ("concat_obs", "concat_act", "concat_next_obs", "concat_bool", "cp_observations", "cp_actions"):
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda and dev[k].dtype == torch.float32
        np.testing.assert_array_equal(dev[k].cpu().numpy().astype(np.float64), ref[k], err_msg=k)
    assert dev["concat_obs"].shape[0] == int(np.sum(np.maximum(lengths, F + 1) - 1))
    # empty-history model (vanilla shape: Hh = 0 columns) goes through the same kernel
    for p in paths:
        p["cp_obs"], p["cp_act"] = p["cp_obs"][:, :0], p["cp_act"][:, :0]
    out = ModelSampleProcessor(context=True, future_length=F).process_samples(paths)
    np.testing.assert_array_equal(out["concat_obs"].astype(np.float64), ref["concat_obs"])
    assert out["cp_observations"].shape == (ref["concat_obs"].shape[0], 0)


# ------------------------------------------------------------------------------------------------ the hand-off into fit
def test_device_windows_go_into_fit_as_the_numpy_ones_do(gpu):
    """process_samples(as_device=True) -> fit against process_samples() -> fit on a twin, under one recorded index stream, 2 epochs:
    the loss traces, the twelve statistic vectors and every weight are the same bits.  (float32 paths: the device tensors hold the
    values the float64 numpy output holds, and `fit` brings them to the host as float64.)"""
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import FitIndexStream, RecordingIndexStream, ReplayIndexStream
    from test_gpu_model import CaDMModel, _cadm_kwargs
    rng = np.random.default_rng(21)
    D, A, Hh, F = 18, 6, 10, 10
    paths = [dict(observations=rng.standard_normal((L, D)).astype(np.float32), actions=rng.uniform(-1, 1, (L, A)).astype(np.float32),
                  rewards=rng.standard_normal(L), cp_obs=(0.1 * rng.standard_normal((L, D * Hh))).astype(np.float32),
                  cp_act=rng.uniform(-1, 1, (L, A * Hh)).astype(np.float32)) for L in (30, 45, 12, 3)]
    proc = ModelSampleProcessor(context=True, future_length=F)
    host = proc.process_samples([dict(p) for p in paths])
    dev = proc.process_samples([dict(p) for p in paths], as_device=True)
    keys = ("concat_obs", "concat_act", "concat_next_obs", "cp_observations", "cp_actions", "concat_bool")
    for k in keys:
        assert isinstance(host[k], np.ndarray) and host[k].dtype == np.float64
        assert isinstance(dev[k], torch.Tensor) and dev[k].is_cuda and dev[k].dtype == torch.float32
        np.testing.assert_array_equal(dev[k].cpu().numpy().astype(np.float64), host[k], err_msg=k)
    a, b = CaDMModel(**_cadm_kwargs()), CaDMModel(**_cadm_kwargs())
    rec = RecordingIndexStream(FitIndexStream(np.random.default_rng(3)))
    a.fit(*[host[k] for k in keys], epochs=2, index_stream=rec)
    b.fit(*[dev[k] for k in keys], epochs=2, index_stream=ReplayIndexStream(rec.log))
    assert host["concat_obs"].shape[0] == 29 + 44 + 11 + 10 == a._dataset["obs"].shape[0] == b._dataset["obs"].shape[0]
    ta, tb = a.last_fit_trace, b.last_fit_trace
    assert len(ta["train"]) == len(tb["train"]) == 2 and len(ta["valid"]) == len(tb["valid"]) == 2
    for x, y in zip(ta["train"] + ta["valid"], tb["train"] + tb["valid"]):
        x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
        assert np.isfinite(x).all() and x.size > 0
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    sa, sb = a._stats12(), b._stats12()
    assert len(sa) == len(sb) == 12
    for x, y in zip(sa, sb):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        np.testing.assert_array_equal(x.view(np.uint64), y.view(np.uint64))
    n = 0
    for net in a.engine.net_names():
        for name, w in a.engine.nets[net].items():
            np.testing.assert_array_equal(w.cpu().numpy().view(np.uint32), b.engine.nets[net][name].cpu().numpy().view(np.uint32),
                                          err_msg="%s/%s" % (net, name))
            n += 1
    assert n >= 8 + 12 + 12      # context, forward and backward nets


# ------------------------------------------------------------------------------------------------ three corners of the kernel
SHAPES = [(3, 1, 1), (5, 2, 3), (18, 6, 10)]      # D, A, Hh
CORNERS = {  # F, dtype, path lengths
    "f1": (1, np.float32, (1, 2, 5, 9, 2)),                     # the concat_bool cut can never fire: only a path's row 0 is zero
    "len1": (4, np.float32, (1,) * 6),                          # every path is one recorded step and F zero-padded ones
    "f64_ragged": (4, np.float64, tuple(int(v) for v in np.random.default_rng(9).integers(1, 24, size=40))),
}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%dA%dHh%d" % s)
@pytest.mark.parametrize("corner", sorted(CORNERS))
def test_device_windows_corners_equal_the_oracle(gpu, corner, shape):
    D, A, Hh = shape
    F, dtype, lengths = CORNERS[corner]
    rng = np.random.default_rng(31)
    paths = [dict(observations=rng.standard_normal((L, D)).astype(dtype), actions=rng.uniform(-1, 1, (L, A)).astype(dtype),
                  rewards=rng.standard_normal(L), cp_obs=rng.standard_normal((L, D * Hh)).astype(dtype),
                  cp_act=rng.uniform(-1, 1, (L, A * Hh)).astype(dtype)) for L in lengths]
    ref = ow.process_samples([{k: np.asarray(v, np.float64) for k, v in p.items()} for p in paths], F)
    proc = ModelSampleProcessor(context=True, future_length=F)
    host = proc.process_samples([dict(p) for p in paths])
    dev = proc.process_samples([dict(p) for p in paths], as_device=True)
    rows = np.maximum(np.array(lengths), F + 1) - 1
    for k in ("concat_obs", "concat_act", "concat_next_obs", "concat_bool", "cp_observations", "cp_actions"):
        assert host[k].dtype == np.float64 and host[k].shape == ref[k].shape and host[k].shape[0] == rows.sum()
        np.testing.assert_array_equal(host[k].view(np.uint64), ref[k].view(np.uint64), err_msg=k)
        assert dev[k].dtype == (torch.float32 if dtype == np.float32 else torch.float64)
        got = dev[k].cpu().numpy()
        want = ref[k].astype(dtype)
        np.testing.assert_array_equal(got.view(np.uint32 if dtype == np.float32 else np.uint64),
                                      want.view(np.uint32 if dtype == np.float32 else np.uint64), err_msg=k)
    first = np.concatenate([[0], np.cumsum(rows)[:-1]])
    if corner == "f1":
        want = np.ones((rows.sum(), 1))
        want[first] = 0
        np.testing.assert_array_equal(host["concat_bool"], want)
    if corner == "len1":      # rows = F: row 0 masked, row s > 0 keeps max(F - s - F, 0) = 0 columns -> nothing survives
        assert not host["concat_bool"].any() and not host["concat_obs"][:, D:].any()
        np.testing.assert_array_equal(host["concat_obs"][first, :D], np.concatenate([p["observations"] for p in paths]).astype(np.float64))


# ------------------------------------------------------------------------------------------------ refusals of the export
def test_build_windows_argument_checks_return_einval(gpu):
    """`cadm_build_windows` refuses an element size of 2 bytes, F = 0, D = 0, a null output and a null history input with Dh > 0 with
    CADM_EINVAL and its own message, before any launch: the outputs keep their sentinel.  N = 0 is legal and writes nothing."""
    import ctypes as ct
    from cadm_amd import _lib
    lib = _lib.load()
    D, A, Dh, Ah, F, L = 3, 2, 6, 4, 2, 5
    N = L - 1
    f = lambda n, v: torch.full((n,), v, dtype=torch.float32, device=gpu)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=gpu)
    obs, act, cpo, cpa = f(L * D, 1.0), f(L * A, 2.0), f(L * Dh, 3.0), f(L * Ah, 4.0)
    off, rp, rs = i32([0, L]), i32([0] * N), i32(list(range(N)))
    outs = dict(co=f(N * F * D, 9.0), ca=f(N * F * A, 9.0), cn=f(N * F * D, 9.0), cb=f(N * F, 9.0), ho=f(N * Dh, 9.0), ha=f(N * Ah, 9.0))
    P = lambda x: None if x is None else ct.c_void_p(x.data_ptr())

    def call(elem=4, D=D, F=F, N=N, cpo=cpo, **over):
        o = dict(outs, **over)
        return lib.cadm_build_windows(P(obs), P(act), P(cpo), P(cpa), elem, D, A, Dh, Ah, P(off), P(rp), P(rs), N, F, P(o["co"]), P(o["ca"]),
                                      P(o["cn"]), P(o["cb"]), P(o["ho"]), P(o["ha"]), None)

    def untouched():
        torch.cuda.synchronize()
        for k, v in outs.items():
            assert (v == 9.0).all(), "%s was written" % k

    def einval(rc, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "expected CADM_EINVAL, got %d (%s)" % (rc, msg)
        assert msg.startswith("cadm_build_windows:") and frag in msg, msg
        untouched()
    einval(call(elem=2), "elements must be 4 or 8 bytes, got 2")
    einval(call(F=0), "bad dimensions")
    einval(call(D=0), "bad dimensions")
    einval(call(cb=None), "null argument")
    einval(call(co=None), "null argument")
    einval(call(cpo=None), "history arrays missing")
    einval(call(ho=None), "history arrays missing")
    assert call(N=0) == 0
    untouched()
    assert call() == 0      # whole: the kernel runs and every output word is written
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert not (v == 9.0).any(), k
    assert (outs["cb"].cpu().numpy().reshape(N, F) == np.array([[0, 0], [1, 1], [1, 1], [1, 0]])).all()
