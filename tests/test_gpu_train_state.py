"""The fused training step's state ACROSS calls: a step's result must not depend on what the engine did before it.

`fit` configures with max_batch = 0 (the workspace is allocated and grown inside steps), ends every epoch on a partial batch, follows
it with a validation step larger than the training batch, and from step 2 on reads packed weight streams that dw_adam_kernel's
epilogue keeps current.  A training step is bit-reproducible across engines and kernel flavours, so an engine WITH a history is
held to a FRESH engine in the same state, bit for bit (np.testing.assert_array_equal), and the result is anchored to the fp64
oracle with the bars the suite already has (gradients: `_check_gradients`; losses: rtol = atol = 5e-5), so that "both wrong the
same way" is excluded.

Two observables make the comparison exact: with beta1 = 0 Adam's first moment after a step IS that step's gradient, whatever the
moments were before (`dev_read_adam_moment`); with learning_rate = 0 the weights do not move."""
import numpy as np
import pytest
import torch

from cadm_amd import synth
from helpers import CWD, WD, _cfg, _check_gradients, _dev_batch, _dev_engine, make_engine
from oracle import train as otrain

pytestmark = pytest.mark.gpu

HALFCHEETAH = ("halfcheetah", 3, (200,) * 4, (256, 128, 64))      # E * G < 8: both XCD mappings of the chain kernel are reachable
PENDULUM = ("pendulum", 2, (128,) * 2, (64,))                     # D = 3: Dp / K0p / Cp all padded
CARTPOLE = ("cartpole", 7, (136,) * 2, (72, 36))                  # widths multiples of 4, not of 16: tail tiles in both streams
BOTH = [HALFCHEETAH, PENDULUM]
LARGE = 4 + 16 + 64          # the large-batch plan forced: split forward, one pass of the summed context gradient
JOINT = 8 + 32 + 128         # the joint plan forced
NETS = {"ff_model": "ff", "backward_model": "back", "context_model": "cp"}
_ids = lambda v: v[0] if isinstance(v, tuple) else str(v)


def _problem(shape, seed):
    """(problem, weight decays, context weight decays, oracle cfg) of one model shape: context + backward model."""
    env, E, hid, cph = shape
    prob = synth.make_problem(env=env, context=True, E=E, hidden_sizes=hid, cp_hidden_sizes=cph, trained_like=True, with_back=True,
                              seed=seed)
    wd, cwd = WD[:len(hid)] + (WD[-1],), CWD[:len(cph)] + (CWD[-1],)
    cfg = dict(deterministic=False, back_coeff=0.5, weight_decay_coeff=1.0, weight_decays=wd, context_weight_decays=cwd,
               n_hidden=len(hid), n_cp_hidden=len(cph))
    return prob, wd, cwd, cfg


def _engine(prob, wd, cwd, lr, max_batch, flavour=0, dev=True, **adam):
    eng = _dev_engine(prob, prob["E"]) if dev else make_engine(prob, p=prob["E"])
    if flavour:
        _set_flavour(eng, flavour)
    eng.train_configure(lr, wd, cwd, 1.0, 0.5, max_batch=max_batch, **adam)
    return eng


def _set_flavour(eng, flavour):
    eng._check(eng.lib.cadm_dev_set_train_flavour(eng._ctx, flavour), "cadm_dev_set_train_flavour")


def _step(eng, batch, train=True):
    return eng.train_step(_dev_batch(eng, batch, True, True), train=train).cpu().numpy()


def _weights(eng):
    return {(n, k): v.cpu().numpy() for n in eng.net_names() for k, v in eng.nets[n].items()}


def _moments(eng, second=False):
    """Adam's first / second moment of every trained tensor of every net (the backward model's logvar bounds are never trained and
    have no slot: dynamics.py:213-240).  After a step with beta1 = 0 the first moments are that step's gradient."""
    return {(n, k): eng.dev_read_adam_moment(n, k, second=second).cpu().numpy() for n in eng.net_names() for k in eng.nets[n]
            if not (n == "backward_model" and k in ("max_logvar", "min_logvar"))}


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg="%s %s/%s" % ((what,) + key))


def _with_weights_of(prob, eng):
    """The problem with the engine's CURRENT weights (what a fresh twin is built from)."""
    prob2 = dict(prob)
    for net, key in NETS.items():
        prob2[key] = {k: v.cpu().numpy() for k, v in eng.nets[net].items()}
    return prob2


def _twin_step(prob, wd, cwd, lr, batch, flavour=0, train=True, **adam):
    """A fresh developer-library engine on `prob`, configured for exactly this batch, stepped once: (losses, first moments)."""
    twin = _engine(prob, wd, cwd, lr, batch["obs"].shape[1], flavour, **adam)
    losses = _step(twin, batch, train)
    grad = _moments(twin) if train else None
    twin.close()
    return losses, grad


def _oracle(prob, cfg, batch, grads=True):
    """(losses [mse, back_mse, recon], gradients of every net or None) of the fp64 oracle at the problem's weights."""
    nets = {net: otrain.to_torch(prob[key], torch.float64, grads) for net, key in NETS.items()}
    st = otrain.to_torch(prob["stats"], torch.float64)
    tb = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    out = otrain.train_losses(prob["env"], nets["ff_model"], nets["backward_model"], nets["context_model"], st, tb, cfg)
    losses = np.array([float(out["mse"].detach()), float(out["back_mse"].detach()), float(out["recon"].detach())])
    return losses, (otrain.grads_of(out["loss"], nets) if grads else None)


def _anchor(eng, prob, cfg, batch, losses, before, what):
    """The history engine's last step against fp64: losses at 5e-5, every gradient at `_check_gradients`' bars, and the variables the
    oracle reports without a gradient did not move."""
    want, grads = _oracle(prob, cfg, batch)
    print("%s: losses %r, fp64 oracle %r" % (what, losses.tolist(), want.tolist()))
    np.testing.assert_allclose(losses, want, rtol=5e-5, atol=5e-5, err_msg=what)
    assert _check_gradients(eng, grads, what) >= 8
    after = _weights(eng)
    for (n, k), w0 in before.items():
        if grads[n][k] is None:
            np.testing.assert_array_equal(after[(n, k)], w0, err_msg="%s %s/%s moved although it has no gradient" % (what, n, k))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. / 7.  the batch size goes down and up on one workspace (B is the member stride of every workspace tensor: stale data of the
#          previous B lies scrambled under the current one; B % 32 selects dw_adam_kernel's load path), with and without predictions
#          in between (cadm_predict shares forward_nets, the workspace and the input echoes with the step)
# ------------------------------------------------------------------------------------------------------------------------------
def _down_and_up(shape, flavour, predict):
    prob, wd, cwd, cfg = _problem(shape, 81)
    eng = _engine(prob, wd, cwd, 0.0, 96, flavour, beta1=0.0)
    start = _weights(eng)
    pred_B = [200] + [5] * 4          # the first prediction outgrows the configured workspace: reallocation in front of step 1
    for i, B in enumerate((96, 37, 1, 96, 37)):
        if predict:
            pb = synth.make_train_batch(prob, B=pred_B[i], seed=120 + i)
            got = eng.predict_heads(pb["obs"], pb["act"], pb["cp_obs"], pb["cp_act"])
            fresh = _dev_engine(prob, prob["E"])
            if flavour:
                _set_flavour(fresh, flavour)
            want = fresh.predict_heads(pb["obs"], pb["act"], pb["cp_obs"], pb["cp_act"])
            for g, w, name in zip(got, want, ("mu", "logvar")):
                np.testing.assert_array_equal(g.cpu().numpy(), w.cpu().numpy(), err_msg="prediction %d (B = %d) %s" % (i, pred_B[i], name))
            fresh.close()
        batch = synth.make_train_batch(prob, B=B, seed=100 + i)
        losses = _step(eng, batch)
        if i in (2, 4):               # after the single row and after the second ragged batch
            what = "%s flavour %d step %d (B = %d)" % (shape[0], flavour, i, B)
            t_losses, t_grad = _twin_step(prob, wd, cwd, 0.0, batch, flavour, beta1=0.0)
            np.testing.assert_array_equal(losses, t_losses, err_msg=what)
            _same(_moments(eng), t_grad, what + " gradient")
            _anchor(eng, prob, cfg, batch, losses, start, what)
    _same(_weights(eng), start, "lr = 0: weights")
    eng.close()


@pytest.mark.parametrize("flavour", [0, 8, 4, LARGE])
@pytest.mark.parametrize("shape", BOTH, ids=_ids)
def test_batch_size_down_and_up_on_one_workspace(gpu, shape, flavour):
    _down_and_up(shape, flavour, predict=False)


@pytest.mark.parametrize("flavour", [0, LARGE])
@pytest.mark.parametrize("shape", BOTH, ids=_ids)
def test_predictions_between_training_steps(gpu, shape, flavour):
    _down_and_up(shape, flavour, predict=True)


# ------------------------------------------------------------------------------------------------------------------------------
# 2.  the workspace is allocated and grown inside steps, as `fit` does it (max_batch = 0): hipFree / hipMalloc between queued launches,
#     every NetBufs pointer changes, the stage table is rebuilt and uploaded again, the loss reduction's arrival counter re-cleared
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BOTH, ids=_ids)
def test_workspace_grows_mid_run(gpu, shape):
    """Real Adam steps (lr 1e-3, beta1 = 0), so the chains also read streams that Adam has kept current across the reallocations:
    the twin of every step is built from the weights the history engine holds in front of it.  The validation steps have the size
    of the batch behind them, as in `fit` (they are what makes the workspace grow there)."""
    prob, wd, cwd, cfg = _problem(shape, 82)
    eng = _engine(prob, wd, cwd, 1e-3, 0, beta1=0.0)
    plan = [(37, True), (96, True), (200, False), (200, True), (16, True), (200, False)]
    last_train = max(i for i, (_, train) in enumerate(plan) if train)
    for i, (B, train) in enumerate(plan):
        what = "%s step %d (B = %d, train = %d)" % (shape[0], i, B, train)
        batch = synth.make_train_batch(prob, B=B, seed=200 + i)
        now = _with_weights_of(prob, eng)
        before = _weights(eng)
        losses = _step(eng, batch, train)
        t_losses, t_grad = _twin_step(now, wd, cwd, 1e-3, batch, train=train, beta1=0.0)
        np.testing.assert_array_equal(losses, t_losses, err_msg=what)
        if i == last_train:
            _same(_moments(eng), t_grad, what + " gradient")
            _anchor(eng, now, cfg, batch, losses, before, what)
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 3.  the launch plan changes between steps on one engine (a validation set of >= 1856 rows does that inside `fit`)
# ------------------------------------------------------------------------------------------------------------------------------
def test_launch_plan_changes_between_steps(gpu):
    prob, wd, cwd, _ = _problem(HALFCHEETAH, 83)
    eng = _engine(prob, wd, cwd, 0.0, 96, JOINT, beta1=0.0)
    batches = [synth.make_train_batch(prob, B=96, seed=300 + i) for i in range(3)]
    _step(eng, batches[0])
    for i, fl in ((1, LARGE), (2, JOINT)):
        _set_flavour(eng, fl)
        losses = _step(eng, batches[i])
        t_losses, t_grad = _twin_step(prob, wd, cwd, 0.0, batches[i], fl, beta1=0.0)      # only ever ran this flavour on this batch
        np.testing.assert_array_equal(losses, t_losses, err_msg="flavour %d behind the other plan" % fl)
        _same(_moments(eng), t_grad, "flavour %d behind the other plan: gradient" % fl)
    eng.close()
    # the two plans are told apart: on one batch their gradients differ in at least one bit
    g = [_twin_step(prob, wd, cwd, 0.0, batches[1], fl, beta1=0.0)[1] for fl in (JOINT, LARGE)]
    assert not all(np.array_equal(g[0][key], g[1][key]) for key in g[0]), "the forced plans agree bit for bit -- nothing is being told apart"


# ------------------------------------------------------------------------------------------------------------------------------
# 4.  from step 2 on the chains read the streams dw_adam_kernel's epilogue keeps current, not what train_pack_kernel builds from
#     the master weights: the two must be the same streams
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", [0, LARGE])
@pytest.mark.parametrize("shape", BOTH + [CARTPOLE], ids=_ids)
def test_adam_keeps_the_packed_streams_current(gpu, shape, flavour):
    """Three Adam steps, B = 96 / 37 / 96 (both load paths of dw_adam_kernel write the streams), then a fresh twin from the weights:
    its streams come from train_pack_kernel.  Every reader of the streams must give the same bits on both: predict_heads and an
    evaluation step (forward streams), then a fourth training step (forward and transposed streams: losses and gradient).  The
    training step comes last -- it moves the two engines' weights apart (their second moments differ)."""
    prob, wd, cwd, cfg = _problem(shape, 84)
    eng = _engine(prob, wd, cwd, 1e-3, 96, flavour, beta1=0.0)
    for i, B in enumerate((96, 37, 96)):
        _step(eng, synth.make_train_batch(prob, B=B, seed=400 + i))
    now = _with_weights_of(prob, eng)
    before = _weights(eng)
    twin = _engine(now, wd, cwd, 1e-3, 96, flavour, beta1=0.0)
    what = "%s flavour %d" % (shape[0], flavour)
    pb = synth.make_train_batch(prob, B=37, seed=405)
    for g, w, name in zip(eng.predict_heads(pb["obs"], pb["act"], pb["cp_obs"], pb["cp_act"]),
                          twin.predict_heads(pb["obs"], pb["act"], pb["cp_obs"], pb["cp_act"]), ("mu", "logvar")):
        np.testing.assert_array_equal(g.cpu().numpy(), w.cpu().numpy(), err_msg="%s predict_heads %s" % (what, name))
    ev = synth.make_train_batch(prob, B=96, seed=404)
    np.testing.assert_array_equal(_step(eng, ev, train=False), _step(twin, ev, train=False), err_msg=what + " evaluation step")
    batch = synth.make_train_batch(prob, B=37, seed=403)
    losses = _step(eng, batch)
    np.testing.assert_array_equal(losses, _step(twin, batch), err_msg=what + " fourth step")
    _same(_moments(eng), _moments(twin), what + " fourth step: gradient")
    _anchor(eng, now, cfg, batch, losses, before, what + " fourth step")
    twin.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 5.  train_reset: zero moments, step counter (and with it lr_t) back to the start
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BOTH, ids=_ids)
def test_train_reset_restarts_adam(gpu, shape):
    prob, wd, cwd, _ = _problem(shape, 85)
    eng = _engine(prob, wd, cwd, 1e-3, 96)                       # default betas
    for i, B in enumerate((96, 37, 96)):
        _step(eng, synth.make_train_batch(prob, B=B, seed=500 + i))
    assert max(np.abs(m).max() for m in _moments(eng).values()) > 0.0
    eng.train_reset()
    twin = _engine(_with_weights_of(prob, eng), wd, cwd, 1e-3, 96)
    for i, B in enumerate((37, 96)):                             # the second step: lr_t of t = 2, not of t = 5
        what = "%s step %d behind the reset" % (shape[0], i + 1)
        batch = synth.make_train_batch(prob, B=B, seed=510 + i)
        np.testing.assert_array_equal(_step(eng, batch), _step(twin, batch), err_msg=what)
        _same(_weights(eng), _weights(twin), what + ": weights")
        _same(_moments(eng), _moments(twin), what + ": first moments")
        _same(_moments(eng, second=True), _moments(twin, second=True), what + ": second moments")
    twin.close()
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 6.  weights reloaded into an engine that has trained: the training chains' streams follow (cadm_repack: train_packs_stale)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BOTH, ids=_ids)
def test_reloaded_weights_reach_the_training_streams(gpu, shape):
    prob, wd, cwd, _ = _problem(shape, 86)
    other = dict(prob)
    for key in NETS.values():
        other[key] = _problem(shape, 87)[0][key]                 # another seed's weights, this problem's statistics
    eng = _engine(prob, wd, cwd, 1e-3, 96, beta1=0.0)
    for i, B in enumerate((96, 37)):
        _step(eng, synth.make_train_batch(prob, B=B, seed=600 + i))
    for net, key in NETS.items():
        for name, t in eng.nets[net].items():
            t.copy_(eng._t(other[key][name]))
    eng.repack()
    batch = synth.make_train_batch(prob, B=37, seed=602)
    losses = _step(eng, batch)
    t_losses, t_grad = _twin_step(other, wd, cwd, 1e-3, batch, beta1=0.0)
    np.testing.assert_array_equal(losses, t_losses, err_msg=shape[0])
    _same(_moments(eng), t_grad, shape[0] + " gradient")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 8.  train_step_rows the way `fit` calls it: idx a column slice of [E, n_train] (idx_ld > B), the epoch's last batch one row
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", [None, LARGE])      # the product's launch plan / the large-batch plan forced (developer library)
def test_train_step_rows_on_column_slices_with_a_one_row_tail(gpu, flavour):
    env, E, B, N, F, Hh = "halfcheetah", 5, 48, 40, 3, 10
    prob = synth.make_problem(env=env, context=True, E=E, trained_like=True, with_back=True, seed=41)
    r = np.random.default_rng(5)
    D, A = 18, 6
    ds = dict(obs=r.standard_normal((N, F * D)), act=r.standard_normal((N, F * A)), delta=r.standard_normal((N, F * D)),
              obs_next=r.standard_normal((N, F * D)), back_delta=r.standard_normal((N, F * D)),
              cp_obs=0.1 * r.standard_normal((N, D * Hh)), cp_act=r.uniform(-1, 1, (N, A * Hh)))
    fb = r.uniform(size=(N, F)) < 0.8
    w, f = np.nonzero(fb)
    idx_all = r.integers(0, w.shape[0], size=(E, 2 * B + 1))
    results = []
    for mode in ("rows", "gathered"):
        eng = make_engine(prob, p=E) if flavour is None else _dev_engine(prob, E)
        if flavour is not None:
            _set_flavour(eng, flavour)
        eng.train_configure(1e-3, WD, CWD, 1.0, 0.5, max_batch=B)
        dev = {k: eng._t(v) for k, v in ds.items()}
        tw, tf_, ti_all = (torch.as_tensor(x, device=eng.device) for x in (w, f, idx_all))
        losses = []
        for lo, hi in ((0, B), (B, 2 * B), (2 * B, 2 * B + 1)):
            ti = ti_all[:, lo:hi]
            assert ti.stride(0) > ti.shape[1] and ti.stride(0) == 2 * B + 1      # a strided view: idx_ld > B reaches the kernels
            if mode == "rows":
                losses.append(eng.train_step_rows(dev, F, tw, tf_, ti, train=True))
            else:
                ww, ff = tw[ti], tf_[ti]
                batch = {k: dev[k].view(N, F, -1)[ww, ff] for k in ("obs", "act", "delta", "obs_next", "back_delta")}
                batch["cp_obs"], batch["cp_act"] = dev["cp_obs"][ww], dev["cp_act"][ww]
                losses.append(eng.train_step({k: v.contiguous() for k, v in batch.items()}, train=True))
        results.append((torch.stack(losses).cpu().numpy(), _weights(eng)))
        eng.close()
    np.testing.assert_array_equal(results[0][0], results[1][0])
    _same(results[0][1], results[1][1], "final weights")


# ------------------------------------------------------------------------------------------------------------------------------
# 9.  evaluation on the split large-batch forward: the loss partials' in-launch hand-off across TWO launches
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [96, 37])
def test_eval_hand_off_on_the_split_forward(gpu, B):
    """tests/test_gpu_train.py: test_eval_losses_equal_the_training_steps_reduction with the split forward forced (+ 16: one launch
    per net, the last-arriving workgroup of either takes the sums): two very different batches alternate in back-to-back evaluation
    steps without a sync between them; each equals the loss the lr = 0 training step reports (same partials, handed over at the kernel
    boundary), to fp32 reduction-order roundoff."""
    env, E, rounds = "halfcheetah", 5, 40
    prob = synth.make_problem(env=env, context=True, E=E, trained_like=True, with_back=True, seed=61)
    eng = _dev_engine(prob, E)
    _set_flavour(eng, 16)
    eng.train_configure(0.0, WD, CWD, 1.0, 0.5, max_batch=B)
    b1 = synth.make_train_batch(prob, B=B, seed=8)
    b2 = synth.make_train_batch(prob, B=B, seed=9)
    for k in ("delta", "back_delta"):
        b2[k] = 7.0 * b2[k]
    devs = [_dev_batch(eng, b, True, True) for b in (b1, b2)]
    want = [eng.train_step(d, train=True).cpu().numpy() for d in devs]          # reduction across the kernel boundary
    assert abs(want[0][2] - want[1][2]) > 0.5 * abs(want[0][2])                  # the two batches are told apart easily
    outs = []
    for r in range(rounds):
        outs.append(eng.train_step(devs[r & 1], train=False))                    # no sync in between: back-to-back launches
    outs = torch.stack(outs).cpu().numpy()
    for r in range(rounds):
        np.testing.assert_allclose(outs[r], want[r & 1], rtol=3e-6, atol=0, err_msg="evaluation step %d" % r)
    again = [eng.train_step(d, train=True).cpu().numpy() for d in devs]
    for w, a in zip(want, again):
        np.testing.assert_array_equal(w, a)                                      # lr = 0: nothing moved, the reduction is deterministic
    eng.close()


def test_eval_where_the_launcher_splits_on_its_own(gpu):
    """Product library, 5 members + backward model, B = 1856: the launcher's own switch to the split forward (what a validation set
    of that many rows takes).  Then B = 64 on the same engine: back to the joint launch, the arrival counter reused."""
    E = 5
    prob = synth.make_problem(env="halfcheetah", context=True, E=E, trained_like=True, with_back=True, seed=62)
    cfg = _cfg(prob, False, 0.5)
    eng = make_engine(prob, p=E)
    eng.train_configure(0.0, WD, CWD, 1.0, 0.5, max_batch=1856)
    for B, seed in ((1856, 10), (64, 11)):
        batch = synth.make_train_batch(prob, B=B, seed=seed)
        dev = _dev_batch(eng, batch, True, True)
        got = eng.train_step(dev, train=False).cpu().numpy()
        want = _oracle(prob, cfg, batch, grads=False)[0]
        print("B = %d: evaluation losses %r, fp64 oracle %r" % (B, got.tolist(), want.tolist()))
        np.testing.assert_allclose(got, want, rtol=5e-5, atol=5e-5, err_msg="B = %d evaluation vs fp64" % B)
        if B == 1856:
            trained = eng.train_step(dev, train=True).cpu().numpy()              # lr = 0
            np.testing.assert_allclose(got, trained, rtol=3e-6, atol=0, err_msg="evaluation vs the training step's reduction")
    eng.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 10.  class level: a `fit` whose shapes hit all of the above, replayed step by step through a second engine
# ------------------------------------------------------------------------------------------------------------------------------
def test_fit_equals_its_replay_on_a_preallocated_engine(gpu):
    """`fit` (max_batch = 0, rows addressed through strided index slices, a one-row batch at the end of every epoch, a validation batch
    larger than the training batch: the workspace grows mid-fit) against the same feeds -- oracle.train.fit_feed_sequence on the
    recorded draws -- gathered on the host and stepped through an engine that was configured once for the largest batch: per-step
    training losses, per-epoch validation losses and the final weights of every net, bit for bit (rows == gathered is pinned bitwise
    by tests/test_gpu_train.py).  The oracle comparison of the same run is tests/test_gpu_fit.py's."""
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import (FitIndexStream, MLPEnsembleCEMDynamicsModel, RecordingIndexStream,
                                                                  ReplayIndexStream)
    from cadm_amd.engine import STAT_KEYS
    from cadm_amd.envs import make_env_spec
    from oracle import envs as oenvs
    E, bs, epochs, N, ratio, D, A, Hh, F = 5, 40, 2, 14, 0.36, 18, 6, 10, 10
    model = MLPEnsembleCEMDynamicsModel("dyn", make_env_spec("halfcheetah"), hidden_nonlinearity="swish", batch_size=bs,
                                        n_forwards=5, n_candidates=64, ensemble_size=E, n_particles=5, use_cem=True,
                                        weight_decays=WD, weight_decay_coeff=1.0, context_weight_decays=CWD, state_diff=1,
                                        back_coeff=0.5, normalize_input=True, valid_split_ratio=ratio, seed=4)
    eng = model.engine
    start = {net: {k: v.detach().cpu().numpy().copy() for k, v in eng.nets[net].items()} for net in eng.net_names()}
    rng = np.random.default_rng(3)
    obs = rng.standard_normal((N, F * D))
    fb = np.ones((N, F))
    fb[np.arange(N), rng.integers(1, F, N)] = 0          # ragged futures, the same number of rows (F - 1) in every window
    data = dict(obs=obs, act=rng.uniform(-1, 1, (N, F * A)), obs_next=obs + 0.05 * rng.standard_normal((N, F * D)),
                cp_obs=0.1 * rng.standard_normal((N, D * Hh)), cp_act=rng.uniform(-1, 1, (N, A * Hh)), future_bool=fb)
    n_valid = int(N * ratio)
    n_train, n_valid_rows = (N - n_valid) * (F - 1), n_valid * (F - 1)
    assert n_train % bs == 1 and n_valid_rows > bs          # a one-row tail; the validation step outgrows the training workspace
    rec = RecordingIndexStream(FitIndexStream(np.random.default_rng(9)))
    model.fit(epochs=epochs, index_stream=rec, **data)
    got_train = np.concatenate(model.last_fit_trace["train"])
    got_valid = np.asarray(model.last_fit_trace["valid"], np.float32)
    assert [k for k, _ in rec.log] == ["permutation", "bootstrap"] + ["epoch_order"] * epochs
    assert got_train.shape == (epochs * (n_train // bs + 1), 3) and got_valid.shape == (epochs, 3)

    stats, feeds = otrain.fit_feed_sequence(oenvs.make_env("halfcheetah"), data, ReplayIndexStream(rec.log), E, epochs, bs,
                                            valid_split_ratio=ratio)
    assert [b["obs"].shape[1] for b in feeds[0][0]] == [bs] * (n_train // bs) + [1] and feeds[0][1]["obs"].shape[1] == n_valid_rows
    prob = dict(env="halfcheetah", E=E, D=D, A=A, P=18, C=10, H=5, Hh=Hh, discrete=False, hidden_sizes=(200,) * 4,
                cp_hidden_sizes=(256, 128, 64), ff=start["ff_model"], cp=start["context_model"], back=start["backward_model"],
                stats=dict(zip(STAT_KEYS, model.get_normalization_stats())))
    rep = make_engine(prob, p=5)
    rep.train_configure(1e-3, WD, CWD, 1.0, 0.5, max_batch=max(bs, n_valid_rows))
    rep_train, rep_valid = [], []
    for batches, vb in feeds:
        for b in batches:
            rep_train.append(rep.train_step(_dev_batch(rep, b, True, True), train=True))
        rep_valid.append(rep.train_step(_dev_batch(rep, vb, True, True), train=False))
    np.testing.assert_array_equal(got_train, torch.stack(rep_train).cpu().numpy())
    np.testing.assert_array_equal(got_valid, torch.stack(rep_valid).cpu().numpy())
    _same(_weights(eng), _weights(rep), "final weights")
    rep.close()
