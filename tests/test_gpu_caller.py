"""GPU: the device-resident caller state (cadm_amd/caller.py DevicePlannerState; cadm_amd/csrc/caller.hip `cadm_warm_start_shift`,
`cadm_history_update`) against the samplers' numpy bookkeeping -- oracle/caller.py SamplerState and CEMWarmStart, both pinned to the
reference's own Sampler run by tests/test_sampler_golden.py -- on every model kind, off the one half-cheetah geometry, under every
planner route, and at the exports' refusals.  The kernels move and subtract float32 values: every comparison with a float32
reference is bit for bit."""
import ctypes as ct
import types

import numpy as np
import pytest
import torch

from cadm_amd import synth
from cadm_amd.caller import DevicePlannerState
from cadm_amd.policies.mpc_controller import CEMWarmStart, MPCController
from helpers import _np, plan_model, planner_engine
from oracle.caller import SamplerState
from test_sampler_golden import CASES, stream

pytestmark = pytest.mark.gpu


def f32(x):
    return np.ascontiguousarray(np.asarray(x, np.float32))


def same_bits(got, want, what=""):
    got, want = f32(_np(got) if isinstance(got, torch.Tensor) else got), f32(want)
    assert got.shape == want.shape, "%s: shape %r, expected %r" % (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------- A1
def _golden_model(s, case):
    """A CaDM model of the stream's shapes: the half-cheetah one as the reference's scripts build it, the others on a declared env."""
    if case == "hc_shape":
        from test_gpu_model import CaDMModel, _cadm_kwargs
        return CaDMModel(**_cadm_kwargs(normalize_input=False, n_candidates=64, n_forwards=s["H"], history_length=s["Hh"],
                                        state_diff=int(s["state_diff"])))
    from cadm_amd.env_spec import EnvDecl
    env = EnvDecl(s["D"], s["A"], preproc=["id"] * s["D"], reward=[dict(kind="linear", dim=0)])
    return _declared_model(env, s)


def _declared_model(env, s):
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDMModel
    return CaDMModel("dyn", env, hidden_sizes=(32,) * 4, hidden_nonlinearity="swish", n_forwards=s["H"], n_candidates=64, ensemble_size=5,
                     n_particles=5, use_cem=True, normalize_input=False, history_length=s["Hh"], state_diff=int(s["state_diff"]), seed=7)


@pytest.mark.parametrize("case", CASES)
def test_device_caller_kernels_reproduce_the_reference_sampler(gpu, case):
    """cadm_warm_start_shift / cadm_history_update driven with the reference run's plans and transitions, on every recorded stream.
    Warm start, actions and hist_act: the float32 cast of the recording, bit for bit; hist_obs too where the history holds raw
    observations (plain_h2).  With state differences the device subtracts float32 observations and the reference float64 ones: one rounding
    per operand and one of the difference, 3 * 2^-24 * max(|obses|, |next_obses|) of the stream (half-cheetah: never more than the
    5e-7 it was held to before).  Against a SamplerState fed the float32 casts, everything is bit for bit.
    Worst |hist_obs - float64 recording| next to its bar (float32 subtraction of the recorded values): diff_h3 5.5e-08 / 1.80e-07,
    hc_shape 9.9e-08 / 2.67e-07."""
    from cadm_amd._lib import check, ptr
    s = stream(case)
    model = _golden_model(s, case)
    dev = DevicePlannerState(model, s["n_env"])
    eng = dev.eng
    assert (eng.D, eng.A, eng.H, eng.Hh) == (s["D"], s["A"], s["H"], s["Hh"]) and bool(model.state_diff) == s["state_diff"]
    ref32 = SamplerState(s["n_env"], s["H"], s["D"], s["A"], s["Hh"], s["state_diff"])
    bar = 3.0 * 2.0 ** -24 * max(np.abs(s["obses"]).max(), np.abs(s["next_obses"]).max()) if s["state_diff"] else 0.0
    if case == "hc_shape":
        bar = min(bar, 5e-7)
    worst = 0.0
    for t in range(s["T"]):
        same_bits(dev.prev_sol, s["init_mean"][t], "prev_sol, step %d" % t)
        same_bits(dev.init_var, s["init_var"][t], "init_var, step %d" % t)
        same_bits(dev.hist_act, s["cp_act"][t], "hist_act, step %d" % t)
        ho = _np(dev.hist_obs)
        if s["state_diff"]:
            err = float(np.abs(ho.astype(np.float64) - s["cp_obs"][t]).max())
            worst = max(worst, err)
            assert err <= bar, "hist_obs, step %d: off the float64 recording by %.3e, bar %.3e" % (t, err, bar)
        else:
            same_bits(ho, s["cp_obs"][t], "hist_obs, step %d" % t)
        same_bits(ho, ref32.history_state, "hist_obs against the float32 sampler state, step %d" % t)
        same_bits(dev.prev_sol, ref32.prev_sol, "prev_sol against the float32 sampler state, step %d" % t)
        same_bits(dev.hist_act, ref32.history_act, "hist_act against the float32 sampler state, step %d" % t)
        plan = eng._t(f32(s["plans"][t]))
        check(eng.lib.cadm_warm_start_shift(eng._ctx, ptr(plan), dev.m, ptr(dev.prev_sol), ptr(dev.action), eng.stream),
              "cadm_warm_start_shift")
        same_bits(dev.action, s["actions"][t], "action, step %d" % t)
        same_bits(dev.action, ref32.after_plan(f32(s["plans"][t])), "action against the float32 sampler state, step %d" % t)
        dev.observe(f32(s["obses"][t]), f32(s["actions"][t]), f32(s["next_obses"][t]), s["dones"][t])
        ref32.after_step(f32(s["obses"][t]), f32(s["actions"][t]), f32(s["next_obses"][t]), s["dones"][t])
    np.testing.assert_array_equal(_np(dev.counts), np.array(ref32.state_counts, np.int32))
    print("%s: worst |hist_obs - float64 recording| %.3e, bar %.3e" % (case, worst, bar))


# ---------------------------------------------------------------------------------------------------------------------- A2
class _CountingLib:
    """The engine's library with every cadm_* call it is asked for written down."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("cadm_"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def test_vanilla_model_end_to_end(gpu):
    """A model without a history window through DevicePlannerState: the action is get_action's first step from the samplers' warm
    start under the same call counter, and a finished env's warm start is zero before its next plan (sampler.py:193-195 resets it with
    or without a context) -- by `observe` itself: `cadm_history_update` refuses such a model and is never called."""
    m, H, A, D = 3, 6, 6, 18
    model, _ = plan_model(False, H, m=m)
    dev = DevicePlannerState(model, m)
    eng = dev.eng
    assert not dev.context and eng.Hh == 0
    warm = CEMWarmStart(m, H, A)
    lib = eng.lib = _CountingLib(eng.lib)
    rng = np.random.default_rng(0)
    obs = f32(rng.standard_normal((m, D)))
    for step in range(12):
        same_bits(dev.prev_sol, warm.prev_sol, "prev_sol before step %d" % step)
        same_bits(dev.init_var, warm.init_var, "init_var before step %d" % step)
        call_before = model._call
        plan = model.get_action(obs, warm.prev_sol, warm.init_var)
        model._call = call_before
        act = _np(dev.act(obs)).copy()
        assert model._call == call_before + 1
        same_bits(act, warm.step(plan), "action, step %d" % step)
        assert np.abs(act).max() > 0
        nxt = f32(obs + 0.1 * rng.standard_normal((m, D)))
        done = np.array([step == 4, False, step in (2, 9)])
        before = _np(dev.prev_sol).copy()
        dev.observe(obs, act, nxt, done)
        after = _np(dev.prev_sol)
        for i in range(m):
            if done[i]:
                warm.reset(i)
                assert not after[i].any() and before[i].any(), "env %d, step %d: the warm start survived the episode's end" % (i, step)
            else:
                same_bits(after[i], before[i], "env %d, step %d: untouched by another env's reset" % (i, step))
        obs = nxt
    same_bits(dev.prev_sol, warm.prev_sol, "prev_sol after the last step")
    assert "cadm_history_update" not in lib.calls and lib.calls.count("cadm_warm_start_shift") == 12
    # the C entry still refuses this model: nothing on the device could have reset the warm start
    z = torch.zeros(m * D, dtype=torch.float32, device=eng.device)
    cnt = torch.zeros(m, dtype=torch.int32, device=eng.device)
    P = lambda t: ct.c_void_p(t.data_ptr())
    keep = _np(dev.prev_sol).copy()
    rc = eng.lib._lib.cadm_history_update(eng._ctx, P(z), P(z), P(z), None, m, 0, P(cnt), P(dev.hist_obs), P(dev.hist_act), P(dev.prev_sol), None)
    msg = eng.lib._lib.cadm_last_error().decode()
    assert rc == -1 and msg.startswith("cadm_history_update:") and "no history window" in msg, (rc, msg)
    same_bits(dev.prev_sol, keep)


# ---------------------------------------------------------------------------------------------------------------------- A3
GEOMETRIES = {  # env, m, H, Hh, state_diff
    "m1": ("halfcheetah", 1, 8, 10, 1),                   # a single env
    "m50": ("halfcheetah", 50, 8, 10, 0),                 # 50 * 8 * 6 = 2400 elements: ten workgroups of warm_start_kernel, the last one ragged
    "hh1": ("halfcheetah", 3, 5, 1, 1),                   # the shift loop has nothing to move; the slot is always 0
    "hh3": ("halfcheetah", 3, 5, 3, 0),                   # a short history
    "h1": ("halfcheetah", 3, 1, 3, 1),                    # every prev_sol entry is the zeroed tail
    "pendulum": ("pendulum", 4, 7, 3, 1),                 # the narrowest env: D = 3, A = 1
    "slim_humanoid": ("slim_humanoid", 2, 4, 10, 1),      # D = 45: the zero fill of 450 floats runs 8 trips per thread
}


@pytest.mark.parametrize("geo", sorted(GEOMETRIES))
def test_kernel_geometry_corners(gpu, geo):
    """Both kernels off the half-cheetah point, against SamplerState at float32, bit for bit before every step: 2 Hh + 4 steps (the
    window fills, shifts, is reset while filling and after it has shifted) of random plans and transitions.  `done` arrives as a bool
    numpy array, an int32 device tensor, a bool device tensor, and as None on steps where no episode ends."""
    env, m, H, Hh, sd = GEOMETRIES[geo]
    prob = synth.make_problem(env=env, context=True, E=5, m=m, H=H, Hh=Hh, seed=11, hidden_sizes=(32,) * 4)
    eng = synth.make_engine(prob, p=5)
    D, A = prob["D"], prob["A"]
    assert (D, A) == {"halfcheetah": (18, 6), "pendulum": (3, 1), "slim_humanoid": (45, 17)}[env]
    # (the kernels read the engine alone: no plan is made, so no model is built)
    dev = DevicePlannerState(types.SimpleNamespace(engine=eng, state_diff=sd, use_cem=True, _opt=None), m)
    ref = SamplerState(m, H, D, A, Hh, bool(sd))
    rng = np.random.default_rng(12)
    steps = 2 * Hh + 4
    dones = np.zeros((steps, m), bool)
    dones[1, 0] = True                     # while the window fills
    dones[Hh + 1, m - 1] = True            # a full window (m = 1: the refilled one, which then shifts at the last steps)
    if m > 1:
        dones[Hh + 3, m // 2] = True       # after a shift
    obs = f32(rng.standard_normal((m, D)))
    shifted = 0
    for t in range(steps):
        same_bits(dev.prev_sol, ref.prev_sol, "prev_sol before step %d" % t)
        same_bits(dev.hist_obs, ref.history_state, "hist_obs before step %d" % t)
        same_bits(dev.hist_act, ref.history_act, "hist_act before step %d" % t)
        np.testing.assert_array_equal(_np(dev.counts), np.array(ref.state_counts, np.int32))
        shifted += sum(c >= Hh for c in ref.state_counts)
        plan = f32(rng.uniform(-1, 1, (m, H, A)))
        eng._check(eng.lib.cadm_warm_start_shift(eng._ctx, ct.c_void_p(eng._t(plan).data_ptr()), m, ct.c_void_p(dev.prev_sol.data_ptr()),
                                                 ct.c_void_p(dev.action.data_ptr()), eng.stream), "cadm_warm_start_shift")
        act = ref.after_plan(plan)
        same_bits(dev.action, act, "action, step %d" % t)
        nxt = f32(obs + 0.1 * rng.standard_normal((m, D)))
        done = dones[t]
        if not done.any() and t % 2 == 0:
            as_given = None
        else:
            as_given = (done, torch.as_tensor(done.astype(np.int32), device=eng.device), torch.as_tensor(done, device=eng.device))[t % 3]
        dev.observe(obs, act, nxt, as_given)
        ref.after_step(obs, act, nxt, done)
        obs = nxt
    same_bits(dev.prev_sol, ref.prev_sol, "prev_sol at the end")
    same_bits(dev.hist_obs, ref.history_state, "hist_obs at the end")
    same_bits(dev.hist_act, ref.history_act, "hist_act at the end")
    same_bits(dev.init_var, ref.init_var, "init_var")
    assert shifted >= 2 and dones.any()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------- A4
ROUTES = {
    "cem": dict(),
    "icem_carry": dict(cem_keep_elites=3, cem_noise_beta=1.0),
    "mppi": dict(cem_update="mppi", cem_temperature=0.5),
    "cvar": dict(cem_score="cvar", cem_risk=0.2, n_particles=10),
    "constraint": dict(cem_constraints=[dict(dim=0, lo=-1e6, hi=1e6)], cem_constraint_weight=1.0),      # never binds
}


@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_device_state_under_each_planner_route(gpu, route, context):
    """A closed loop of 8 steps, one episode end in the middle, on two models built alike: one driven the samplers' way
    (MPCController.get_actions + CEMWarmStart(model=...) + a host-side history), the other through DevicePlannerState.  After every step
    the action, the warm start, both histories and the planner's carried elites with their valid flags are the same bits: a `done`
    invalidates the same env's elites on both sides."""
    m, H, A, D, Hh = 3, 5, 6, 18, 10
    kw = dict(ROUTES[route], m=m, **(dict(state_diff=1) if context else {}))
    host, _ = plan_model(context, H, **kw)
    twin, _ = plan_model(context, H, **kw)
    assert (host._opt is None) == (route == "cem")
    ctrl = MPCController("mpc", host.env, host, use_cem=True, n_candidates=64, horizon=H, num_rollouts=m, context=context)
    warm = CEMWarmStart(m, H, A, model=host)
    hist = SamplerState(m, H, D, A, Hh, True) if context else None
    dev = DevicePlannerState(twin, m)
    rng = np.random.default_rng(5)
    obs = f32(rng.standard_normal((m, D)))
    for step in range(8):
        if context:
            plan, _ = ctrl.get_actions(obs, cp_obs=hist.history_state, cp_act=hist.history_act, init_mean=warm.prev_sol, init_var=warm.init_var)
        else:
            plan, _ = ctrl.get_actions(obs, init_mean=warm.prev_sol, init_var=warm.init_var)
        act = warm.step(plan)
        got = _np(dev.act(obs)).copy()
        assert host._call == twin._call == step + 1
        same_bits(got, act, "action, step %d" % step)
        assert np.isfinite(act).all() and np.abs(act).max() > 0
        nxt = f32(obs + 0.1 * rng.standard_normal((m, D)))
        done = np.array([False, step == 3, False])
        if context:
            hist.after_step(obs, f32(act), nxt, done)
        for i in np.flatnonzero(done):
            warm.reset(i)
        dev.observe(obs, got, nxt, done)
        same_bits(dev.prev_sol, warm.prev_sol, "prev_sol after step %d" % step)
        if context:
            same_bits(dev.hist_obs, hist.history_state, "hist_obs after step %d" % step)
            same_bits(dev.hist_act, hist.history_act, "hist_act after step %d" % step)
        if route == "icem_carry":
            same_bits(twin._plan_carry, _np(host._plan_carry), "carried elites after step %d" % step)
            np.testing.assert_array_equal(_np(twin._plan_carry_valid), _np(host._plan_carry_valid))
            np.testing.assert_array_equal(_np(host._plan_carry_valid), [1, 0 if step == 3 else 1, 1])
            if step == 3:
                assert not _np(dev.prev_sol)[1].any()
        else:
            assert host._plan_carry is None and twin._plan_carry is None
        obs = nxt


# ---------------------------------------------------------------------------------------------------------------------- A5
@pytest.mark.parametrize("context", [False, True], ids=["vanilla", "cadm"])
def test_random_shooting_model_acts_by_random_shooting(gpu, context):
    """A model built with use_cem=False plans by random shooting (sampler.py:121-127): `act` is get_action's first action -- clipped to
    [-1, 1], [m, A] -- of a twin under the same call counter, and the warm start is left alone."""
    m, H, A, D = 3, 5, 6, 18
    model, _ = plan_model(context, H, m=m, use_cem=False)
    twin, _ = plan_model(context, H, m=m, use_cem=False)
    dev = DevicePlannerState(model, m)
    dev.prev_sol.fill_(0.5)
    rng = np.random.default_rng(8)
    obs = f32(rng.standard_normal((m, D)))
    for step in range(3):
        args = (_np(dev.hist_obs).astype(np.float64), _np(dev.hist_act).astype(np.float64)) if context else ()
        want = twin.get_action(obs, *args)
        got = _np(dev.act(obs)).copy()
        assert model._call == twin._call == step + 1
        assert want.shape == (m, A) and np.abs(want).max() <= 1.0
        same_bits(got, want, "random-shooting action, step %d" % step)
        same_bits(dev.prev_sol, np.full((m, H, A), 0.5), "the warm start, step %d" % step)
        nxt = f32(obs + 0.1 * rng.standard_normal((m, D)))
        dev.observe(obs, got, nxt)
        obs = nxt
    if context:
        assert _np(dev.hist_act)[:, :3 * A].any() and _np(dev.counts).tolist() == [3] * m


def test_discrete_actions_are_refused(gpu):
    """The samplers one-hot encode a discrete action before it enters the history (sampler.py:145-146); this class keeps raw actions."""
    from cadm_amd.envs import make_env_spec
    from test_gpu_model import CaDMModel, _cadm_kwargs
    model = CaDMModel(**_cadm_kwargs(env=make_env_spec("cartpole"), use_cem=False, normalize_input=False, n_candidates=50))
    with pytest.raises(NotImplementedError, match="discrete actions"):
        DevicePlannerState(model, 2)


# ---------------------------------------------------------------------------------------------------------------------- A6
def test_argument_checks_return_einval(gpu):
    """Both exports refuse bad arguments with CADM_EINVAL and a message that begins with their own name.  The checks run before any HIP
    call: the state next to the bad argument keeps its sentinel, and the same arguments made whole work afterwards."""
    m, H, A, D, Hh = 2, 5, 6, 18, 10
    _, eng = planner_engine(H, True)
    vanilla = plan_model(False, H)[0].engine      # a vanilla MODEL's engine: no context and no history window
    assert (eng.H, eng.A, eng.D, eng.Hh) == (H, A, D, Hh) and (vanilla.H, vanilla.A, vanilla.C, vanilla.Hh) == (H, A, 0, 0)
    lib, ctx = eng.lib, eng._ctx
    dv = eng.device
    t = lambda n, v, dt=torch.float32: torch.full((n,), v, dtype=dt, device=dv)
    plan, prev, action = t(m * H * A, 0.25), t(m * H * A, 7.0), t(m * A, 9.0)
    obs, nxt, act = t(m * D, 1.0), t(m * D, 2.0), t(m * A, 3.0)
    counts, ho, ha = t(m, 3, torch.int32), t(m * D * Hh, 5.0), t(m * A * Hh, 6.0)
    state = dict(prev=prev, action=action, counts=counts, ho=ho, ha=ha)
    sentinel = {k: _np(v).copy() for k, v in state.items()}
    P = lambda x: None if x is None else ct.c_void_p(x.data_ptr())

    def einval(rc, name, frag):
        msg = lib.cadm_last_error().decode()
        assert rc == -1, "%s: expected CADM_EINVAL, got %d (%s)" % (name, rc, msg)
        assert msg.startswith(name + ":") and frag in msg, msg
        for k, v in state.items():
            np.testing.assert_array_equal(_np(v), sentinel[k], err_msg="%s after a refused %s" % (k, name))

    def shift(c=ctx, pl=plan, n=m, pv=prev, ac=action):
        return lib.cadm_warm_start_shift(c, P(pl), n, P(pv), P(ac), None)

    def update(c=ctx, o=obs, nx=nxt, a=act, n=m, cn=counts, hob=ho, hac=ha, pv=prev):
        return lib.cadm_history_update(c, P(o), P(nx), P(a), None, n, 1, P(cn), P(hob), P(hac), P(pv), None)
    for bad in (dict(c=None), dict(pl=None), dict(pv=None), dict(ac=None), dict(n=0), dict(n=-1)):
        einval(shift(**bad), "cadm_warm_start_shift", "bad arguments")
    for bad in (dict(c=None), dict(o=None), dict(nx=None), dict(a=None), dict(cn=None), dict(hob=None), dict(hac=None), dict(n=0), dict(n=-1)):
        einval(update(**bad), "cadm_history_update", "bad arguments")
    einval(update(c=vanilla._ctx), "cadm_history_update", "no history window")
    # whole again: both work, on this ctx and (the shift, which needs no history) on the vanilla one
    assert shift() == 0 and update() == 0 and shift(c=vanilla._ctx) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(action), np.full(m * A, 0.25, np.float32))
    np.testing.assert_array_equal(_np(prev).reshape(m, H, A)[:, -1], np.zeros((m, A), np.float32))
    np.testing.assert_array_equal(_np(counts), [4, 4])
    # a null prev_sol is legal for the history update (nothing to reset), and a null done resets nothing
    assert update(pv=None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(counts), [5, 5])
