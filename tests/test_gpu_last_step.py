"""The rollout's step loop leaves before the model evaluation of the LAST step when nothing reads the state it would produce: no
trajectory output, and a reward that reads only the pre-step observation (halfcheetah, ant, slim humanoid, pendulum; cart-pole and a
declared env with a next-observation term keep the full loop).  A call with a trajectory output keeps the full loop too, so it is the
reference here: the returns of a call without `want_traj` must equal the returns of the same call with it BIT FOR BIT -- in every
flavour (row_tiles 0..4: the launcher's plan, cooperative one / two row tiles, wave-tile 8 / 4) and in the fp32 comparison kernel, in
every noise mode, at H = 1 (no dense sweep at all), 2 and 3, on three batches.  40 rows per member: 3 row tiles, the last one partial, an
odd count for the pair flavour.  1024 rows per member: 64 tiles, more than a member's workgroups (a CU share: 51 on 256 CUs), so a
one-tile workgroup starts a second tile right behind the early exit.  6656 rows per member: 416 tiles -- 208 pairs, and more than one
round of the wave-tile kernels (51 x 8 = 408 and 51 x 4 = 204 tiles a round) --, so in EVERY forced flavour a workgroup goes on to
further tiles behind the exit and must find the weight ring and its LDS buffers as a full loop leaves them.
(A call with a trajectory output never took the exit, before or after it existed: these tests guard that the exit changes no result,
not that it is taken -- that is the matrix-instruction count of profiles/last_step_ab.md.)"""
import numpy as np
import pytest
import torch

from cadm_amd import _lib, synth
from helpers import make_engine

pytestmark = pytest.mark.gpu

E, P_ = 5, 20
FLAVOURS = [("xdl", 0), ("xdl", 1), ("xdl", 2), ("xdl", 3), ("xdl", 4), ("f32", 0)]
SHAPES = {"m2-n5": (2, 5), "m1-n256": (1, 256), "m1-n1664": (1, 1664)}
PHILOX = {"seed": 5, "call": 3, "it": 1}


@pytest.fixture(scope="module")
def world(gpu):
    """One halfcheetah + context problem (hidden 200 x 4, E = 5: compiled-in geometry) and its engines on the developer library, by
    (horizon, deterministic); shared by the tests below and left unchanged by them."""
    prob = synth.make_problem(env="halfcheetah", context=True, E=E, m=2, H=3, trained_like=True, seed=31)
    engines = {}

    def engine(H, det=False):
        if (H, det) not in engines:
            engines[H, det] = make_engine(prob, p=P_, H=H, deterministic=det, lib=_lib.load_dev())
        return engines[H, det]
    yield prob, engine
    for eng in engines.values():
        eng.close()


class forced:
    def __init__(self, eng, kind, row_tiles):
        self.eng, self.kind, self.row_tiles = eng, kind, row_tiles

    def __enter__(self):
        self.eng.dev_set_rollout(self.kind, row_tiles=self.row_tiles)

    def __exit__(self, *exc):
        self.eng.dev_set_rollout("xdl", row_tiles=0)


def _inputs(prob, eng, m, n, H, seed):
    rng = np.random.default_rng(seed)
    acts = eng._t(rng.uniform(-1, 1, (m, n, H, prob["A"])).astype(np.float32))
    ctx = eng.context_forward(prob["cp_obs"][:m], prob["cp_act"][:m])
    eps = eng._t(rng.standard_normal((H, m, n, P_, prob["D"])).astype(np.float32))
    return prob["obs"][:m], ctx, acts, eps


def _both(eng, obs, ctx, acts, **kw):
    rows = eng.rollout_returns(obs, ctx, acts, **kw)
    rows_t, traj = eng.rollout_returns(obs, ctx, acts, want_traj=True, **kw)
    torch.cuda.synchronize()
    return rows, rows_t, traj


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("H", [1, 2, 3])
def test_returns_without_trajectory_equal_returns_with_it(world, H, shape):
    prob, engine = world
    m, n = SHAPES[shape]
    for mode in ("deterministic", "inject", "philox"):
        eng = engine(H, det=mode == "deterministic")
        obs, ctx, acts, eps = _inputs(prob, eng, m, n, H, seed=7)
        kw = {"eps": eps} if mode == "inject" else dict(PHILOX) if mode == "philox" else {}
        for kind, rt in FLAVOURS:
            with forced(eng, kind, rt):
                rows, rows_t, _ = _both(eng, obs, ctx, acts, **kw)
            what = "H=%d %s %s %s row_tiles=%d" % (H, shape, mode, kind, rt)
            assert torch.isfinite(rows_t).all(), what
            assert torch.equal(rows, rows_t), what


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("H", [1, 2, 3])
def test_last_steps_injected_noise_does_not_reach_the_returns(world, H, shape):
    """eps[H-1] is the noise of the step that produces state H, which the returns never read: overwriting it -- with inf and NaN for
    one row -- changes neither the returns (still finite) nor the states 1 .. H-1 of a trajectory call."""
    prob, engine = world
    m, n = SHAPES[shape]
    eng = engine(H)
    obs, ctx, acts, eps = _inputs(prob, eng, m, n, H, seed=11)
    eps2 = eps.clone()
    eps2[H - 1] = 100.0 * torch.randn_like(eps2[H - 1])
    eps2[H - 1, m - 1, n // 2, 3, 0::2] = float("inf")
    eps2[H - 1, m - 1, n // 2, 3, 1::2] = float("nan")
    for kind, rt in FLAVOURS:
        with forced(eng, kind, rt):
            rows, rows_t, traj = _both(eng, obs, ctx, acts, eps=eps)
            rows2, rows2_t, traj2 = _both(eng, obs, ctx, acts, eps=eps2)
        what = "H=%d %s %s row_tiles=%d" % (H, shape, kind, rt)
        assert torch.isfinite(rows2).all(), what
        assert torch.equal(rows2, rows), what
        assert torch.equal(rows, rows_t) and torch.equal(rows2, rows2_t), what
        assert torch.equal(traj2[:H - 1], traj[:H - 1]), what


@pytest.mark.parametrize("H", [1, 2])
def test_cartpole_keeps_its_last_step(gpu, H):
    """Cart-pole's reward reads the NEXT state (rollout_env.h: 1 - [|x| > 2.4] - [|theta| > 12 * 2 pi / 360], dims 0 and 2), so its last
    model evaluation stays: the returns equal the reward recomputed on the host from the trajectory the same call returned (small
    integers: exact in any summation order), with and without the trajectory output.  33 rows per member: 3 tiles, the last partial."""
    m, n, p = 1, 33, 5
    prob = synth.make_problem(env="cartpole", context=True, E=E, m=m, H=H, trained_like=True, seed=13)
    eng = make_engine(prob, p=p, lib=_lib.load_dev())
    rng = np.random.default_rng(17)
    acts = eng._t(rng.uniform(-1, 1, (m, n, H, prob["A"])).astype(np.float32))
    ctx = eng.context_forward(prob["cp_obs"], prob["cp_act"])
    eps = eng._t(rng.standard_normal((H, m, n, p, prob["D"])).astype(np.float32))
    obs_rows = (1.5 * rng.standard_normal((m, n, p, prob["D"]))).astype(np.float32)      # rows on both sides of both thresholds
    xlim, th = np.float32(2.4), np.float32(0.20943951023931953)
    seen = set()
    for kind, rt in FLAVOURS:
        with forced(eng, kind, rt):
            rows, rows_t, traj = _both(eng, prob["obs"], ctx, acts, eps=eps, obs_rows=obs_rows)
        what = "H=%d %s row_tiles=%d" % (H, kind, rt)
        t = traj.cpu().numpy()
        x, theta = t[..., 0], t[..., 2]
        step = 1.0 - ((x > xlim).astype(np.float32) + (x < -xlim)) - ((theta > th).astype(np.float32) + (theta < -th))
        want = step.sum(axis=0).astype(np.float32)
        np.testing.assert_array_equal(rows_t.cpu().numpy(), want, err_msg=what)
        assert torch.equal(rows, rows_t), what
        seen |= set(np.unique(want).tolist())
    assert len(seen) >= 3, "the rows do not exercise the thresholds: returns %r" % sorted(seen)
    eng.close()


def test_planner_is_the_same_in_every_flavour(gpu):
    """cem_plan (no trajectory: every rollout takes the early exit) at cfg2's class constants -- halfcheetah + context, E = 5, p = 20,
    5 CEM iterations, alpha 0.1 -- with n = 16, H = 3: the same plan whether the launcher chooses the flavour or one is forced.
    (cfg2's 50 elites of 200 candidates do not fit n = 16 -- the refit refuses n < num_elites --: the same fraction, 4 of 16.)"""
    H, n = 3, 16
    prob = synth.make_problem(env="halfcheetah", context=True, E=E, m=1, H=H, trained_like=True, seed=19)
    eng = make_engine(prob, p=P_, num_elites=4, lib=_lib.load_dev())
    args = [eng._t(prob[k]) for k in ("obs", "cp_obs", "cp_act", "init_mean", "init_var")]
    plan0 = eng.cem_plan(*args, n, seed=3, call=1).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(plan0).all() and float(plan0.abs().max()) > 0.0
    for rt in (1, 2, 3, 4):
        with forced(eng, "xdl", rt):
            plan = eng.cem_plan(*args, n, seed=3, call=1).clone()
            torch.cuda.synchronize()
        assert torch.equal(plan, plan0), "row_tiles=%d" % rt
    eng.close()
