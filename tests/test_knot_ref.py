"""CPU: the numpy restatement of the knot grid (tests/knot_ref.py) on the properties the GPU tests rely on, every validation rule of
`PlanOptions.from_kwargs` for the `cem_knot*` kwargs, and the `cadm_knot_params` struct as the header lays it out."""
import ctypes
import os
import re

import numpy as np
import pytest

import knot_ref as kref
from cadm_amd import _lib
from cadm_amd.engine import HipEngine
from cadm_amd.planner import PlanOptions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 3
GRID = [(H, r, phi) for H in (1, 5, 6, 7, 30) for r in sorted({1, 2, 3, 4, H, H + 3}) for phi in range(r)]


def test_knot_steps_of_the_header_s_examples():
    assert kref.knot_steps(7, 3, 0) == [0, 3, 6] and kref.knot_steps(7, 3, 1) == [0, 2, 5] and kref.knot_steps(7, 3, 2) == [0, 1, 4]
    assert kref.knot_steps(5, 8, 5) == [0, 3]
    assert kref.knot_steps(5, 8, 0) == [0] and kref.knot_steps(1, 2, 1) == [0] and kref.knot_steps(6, 1, 0) == list(range(6))
    assert kref.knot_steps(7, 3, -2) == kref.knot_steps(7, 3, 1) == kref.knot_steps(7, 3, 4)      # the phase is taken modulo r, non-negative


@pytest.mark.parametrize("H,r,phi", GRID, ids=lambda v: None)
def test_grid_properties(H, r, phi):
    """The knot steps are those the per-step segments name, strictly increasing from 0 inside [0, H), J of them; and on random sequences,
    sequences on +-1 and sequences alternating between the bounds: shaping is idempotent, keeps the knot steps' bits, stays inside
    [-1, 1], is the identity for r = 1, and a HOLD-shaped sequence moved one step on lies on the grid of phase phi + 1 over steps
    [0, H - 1) (step H - 1 is what the sampler drew)."""
    knots = kref.knot_steps(H, r, phi)
    assert knots[0] == 0 and all(b > a for a, b in zip(knots, knots[1:])) and knots[-1] <= H - 1 and len(knots) == (H - 1 + phi) // r + 1
    assert sorted({kref.segment(t, H, r, phi)[0] for t in range(H)}) == knots
    for t in range(H):
        k, k1 = kref.segment(t, H, r, phi)
        assert k <= t < k1 and k in knots and (k1 in knots or k1 > H - 1)
    rng = np.random.default_rng(1000 * H + 10 * r + phi)
    alt = np.where((np.arange(H)[:, None] + np.arange(A)[None]) % 2 == 0, 1.0, -1.0).astype(np.float32)
    seqs = [rng.uniform(-1, 1, (H, A)).astype(np.float32), np.ones((H, A), np.float32), -np.ones((H, A), np.float32), alt, -alt,
            rng.choice(np.array([-1.0, 1.0], np.float32), (H, A))]
    for interp in (kref.HOLD, kref.LINEAR):
        exact = kref.exact_steps(H, r, interp, phi)
        assert exact[knots].all()
        for a in seqs:
            s = kref.shape_one(a, r, interp, phi)
            assert s.dtype == np.float32 and s.min() >= -1.0 and s.max() <= 1.0
            np.testing.assert_array_equal(s[knots].view(np.uint32), a[knots].view(np.uint32))
            np.testing.assert_array_equal(kref.shape_one(s, r, interp, phi).view(np.uint32), s.view(np.uint32))
            if r == 1:
                np.testing.assert_array_equal(s.view(np.uint32), a.view(np.uint32))
            for t in np.nonzero(exact)[0]:
                np.testing.assert_array_equal(s[t].view(np.uint32), a[kref.segment(t, H, r, phi)[0]].view(np.uint32))
            for t in np.nonzero(~exact)[0]:      # the kernel's own fp32 expression on bound values: inside the bounds, next to the reference
                k, k1 = kref.segment(t, H, r, phi)
                v = np.array([kref.linear_f32(a[k, d], a[k1, d], t, k, k1) for d in range(A)]) if np.abs(a).min() == 1.0 else s[t]
                assert v.min() >= -1.0 and v.max() <= 1.0 and np.abs(v.astype(np.float64) - s[t]).max() <= 2.0 ** -22
            if interp == kref.HOLD and H > 1:
                moved = np.concatenate([s[1:], rng.uniform(-1, 1, (1, A)).astype(np.float32)])
                again = kref.shape_one(moved, r, interp, phi + 1)
                np.testing.assert_array_equal(again[:H - 1].view(np.uint32), moved[:H - 1].view(np.uint32))


def test_shape_takes_a_phase_per_env():
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, (3, 4, 7, A)).astype(np.float32)
    got = kref.shape(a, 3, kref.LINEAR, [0, 1, -1])
    for mi, phi in enumerate((0, 1, 2)):
        for c in range(4):
            np.testing.assert_array_equal(got[mi, c], kref.shape_one(a[mi, c], 3, kref.LINEAR, phi))
    np.testing.assert_array_equal(kref.shape(a[:, 0], 3, kref.HOLD), kref.shape(a[:, :1], 3, kref.HOLD)[:, 0])
    assert kref.breakpoints(kref.shape_one(a[0, 0], 3, kref.HOLD, 1)) == [2, 5]


# ---------------------------------------------------------------------------------------------------------------------- PlanOptions
def test_plan_options_defaults_and_the_opt_in_route():
    assert PlanOptions.from_kwargs() is None
    assert PlanOptions.from_kwargs(cem_knots=1, cem_knot_interp="hold", cem_knot_anchor="call") is None
    assert PlanOptions.from_kwargs(use_cem=False, discrete=True, cem_knots=np.int64(1)) is None
    opt = PlanOptions.from_kwargs(use_cem=True, cem_knots=3)
    assert opt.knots == (3, "hold", "call") and isinstance(opt.knot_params, _lib.KnotParams)
    assert (opt.knot_params.spacing, opt.knot_params.interp) == (3, 0)
    assert opt.score_params is None and opt.constraint_params is None and opt.update == "cem" and opt.keep_elites == 0
    assert type(opt.params) is _lib.IcemParams
    opt = PlanOptions.from_kwargs(use_cem=True, cem_knots=np.int32(4), cem_knot_interp="linear")
    assert opt.knots == (4, "linear", "call") and (opt.knot_params.spacing, opt.knot_params.interp) == (4, 1)
    opt = PlanOptions.from_kwargs(use_cem=True, cem_knots=2, cem_knot_anchor="episode", cem_update="mppi", cem_score="cvar", cem_risk=0.5)
    assert opt.knots == (2, "hold", "episode") and opt.knot_params.spacing == 2 and opt.update == "mppi" and opt.score_params.mode == 3
    plain = PlanOptions.from_kwargs(use_cem=True, cem_noise_beta=1.0)
    assert plain.knots is None and plain.knot_params is None
    with pytest.raises(AttributeError):
        opt.knots = None
    with pytest.raises(TypeError):      # keyword-only, behind the existing positional order
        PlanOptions.from_kwargs(0.0, 0, 1.0, "mean", False, "cem", 1.0, False, "mean", None, True, False, None, 20, None, "penalty", None, 3)


@pytest.mark.parametrize("kw,msg", [
    (dict(use_cem=False, cem_knots=3), "need use_cem=True"),
    (dict(use_cem=False, cem_knot_interp="linear"), "need use_cem=True"),
    (dict(cem_knots=0), "cem_knots must be an integer >= 1"),
    (dict(cem_knots=-2), "cem_knots must be an integer >= 1"),
    (dict(cem_knots=2.0), "cem_knots must be an integer >= 1"),
    (dict(cem_knots=True), "cem_knots must be an integer >= 1"),
    (dict(cem_knots="3"), "cem_knots must be an integer >= 1"),
    (dict(cem_knots=3, cem_knot_interp="cubic"), "cem_knot_interp must be"),
    (dict(cem_knots=3, cem_knot_anchor="step"), "cem_knot_anchor must be"),
    (dict(cem_knot_interp="linear"), "configure knots: they need cem_knots > 1"),
    (dict(cem_knot_anchor="episode"), "configure knots: they need cem_knots > 1"),
    (dict(cem_knots=1, cem_knot_anchor="episode", cem_noise_beta=1.0), "configure knots: they need cem_knots > 1"),
])
def test_plan_options_refusals(kw, msg):
    kw = dict(dict(use_cem=True), **kw)
    with pytest.raises(ValueError, match=msg):
        PlanOptions.from_kwargs(**kw)


def test_plan_options_keeps_its_other_refusals(monkeypatch):
    with pytest.raises(NotImplementedError, match="continuous actions only"):
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_knots=3)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="more than one rank"):
        PlanOptions.from_kwargs(use_cem=True, process_group=object(), cem_knots=3)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="cem_knots must be"):      # the values before discreteness
        PlanOptions.from_kwargs(use_cem=True, discrete=True, cem_knots=0)
    with pytest.raises(ValueError, match="cem_risk configures"):
        PlanOptions.from_kwargs(use_cem=True, cem_risk=1.0, cem_knots=3)


def test_knot_params_directly():
    k = HipEngine.knot_params(np.int64(5), "linear")
    assert (k.spacing, k.interp) == (5, 1) and HipEngine.knot_params(2).interp == 0 and HipEngine.knot_params(2, 1).interp == 1
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="integer >= 1"):
            HipEngine.knot_params(bad)
    for bad in ("Hold", 2, -1):
        with pytest.raises(ValueError, match="'hold' or 'linear'"):
            HipEngine.knot_params(3, bad)


def test_struct_layout_matches_the_header():
    names = [f[0] for f in _lib.KnotParams._fields_]
    assert names == ["spacing", "interp"]
    assert ctypes.sizeof(_lib.KnotParams) == 8 and [getattr(_lib.KnotParams, k).offset for k in names] == [0, 4]
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    body = re.search(r"typedef struct cadm_knot_params \{(.*?)\} cadm_knot_params;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\bint32_t (\w+);", body) == names
    assert re.search(r"#define CADM_KNOT_HOLD (\d+)", src).group(1) == "0" and _lib.KNOT_INTERPS["hold"] == 0 == kref.HOLD
    assert re.search(r"#define CADM_KNOT_LINEAR (\d+)", src).group(1) == "1" and _lib.KNOT_INTERPS["linear"] == 1 == kref.LINEAR
    sig = _lib.SIGNATURES
    assert len(sig["cadm_shape_actions"][1]) == 7 and len(sig["cadm_knot_plan"][1]) == len(sig["cadm_constrained_plan"][1]) + 2
    assert sig["cadm_knot_plan"][1][1] == ctypes.POINTER(_lib.KnotParams) == sig["cadm_shape_actions"][1][1]
