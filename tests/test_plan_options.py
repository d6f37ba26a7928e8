"""CPU: `cadm_amd.planner.PlanOptions` -- what a model's `cem_*` kwargs mean, their checks, and the structs built from them."""
import pytest

from cadm_amd import _lib
from cadm_amd.planner import PlanOptions

DEFAULTS = dict(cem_noise_beta=0.0, cem_keep_elites=0, cem_decay=1.0, cem_return="mean", cem_add_mean=False, cem_update="cem", cem_temperature=1.0,
                cem_temperature_relative=False, cem_score="mean", cem_risk=None)


def _opt(**kw):
    kw.setdefault("use_cem", True)
    return PlanOptions.from_kwargs(**kw)


def test_defaults_are_the_reference_route():
    """None at the defaults, spelled out or not -- whatever the other arguments are: nothing else is looked at."""
    assert PlanOptions.from_kwargs() is None and _opt() is None and _opt(**DEFAULTS) is None
    assert PlanOptions.from_kwargs(use_cem=False, discrete=True, process_group=object(), **DEFAULTS) is None


@pytest.mark.parametrize("kw,field,value,mppi", [
    (dict(cem_noise_beta=2.0), "noise_beta", 2.0, False), (dict(cem_keep_elites=3), "keep_elites", 3, False),
    (dict(cem_decay=1.25), "decay", 1.25, False), (dict(cem_return="best"), "return_best", True, False),
    (dict(cem_add_mean=True), "add_mean_last", True, False), (dict(cem_update="mppi"), "update", "mppi", True),
    (dict(cem_update="mppi", cem_temperature=0.5), "temperature", 0.5, True),
    (dict(cem_update="mppi", cem_temperature_relative=True), "relative", True, True),
    (dict(cem_score="mean_std", cem_risk=2.0), "score", ("mean_std", 2.0, None), False),
    (dict(cem_score="member_std", cem_risk=-1.0), "score", ("member_std", -1.0, None), False)], ids=lambda v: None)
def test_one_kwarg_off_its_default(kw, field, value, mppi):
    """The field follows its kwarg, every other field keeps its default, and the structs say the same (temperature and relative need
    cem_update="mppi" to be legal, a score its cem_risk)."""
    opt = _opt(**kw)
    want = dict(noise_beta=0.0, keep_elites=0, decay=1.0, return_best=False, add_mean_last=False, update="mppi" if mppi else "cem",
                temperature=1.0, relative=False, score=None)
    want[field] = value
    assert {k: getattr(opt, k) for k in want} == want
    assert type(opt.params) is (_lib.MppiParams if mppi else _lib.IcemParams)
    icem = opt.params.icem if mppi else opt.params
    assert (icem.noise_beta, icem.keep_elites, icem.decay, icem.return_best, icem.add_mean_last) == (
        want["noise_beta"], want["keep_elites"], want["decay"], int(want["return_best"]), int(want["add_mean_last"]))
    if mppi:
        assert (opt.params.temperature, opt.params.relative) == (want["temperature"], int(want["relative"]))
    if want["score"] is None:
        assert opt.score_params is None
    else:
        assert (opt.score_params.mode, opt.score_params.kappa, opt.score_params.k) == (_lib.SCORE_MODES[value[0]], value[1], 0)


def test_cvar_counts_the_tail_and_the_object_is_frozen():
    opt = _opt(cem_score="cvar", cem_risk=0.1, n_particles=20)
    assert opt.score == ("cvar", 0.0, 2) and (opt.score_params.mode, opt.score_params.k) == (3, 2) and type(opt.params) is _lib.IcemParams
    for name, value in (("keep_elites", 5), ("params", None), ("score_params", None), ("new_field", 1)):
        with pytest.raises(AttributeError):
            setattr(opt, name, value)
    assert opt.keep_elites == 0 and opt.params is not None


# the refusals of test_refusals_at_construction in tests/test_gpu_icem.py, test_gpu_mppi.py and test_gpu_risk.py, but the one that needs an
# engine (cem_keep_elites above its num_elites: the model raises it once the engine is built)
REFUSALS = [
    (dict(use_cem=False, cem_keep_elites=3), "need use_cem=True"), (dict(use_cem=False, cem_noise_beta=1.0), "need use_cem=True"),
    (dict(cem_return="first"), "cem_return"), (dict(cem_decay=0.5), "cem_decay"), (dict(cem_keep_elites=-1), "cem_keep_elites"),
    (dict(cem_noise_beta=-1.0), "cem_noise_beta"),
    (dict(cem_update="softmax"), "cem_update must be"), (dict(cem_update="mppi", cem_temperature=0.0), "cem_temperature"),
    (dict(cem_update="mppi", cem_temperature=-1.0), "cem_temperature"), (dict(cem_update="mppi", cem_temperature=float("nan")), "cem_temperature"),
    (dict(cem_update="mppi", cem_temperature=float("inf")), "cem_temperature"), (dict(cem_temperature=0.5), "need cem_update='mppi'"),
    (dict(cem_temperature_relative=True), "need cem_update='mppi'"), (dict(cem_keep_elites=2, cem_temperature=2.0), "need cem_update='mppi'"),
    (dict(use_cem=False, cem_update="mppi"), "need use_cem=True"), (dict(use_cem=False, cem_temperature=0.5), "need use_cem=True"),
    (dict(cem_score="variance", cem_risk=1.0), "cem_score must be"), (dict(cem_score="mean", cem_risk=0.5), "cem_risk configures"),
    (dict(cem_risk=2.0, cem_keep_elites=2), "cem_risk configures"), (dict(cem_score="mean_std"), "needs a finite cem_risk"),
    (dict(cem_score="member_std", cem_risk=float("nan")), "needs a finite cem_risk"), (dict(cem_score="cvar", cem_risk=float("inf")), "needs a finite cem_risk"),
    (dict(cem_score="cvar", cem_risk=0.0), "tail fraction"), (dict(cem_score="cvar", cem_risk=1.01), "tail fraction"),
    (dict(use_cem=False, cem_score="cvar", cem_risk=0.1), "need use_cem=True")]


def test_refusals(monkeypatch):
    for bad, msg in REFUSALS:
        with pytest.raises(ValueError, match=msg):
            _opt(**bad)
    for kw in (dict(cem_return="best"), dict(cem_update="mppi"), dict(cem_score="mean_std", cem_risk=1.0)):
        with pytest.raises(NotImplementedError, match="continuous actions only"):
            _opt(discrete=True, **kw)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    for kw in (dict(cem_decay=1.25), dict(cem_update="mppi"), dict(cem_score="cvar", cem_risk=0.5)):
        with pytest.raises(NotImplementedError, match="more than one rank"):
            _opt(process_group=object(), **kw)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    assert _opt(process_group=object(), cem_decay=1.25).decay == 1.25
    # the order of the checks: use_cem first, the score before the update, discreteness after the values
    with pytest.raises(ValueError, match="need use_cem=True"):
        _opt(use_cem=False, discrete=True, cem_score="variance")
    with pytest.raises(ValueError, match="cem_score must be"):
        _opt(cem_score="variance", cem_update="softmax")
    with pytest.raises(ValueError, match="cem_keep_elites must be"):
        _opt(discrete=True, cem_keep_elites=-1)
