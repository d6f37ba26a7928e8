"""CPU: the open-loop prediction-error entry points exist in the built library, are bound with the header's argument counts, and
cadm_horizon_error refuses bad arguments before any HIP call (no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cadm_horizon_error", "cadm_eval_horizon", "cadm_eval_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from cadm_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _header_arg_counts():
    src = open(os.path.join(ROOT, "include", "cadm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: len(args.split(",")) for name, args in re.findall(r"\b(cadm_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", src)}


def test_new_entry_points_are_exported_and_bound(lib):
    from cadm_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    counts = _header_arg_counts()
    for name in NEW:
        assert hasattr(raw, name), "libcadm_hip.so does not export %s" % name
        assert name in _lib.SIGNATURES, "python binding lacks %s" % name
        assert len(_lib.SIGNATURES[name][1]) == counts[name], "%s: binding has %d arguments, header %d" % (
            name, len(_lib.SIGNATURES[name][1]), counts[name])


def _call(lib, traj=1, m=64, F=4, p=10, E=5, D=18, window0=0):
    """cadm_horizon_error with dummy non-null pointers (never dereferenced: every refusal comes before the first HIP call)."""
    buf = ctypes.create_string_buffer(64)
    P = ctypes.c_void_p(ctypes.addressof(buf))
    rc = lib.cadm_horizon_error(P if traj else None, P, F * D, P, m, F, p, E, D, window0, P, 1024, P, P, P, P, P, 1, None)
    return rc, lib.cadm_last_error().decode()


@pytest.mark.parametrize("kw,names", [
    (dict(p=10, E=4), ("p (10)", "E (4)")),
    (dict(window0=32), ("window0 (32)",)),
    (dict(F=0), ("F=0",)),
    (dict(traj=0), ("traj",)),
])
def test_horizon_error_refuses_bad_arguments_without_a_gpu(lib, kw, names):
    rc, msg = _call(lib, **kw)
    assert rc == -1, "expected CADM_EINVAL, got %d (%s)" % (rc, msg)
    assert msg.startswith("cadm_horizon_error:")
    for n in names:
        assert n in msg, "message %r does not name %s" % (msg, n)


def test_other_limits_are_argument_errors_too(lib):
    assert _call(lib, D=65)[0] == -1 and "D (65)" in lib.cadm_last_error().decode()
    assert _call(lib, window0=64 * 1024)[0] == -1 and "partials_blocks" in lib.cadm_last_error().decode()
    assert lib.cadm_eval_workspace_bytes(None, 100, 4, 64) == 0


def test_both_classes_have_evaluate_horizon():
    from cadm_amd.dynamics.mlp_cadm_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as CaDM
    from cadm_amd.dynamics.mlp_ensemble_cem_dynamics import MLPEnsembleCEMDynamicsModel as Vanilla
    import inspect
    assert list(inspect.signature(CaDM.evaluate_horizon).parameters) == ["self", "obs", "act", "obs_next", "cp_obs", "cp_act", "future_bool",
                                                                          "seed", "chunk"]
    assert list(inspect.signature(Vanilla.evaluate_horizon).parameters) == ["self", "obs", "act", "obs_next", "seed", "chunk"]
    assert "evaluate_horizon" in Vanilla.__dict__
