"""The inputs of tests/test_gpu_context_stats.py, judged on the oracle alone (no GPU): a GPU test under non-identity history
statistics is worth something only if a slipped statistic -- a mean or a std read from the neighbouring column, statistics not
applied at all -- moves the answer far beyond the bar the kernels are held to, while the reference itself stays well inside it.

Context vectors: oracle/nets.context_forward in float64 on helpers.raw_history_problem's float32-valued histories and statistics,
every geometry of helpers.RAW_GEOMETRIES at m = 65 rows.  Measured (max |change| in units of the context tensor's rms, range
over the seven geometries): mean rolled by one column 16 - 31, std rolled by one column 1.6 - 5.1, identity statistics 8.3 - 16;
float32 oracle against float64 oracle at most 1.8e-6 in assert_close's floored-relative measure (5e-6 asserted: half the GPU
tests' 1e-5).  The gradient twin: cp_hidden_0_weight's float64 gradient under identity statistics is 7.8 / 13 x the tensor's max
away from the one under the raw statistics (ant / halfcheetah)."""
import numpy as np
import pytest
import torch

from helpers import (RAW_GEOMETRIES, _cfg, _oracle_nets, floored_rel, identity_history_stats, oracle_problem, raw_history_problem,
                     raw_train_batch, rolled_stats)
from oracle import nets as onets
from oracle import train as otrain

M = 65
IDS = ["%s-E%d-Hh%d-%s" % (g[0], g[1], g[2], "x".join(map(str, g[3]))) for g in RAW_GEOMETRIES]


def _ctx(prob, cp_obs, cp_act, dtype, stats=None):
    o = oracle_problem(prob, dtype)
    st = o["st"] if stats is None else onets.cast_stats(stats, dtype)
    return onets.context_forward(o["cp"], cp_obs.astype(dtype), cp_act.astype(dtype), st)


@pytest.mark.parametrize("env,E,Hh,cp_sizes,C", RAW_GEOMETRIES, ids=IDS)
def test_a_slipped_statistic_moves_the_context_far_beyond_the_bar(env, E, Hh, cp_sizes, C):
    prob, cp_obs, cp_act = raw_history_problem(env, E, Hh, cp_sizes, C, M, seed=5)
    st = prob["stats"]
    assert np.array_equal(cp_obs, cp_obs.astype(np.float32)) and all(np.array_equal(v, v.astype(np.float32)) for v in st.values())
    assert np.abs(st["cp_obs_mean"]).max() > 2.0 and st["cp_obs_std"].min() >= 0.5 and st["cp_obs_std"].max() > 1.2
    ref = _ctx(prob, cp_obs, cp_act, np.float64)
    assert ref.shape == (E, M, C) and np.isfinite(ref).all()
    rms = np.sqrt(np.mean(ref ** 2))
    for what, stats in (("cp_obs_mean rolled by one column", rolled_stats(st, "cp_obs_mean")),
                        ("cp_obs_std rolled by one column", rolled_stats(st, "cp_obs_std")),
                        ("identity statistics", identity_history_stats(st))):
        change = np.abs(_ctx(prob, cp_obs, cp_act, np.float64, stats) - ref).max() / rms
        print("%s %s: context moves by %.2f rms" % (env, what, change))
        assert change > 1.0, "%s: the context moves by only %.3f of its rms" % (what, change)
    err = floored_rel(_ctx(prob, cp_obs, cp_act, np.float32), ref)
    print("%s float32 oracle vs float64 oracle: %.2e" % (env, err))
    assert err <= 5e-6


@pytest.mark.parametrize("env,E,Hh,cp_sizes,C", RAW_GEOMETRIES, ids=IDS)
def test_a_zero_std_column_stays_finite(env, E, Hh, cp_sizes, C):
    """std = 0: the column divides by 1e-10.  It sits exactly on its mean, so it normalises to 0, not to a rounding error times 1e10."""
    prob, cp_obs, cp_act = raw_history_problem(env, E, Hh, cp_sizes, C, M, seed=6, zero_std_cols=(1,))
    assert prob["stats"]["cp_obs_std"][1] == 0.0 and (cp_obs[:, 1] == prob["stats"]["cp_obs_mean"][1]).all()
    ref = _ctx(prob, cp_obs, cp_act, np.float64)
    got = _ctx(prob, cp_obs, cp_act, np.float32)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    err = floored_rel(got, ref)
    print("%s zero-std column, float32 oracle vs float64 oracle: %.2e" % (env, err))
    assert err <= 5e-6


@pytest.mark.parametrize("env,with_back,E,B", [("halfcheetah", True, 3, 37), ("ant", False, 2, 50)])
def test_identity_statistics_move_the_first_layers_gradient(env, with_back, E, B):
    """The training twin: the first encoder layer's weight gradient is x^T dz with x the normalised history."""
    prob, _, _ = raw_history_problem(env, E, 10, (256, 128, 64), 10, 1, seed=22, with_back=with_back)
    batch = raw_train_batch(prob, B, seed=3)
    tb = {k: torch.tensor(v, dtype=torch.float64) for k, v in batch.items()}
    bc = 0.5 if with_back else 0.0
    grads = []
    for stats in (prob["stats"], identity_history_stats(prob["stats"])):
        ff, back, cp, _ = _oracle_nets(prob, torch.float64)
        out = otrain.train_losses(env, ff, back, cp, otrain.to_torch(stats, torch.float64), tb, _cfg(prob, False, bc))
        g = otrain.grads_of(out["loss"], {"ff_model": ff, "backward_model": back, "context_model": cp})
        grads.append(g["context_model"]["cp_hidden_0_weight"].numpy())
    change = np.abs(grads[1] - grads[0]).max() / np.abs(grads[0]).max()
    print("%s: cp_hidden_0_weight gradient moves by %.2f of its max" % (env, change))
    assert change > 1.0
