"""GPU: the three `*_workspace_bytes` entry points against their sums restated here (csrc/plan.hip carve, csrc/icem.hip icem_carve,
csrc/horizon.hip eval_carve).  Callers resolve raw pointers into these workspaces (`dist_init_external`), so the byte totals are part
of the contract.  Every view is 4-byte words, rounded up to 256 bytes.  No kernel is launched: the entry points only add."""
import pytest

from cadm_amd import synth
from helpers import make_engine

pytestmark = pytest.mark.gpu

E, P_, H, D, A = 5, 5, 5, 18, 6      # halfcheetah


def a(x):
    return (x + 255) // 256 * 256


def plan_bytes(m, n, C):
    return (a(4 * E * m * max(C, 1)) + a(4 * m * n * H * A) + a(4 * m * n * P_) + a(4 * m * n) + a(4 * (m * n + 1024)) + 2 * a(4 * m * H * A)
            + a(4 * m * n * H) + 256)


def icem_bytes(m, n, C, K, num_elites):
    return (a(4 * E * m * max(C, 1)) + a(4 * m * n * H * A) + a(4 * m * n * P_) + a(4 * m * n) + 3 * a(4 * m * H * A)
            + a(4 * m * max(K, 1) * H * A) + a(4 * m) + a(4 * m * H * A) + a(4 * m * num_elites))


def eval_bytes(N, F, chunk, C):
    b = (N + 63) // 64
    mc = min(chunk, 64 * b)
    return a(4 * mc * D) + a(4 * E * mc * max(C, 1)) + a(4 * mc * P_) + 2 * a(4 * F * mc * P_ * D) + a(4 * b * F * ((2 + E) * D + 2))


@pytest.mark.parametrize("context,shapes", [(True, [(2, 37), (1, 64)]), (False, [(1, 64)])], ids=["context", "vanilla"])
def test_workspace_bytes_are_the_restated_sums(gpu, context, shapes):
    prob = synth.make_problem(env="halfcheetah", context=context, E=E, m=1, H=H, seed=1, hidden_sizes=(32,) * 4)
    eng = make_engine(prob, p=P_)
    C = prob["C"]
    assert (prob["D"], prob["A"], C) == (D, A, 10 if context else 0)
    for m, n in shapes:
        assert eng.lib.cadm_plan_workspace_bytes(eng._ctx, m, n) == plan_bytes(m, n, C), (m, n)
        for K in (0, 3):
            assert eng.lib.cadm_icem_workspace_bytes(eng._ctx, m, n, K) == icem_bytes(m, n, C, K, eng.num_elites), (m, n, K)
    for N, F, chunk in ((70, 3, 64), (10, 2, 128)):
        assert eng.lib.cadm_eval_workspace_bytes(eng._ctx, N, F, chunk) == eval_bytes(N, F, chunk, C), (N, F, chunk)
    eng.close()
