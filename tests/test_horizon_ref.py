"""CPU: the references of the open-loop prediction-error tests on their own (tests/horizon_ref.py) -- the kernel's documented
reduction order restated in numpy float32 stays inside `kernel_bound` of the float64 statistics at every shape of the GPU tests'
table, with a factor of two to spare, the table's masks count what the rows say they count, and the WT column is the LDS
budget's arithmetic."""
import numpy as np
import pytest

from horizon_ref import IDS, INVARIANT_ROWS, NONFINITE_ROWS, SHAPES, chain, kernel_bound, make_mask, restate32, row_inputs, row_mask, stats64, worst_ratio


@pytest.mark.parametrize("row", SHAPES, ids=IDS)
def test_float32_restatement_stays_inside_half_the_bar(row):
    """Worst |diff| / bound of the float32 restatement, numpy on the host (seed 3), in table order:
    0.058, 0.059, 0.048, 0.060, 0.074, 0.045, 0.063, 0.079, 0.044, 0.135, 0.435 (one window: nothing averages its roundings out)."""
    traj, truth = row_inputs(row)
    mask = row_mask(row)
    ref = stats64(traj, truth, mask, row["E"])
    got = restate32(traj, truth, mask, row["E"], row["WT"])
    assert ref["count"].min() > 0 and ref["diverged"].sum() == 0
    np.testing.assert_array_equal(got["count"], ref["count"])
    assert all(got[k].dtype == np.float32 for k in ("se", "spread", "se_member"))
    worst = worst_ratio(got, ref, kernel_bound(traj, truth, mask, row["E"], chain(row)))
    print("%s: float32 restatement vs float64, worst |diff| / bound %.3f (chain %d)" % (row["what"], worst, chain(row)))
    assert worst <= 0.5
    if row["p"] == row["E"] == 1:                # one particle: no spread, the member is the ensemble
        assert (got["spread"] == 0).all() and (ref["spread"] == 0).all() and np.array_equal(got["se_member"][0], got["se"])


@pytest.mark.parametrize("row", [r for r in SHAPES if r["m"] < 20], ids=[i for i, r in zip(IDS, SHAPES) if r["m"] < 20])
def test_all_invalid_mask_counts_nothing(row):
    traj, truth = row_inputs(row)
    mask = np.zeros((row["m"], row["F"]), np.float32)
    ref = stats64(traj, truth, mask, row["E"])
    got = restate32(traj, truth, mask, row["E"], row["WT"])
    bound = kernel_bound(traj, truth, mask, row["E"], chain(row))
    for r in (ref, got):
        assert (r["count"] == 0).all() and (r["diverged"] == 0).all()
        assert all((r[k] == 0).all() for k in ("se", "spread", "se_member"))
    assert all((bound[k] == 0).all() for k in bound)


def test_masks_hold_what_the_tests_rely_on():
    m4 = make_mask(150, 4)                                   # tests/test_gpu_horizon.py's mask, unchanged by the generalisation
    assert (m4[5] == 0).all() and tuple(m4[9]) == (1, 1, 0, 1) and (m4[:5] == 1).all()
    assert sorted(set(m4.sum(1).tolist())) == [0, 1, 2, 3, 4]
    for row in SHAPES:
        if row["mask"] != "mixed":
            assert row["m"] < 20
            continue
        mask = row_mask(row)
        f = row["F"]
        assert (mask[5] == 0).all(), row["what"]
        lengths = set(np.cumprod(mask, axis=1).sum(1).astype(int).tolist())
        assert lengths == set(range(f + 1)), "%s: prefix lengths %r" % (row["what"], sorted(lengths))
        if f >= 2:                                           # a hole: a set step behind an unset one, which the prefix rule leaves out
            assert mask[9, f - 2] == 0 and mask[9, f - 1] == 1, row["what"]
            assert np.cumprod(mask[9])[f - 1] == 0
    for i in NONFINITE_ROWS:                                 # the windows the non-finite tests plant in are all-valid
        mask = row_mask(SHAPES[i])
        assert (mask[[10, 11, SHAPES[i]["m"] - 1]] == 1).all(), SHAPES[i]["what"]
    assert [SHAPES[i]["WT"] for i in INVARIANT_ROWS] == [4, 1, 1, 16, 16] and SHAPES[5]["p"] == 1 and SHAPES[7]["E"] == 9


def test_wt_column_is_the_lds_budget():
    """4 D (p + 2 + E) + 16 bytes per window; WT windows + 32 bytes within 48 KiB; WT the largest power of two <= 16."""
    def wt(p, e, d):
        per, w = 4 * d * (p + 2 + e) + 16, 16
        while w >= 1 and w * per + 32 > 48 * 1024:
            w //= 2
        return w
    for row in SHAPES:
        assert wt(row["p"], row["E"], row["D"]) == row["WT"], row["what"]
    assert wt(185, 5, 64) == 0 and wt(180, 5, 64) == 1
    assert sorted({r["WT"] for r in SHAPES}) == [1, 2, 4, 8, 16]
