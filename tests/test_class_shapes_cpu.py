"""The batches of tests/test_gpu_feat_classes.py on the oracle alone (no GPU): every one must hold what it is named for BEFORE it travels.

  1. the restated partition (class_shapes.expected_partition) names the classes the catalogue lists, covers every feature exactly once, and its
     slot ranges are contiguous in the order of the track sort;
  2. every class holds a feature the update USES, and the gate rejects the outlier planted in a class (every class of three or more gated
     tracks has one);
  3. no gated feature has |chi2 / threshold - 1| < 1e-6: the GPU tests compare feat_status with no excuse, and this keeps that equality from
     hiding a rounding flip.  A condition on the INPUTS (the seeds in class_shapes.py were chosen until the oracle alone meets it), not a tolerance
     of the GPU.
"""
import numpy as np
import pytest

import class_shapes as cs
import track_shapes as ts
from open_vins_amd import capi


@pytest.mark.parametrize("cid", [c.id for c in cs.CASES])
def test_partition_covers_the_batch(cid):
    case = cs.BY_ID[cid]
    m = case.lengths
    part = case.partition
    assert tuple(k for k, _, _, _ in part) == case.classes
    assert part[0][1] == 0 and part[-1][2] == case.prob.F
    for (_, _, b0, _), (_, a1, _, _) in zip(part, part[1:]):
        assert b0 == a1                                                  # contiguous, no slot twice, none left out
    order = cs.slot_order(m)
    assert sorted(order.tolist()) == list(range(case.prob.F))
    assert np.all(np.diff(m[order]) <= 0)
    for k, a, b, m_max in part:
        mm = m[order[a:b]]
        assert b > a and mm[0] == m_max == mm.max()
        assert all(ts.expected_kernel(int(x)) == k for x in mm if x >= 2)  # every track on the smallest shape that holds it
        assert ts.expected_kernel(int(m_max)) == k
    assert sum(case.counts) == case.prob.F and case.mask == sum(1 << k for k in case.classes)
    print(f"classes {cid}: " + " | ".join(f"kernel {k}: {b - a} tracks, longest {mm}" for k, a, b, mm in part))


@pytest.mark.parametrize("cid", [c.id for c in cs.CASES])
def test_gpu_case_is_not_vacuous(oracle, cid):
    case = cs.BY_ID[cid]
    m = case.lengths
    tri, ref = cs.oracle_run(oracle, case)
    st, chi2, thr = ref["feat_status"], ref["chi2"], ref["chi2_thresh"]
    cls = cs.class_of_feature(m)
    gate = np.isfinite(chi2)
    for k in case.classes:
        in_k = (cls == k) & (m >= 2)
        assert (in_k & (st == capi.FEAT_USED) & gate).any(), k                # an accepted feature in every class
        if (in_k & gate).sum() >= 3:
            assert any(cls[f] == k for f in case.planted), k                  # three or more gated tracks: an outlier was planted there
    for f in case.planted:
        assert st[f] == capi.FEAT_CHI2_REJECTED, f                            # ... and the gate rejects it
    assert np.abs(chi2[gate] / thr[gate] - 1.0).min() > 1e-6                  # no verdict on a knife's edge
    assert np.array_equal(st[m < 2], np.full((m < 2).sum(), capi.FEAT_TOO_FEW_MEAS))


def test_independence_leg_is_not_vacuous(oracle):
    """`two` without its long track: the same short tracks, all of one class, and the oracle's statistics of them unchanged by the long track's presence
    (every feature's gate reads the prior and its own measurements alone)."""
    case = cs.BY_ID["two"]
    short = cs.two_without_long()
    assert np.array_equal(np.diff(short.meas_offsets), case.lengths[1:])
    assert [k for k, _, _, _ in cs.expected_partition(np.diff(short.meas_offsets))] == [1]
    _, ref = cs.oracle_run(oracle, case)
    _, ref_s = cs.oracle_run(oracle, case, short)
    g = np.isfinite(ref_s["chi2"])
    assert g.sum() >= 2 and np.array_equal(ref_s["chi2"][g], ref["chi2"][1:][g])


def test_partition_rule_small_cases():
    assert cs.expected_partition([]) == []
    assert cs.expected_partition([0, 1, 0]) == [(0, 0, 3, 1)]
    assert cs.expected_partition([9]) == [(1, 0, 1, 9)]
    assert cs.expected_partition([1, 63, 0]) == [(2, 0, 3, 63)]
    assert cs.expected_partition([62, 233, 63, 127, 1]) == [(0, 0, 1, 233), (3, 1, 2, 127), (2, 2, 3, 63), (1, 3, 5, 62)]
