"""CPU test of the identity the anchored fast path stands on: for an MSCKF feature in an anchored representation
H_f = A dl and the anchor blocks are A H_anc, A H_calib with the same A = dz / dp_FinG row by row (UpdaterHelper.cpp:374-421); every MSCKF
representation is 3-dof (UpdaterMSCKF.cpp:180-183), so dl is invertible, the left nullspace of H_f is A's, and the nullspace projection
annihilates both anchor blocks.  With do_fej the anchored feature is linearised at the "best" p_FinG (UpdaterHelper.cpp:282-287), the point a
global feature uses.  So the oracle's update under feat_rep_msckf = 2 .. 5 is its update under 0, up to rounding, on the same triangulation.

The oracle is pinned by the reference's own sources (tests/test_ref_fixtures.py); nothing here needs a GPU.  Tolerances are the GPU parity suite's
own, imported.  The accept sets are compared without excuses: the test asserts that no feature of these inputs sits within GATE_MARGIN of its
threshold."""
import numpy as np
import pytest

from open_vins_amd import capi, synth
from parity_util import GATE_MARGIN
from test_gpu_parity import TOL_CHI2, TOL_DX, TOL_P

# 14 clones stereo; a ragged window with 30 % outliers; four cameras; 11 clones mono; fisheye
SHAPES = {
    "14_clones_stereo": dict(F=60, C=14),
    "ragged_outliers": dict(F=200, track="ragged", outlier_frac=0.3),
    "cfg4": dict(cfg=4, F=100),
    "11_clones_mono": dict(F=150, C=11, K=1),
    "fisheye": dict(F=100, fisheye=True),
}
ANCHORED = [capi.REP_ANCHORED_3D, capi.REP_ANCHORED_FULL_INVERSE_DEPTH, capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]


def make(shape):
    kw = dict(SHAPES[shape])
    return synth.make_problem(kw.pop("cfg", 2), **kw)


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.fixture(scope="module")
def updates(oracle):
    """per shape: the oracle's update under GLOBAL_3D and under every anchored representation, on one triangulation (computed once, shared)"""
    cache = {}

    def get(shape):
        if shape not in cache:
            prob = make(shape)
            v = capi.Views(prob)
            tri = oracle.triangulate(capi.default_options(chi2_multipler=1.0), v)
            cache[shape] = {rep: oracle.msckf_update(capi.default_options(chi2_multipler=1.0, feat_rep_msckf=rep), v, given=tri)
                            for rep in [capi.REP_GLOBAL_3D] + ANCHORED}
        return cache[shape]
    return get


@pytest.mark.parametrize("shape", list(SHAPES))
def test_no_feature_sits_at_its_gate_threshold(updates, shape):
    for rep, ref in updates(shape).items():
        gate = np.isfinite(ref["chi2"])
        assert gate.sum() >= 10
        margin = np.abs(ref["chi2"][gate] / ref["chi2_thresh"][gate] - 1.0).min()
        print(f"{shape} rep {rep}: closest feature {margin:.3e} (relative) from its threshold")
        assert margin > GATE_MARGIN


@pytest.mark.parametrize("rep", ANCHORED)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_anchored_update_is_the_global_update(updates, shape, rep):
    g, a = updates(shape)[capi.REP_GLOBAL_3D], updates(shape)[rep]
    assert g["stats"]["status"] == 0 and a["stats"]["status"] == 0
    assert np.array_equal(a["feat_status"], g["feat_status"])
    assert (g["feat_status"] == capi.FEAT_USED).sum() >= 10
    if shape == "ragged_outliers":
        assert (g["feat_status"] == capi.FEAT_CHI2_REJECTED).sum() >= 5  # the gate was exercised
    gate = np.isfinite(g["chi2"])
    assert np.array_equal(gate, np.isfinite(a["chi2"]))
    e_chi2 = np.abs(a["chi2"][gate] / g["chi2"][gate] - 1.0).max()
    e_dx, e_P = _rel(a["dx"], g["dx"]), _rel(a["P"], g["P"])
    print(f"{shape} rep {rep}: chi2 {e_chi2:.3e}  dx {e_dx:.3e}  P {e_P:.3e}")
    assert np.array_equal(a["chi2_thresh"][gate], g["chi2_thresh"][gate])
    assert a["stats"]["n_used"] == g["stats"]["n_used"] and a["stats"]["n_rows"] == g["stats"]["n_rows"]
    assert e_chi2 < TOL_CHI2 and e_dx < TOL_DX and e_P < TOL_P


@pytest.mark.parametrize("shape", list(SHAPES))
def test_single_depth_is_the_msckf_inverse_depth(updates, shape):
    """UpdaterMSCKF.cpp:180-183: ANCHORED_INVERSE_DEPTH_SINGLE is replaced by ANCHORED_MSCKF_INVERSE_DEPTH — the same arithmetic, the same bits"""
    a, b = updates(shape)[capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH], updates(shape)[capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE]
    assert np.array_equal(a["feat_status"], b["feat_status"]) and np.array_equal(a["chi2"], b["chi2"], equal_nan=True)
    assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["P"], b["P"])
