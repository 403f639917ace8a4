"""k_triangulate and the anchors of k_batch_layout at every rejection clause, loop exit, stride-loop trip and seeded refusal (run with `-m gpu` on an
MI355X).

Every case of tests/tri_shapes.py — shown on the oracle alone, by tests/test_tri_shapes_cpu.py, to reach what it is named for with nothing
within 1e-6 of a threshold or 1e-10 of an LM decision — runs through ovgpu_triangulate / ovgpu_refine on a fresh context and is held to the ORACLE:
statuses and anchor measurements equal for EVERY feature, no exclusions; accepted p_FinA and p_FinG within the suite's TOL_TRI = 1e-9 m; every
feature the device rejects all NaN, and where the oracle's own arrays are NaN (TOO_FEW_MEAS, TRI_FAILED, and every refusal of pyoracle.refine) the
patterns are equal.  One difference is by contract, not by accident: for GN_FAILED the reference leaves the refined p_FinA and the linear p_FinG on
its Feature, and oracle.triangulate reports them; the device reports NaN (include/ovgpu.h: entries of failed features are unspecified).

Groups: the thresholds and loop exits on B in the four modes (3-D / 1-D, with / without refinement), tracks of 0 .. 254 observations (one to four
trips of the 64-lane stride loops), the anchor rule on camera runs carried across 64-measurement chunks, degenerate inputs among healthy
neighbours, forced workgroup sizes, the seeded path, and the pose table at the LDS limit (over the limit: OVGPU_ERR_CAPACITY from the host,
nothing launched).  Each case prints one line `tri ...` with its deviations (DESIGN.md quotes them)."""
import numpy as np
import pytest

import tri_shapes as t
from open_vins_amd import capi

pytestmark = pytest.mark.gpu

TOL_TRI = 1e-9  # tests/test_gpu_parity.py: measured max 5e-11 m


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _hold_to_the_oracle(out, ref, who, anchors=True):
    ok = ref["status"] == t.USED
    dA = np.abs(out["p_FinA"][ok] - ref["p_FinA"][ok]).max() if ok.any() else 0.0
    dG = np.abs(out["p_FinG"][ok] - ref["p_FinG"][ok]).max() if ok.any() else 0.0
    wrong = np.flatnonzero(out["status"] != ref["status"])
    print(f"tri {who}: F {len(ok)} used {int(ok.sum())} status differs at {wrong.tolist()} |dp_FinA| {dA:.2e} |dp_FinG| {dG:.2e}")
    assert len(wrong) == 0, (wrong, out["status"][wrong], ref["status"][wrong])  # every feature, no excuse
    if anchors:
        assert np.array_equal(out["anchor_meas"], ref["anchor_meas"])
    # NaN patterns: the device leaves NaN for whatever it rejects and finite values for whatever it accepts; the oracle's NaN entries are among them
    for k in ("p_FinA", "p_FinG"):
        assert np.isnan(out[k][~ok]).all() and np.isfinite(out[k][ok]).all() and np.isfinite(ref[k][ok]).all()
        hard = np.isin(ref["status"], [t.TOO_FEW, t.TRI_FAILED])
        assert np.isnan(ref[k][hard]).all() and np.array_equal(np.isnan(out[k][hard]), np.isnan(ref[k][hard]))
    assert dA < TOL_TRI and dG < TOL_TRI


def _claims(case, out, oracle):
    for (kind, name), least in case.claims.items():
        if kind == "status":
            assert int((out["status"] == name).sum()) >= least, (name, least)


def _triangulate(Updater, opts, prob, **debug):
    up = Updater(opts)
    for name, val in debug.items():
        up.debug_option(name, val)
    up.set_problem(prob)
    out = up.triangulate()
    up.close()
    return out


@pytest.mark.parametrize("cid", [c.id for c in t.CASES])
def test_tri_edge(Updater, oracle, cid):
    case = t.BY_ID[cid]
    prob, ref = t.problem(oracle, cid), t.oracle_trace(oracle, cid)
    for (kind, name), least in case.claims.items():  # the case still is what it says (tests/test_tri_shapes_cpu.py says why)
        assert t.count(ref, kind, name, oracle) >= least
    out = _triangulate(Updater, case.opts(), prob)
    _hold_to_the_oracle(out, ref, cid)
    _claims(case, out, oracle)
    for f in case.named:
        assert out["status"][f] == t.TRI_FAILED


@pytest.mark.parametrize("n", [13, 1])
def test_forced_workgroup_sizes_change_nothing(Updater, oracle, n):
    """ovgpu_debug_option "tri_waves": 1, 3, 8 and 16 features per workgroup — a last workgroup that is partly empty, a batch smaller than one
    workgroup — give the unforced launch's result bit for bit."""
    prob = t.base().subset(np.arange(n))
    opts = capi.default_options()
    ref = oracle.triangulate(opts, capi.Views(prob))
    base = _triangulate(Updater, opts, prob)
    _hold_to_the_oracle(base, ref, f"first-{n}")
    for w in (1, 3, 8, 16):
        out = _triangulate(Updater, opts, prob, tri_waves=w)
        for k in ("status", "anchor_meas", "p_FinA", "p_FinG"):
            assert _bits(out[k], base[k]), (w, k)


def _refine(Updater, opts, prob, pA, an):
    up = Updater(opts)
    up.set_problem(prob)
    out = up.refine(pA, an)
    got = up.get_triangulation()
    up.close()
    for k in ("p_FinA", "p_FinG"):  # ovgpu_get_triangulation afterwards: the same arrays
        assert _bits(got[k], out[k]), k
    out["anchor_meas"] = got["anchor_meas"]
    return out


@pytest.mark.parametrize("cid", [c.id for c in t.SEED_CASES])
def test_seeded_refinement(Updater, oracle, cid):
    case = t.SEED_BY_ID[cid]
    prob, pA, an, where = t.seed_setup(oracle, cid)
    ref = t.oracle_refine(oracle, cid)
    for (kind, name), least in case.claims.items():
        assert t.count(ref, kind, name, oracle) >= least
    out = _refine(Updater, case.opts(), prob, pA, an)
    _hold_to_the_oracle(out, ref, cid)
    assert np.array_equal(np.isnan(out["p_FinA"]), np.isnan(ref["p_FinA"])) and np.array_equal(np.isnan(out["p_FinG"]), np.isnan(ref["p_FinG"]))
    _claims(case, out, oracle)
    for f in case.refused:
        g = where[f]
        assert out["status"][g] == t.TRI_FAILED and out["anchor_meas"][g] == -1
    for f in case.nan_seed:
        assert out["status"][where[f]] == t.GN_FAILED
    if case.refused:  # the neighbours of a refused feature: bit-equal to a run in which every anchor is good
        prob0, pA0, an0, _ = t.seed_setup(oracle, "seed-default")
        assert prob0.F == prob.F and _bits(pA0, pA)
        good = _refine(Updater, case.opts(), prob0, pA0, an0)
        others = np.setdiff1d(np.arange(prob.F), [where[f] for f in case.refused])
        assert (good["status"][[where[f] for f in case.refused]] != t.TRI_FAILED).all()
        for k in ("status", "anchor_meas", "p_FinA", "p_FinG"):
            assert _bits(out[k][others], good[k][others]), k


def _dp(a):
    return a.ctypes.data_as(capi.c_double_p)


def test_pose_table_at_the_lds_limit(Updater, oracle):
    """ovgpu_set_camera_poses with B's clones at 823 .. 852 of an 853-clone stereo table: 163 776 of the 163 840 bytes of LDS, the kernel's whole
    staging loop and its highest table indices.  One clone more, or the largest rig the entry admits, is refused by enqueue_triangulate with
    OVGPU_ERR_CAPACITY before anything is launched (a refusal by the runtime would be OVGPU_ERR_HIP), and the context goes on working."""
    opts = capi.default_options()
    ref = oracle.triangulate(opts, capi.Views(t.base()))
    prob = t.shifted_base()
    up = Updater(opts)
    assert up.debug_option("sys_lds_limit") == t.LDS_LIMIT

    def run(Cn, K):
        R, p = t.embedded_pose_table(Cn, K)
        capi.check(up.lib.ovgpu_set_camera_poses(up._ctx, Cn, K, _dp(R), _dp(p)), "ovgpu_set_camera_poses")
        up.set_features(prob)
        out = dict(p_FinA=np.zeros((prob.F, 3)), p_FinG=np.zeros((prob.F, 3)), anchor_meas=np.zeros(prob.F, np.int32), status=np.zeros(prob.F, np.int32))
        rc = up.lib.ovgpu_triangulate(up._ctx, _dp(out["p_FinA"]), _dp(out["p_FinG"]), out["anchor_meas"].ctypes.data_as(capi.c_int32_p),
                                      out["status"].ctypes.data_as(capi.c_int32_p))
        return rc, out

    rc, first = run(t.LDS_C, 2)
    assert rc == capi.OK, up.lib.ovgpu_last_error()
    _hold_to_the_oracle(first, ref, f"C-{t.LDS_C}")
    for Cn, K in ((t.LDS_C + 1, 2), (1024, 64)):
        rc, _ = run(Cn, K)
        msg = up.lib.ovgpu_last_error().decode()
        assert rc == capi.ERR_CAPACITY, (rc, msg)
        assert f"K = {K}" in msg and f"C = {Cn}" in msg and str(t.LDS_LIMIT) in msg, msg
    rc, again = run(t.LDS_C, 2)
    assert rc == capi.OK, up.lib.ovgpu_last_error()
    for k in ("status", "anchor_meas", "p_FinA", "p_FinG"):
        assert _bits(again[k], first[k]), k
    up.close()
