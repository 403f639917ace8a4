"""k_feat_y with its requests ahead ("featy_chains" = 1, the default) against the kernel without them (= 0), bit for bit (run with `-m gpu`).

The chains form (open_vins_amd/csrc/k_featy.h: CH) takes the run list of the unprojected stack from k_batch_layout's table, requests the next slot's
record and status a feature ahead and the head's scalars in one go, and takes the bound's verdict behind the first sweep.  It changes no
floating-point operation and no order of one, so for every batch below
  (a) feat_status, chi2, chi2_thresh, dx, P' and the pose tables of the two forms are EQUAL (np.array_equal, NaNs of features that never reach the
      gate included), on the same prior and the same injected triangulation;
  (b) the chains form is held to the oracle at the suite's tolerances (TOL_DX, TOL_P of test_gpu_parity), accept sets identical.
The batches are the smallest at which each change can go wrong: tile rows (2, 8, 9, 25, 33, 60, 63 observations), column blocks (D = 64, 70, 208),
the slot loop (no second slot; exactly one workgroup with a second slot; a feature that fails before the gate between two good ones of one
workgroup), the run list (one region, every region, a single observation in the narrowest, a rejected feature, the projected stack), and two
updates of one batch with the tables rebuilt in between."""
import functools

import numpy as np
import pytest

import track_shapes as ts
from open_vins_amd import capi
from test_gpu_parity import TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

BITWISE = ("feat_status", "chi2", "chi2_thresh", "dx", "P", "clone_q_p", "calib_q_p", "intrinsics")


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _run(Updater, case, tri, chains, updates=1, **debug):
    up = Updater(case.opts())
    for name, val in {**case.debug, **debug, "featy_chains": chains}.items():
        up.debug_option(name, val)
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    outs = []
    for k in range(updates):
        if k:  # the same prior and the same positions again (an update moves the state and the statuses)
            up.reset_state()
            up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        out = up.update()
        out["kernel"], out["raw"] = up.debug_option("last_feature_kernel"), up.debug_option("last_stack_raw")
        outs.append(out)
    up.close()
    return outs


def _assert_same_bits(a, b, what):
    for k in BITWISE:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k)
        assert np.array_equal(x, y, equal_nan=True), (what, k, int(np.sum(~((x == y) | ((x != x) & (y != y))))))


def _hold(case, out, ref, kernel, raw):
    ddx, dP = _rel(out["dx"], ref["dx"]), _rel(out["P"], ref["P"])
    print(f"chains {case.id}: kernel {out['kernel']} raw {out['raw']} F {case.prob.F} used {out['stats']['n_used']} dx {ddx:.2e} P {dP:.2e}")
    assert out["kernel"] == kernel and out["raw"] == raw, (out["kernel"], out["raw"])
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert ddx < TOL_DX and dP < TOL_P


# --------------------------------------------------------------------------- the batches
def _lengths(state, lengths, seed, outlier=None):
    p = ts.with_lengths(ts._window(state, len(lengths), seed), lengths, patterns=("stride",))
    return p if outlier is None else ts.make_outlier(p, outlier, 15.0, seed)


def _two_obs(F):
    return _lengths(ts.SMALL, [2] * F, 410)


def _failed_between(F=1030, f_bad=600, cut=True):
    """1030 tracks of four observations on 512 workgroups.  cut: feature 600 keeps ONE observation and never reaches the gate — the slots go by
    descending track length, so it takes the last one (1029, behind 5 and 517).  Not cut: every track keeps its length and its slot, and _oracle_run fails
    the injected triangulation of feature 515 instead: slot 515, BETWEEN 3 and 1027 in workgroup 3's list (only workgroups 0 .. 5 hold three slots)."""
    lengths = [4] * F
    if cut:
        lengths[f_bad] = 1
    return _lengths(ts.SMALL, lengths, 411)


def _oracle_run(oracle, case):
    """ts.oracle_run with the injected triangulation (the same for the oracle and both forms of the kernel) adjusted: the features of case.tri_failed
    fail; with case.truth_where_failed a track the oracle cannot triangulate (a window of six clones, the clones of one region alone) gets the synthetic
    truth as its position instead, so that it reaches the kernel.  The representation is the global one: p_FinG is all the update reads."""
    fail, truth = getattr(case, "tri_failed", ()), getattr(case, "truth_where_failed", False)
    if not fail and not truth:
        return ts.oracle_run(oracle, case)
    if not hasattr(case, "_ref"):
        v = capi.Views(case.prob)
        tri = {k: np.array(a, copy=True) for k, a in oracle.triangulate(case.opts(), v).items()}
        if truth:
            m = np.diff(case.prob.meas_offsets)
            bad = (tri["status"] != capi.FEAT_USED) & (m >= 2)
            tri["p_FinG"].reshape(-1, 3)[bad] = case.prob.p_FinG_true.reshape(-1, 3)[bad]
            tri["p_FinA"].reshape(-1, 3)[bad] = case.prob.p_FinG_true.reshape(-1, 3)[bad]
            tri["anchor_meas"][bad] = case.prob.meas_offsets[:-1][bad]
            tri["status"][bad] = capi.FEAT_USED
        tri["status"][list(fail)] = capi.FEAT_TRI_FAILED
        case._ref = (tri, oracle.msckf_update(case.opts(), v, want_compressed=False, given=tri))
    return case._ref


def _regions(name_or_state):
    """Eight full tracks cut to the run lists that matter: 0 all in the narrowest region, 1 one observation per region, 2 a single observation in the
    narrowest region and the rest in the top one, 3 .. 6 as they are, 7 a 15 px outlier."""
    st = ts.REGION_STATES[name_or_state] if isinstance(name_or_state, str) else name_or_state
    p = ts._window(st, 8, 420)
    cls, ncls = ts.region_classes(st["C"], st["K"], st.get("pose", 1), st.get("intr", 1))
    picks = []
    for f in range(p.F):
        k = cls[p.clone_idx[int(p.meas_offsets[f]):int(p.meas_offsets[f + 1])]]
        if f == 0:
            pk = np.flatnonzero(k == 0)
        elif f == 1:
            pk = np.asarray(sorted(int(np.flatnonzero(k == c)[0]) for c in np.unique(k)))
        elif f == 2:
            pk = np.concatenate([np.flatnonzero(k == 0)[:1], np.flatnonzero(k == ncls - 1)])
        else:
            pk = np.arange(k.size)
        picks.append(pk)
    assert len(picks[0]) >= 2 and len(picks[1]) == ncls and (cls[0] == 0) and len(picks[2]) >= 3
    return ts.make_outlier(ts.keep_tracks(p, picks), 7, 15.0, 0)


D64, D70 = dict(C=6, K=2), dict(C=7, K=2)  # 6 C + 14 K columns: exactly one block of 64, and a second block of 6 columns


def _case(cid, build, state, **kw):
    return ts.Case(cid, "chains", build, state, **kw)


CASES = [_case(f"m{m}", functools.partial(ts.uniform_batch, m), ts.state_for(m), m_max=m) for m in (2, 8, 9, 25, 33, 60, 63)]
CASES += [_case(f"m{m}-bound", functools.partial(ts.uniform_batch, m), ts.state_for(m), options=dict(gate_always_factor=0), m_max=m) for m in (9, 60)]
CASES += [
    _case("D64", functools.partial(_lengths, D64, [12, 12, 9, 8, 5, 12], 400, 5), D64),
    _case("D70", functools.partial(_lengths, D70, [14, 14, 9, 8, 5, 14], 401, 5), D70),
    _case("F3", functools.partial(_lengths, ts.SMALL, [33, 9, 2], 402), ts.SMALL),
    _case("F513", functools.partial(_two_obs, 513), ts.SMALL),
    _case("F1030-failed", _failed_between, ts.SMALL),
    _case("F1030-failed-between", functools.partial(_failed_between, cut=False), ts.SMALL),
    _case("runs-small", functools.partial(_regions, ts.SMALL), ts.SMALL),
    _case("runs-nt15", functools.partial(_regions, "nt15"), ts.REGION_STATES["nt15"]),
    _case("runs-small-projected", functools.partial(_regions, ts.SMALL), ts.SMALL, debug=dict(raw_stack=0)),
    _case("runs-nt15-projected", functools.partial(_regions, "nt15"), ts.REGION_STATES["nt15"], debug=dict(raw_stack=0)),
]
BY_ID = {c.id: c for c in CASES}
BY_ID["F1030-failed-between"].tri_failed = (515,)
for _c in CASES:
    _c.truth_where_failed = _c.id.startswith(("D64", "D70", "runs-"))


@pytest.mark.parametrize("cid", list(BY_ID))
def test_chains_equal_the_kernel_without_them(Updater, oracle, cid):
    case = BY_ID[cid]
    if cid == "F513":
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        if 2 * cus != 512:
            pytest.skip(f"needs 512 resident workgroups of k_feat_y<4, 9, 2> (two per compute unit), this device holds {2 * cus}")
    tri, ref = _oracle_run(oracle, case)
    kernel = ts.expected_kernel(case.longest_track)
    raw = ts.expected_raw(case.D, kernel) if case.debug.get("raw_stack", 1) else 0
    on, off = _run(Updater, case, tri, 1)[0], _run(Updater, case, tri, 0)[0]
    assert off["kernel"] == kernel and off["raw"] == raw
    _assert_same_bits(on, off, cid)
    _hold(case, on, ref, kernel, raw)
    st = np.asarray(ref["feat_status"])
    if cid.startswith("runs-"):  # the batch holds what it is for: a feature the gate rejects (its rows zeroed through the table) next to accepted ones
        assert st[7] == capi.FEAT_CHI2_REJECTED and np.all(st[:3] == capi.FEAT_USED), st
    if cid in ("D64", "D70"):
        assert st[5] == capi.FEAT_CHI2_REJECTED and np.sum(st == capi.FEAT_USED) >= 3, st
    if cid == "F1030-failed":
        assert st[600] == capi.FEAT_TOO_FEW_MEAS and st[5] == capi.FEAT_USED and st[518] == capi.FEAT_USED, st[[5, 518, 600]]  # (slot 517 holds feature 518)
    if cid == "F1030-failed-between":
        assert st[515] == capi.FEAT_TRI_FAILED and st[3] == capi.FEAT_USED and st[1027] == capi.FEAT_USED, st[[3, 515, 1027]]


@pytest.mark.parametrize("cid", ["runs-small", "m33"])
def test_chains_tables_rebuilt_in_place(Updater, oracle, cid):
    """Two updates of one batch with layout_every_update = 1: the run table is rebuilt in place in front of the second, whose results equal the first's."""
    case = BY_ID[cid]
    tri, ref = _oracle_run(oracle, case)
    first, second = _run(Updater, case, tri, 1, updates=2, layout_every_update=1)
    _assert_same_bits(second, first, cid)
    _hold(case, second, ref, ts.expected_kernel(case.longest_track), ts.expected_raw(case.D, ts.expected_kernel(case.longest_track)))
