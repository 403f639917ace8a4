"""k_gram_regions and its reduction on small batches that reach every branch (run with `-m gpu` on an MI355X).

The Gram route stacks the unprojected rows in regions by column reach (k_gram.h): region t = 4, 6, .. tile columns below the top one, the top one
(the state's own count rounded up to even, or 15), and the region of the rows the nullspace projection drops, whose tiles are subtracted.  Every
region runs its own instantiation of the k-step loop, 32 rows to an LDS stage, with the operand reads of a 4-row step issued during the products of
the step before; the reduction sums all of an element's partial tiles in a fixed tree.  The batches below are chosen so that between them

  * every instantiated tile-column count (4, 6, 8, 10, 12, 14, 15) has rows and a workgroup             all-counts (D = 238)
  * a region's rows are no multiple of the 32-row stage                                                 every batch (asserted from the plan)
  * a region fits in ONE stage, so no stage s + 2 exists and the clamped fetch runs                     one-stage (30 rows in the narrowest region)
  * a region has no rows and no workgroup                                                               top-only (K = 4, newest clones only)
  * workgroups run several stages (the LDS double buffer turns over, stage s + 2 is fetched)            deep (256 tracks: ~3 stages per workgroup)
  * a feature is rejected before the gate and one by the gate, so their rows are zeroed                 every batch
  * the dropped rows' region is subtracted                                                              every batch (no update is right without it)

Assertions per batch: (1) dx and P' against the oracle at the suite's tolerances (dx 1e-8, P 1e-9, accept sets identical: the oracle's own
triangulation is injected); (2) two consecutive updates of the same prior agree bit for bit; (3) the Gram matrix with the operand reads a k-step
ahead equals bit for bit the one with every k-step opening on its own reads (ovgpu_debug_option "gram_read_ahead" = 0: the same products in the
same order); (4) the executed tile-row count the library reports ("raw_gram_tile_rows") is the one the rows' reaches predict, computed here from
the clone indices alone (track_shapes.region_classes restates the host's rule).

The clone counts (20 .. 35) are what the tile-column counts need: 15 tile columns are 238 Jacobian columns."""
import functools

import numpy as np
import pytest

import track_shapes as ts
from open_vins_amd import capi
from test_gpu_parity import TOL_DX, TOL_P

pytestmark = pytest.mark.gpu

STAGE = 32                  # rows per LDS stage (k_gram.h: GR_ROWS)


def _state_args(st):
    return st["C"], st["K"], st.get("pose", 1), st.get("intr", 1)


def _batch(state, F, seed, drop_class0_from=None, newest_only=False, px=15.0):
    """F full tracks of the window; feature 0 cut to ONE observation (rejected before the gate), feature F - 1 an outlier of px pixels (rejected
    by the gate; on the short baseline of newest_only a 15-pixel offset fails the triangulation instead of reaching the gate: 8 there).
    drop_class0_from = n: features n .. lose their observations in the clones of the narrowest region; newest_only: every track keeps the
    clones of the top region only."""
    p = ts._window(state, F, seed)
    cls, n = ts.region_classes(*_state_args(state))
    if newest_only:
        p = ts.clone_range(p, int(np.sum(cls < n - 1)), state["C"])
    picks = []
    for f in range(p.F):
        a, b = int(p.meas_offsets[f]), int(p.meas_offsets[f + 1])
        keep = np.arange(b - a)
        if f == 0:
            keep = keep[:1]
        elif drop_class0_from is not None and f >= drop_class0_from:
            keep = keep[cls[p.clone_idx[a:b]] != 0]
        picks.append(keep)
    return ts.make_outlier(ts.keep_tracks(p, picks), F - 1, px, seed)


NT15, D208, K4, NT14 = ts.REGION_STATES["nt15"], ts.SMALL, ts.REGION_STATES["K4"], ts.REGION_STATES["nt14"]
CASES = [
    ts.Case("all-counts", "g", functools.partial(_batch, NT15, 24, 400), NT15),
    ts.Case("deep", "g", functools.partial(_batch, D208, 256, 401), D208),
    ts.Case("top-only", "g", functools.partial(_batch, K4, 20, 402, newest_only=True, px=8.0), K4),
    ts.Case("one-stage", "g", functools.partial(_batch, NT14, 20, 403, drop_class0_from=3), NT14),
]
BY_ID = {c.id: c for c in CASES}


def _plan(case):
    """(tile columns, rows) of every region of the unprojected stack, the dropped rows' region last — from the clone indices of the batch alone."""
    C, K, pose, intr = _state_args(case.state)
    D = ts.n_columns(C, K, pose, intr)
    calib_end, ntf = D - 6 * C, (D + 1 + 15) // 16
    top = 15 if ntf == 15 else (ntf + 1) & ~1
    ntc = [t for t in range(4, top, 2) if 16 * t - 4 >= calib_end + 6] + [top]
    cls, n = ts.region_classes(C, K, pose, intr)
    assert n == len(ntc)
    rows = [2 * int(np.sum(cls[case.prob.clone_idx] == k)) for k in range(n)]
    return ntc + [top], rows + [4 * case.prob.F]


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _updater(Updater, case, tri, **debug):
    up = Updater(case.opts())
    for name, val in debug.items():
        up.debug_option(name, val)
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
    return up


def _gram(Updater, case, tri, **debug):
    import torch
    up = _updater(Updater, case, tri, **debug)
    g = torch.empty(up.gram_len(), dtype=torch.float64, device="cuda")
    up.local_gram(g.data_ptr(), want_outputs=False)
    torch.cuda.synchronize()
    assert up.debug_option("last_stack_raw") == 1
    up.close()
    return g.cpu().numpy()


def test_the_batches_cover_the_branches():
    """The plan of every batch, from its clone indices: the coverage the module's docstring claims."""
    plans = {c.id: _plan(c) for c in CASES}
    ntc, rows = plans["all-counts"]
    assert ntc[:-1] == [4, 6, 8, 10, 12, 14, 15] and all(r > 0 for r in rows)
    for cid, (ntc, rows) in plans.items():
        assert any(r % STAGE for r in rows), cid
    ntc, rows = plans["one-stage"]
    assert 0 < rows[0] <= STAGE and rows[0] % STAGE
    ntc, rows = plans["top-only"]
    assert len(rows) >= 3 and not any(rows[:-2]) and rows[-2] > 0
    ntc, rows = plans["deep"]
    assert sum((r + STAGE - 1) // STAGE for r in rows) >= 2.5 * 256  # stages per workgroup at one workgroup per compute unit


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_gram_regions_batch(Updater, oracle, cid):
    case = BY_ID[cid]
    tri, ref = ts.oracle_run(oracle, case)
    st = ref["feat_status"]
    assert (st == capi.FEAT_CHI2_REJECTED).any() and (st == capi.FEAT_USED).any()
    assert ((st != capi.FEAT_CHI2_REJECTED) & (st != capi.FEAT_USED)).any(), "no feature is rejected before the gate"
    up = _updater(Updater, case, tri)
    out = up.update()
    assert up.debug_option("last_stack_raw") == 1 and out["route"] == capi.COMPRESS_GRAM
    # (4) the executed products: rows x tiles of the region's triangle, from the rows' reaches
    ntc, rows = _plan(case)
    want = sum(r * t * (t + 1) // 2 for t, r in zip(ntc, rows))
    got = up.debug_option("raw_gram_tile_rows")
    print(f"gram regions {cid}: D {case.D} regions {list(zip(ntc, rows))} tile rows {got}")
    assert got == want, (got, want)
    # (1) the oracle
    ddx, dP = _rel(out["dx"], ref["dx"]), _rel(out["P"], ref["P"])
    print(f"gram regions {cid}: dx {ddx:.2e} P {dP:.2e}")
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    assert ddx < TOL_DX and dP < TOL_P
    assert np.array_equal(out["P"], out["P"].T)
    # (2) the same prior again
    up.reset_state()
    again = up.update()
    up.close()
    assert np.array_equal(again["dx"], out["dx"]) and np.array_equal(again["P"], out["P"])
    # (3) the k-step with its reads ahead against the k-step that opens on its own reads
    g1, g0 = _gram(Updater, case, tri), _gram(Updater, case, tri, gram_read_ahead=0)
    n = 16 * ((case.D + 1 + 15) // 16)
    G = g1[:-1].reshape(n, n)
    assert g1[-1] == ref["stats"]["n_rows"] and np.array_equal(G, G.T) and np.abs(G[:case.D + 1, :case.D + 1]).max() > 0
    assert np.array_equal(g1, g0)
