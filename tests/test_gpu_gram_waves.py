"""k_gram_regions with two wavefronts per SIMD against the form with one (run with `-m gpu` on an MI355X).

ovgpu_debug_option "gram_waves" = 8 | 4 selects the workgroup of k_gram_regions (k_gram.h): eight wavefronts that share a region's tile triangle by
a compile-time deal per tile-column count (a tile row may be split between two of them by column range) and stage 32 rows with 512 threads, or
the four wavefronts with four tile rows each.  Either way one wavefront accumulates a tile over the rows in ascending order, four rows to a
product, from zero — so on the same workgroup table (the same "raw_work_const") the Gram matrices are equal BIT FOR BIT, and that is what is
asserted here, on the four small batches of test_gpu_gram_regions_shapes.py (every instantiated tile-column count, a region inside one stage,
regions without rows, workgroups of several stages: that file asserts the coverage from the plans).  Per batch:

  (1) G under 8 wavefronts == G under 4, bit for bit;   (2) two consecutive runs at 8 agree bit for bit;
  (3) "raw_gram_tile_rows" is the same under both and is what the rows' reaches predict.

One batch more is asked for: a workgroup with a SINGLE chunk whose region's row count is no multiple of 32, at the narrowest width (4 tile
columns: wavefronts with one or two tiles, more staging slots than tiles).  `one-stage` is that batch; its plan is asserted below."""
import numpy as np
import pytest

import track_shapes as ts
from test_gpu_gram_regions_shapes import CASES, STAGE, _gram, _plan, _updater

pytestmark = pytest.mark.gpu

BY_ID = {c.id: c for c in CASES}
WORK_CONST = 12  # the same workgroup table on both sides, whatever the library's default becomes


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


def _gram_runs(Updater, case, tri, waves, runs):
    """`runs` Gram matrices of the batch from ONE context under `waves` wavefronts, and the executed tile-row count it reports."""
    import torch
    up = _updater(Updater, case, tri, gram_waves=waves, raw_work_const=WORK_CONST)
    assert up.debug_option("gram_waves") == waves
    out = []
    for _ in range(runs):
        g = torch.zeros(up.gram_len(), dtype=torch.float64, device="cuda")
        up.reset_state()
        up.local_gram(g.data_ptr(), want_outputs=False)
        torch.cuda.synchronize()
        out.append(g.cpu().numpy())
    assert up.debug_option("last_stack_raw") == 1 and up.debug_option("last_gram_kernel") == 4
    tile_rows = up.debug_option("raw_gram_tile_rows")
    up.close()
    return out, tile_rows


def test_one_stage_is_a_single_partial_chunk_at_four_columns():
    """The narrowest region of `one-stage`: 4 tile columns, between 1 and 31 rows — one workgroup, one chunk, the clamped fetch, a partial stage."""
    ntc, rows = _plan(BY_ID["one-stage"])
    assert ntc[0] == 4 and 0 < rows[0] < STAGE


def test_the_option_takes_4_and_8_only(Updater, oracle):
    from open_vins_amd import capi
    case = BY_ID["one-stage"]
    tri, _ = ts.oracle_run(oracle, case)
    up = _updater(Updater, case, tri)
    assert up.debug_option("gram_waves") in (4, 8)
    for bad in (0, 2, 6, 16):
        with pytest.raises(capi.OvgpuError):
            up.debug_option("gram_waves", bad)
    up.close()


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_eight_wavefronts_equal_four_bit_for_bit(Updater, oracle, cid):
    case = BY_ID[cid]
    tri, ref = ts.oracle_run(oracle, case)
    (g8, g8_again), rows8 = _gram_runs(Updater, case, tri, 8, 2)
    (g4,), rows4 = _gram_runs(Updater, case, tri, 4, 1)
    n = 16 * ((case.D + 1 + 15) // 16)
    G = g8[:-1].reshape(n, n)
    assert g8[-1] == ref["stats"]["n_rows"] and np.array_equal(G, G.T) and np.abs(G[:case.D + 1, :case.D + 1]).max() > 0
    differ = int(np.sum(g8 != g4))
    print(f"gram waves {cid}: {g8.size} doubles, {differ} differ between 8 and 4 wavefronts, tile rows {rows8} / {rows4}")
    assert np.array_equal(g8, g4)                      # (1)
    assert np.array_equal(g8, g8_again)                # (2)
    ntc, rows = _plan(case)                            # (3)
    assert rows8 == rows4 == sum(r * t * (t + 1) // 2 for t, r in zip(ntc, rows))
    # the library's default form gives the same matrix as well
    assert np.array_equal(_gram(Updater, case, tri, raw_work_const=WORK_CONST), g8)
