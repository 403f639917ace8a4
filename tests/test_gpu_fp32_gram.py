"""The two fp32 Gram kernels of options.gram_fp32 against a float64 Gram matrix, element by element (run with `-m gpu` on an MI355X).

ovgpu_msckf_local_gram hands back G = [H L | r]^T [H L | r] of the whitened stack from gram32::k_gram_f32 (group A: the float stack of the fused
per-feature kernels, "last_gram_kernel" 5) and from gram::k_gram_blk<true> (group B: a float64 stack on a gram_fp32 context, 2).  tests/
fp32_gram_shapes.py holds the cases, the plan of every case, the reference G_ref and the bound 40 u = 2.4e-6 on
e(G) = max |G_ij - G_ref_ij| / (n_i n_j), derived there from the arithmetic; tests/test_fp32_gram_shapes_cpu.py proves on a numpy emulation that
every case sees the faults it is named for at four times that bound.  Per case:

  (1) e32 <= 40 u, and exact zeros where the reference's column is empty;
  (2) every element of the 16 NT square at a row or column >= LD is exactly zero, G == G^T bit for bit, the trailing count is the oracle's n_rows;
  (3) the same batch on a float64 context, by default and with "raw_stack" = 0: e64 <= 1 % of the bound (else the reference is too coarse);
  (4) G32 != G64 and e32 > e64: it really is another arithmetic;
  (5) two runs on one context agree bit for bit;
  (6) update() on the fp32 context: status sets, n_used, n_rows the oracle's, dx and P within the suite's fp32 tolerances, P symmetric;
  (7) "last_gram_kernel", "stack_is_f32", "last_stack_raw" and "last_gram_workgroups" are what the plan says.

test_stale_rows runs three batches through ONE context (a context takes a state of another size with the next ovgpu_set_state, so the third
step changes the macro-column count and the cached tile table is rebuilt): G of every later batch equals bit for bit G of that batch on a fresh
context — the rows of rejected features and the rows behind the stack read as zeros whatever an earlier batch left there."""
import numpy as np
import pytest

import fp32_gram_shapes as fg
from open_vins_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return dict(torch=torch, Updater=UpdaterMSCKF, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _load(up, case, tri):
    up.set_problem(case.prob)
    up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])


def _context(gpu, case, tri, fp32, **debug):
    up = gpu["Updater"](case.opts(fp32=fp32))
    for name, val in {**case.debug, **debug}.items():
        up.debug_option(name, val)
    _load(up, case, tri)
    return up


def _gram(gpu, up, case):
    """(G [LG x LG], the trailing count) of the batch in force"""
    torch = gpu["torch"]
    lg = 16 * ((case.D + 1 + 15) // 16)
    assert up.gram_len() == lg * lg + 1
    g = torch.full((lg * lg + 1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    up.local_gram(g.data_ptr(), want_outputs=False)
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    return g[:-1].reshape(lg, lg).copy(), g[-1]


def _codes(up):
    return {k: up.debug_option(k) for k in ("last_gram_kernel", "stack_is_f32", "last_stack_raw", "last_gram_workgroups")}


def _expected_codes(case, plan):
    if case.group == "A":
        return dict(last_gram_kernel=fg.GK_F32, stack_is_f32=1, last_stack_raw=0, last_gram_workgroups=plan.Gw)
    return dict(last_gram_kernel=fg.GK_BLK, stack_is_f32=0, last_stack_raw=0, last_gram_workgroups=plan.Gb)


def _control(gpu, case, tri, R, **debug):
    up = _context(gpu, case, tri, 0, **debug)
    G, count = _gram(gpu, up, case)
    kernel, wgs = up.debug_option("last_gram_kernel"), up.debug_option("last_gram_workgroups")
    up.close()
    assert kernel not in (0, fg.GK_F32) and count == R["ref"]["stats"]["n_rows"]
    assert wgs == 0 or kernel == fg.GK_BLK
    return G, fg.gram_error(G, R)


@pytest.mark.parametrize("cid", fg.A_IDS + fg.B_IDS)
def test_fp32_gram(gpu, oracle, cid):
    case = fg.BY_ID[cid]
    R = fg.reference(oracle, case)
    tri, ref = R["tri"], R["ref"]
    plan = case.plan(gpu["num_cu"])
    if cid == "deep":
        assert case.rows >= 2.5 * 32 * gpu["num_cu"] and plan.Gb == gpu["num_cu"]
    up = _context(gpu, case, tri, 1)
    G32, count = _gram(gpu, up, case)
    codes = _codes(up)
    G32_again, _ = _gram(gpu, up, case)
    # (3) the float64 controls
    G64, e64 = _control(gpu, case, tri, R)
    G64p, e64p = _control(gpu, case, tri, R, raw_stack=0)
    e32 = fg.gram_error(G32, R)                                                    # (asserts the exact zeros of (1))
    wi, wj = fg.worst_element(G32, R)
    print(f"fp32 gram {cid}: D {case.D} rows {case.rows} kernel {codes['last_gram_kernel']} workgroups {codes['last_gram_workgroups']}  "
          f"e32 {e32 / fg.U:.2f} u at ({wi}, {wj})  e64 {e64:.2e} (raw_stack 0: {e64p:.2e})")
    # (7)
    assert codes == _expected_codes(case, plan), (codes, _expected_codes(case, plan))
    # (1)
    assert e32 <= fg.BOUND, f"e32 {e32 / fg.U:.1f} u at element ({wi}, {wj})"
    # (2)
    ld = case.D + 1
    assert not G32[ld:, :].any() and not G32[:, ld:].any()
    assert np.array_equal(G32, G32.T)
    assert count == ref["stats"]["n_rows"]
    # (3), (4)
    assert e64 <= fg.CONTROL and e64p <= fg.CONTROL, (e64, e64p)
    assert not np.array_equal(G32, G64) and not np.array_equal(G32, G64p)
    assert e32 > e64 and e32 > e64p
    # (5)
    assert np.array_equal(G32, G32_again)
    # (6)
    up.reset_state()
    out = up.update()
    after = _codes(up)
    up.close()
    assert after == codes and out["route"] == capi.COMPRESS_GRAM
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    assert out["stats"]["n_used"] == ref["stats"]["n_used"] and out["stats"]["n_rows"] == ref["stats"]["n_rows"]
    ddx, dP = _rel(out["dx"], ref["dx"]), _rel(out["P"], ref["P"])
    print(f"fp32 gram {cid}: update dx {ddx:.2e} P {dP:.2e}")
    assert ddx < fg.TOL_DX_F32 and dP < fg.TOL_P_F32
    assert np.array_equal(out["P"], out["P"].T)


def test_stale_rows(gpu, oracle):
    """Three batches through one context; see the module's docstring.  (tests/test_fp32_gram_shapes_cpu.py::test_stale_sequence asserts from the
    oracle's stacks that the second batch's rejected features, its tail and the rows its last stage reads behind it lie on rows the first batch
    left non-zero.)"""
    seq = [fg.STALE_FIRST, fg.STALE_SECOND, fg.STALE_THIRD]
    refs = [fg.reference(oracle, c) for c in seq]
    up = gpu["Updater"](seq[0].opts(fp32=1))
    assert up.debug_option("last_gram_workgroups") == 0 and up.debug_option("last_gram_kernel") == 0   # before the first launch
    got = []
    for c, R in zip(seq, refs):
        _load(up, c, R["tri"])
        G, count = _gram(gpu, up, c)
        assert _codes(up) == _expected_codes(c, c.plan(gpu["num_cu"]))
        assert count == R["ref"]["stats"]["n_rows"]
        got.append(G)
    up.close()
    for c, R, G in zip(seq, refs, got):
        fresh = _context(gpu, c, R["tri"], 1)
        Gf, _ = _gram(gpu, fresh, c)
        fresh.close()
        e = fg.gram_error(G, R)
        differ = int(np.sum(G != Gf))
        print(f"fp32 gram {c.id}: rows {c.rows} e32 {e / fg.U:.2f} u, {differ} elements differ from a fresh context")
        assert e <= fg.BOUND
        assert np.array_equal(G, Gf), f"{c.id}: {differ} elements differ from the batch on a fresh context"
