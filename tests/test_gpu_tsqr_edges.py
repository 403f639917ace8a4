"""GPU tests (`-m gpu`) that pin the Householder TSQR (csrc/k_tsqr_pw.h, k_tsqr.h, k_compress.h; configure_tsqr, enqueue_compress,
enqueue_merge_tree) and the dense EKF update at every dispatch edge.  All through the C ABI, one context per case.

The systems, the restated dispatch rule, the metric and its bound are tests/tsqr_shapes.py's (checked on numpy alone by
tests/test_tsqr_shapes_cpu.py).  Every compression asserts: the dispatch ovgpu_debug_option reports ("tsqr_leaves", "tsqr_rows_per_node",
"tsqr_last_leaf_kernel", "tsqr_last_tree", "tsqr_last_qh") equals the rule at THIS device's CU count; Hc is cols x cols, its strict lower triangle
exactly zero, everything finite; and

    err = max_ij |(M^T M)_ij - G_ij| / (n_i n_j) <= max(16 e_ref, 256 eps)   (M = [Hc | rc], G in np.longdouble, (i, j) != (cols, cols))

with e_ref the same quantity for numpy.linalg.qr (LAPACK's Householder QR) on the same input, per case.

Measured on the MI355X (256 CUs), worst over the cases of a kernel family: see DESIGN.md §3."""
import ctypes as C

import numpy as np
import pytest

import tsqr_shapes as ts
from open_vins_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Updater():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import UpdaterMSCKF
    return UpdaterMSCKF


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _dp(a):
    return a.ctypes.data_as(capi.c_double_p)


def raw_compress(up, H, r, H_out, r_out):
    """ovgpu_measurement_compress as the C caller sees it: returns (status, rows_out); the outputs are whatever buffers were handed in."""
    rows, cols = H.shape
    n = C.c_int32(-7)
    rc = up.lib.ovgpu_measurement_compress(up._ctx, rows, cols, _dp(H), _dp(r), _dp(H_out), _dp(r_out), C.byref(n))
    return rc, n.value


def read_dispatch(up):
    return tuple(up.debug_option(k) for k in ("tsqr_leaves", "tsqr_rows_per_node", "tsqr_last_leaf_kernel", "tsqr_last_tree", "tsqr_last_qh"))


def want_dispatch(d):
    return (d.W, d.rpn, d.leaf, d.tree, d.qh)


def run_case(Updater, c, num_cu, inplace=False):
    H, r = ts.make_input(c)
    up = Updater(capi.default_options(tsqr_workers=c.workers, **c.opts))
    assert up.debug_option("tsqr_last_leaf_kernel") == -1
    if inplace:
        Hb, rb = H.copy(), r.copy()
        rc, n = raw_compress(up, Hb, rb, Hb, rb)
        Hc, rcv = Hb.reshape(-1)[: c.cols * c.cols].reshape(c.cols, c.cols).copy(), rb[: c.cols].copy()
    else:
        Hc, rcv = np.full((c.cols, c.cols), np.nan), np.full(c.cols, np.nan)
        rc, n = raw_compress(up, H, r, Hc, rcv)
    got = read_dispatch(up)
    up.close()
    assert rc == capi.OK and n == c.cols
    assert got == want_dispatch(c.dispatch(num_cu)), (c.id, got)
    return Hc, rcv


def check_case(c, Hc, rcv, tag=""):
    G, n, e_ref = ts.reference(c)
    assert Hc.shape == (c.cols, c.cols) and rcv.shape == (c.cols,)
    assert np.isfinite(Hc).all() and np.isfinite(rcv).all()
    assert not np.tril(Hc, -1).any()
    err = ts.metric(Hc, rcv, G, n)
    print(f"{c.id}{tag}: family {ts.family(c.dispatch(256))}  err {err:.3e}  e_ref {e_ref:.3e}  err/e_ref {err / max(e_ref, 1e-300):.2f}  bound {ts.bound(e_ref):.3e}")
    assert err <= ts.bound(e_ref), (c.id, err, e_ref)
    for k in c.zero_cols:
        assert not Hc[:, k].any(), (c.id, k)
    return err


# --------------------------------------------------------------------------- (a) column tiles, (b) rows, (c) leaves and tree, (d) degenerate inputs
@pytest.mark.parametrize("cid", ts.CASE_IDS)
def test_compression_at_the_edge(Updater, num_cu, cid):
    c = ts.case(cid, num_cu)
    Hc, rcv = run_case(Updater, c, num_cu, inplace=c.inplace)
    check_case(c, Hc, rcv)
    if c.inplace:  # the same system with separate buffers: the same bits
        H2, r2 = run_case(Updater, c, num_cu)
        assert np.array_equal(H2, Hc) and np.array_equal(r2, rcv)


@pytest.mark.parametrize("name", list(ts.VARIANT_SETS))
def test_tree_variants_agree(Updater, num_cu, name):
    """One input through every merge mode: each within the bound of the truth (test_compression_at_the_edge), and within twice the bound of each
    other — the triangle inequality, on the same column-normalised Gram matrix.  More than that: the modes differ in WHEN a merge node runs, not
    in what it computes (the same leaves, the same pairs (i, i + stride), the same kernels' arithmetic per node), so the bits are the same; a
    node that read a panel before its producer had written it would show here.  The equality of bits is intended: a failure of it is a
    finding about the hand-off between nodes, not noise.  (Each variant is held to the truth by test_compression_at_the_edge.)"""
    ids = ts.VARIANT_SETS[name]
    out = [run_case(Updater, ts.case(cid, num_cu), num_cu) for cid in ids]
    c0 = ts.case(ids[0], num_cu)
    G, n, e_ref = ts.reference(c0)
    M0 = np.concatenate([out[0][0], out[0][1][:, None]], axis=1).astype(np.longdouble)
    G0 = M0.T @ M0
    G0[-1, -1] = G[-1, -1]  # (the residual's own diagonal entry is not part of the metric)
    for cid, (Hc, rcv) in zip(ids[1:], out[1:]):
        e = ts.metric(Hc, rcv, G0, n)
        print(f"{cid} against {ids[0]}: {e:.3e}  identical bits: {np.array_equal(Hc, out[0][0]) and np.array_equal(rcv, out[0][1])}")
        assert e <= 2 * ts.bound(e_ref)
        assert np.array_equal(Hc, out[0][0]) and np.array_equal(rcv, out[0][1]), cid


def test_512_columns_are_refused_and_nothing_is_written(Updater):
    rng = np.random.default_rng(512)
    H, r = rng.normal(size=(512 + 131, 512)), rng.normal(size=512 + 131)
    Ho, ro = np.full((512, 512), 7.0), np.full(512, 7.0)
    up = Updater(capi.default_options())
    rc, n = raw_compress(up, H, r, Ho, ro)
    assert up.debug_option("tsqr_last_leaf_kernel") == -1
    up.close()
    assert rc == capi.ERR_INVALID and n == -7
    assert (Ho == 7.0).all() and (ro == 7.0).all()


@pytest.mark.parametrize("rows,cols", ts.PASS_THROUGH)
def test_pass_through_is_bit_exact(Updater, rows, cols):
    """rows <= cols: nothing to compress (UpdaterHelper.cpp:459-460) — the outputs are the inputs bit for bit, in place and with separate buffers."""
    rng = np.random.default_rng([rows, cols])
    H = rng.normal(size=(rows, cols)) * 10.0 ** rng.uniform(-3, 3, cols)
    r = rng.normal(size=rows)
    up = Updater(capi.default_options())
    Ho, ro = np.full((rows, cols), np.nan), np.full(rows, np.nan)
    rc, n = raw_compress(up, H, r, Ho, ro)
    assert rc == capi.OK and n == rows
    assert Ho.tobytes() == H.tobytes() and ro.tobytes() == r.tobytes()
    Hb, rb = H.copy(), r.copy()
    rc, n = raw_compress(up, Hb, rb, Hb, rb)
    assert rc == capi.OK and n == rows
    assert Hb.tobytes() == H.tobytes() and rb.tobytes() == r.tobytes()
    assert up.debug_option("tsqr_last_leaf_kernel") == -1  # no kernel ran
    up.close()


# --------------------------------------------------------------------------- (e) ovgpu_ekf_update below 240 columns
E_D = [1, 15, 16, 17, 33, 129]
E_NMOD = {1: 15, 15: 0, 16: 1, 17: 15, 33: 0, 129: 1}  # N % 16
_dense = {}


def e_rows(D):
    return sorted({0, 1, D - 1, D, D + 1, D + 130})


def dense_state(D):
    """20 clones and padding rows of P up to N (the smallest beyond the state's own size and D + 8 with N % 16 as E_NMOD says), a random SPD P of
    condition 1e3 and a shuffled subset of its columns; built once per D and never modified (tests/test_gpu_chol_wide.py's dense_case at small D)."""
    if D not in _dense:
        rng = np.random.default_rng(2000 + D)
        prob = synth.make_problem(1, C=20, K=1, F=4, seed=7)
        N = max(prob.N + 1, D + 8)
        while N % 16 != E_NMOD[D]:
            N += 1
        Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
        P = (Q * np.logspace(-3, 0, N)) @ Q.T
        prob.N, prob.P = N, np.ascontiguousarray(0.5 * (P + P.T))
        prob.P.setflags(write=False)
        _dense[D] = (prob, rng.permutation(N)[:D].astype(np.int32))
    return _dense[D]


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("D,rows", [(D, m) for D in E_D for m in e_rows(D)])
def test_dense_ekf_update(Updater, num_cu, D, rows):
    """dx and P' against float64 numpy at the suite's tolerances for this call (dx 1e-8, P' 1e-9 relative, P' exactly symmetric).  rows = 0: the
    library runs the update on a zero triangle — dx is exactly zero and P' is P."""
    prob, cols = dense_state(D)
    rng = np.random.default_rng([D, rows])
    H = rng.normal(size=(rows, D)) / np.sqrt(D)
    r = rng.normal(size=rows) * 0.01
    Pc = prob.P[cols, :]
    S = H @ prob.P[np.ix_(cols, cols)] @ H.T + np.eye(rows)
    K = np.linalg.solve(S, H @ Pc).T if rows else np.zeros((prob.N, 0))
    dx_ref, P_ref = K @ r, prob.P - K @ H @ Pc
    up = Updater(capi.default_options())
    up.set_problem(prob)
    dx, P = up.ekf_update(H, r, cols, 1.0)
    got = read_dispatch(up)
    up.close()
    print(f"D {D} rows {rows} N {prob.N}: dx {rel(dx, dx_ref):.3e}  P {rel(P, P_ref):.3e}")
    assert np.isfinite(dx).all() and np.isfinite(P).all() and np.array_equal(P, P.T)
    if rows == 0:
        assert not dx.any() and rel(P, prob.P) <= 1e-15
        assert got[2] == -1  # no compression kernel ran
        return
    assert rel(dx, dx_ref) < 1e-8 and rel(P, P_ref) < 1e-9
    assert got == want_dispatch(ts.dispatch(rows, D, 0, num_cu))


# --------------------------------------------------------------------------- (f) context hygiene
def test_standalone_calls_leave_the_context_clean(Updater, num_cu):
    """ovgpu_measurement_compress at 300, 40 and 250 columns on a context with a resident problem re-targets the compression buffers three times:
    each result, and the update of a new batch afterwards, equal a fresh context's bit for bit."""
    prob = synth.make_problem(2, F=64)
    opts = capi.default_options(chi2_multipler=1.0)
    cases = [ts.case(i, num_cu) for i in ("b32-300-429-w2", "b-40-257-w0", "b-250-385-w2")]
    fresh = [run_case(Updater, c, num_cu) for c in cases]
    ref = Updater(opts)
    ref.set_problem(prob)
    want = ref.update()
    ref.close()
    up = Updater(opts)
    up.set_problem(prob)
    for c, (H0, r0) in zip(cases, fresh):
        H, r = ts.make_input(c)
        Hc, rcv = up.measurement_compress(H, r)
        assert np.array_equal(Hc, H0) and np.array_equal(rcv, r0), c.id
    up.set_features(prob)
    out = up.update()
    up.close()
    assert out["stats"]["n_used"] > 30
    for k in ("feat_status", "chi2", "dx", "P", "clone_q_p"):
        assert np.array_equal(out[k], want[k], equal_nan=True), k  # (chi2 of a feature that never reached the gate is NaN in both)


def test_update_after_ekf_update_needs_a_new_batch(Updater):
    """ovgpu_ekf_update re-targets Hbig / Rws and drops the resident batch: the next feature update is refused, and runs again after
    ovgpu_set_features."""
    prob = synth.make_problem(2, F=64)
    up = Updater(capi.default_options(chi2_multipler=1.0))
    up.set_problem(prob)
    rng = np.random.default_rng(5)
    cols = np.arange(16, dtype=np.int32)
    _, P1 = up.ekf_update(rng.normal(size=(9, 16)), rng.normal(size=9) * 0.01, cols, 1.0)
    with pytest.raises(capi.OvgpuError) as e:
        up.update()
    assert e.value.code == capi.ERR_NO_STATE
    assert np.array_equal(up.get_state()["P"], P1)  # the refused call touched nothing
    up.set_features(prob)
    out = up.update()
    assert out["stats"]["status"] == 0 and out["stats"]["n_used"] > 30
    up.close()
