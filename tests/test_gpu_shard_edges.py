"""GPU tests (`-m gpu`) of the feature-sharded MSCKF update at every route, tile, rank-count and shard edge: G ranks on ONE device through the
loop-back communicator (MultiUpdater(devices=[0] * G): the production local stage, exchange and update around a test double of the transport), the
building blocks ovgpu_msckf_local / _merge_update and ovgpu_msckf_local_gram / _gram_update on separate contexts, and the native entry
ovgpu_msckf_update_sharded in a world of one.  The batches and what each is named for: tests/shard_shapes.py; tests/test_shard_shapes_cpu.py holds
every one of them to it on the oracle alone and records the floor of the sharded reference against the unsharded one (dx 8e-14, P' 7e-15).

Every rank gets the ORACLE's triangulation of its shard (ovgpu_multi_ctx + ovgpu_set_triangulation, shards by the restated deal) and the contexts
run with gate_always_factor = 1, as tests/test_gpu_track_edges.py runs its own: everything downstream is then compared.  Bounds, against the oracle
and against the single-context update alike: chi2 1e-8 relative, thresholds 1e-12, dx 1e-8, P' 1e-9 relative Frobenius and
exactly symmetric, poses 1e-9; the gram_fp32 case dx 1e-4, P' 1e-3.  Status sets, n_used and n_rows are the oracle's with no excuse: no batch
leaves a statistic within 1e-6 of its threshold.  Every rank's state is bit-identical to rank 0's and to the returned P'.  What each rank reports
(ovgpu_last_update_route, "tsqr_last_tree", "tsqr_last_qh", "last_gram_kernel", "last_feature_kernel", "last_stack_raw", the change of
"chol_wide_factorisations") is compared with shard_shapes' restatement of the rules.

ovgpu_multi_msckf_update cannot repeat an update whose single-launch Cholesky timed out on one rank for want of co-scheduling (include/ovgpu.h:
OVGPU_ERR_HIP, a scheduling event when several processes share the device; "the caller uploads the state again on every rank"): run_frame does
what the header tells a caller to do, ONCE, and test_zz_worst_deviations prints how often it had to.  Buffers handed to the library are
allocated and filled on torch's stream and the device synchronised before the library, on its own stream, writes them.

Worst deviations, measured on the MI355X (every test prints its own, test_zz_worst_deviations the maxima per group): DESIGN.md section 7."""
import ctypes as C

import numpy as np
import pytest

import shard_shapes as sh
from open_vins_amd import capi
from parity_util import assert_chi2

pytestmark = pytest.mark.gpu

G_, T_ = sh.GRAM, sh.TSQR
STATE_KEYS = ("clone_q_p", "calib_q_p", "intrinsics")
FEAT_KEYS = ("feat_status", "chi2", "chi2_thresh", "p_FinG")
REPEATS = []  # the frames whose update was repeated after a rank's time-out (the docstring)
WORST = {}   # (group, comparator, quantity) -> largest deviation so far
_ONE = {}    # the single-context update of a batch: computed once, shared, left unchanged


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    from open_vins_amd.updater import MultiUpdater, UpdaterMSCKF

    class Rank(UpdaterMSCKF):
        """rank g of a set, borrowed: the context belongs to the set"""

        def __init__(self, m, g, prob):
            self.lib, self._ctx = m.lib, C.c_void_p(m.lib.ovgpu_multi_ctx(m._m, g))
            assert self._ctx
            self.N, self.Cn, self.K, self.F = int(prob.N), int(prob.C), int(prob.K), 0

        def close(self):
            self._ctx = C.c_void_p()

    return dict(torch=torch, Multi=MultiUpdater, One=UpdaterMSCKF, Rank=Rank, num_cu=torch.cuda.get_device_properties(0).multi_processor_count)


def note(group, comparator, **dev):
    for k, v in dev.items():
        if np.isfinite(v):
            WORST[(group, comparator, k)] = max(WORST.get((group, comparator, k), 0.0), float(v))


def deviations(a, b):
    gate = np.isfinite(b["chi2"])
    dev = dict(dx=sh.rel(a["dx"], b["dx"]), P=sh.rel(a["P"], b["P"]), poses=max(np.abs(a[k] - b[k]).max() for k in STATE_KEYS))
    if gate.any():
        dev["chi2"] = np.abs(a["chi2"][gate] / b["chi2"][gate] - 1.0).max()
        dev["thr"] = np.abs(a["chi2_thresh"][gate] / b["chi2_thresh"][gate] - 1.0).max()
    return dev


def hold(dev, out, what, tol_dx=sh.TOL_DX, tol_p=sh.TOL_P, tol_pose=sh.TOL_POSE):
    """the bounds of the docstring; every figure is printed before it is asserted"""
    print(f"{what}: " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
    assert dev.get("chi2", 0.0) < sh.TOL_CHI2 and dev.get("thr", 0.0) < sh.TOL_THR, what
    assert dev["dx"] < tol_dx, what
    assert dev["P"] < tol_p and np.array_equal(out["P"], out["P"].T), what
    assert dev["poses"] < tol_pose, what


def same_bits(a, b, what, keys=FEAT_KEYS + ("dx", "P")):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def single_context(gpu, case, tri):
    key = (case.problem_key, case.route, tuple(sorted(case.options.items())), tuple(sorted(case.state.items())))
    if key not in _ONE:
        up = gpu["One"](case.opts())
        up.set_problem(case.prob)
        up.set_triangulation(tri["p_FinG"], tri["p_FinA"], tri["anchor_meas"], tri["status"])
        _ONE[key] = up.update()
        up.close()
    return _ONE[key]


# --------------------------------------------------------------------------- a set of G ranks on device 0
def open_set(gpu, case):
    m = gpu["Multi"](case.opts(), devices=[0] * case.G)
    for g in range(case.G):
        r = gpu["Rank"](m, g, case.prob)
        for name, val in case.debug.items():
            r.debug_option(name, val)
    return m


def run_frame(gpu, m, case, tri):
    """upload, the oracle's triangulation to every rank, one update; what every rank reports and holds afterwards"""
    prob, G, shards = case.prob, case.G, case.deal
    ranks = [gpu["Rank"](m, g, prob) for g in range(G)]

    def upload():
        chol0 = [r.debug_option("chol_wide_factorisations") for r in ranks]
        m.set_problem(prob)
        for g, r in enumerate(ranks):  # the deal, as every rank holds it
            ids = shards[g]
            got, sub = r.get_features(), sh.shard_problem(prob, ids)
            assert np.array_equal(got["meas_offsets"], sub.meas_offsets), (case.id, g, "the deal")
            assert np.array_equal(got["clone_idx"], sub.clone_idx) and np.array_equal(got["cam_idx"], sub.cam_idx) and np.array_equal(got["uv"], sub.uv), (case.id, g)
            if ids:
                r.F = len(ids)
                t = sh.shard_triangulation(prob, tri, ids)
                r.set_triangulation(t["p_FinG"], t["p_FinA"], t["anchor_meas"], t["status"])
        return chol0

    chol0 = upload()
    try:
        out = m.update()
    except capi.OvgpuError as e:
        if e.code != capi.ERR_HIP or "timed out" not in str(e):
            raise
        print(f"{case.id}: {e}: the state uploaded again on every rank, the update repeated once")
        REPEATS.append(case.id)
        chol0 = upload()
        out = m.update()
    out["ranks"] = []
    for g, r in enumerate(ranks):
        rep = dict(route=r.lib.ovgpu_last_update_route(r._ctx), tree=r.debug_option("tsqr_last_tree"), qh=r.debug_option("tsqr_last_qh"),
                   gram=r.debug_option("last_gram_kernel"), kernel=r.debug_option("last_feature_kernel"), raw=r.debug_option("last_stack_raw"),
                   chol=r.debug_option("chol_wide_factorisations") - chol0[g], f32=r.debug_option("stack_is_f32"))
        rep.update(r.get_state())
        out["ranks"].append(rep)
    out.update({k: out["ranks"][0][k] for k in STATE_KEYS})
    return out


def assert_replicas(out, case):
    """every rank holds rank 0's posterior and the returned P', bit for bit"""
    r0 = out["ranks"][0]
    for g, r in enumerate(out["ranks"]):
        for k in ("P",) + STATE_KEYS:
            assert np.array_equal(r[k], r0[k]), (case.id, g, k)
    assert np.array_equal(r0["P"], out["P"]), case.id


def assert_reports(gpu, out, case, ref):
    """what every rank reports against the restated rules"""
    nt, gram, shards = sh.tiles(case.D), case.gram, case.deal
    used = ref["feat_status"] == capi.FEAT_USED
    for g, r in enumerate(out["ranks"]):
        what = (case.id, g, {k: v for k, v in r.items() if not isinstance(v, np.ndarray)})
        assert r["route"] == (G_ if gram else T_), what
        assert (r["chol"] > 0) == sh.chol_is_wide(case.D), what  # (the replicated factorisation: counted where it is enqueued, rows or none)
        if not gram:
            assert r["tree"] == sh.tree_mode(nt, case.G, gpu["num_cu"], case.options.get("tsqr_no_pipeline", 0)), what
            assert r["qh"] == sh.merge_qh(nt), what
        if shards[g]:
            assert gram or r["gram"] == 0, what
            assert r["kernel"] == case.rank_kernel(g), what
            assert r["raw"] == case.rank_raw(g), what
            assert r["f32"] == (1 if gram and case.options.get("gram_fp32", 0) else 0), what
        if shards[g] and used[shards[g]].any():  # a rank with rows
            assert r["gram"] == case.rank_gram_kernel(g), what


def check_case(gpu, oracle, case, m=None):
    tri, ref = sh.oracle_run(oracle, case)
    own = m is None
    m = open_set(gpu, case) if own else m
    out = run_frame(gpu, m, case, tri)
    if own:
        m.close()
    # status sets, counts and the per-feature outputs at the CALLER's indices (the statistics differ pairwise: a permuted feat_of cannot pass)
    assert np.array_equal(out["feat_status"], ref["feat_status"]), (case.id, out["feat_status"], ref["feat_status"])
    for k in ("D", "n_rows", "n_used"):
        assert out["stats"][k] == ref["stats"][k], (case.id, k, out["stats"][k], ref["stats"][k])
    assert_chi2(out, ref, sh.TOL_CHI2, strict=True)
    assert np.array_equal(out["p_FinG"], tri["p_FinG"]), case.id
    assert_replicas(out, case)
    assert_reports(gpu, out, case, ref)
    what = f"{case.id} D {case.D} G {case.G} {'gram' if case.gram else 'triangles'}"
    if ref["stats"]["n_used"] == 0:
        # Nothing accepted anywhere: dx is zero and every rank keeps the upload's covariance, bit for bit.  The poses are the upload [+] 0, as the
        # oracle returns them: a quaternion is normalised again (four roundings at the most: 4 eps), positions and intrinsics keep their bits.
        assert not out["dx"].any() and np.array_equal(out["P"], case.prob.P), case.id
        eps = float(np.finfo(np.float64).eps)
        for k in STATE_KEYS:
            up, dev = np.asarray(getattr(case.prob, k), dtype=np.float64), np.abs(out[k] - ref[k]).max()
            print(f"{what}: nothing accepted, {k} against the upload {np.abs(out[k] - up).max():.3e}, against the oracle {dev:.3e}")
            assert dev < sh.TOL_POSE, (case.id, k)
            assert np.abs(out[k] - up)[..., :4].max() <= 4 * eps and np.array_equal(out[k][..., 4:], up[..., 4:]), (case.id, k)
        return out, ref
    # the poses are the upload [+] dx: where dx is held to the fp32 twins' bound, no component of them can be held to more than that share of |dx|
    tol_pose = sh.TOL_POSE if case.tol_dx == sh.TOL_DX else case.tol_dx * float(np.linalg.norm(ref["dx"]))
    group = case.group + ("-fp32" if case.options.get("gram_fp32", 0) else "")
    d_or = deviations(out, ref)
    note(group, "oracle", **d_or)
    hold(d_or, out, what + " against the oracle", case.tol_dx, case.tol_p, tol_pose)
    one = single_context(gpu, case, tri)
    assert np.array_equal(one["feat_status"], out["feat_status"])
    d_one = deviations(out, one)
    note(group, "single context", **d_one)
    hold(d_one, out, what + " against the single context", case.tol_dx, case.tol_p, tol_pose)
    return out, ref


# --------------------------------------------------------------------------- (a) every state x both exchanges x G
@pytest.mark.parametrize("cid", [c.id for c in sh.CASES if c.group == "a"])
def test_states_exchanges_and_rank_counts(gpu, oracle, cid):
    case = sh.BY_ID[cid]
    out, ref = check_case(gpu, oracle, case)
    assert out["stats"]["n_used"] >= 1 and (out["feat_status"][list(case.rejected)] == capi.FEAT_CHI2_REJECTED).all()
    if case.D == 384:  # triangles on every context, whatever "gram_wide" says
        assert all(r["route"] == T_ and r["kernel"] == 0 for r in out["ranks"])


# --------------------------------------------------------------------------- (b) shards that contribute nothing
@pytest.mark.parametrize("cid", [c.id for c in sh.CASES if c.group == "b"])
def test_shards_that_contribute_nothing(gpu, oracle, cid):
    case = sh.BY_ID[cid]
    out, ref = check_case(gpu, oracle, case)
    if "none" in cid:
        assert out["stats"]["n_used"] == 0 and out["stats"]["n_rows"] == 0
    if "rank-rejected" in cid:
        assert (out["feat_status"][case.deal[1]] == capi.FEAT_CHI2_REJECTED).all() and (out["feat_status"][case.deal[0]] == capi.FEAT_USED).all()


# --------------------------------------------------------------------------- (c) ranks that differ in kind
@pytest.mark.parametrize("cid", [c.id for c in sh.CASES if c.group == "c"])
def test_ranks_that_differ_in_kind(gpu, oracle, cid):
    case = sh.BY_ID[cid]
    out, ref = check_case(gpu, oracle, case)
    r0, r1 = out["ranks"]
    assert r0["route"] == r1["route"] == G_
    if cid == "c-long-track":
        assert (r0["kernel"], r1["kernel"]) == (0, 1)
    if cid == "c-raw-and-projected":
        assert (r0["raw"], r1["raw"]) == (0, 1) and (r0["gram"], r1["gram"]) == (sh.GK_ONE_PASS, sh.GK_REGIONS)
    if cid == "c-fp32":
        assert r0["gram"] == r1["gram"] == sh.GK_F32 and r0["f32"] == r1["f32"] == 1


# --------------------------------------------------------------------------- the cross-checks, on purpose
def _adhoc(D, G, route, F=12, **options):
    return sh.Case(f"x-{D}-G{G}", "x", sh.state_of(D), sh.table_batch(D, F, (3,)), G, route, options=options, rejected=(3,))


def test_gram_exchange_agrees_across_rank_counts(gpu, oracle):
    """one problem on 2, 3, 4 and 8 ranks: every sum of shard Gram matrices gives the single-context update within the bounds"""
    outs = {}
    for G in (2, 3, 4, 8):
        case = _adhoc(250, G, G_)
        outs[G], ref = check_case(gpu, oracle, case)
    for G in (3, 4, 8):
        d = deviations(outs[G], outs[2])
        note("x", "two ranks", **d)
        hold(d, outs[G], f"D 250 gram G {G} against G 2")


@pytest.mark.parametrize("G", [2, 3, 5])
def test_triangle_exchange_is_independent_of_the_merge_mode(gpu, oracle, G):
    """D = 250 (16 tile columns): the one-launch tree and the level-by-level merge (tsqr_no_pipeline) run the same node arithmetic in the same
    pairing — bit-identical posteriors, as tests/test_gpu_tsqr_edges.py holds its merge modes to"""
    a, ref = check_case(gpu, oracle, _adhoc(250, G, T_))
    b, _ = check_case(gpu, oracle, _adhoc(250, G, T_, tsqr_no_pipeline=1))
    assert all(r["tree"] == sh.TREE_BEHIND for r in a["ranks"]) and all(r["tree"] == sh.TREE_LEVELS for r in b["ranks"])
    same_bits(a, b, f"G {G}: one-launch tree against level by level")


# --------------------------------------------------------------------------- (d) life cycle of one set
@pytest.mark.parametrize("route", [G_, T_], ids=["gram", "tsqr"])
def test_life_cycle_of_one_set(gpu, oracle, route):
    """four ranks through four frames (three on the Householder set): a wide batch, two features (ranks 2 and 3 empty after holding work), a new
    state of other column count, the triangle exchange at 384 columns on the same contexts — each frame the bits of a fresh set"""
    frames = range(len(sh.LIFE)) if route == G_ else range(3)
    first = sh.life_case(0, route)
    m = open_set(gpu, first)
    for k in frames:
        case = sh.life_case(k, route)
        tri, ref = sh.oracle_run(oracle, case)
        out, _ = check_case(gpu, oracle, case, m)
        fresh_set = open_set(gpu, case)
        fresh = run_frame(gpu, fresh_set, case, tri)
        fresh_set.close()
        same_bits(out, fresh, f"frame {k}: the set that lived through frames 0 .. {k - 1} against a fresh one")
        for g in range(case.G):
            assert np.array_equal(out["ranks"][g]["P"], fresh["ranks"][g]["P"]), (k, g)
        if k == 1:
            assert case.deal[2] == [] and case.deal[3] == []
    m.close()


@pytest.mark.parametrize("route", [G_, T_], ids=["gram", "tsqr"])
@pytest.mark.parametrize("D", sh.FALLS_EMPTY_AT)
def test_a_rank_that_falls_empty(gpu, oracle, D, route):
    """the life cycle's second frame at the widths its states do not reach: twelve features on four ranks, then two, on the last one-pass Gram kernel
    and k_qr_node leaf (250 columns) and on k_gram_blk and the k_qr_append leaf (256) — ranks 2 and 3 must not leak what they held"""
    name = "gram" if route == G_ else "tsqr"
    full = sh.BY_ID[f"a-{D}-G4-{name}"]
    two = sh.falls_empty_case(D, route)
    m = open_set(gpu, full)
    check_case(gpu, oracle, full, m)
    out, _ = check_case(gpu, oracle, two, m)
    m.close()
    tri, _ = sh.oracle_run(oracle, two)
    fresh_set = open_set(gpu, two)
    fresh = run_frame(gpu, fresh_set, two, tri)
    fresh_set.close()
    same_bits(out, fresh, f"D {D} {name}: two features after twelve against a fresh set")


# --------------------------------------------------------------------------- (e) building blocks on separate contexts
def _shard_context(gpu, case, tri, ids):
    u = gpu["One"](case.opts())
    u.set_problem(sh.shard_problem(case.prob, ids))
    if len(ids):
        t = sh.shard_triangulation(case.prob, tri, ids)
        u.set_triangulation(t["p_FinG"], t["p_FinA"], t["anchor_meas"], t["status"])
    return u


@pytest.mark.parametrize("D", sh.MERGE_D)
@pytest.mark.parametrize("G", sh.MERGE_G)
def test_local_and_merge_update(gpu, oracle, D, G):
    """ovgpu_msckf_local on up to three shards, ovgpu_msckf_merge_update of G triangles (the ones beyond the real shards are zero triangles):
    the reserve of max(G, 16) triangles at 16 | 17, no merge at G = 1"""
    torch = gpu["torch"]
    case = sh.block_case(D, T_)
    tri, ref = sh.oracle_run(oracle, case)
    shards = sh.deal(case.lengths, min(G, sh.MERGE_REAL))
    ups = [_shard_context(gpu, case, tri, ids) for ids in shards]
    n = ups[0].triangle_len()
    assert n == D * (D + 1)
    buf = torch.zeros(G * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = np.zeros(case.prob.F, np.int32)
    chi2 = np.zeros(case.prob.F)
    for k, (u, ids) in enumerate(zip(ups, shards)):
        loc = u.local(buf[k * n:(k + 1) * n].data_ptr())
        st[ids], chi2[ids] = loc["feat_status"], loc["chi2"]
    torch.cuda.synchronize()
    out = ups[-1].merge_update(buf.data_ptr(), G)
    out.update(ups[-1].get_state(P=False))
    tree, qh = ups[-1].debug_option("tsqr_last_tree"), ups[-1].debug_option("tsqr_last_qh")
    for u in ups:
        u.close()
    assert np.array_equal(st, ref["feat_status"])
    np.testing.assert_allclose(chi2, ref["chi2"], rtol=sh.TOL_CHI2)
    if G > 1:
        assert (tree, qh) == (sh.tree_mode(sh.tiles(D), G, gpu["num_cu"]), sh.merge_qh(sh.tiles(D)))
    dev = dict(dx=sh.rel(out["dx"], ref["dx"]), P=sh.rel(out["P"], ref["P"]), poses=max(np.abs(out[k] - ref[k]).max() for k in STATE_KEYS))
    note("e", "oracle", **dev)
    hold(dev, out, f"merge of {G} triangles at D {D} against the oracle")
    one = single_context(gpu, case, tri)
    dev = dict(dx=sh.rel(out["dx"], one["dx"]), P=sh.rel(out["P"], one["P"]), poses=max(np.abs(out[k] - one[k]).max() for k in STATE_KEYS))
    note("e", "single context", **dev)
    hold(dev, out, f"merge of {G} triangles at D {D} against the single context")


@pytest.mark.parametrize("D", sh.LOCAL_GRAM_D)
def test_local_gram_and_gram_update(gpu, oracle, D):
    """ovgpu_msckf_local_gram on two shards and an EMPTY one, the buffers summed, ovgpu_msckf_gram_update on every one of the three contexts (the
    empty shard's too: it whitened nothing itself): the trailing element is the oracle's n_rows, the three posteriors agree bit for bit"""
    torch = gpu["torch"]
    case = sh.block_case(D, G_)
    tri, ref = sh.oracle_run(oracle, case)
    shards = sh.deal(case.lengths, 2) + [[]]
    ups = [_shard_context(gpu, case, tri, ids) for ids in shards]
    nt = sh.tiles(D)
    total = None
    for u, ids in zip(ups, shards):
        n = u.gram_len()
        assert n == (16 * nt) ** 2 + 1
        t = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        loc = u.local_gram(t.data_ptr())
        assert np.array_equal(loc["feat_status"], ref["feat_status"][ids])
        if ids:
            assert u.debug_option("last_gram_kernel") == sh.gram_kernel(D, sh.rank_raw(D, sh.rank_kernel(int(case.lengths[ids].max()), True), True))
        else:
            assert not t.cpu().numpy().any()
        total = t if total is None else total + t
    torch.cuda.synchronize()
    assert int(total[-1].item()) == ref["stats"]["n_rows"]
    Gm = total[:-1].reshape(16 * nt, 16 * nt).cpu().numpy()
    assert np.array_equal(Gm, Gm.T) and not Gm[D + 1:, :].any() and np.isfinite(Gm).all()
    outs = []
    for u in ups:
        o = u.gram_update(total.data_ptr())
        o.update(u.get_state(P=False))
        outs.append(o)
        u.close()
    for k, o in enumerate(outs):
        print(f"D {D}: context {k} ({len(shards[k])} features) against the oracle  dx {sh.rel(o['dx'], ref['dx']):.3e}  P {sh.rel(o['P'], ref['P']):.3e}")
    for k in (1, 2):
        same_bits(outs[k], outs[0], f"D {D}: context {k} against context 0", keys=("dx", "P") + STATE_KEYS)
    dev = dict(dx=sh.rel(outs[2]["dx"], ref["dx"]), P=sh.rel(outs[2]["P"], ref["P"]), poses=max(np.abs(outs[2][k] - ref[k]).max() for k in STATE_KEYS))
    note("e", "oracle", **dev)
    hold(dev, outs[2], f"summed Gram matrices at D {D} against the oracle")
    one = single_context(gpu, case, tri)
    dev = dict(dx=sh.rel(outs[2]["dx"], one["dx"]), P=sh.rel(outs[2]["P"], one["P"]), poses=max(np.abs(outs[2][k] - one[k]).max() for k in STATE_KEYS))
    note("e", "single context", **dev)
    hold(dev, outs[2], f"summed Gram matrices at D {D} against the single context")


def test_gram_blocks_refuse_384_columns(gpu, oracle):
    """ovgpu_gram_len / ovgpu_msckf_local_gram / ovgpu_msckf_gram_update at 25 tile columns: OVGPU_ERR_CAPACITY, the state's bits unchanged"""
    torch = gpu["torch"]
    case = sh.block_case(384, G_)
    tri, _ = sh.oracle_run(oracle, case)
    u = _shard_context(gpu, case, tri, list(range(case.prob.F)))
    before = u.get_state()
    n = C.c_int64(0)
    assert u.lib.ovgpu_gram_len(u._ctx, C.byref(n)) == capi.ERR_CAPACITY
    t = torch.zeros(400 * 400 + 1, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert u.lib.ovgpu_msckf_local_gram(u._ctx, None, None, None, None, C.c_void_p(t.data_ptr()), None) == capi.ERR_CAPACITY
    assert u.lib.ovgpu_msckf_gram_update(u._ctx, C.c_void_p(t.data_ptr()), None, None, None) == capi.ERR_CAPACITY
    after = u.get_state()
    u.close()
    for k in ("P",) + STATE_KEYS:
        assert np.array_equal(before[k], after[k]), k


def test_a_follower_timeout_in_the_gram_block_is_an_error(gpu, oracle):
    """k_chol.h: with the followers' wait bound at zero every follower gives up and the kernels behind the factorisation are switched off.
    ovgpu_msckf_gram_update cannot repeat the update itself: it must say so (OVGPU_ERR_HIP) instead of returning an update that never happened,
    leave the state's bits, and deliver the normal result when called again with the same buffer."""
    torch = gpu["torch"]
    D = 250
    case = sh.block_case(D, G_)
    tri, ref = sh.oracle_run(oracle, case)
    shards = sh.deal(case.lengths, 2)
    ups = [_shard_context(gpu, case, tri, ids) for ids in shards]
    n = ups[0].gram_len()
    bufs = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in ups]
    torch.cuda.synchronize()
    for u, t in zip(ups, bufs):
        u.local_gram(t.data_ptr(), want_outputs=False)
    torch.cuda.synchronize()
    buf = bufs[0] + bufs[1]
    torch.cuda.synchronize()
    u = ups[1]
    bound = u.debug_option("chol_follow_spin_limit", 0)
    assert bound == 1 << 22 and u.debug_option("chol_timeouts") == 0
    with pytest.raises(capi.OvgpuError) as e:
        u.gram_update(buf.data_ptr())
    assert e.value.code == capi.ERR_HIP and u.debug_option("chol_timeouts") == 1
    st = u.get_state()
    assert np.array_equal(st["P"], case.prob.P)
    for k in STATE_KEYS:
        assert np.array_equal(st[k], getattr(case.prob, k)), k
    u.debug_option("chol_follow_spin_limit", bound)
    out = u.gram_update(buf.data_ptr())
    out.update(u.get_state(P=False))
    for x in ups:
        x.close()
    dev = dict(dx=sh.rel(out["dx"], ref["dx"]), P=sh.rel(out["P"], ref["P"]), poses=max(np.abs(out[k] - ref[k]).max() for k in STATE_KEYS))
    hold(dev, out, f"Gram block at D {D}, called again after the time-out, against the oracle")


# --------------------------------------------------------------------------- (f) the native entry in a world of one
@pytest.mark.parametrize("D", sh.WORLD_OF_ONE_D)
def test_native_entry_in_a_world_of_one(gpu, oracle, D):
    """ovgpu_comm_init_rank + ovgpu_msckf_update_sharded, synchronous and _async: the bits of ovgpu_msckf_update on a fresh context"""
    case = sh.block_case(D, G_)
    tri, ref = sh.oracle_run(oracle, case)
    one = single_context(gpu, case, tri)
    ids = list(range(case.prob.F))
    b = _shard_context(gpu, case, tri, ids)
    b.comm_init_single()
    out = b.update_sharded()
    route = b.lib.ovgpu_last_update_route(b._ctx)
    b.reset_state()
    b.update_sharded_async()
    b.synchronize()
    again = b.get_state()
    b.close()
    assert route == (G_ if sh.exchange_is_gram(G_, D) else T_) == one["route"]
    assert np.array_equal(out["feat_status"], ref["feat_status"])
    same_bits(out, one, f"D {D}: ovgpu_msckf_update_sharded against ovgpu_msckf_update", keys=FEAT_KEYS + ("dx", "P") + STATE_KEYS)
    assert np.array_equal(again["P"], one["P"])
    for k in STATE_KEYS:
        assert np.array_equal(again[k], one[k]), k


# --------------------------------------------------------------------------- (g) refusals and error returns
def test_nine_ranks_on_one_device_are_refused(gpu):
    reader = gpu["One"](capi.default_options())
    live = (reader.debug_option("live_allocations"), reader.debug_option("live_allocation_bytes"))
    m = C.c_void_p()
    devs = np.zeros(9, np.int32)
    opts = capi.default_options()
    rc = reader.lib.ovgpu_multi_create(C.byref(opts), 9, devs.ctypes.data_as(capi.c_int32_p), C.byref(m))
    assert rc == capi.ERR_CAPACITY and not m
    assert (reader.debug_option("live_allocations"), reader.debug_option("live_allocation_bytes")) == live
    ok = gpu["Multi"](opts, devices=[0] * sh.LOOP_MAX_RANKS)  # ... and eight are not
    assert ok.lib.ovgpu_multi_size(ok._m) == 8
    ok.close()
    assert (reader.debug_option("live_allocations"), reader.debug_option("live_allocation_bytes")) == live
    reader.close()


def test_the_native_entry_refuses_a_loop_back_rank(gpu, oracle):
    case = sh.BY_ID["a-208-G2-gram"]
    m = open_set(gpu, case)
    m.set_problem(case.prob)
    r = gpu["Rank"](m, 1, case.prob)
    assert r.lib.ovgpu_msckf_update_sharded_async(r._ctx) == capi.ERR_INVALID
    before = r.get_state()
    assert np.array_equal(before["P"], case.prob.P)
    m.close()


def test_a_prior_block_that_does_not_factor(gpu, oracle):
    """D = 208, the two newest clones perfectly correlated.  The world of one repeats through the Householder route (include/ovgpu.h) and matches
    the oracle.  ovgpu_multi_msckf_update does not repeat: OVGPU_ERR_NOT_SPD for the set, every rank's state the upload's bits."""
    case = sh.semi_definite_case(1)
    tri, ref = sh.oracle_run(oracle, case)
    assert ref["stats"]["status"] == 0 and ref["stats"]["n_used"] >= 5
    b = _shard_context(gpu, case, tri, list(range(case.prob.F)))
    b.comm_init_single()
    out = b.update_sharded()
    route = b.lib.ovgpu_last_update_route(b._ctx)
    b.close()
    assert route == T_ and out["stats"]["status"] == 0
    assert np.array_equal(out["feat_status"], ref["feat_status"]) and out["stats"]["n_used"] == ref["stats"]["n_used"]
    assert_chi2(out, ref, sh.TOL_CHI2, strict=True)
    d = deviations(out, ref)
    note("g", "oracle", **d)
    hold(d, out, "semi-definite prior, world of one, against the oracle")
    # the set of two ranks
    case2 = sh.semi_definite_case(2)
    m = open_set(gpu, case2)
    prob = case2.prob
    m.set_problem(prob)
    ranks = [gpu["Rank"](m, g, prob) for g in range(2)]
    for g, r in enumerate(ranks):
        ids = case2.deal[g]
        r.F = len(ids)
        t = sh.shard_triangulation(prob, tri, ids)
        r.set_triangulation(t["p_FinG"], t["p_FinA"], t["anchor_meas"], t["status"])
    with pytest.raises(capi.OvgpuError) as e:
        m.update()
    assert e.value.code == capi.ERR_NOT_SPD
    for r in ranks:
        s = r.get_state()
        assert np.array_equal(s["P"], prob.P)
        for k in STATE_KEYS:
            assert np.array_equal(s[k], getattr(prob, k)), k
    # ... and the set recovers on the Householder exchange after the same upload
    m.close()
    tsqr = sh.semi_definite_case(2, T_)
    tsqr.rejected = tuple(np.flatnonzero(ref["feat_status"] == capi.FEAT_CHI2_REJECTED))
    check_case(gpu, oracle, tsqr)


# --------------------------------------------------------------------------- the worst deviations
def test_zz_worst_deviations():
    """prints the worst deviation per group: against the oracle, and sharded against the single context (DESIGN.md section 7 quotes them)"""
    for (grp, comp, k), v in sorted(WORST.items()):
        print(f"worst ({grp}) against the {comp}: {k} {v:.3e}")
    print(f"updates repeated after a rank's time-out: {len(REPEATS)} {REPEATS}")
    for (grp, comp, k), v in WORST.items():
        if grp.endswith("-fp32"):
            continue  # (its own bounds, asserted where it runs)
        assert v < dict(chi2=sh.TOL_CHI2, thr=sh.TOL_THR, dx=sh.TOL_DX, P=sh.TOL_P, poses=sh.TOL_POSE)[k], (grp, comp, k, v)
