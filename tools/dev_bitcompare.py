"""Two builds of libovgpu.so must give the SAME BYTES: `dump <out.npz>` runs a list of MSCKF updates that reach the fused per-feature
kernel of the headline shape (feat::k_feat_y<4, 11, 2>, both stack precisions) and the other per-feature kernels — the ones only
ovgpu_debug_option "featy_big" and options.feature_kernel_shape reach included — through the library
in the tree and stores every output; `compare <a.npz> <b.npz>` compares two such files bit for bit.  Used when a build changes
nothing but instruction ORDER (a scheduler strategy, ovgpu_featy_tu.hip): no tolerance applies, and no oracle time is spent
(tools/gpu_bitcompare.sh swaps the library files on one box).  `dump` also runs the entries that read the resident feature batch on
small seeded landmark states (batch_scenarios below): used when a change is meant to touch host code only.  `fused <out.npz> <level>` runs
SLAM updates with ovgpu_debug_option "slam_fused" at that level (fused_scenarios below): two builds must agree bit for bit at a level both know;
`fused <out.npz> <level> <big>` also sets "slam_fused_big" and adds the batches only the block-row shapes k_slam_y_big hold.
`init <out.npz> <level>` runs the delayed-initialisation scenarios with "delayed_init_fused" at that level (init_scenarios below), likewise.
`wide <out.npz> [level]` runs updates of 384 .. 511 Jacobian columns (wide_scenarios below), with "gram_wide" at that level when one is given: without
one the name is left alone, and a build that knows the switch must agree bit for bit with one that does not.
`--lib PATH` behind any of the above runs it on that build of the library instead of the tree's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes():
    """(name, synth.make_problem keywords, options, ovgpu_debug_option settings made before the batch is handed over)"""
    for name, pk, ok in default_shapes():
        yield name, pk, ok, {}
    # the per-feature kernels only a switch reaches: k_feat_y_big<8, 17> / <8, 5> on batches the one-pass kernel holds, k_feat_y<8, 17> on one that <4, 9> holds
    for big in (1, 2):
        yield f"14_clones_featy_big{big}", dict(cfg=2, F=60, C=14), {}, dict(featy_big=big)
        yield f"mono_12_clones_featy_big{big}", dict(cfg=2, F=120, C=12, K=1), {}, dict(featy_big=big)
    yield "cfg2_200_kernel_shape2", dict(cfg=2, F=200), dict(feature_kernel_shape=2), {}


def default_shapes():
    from open_vins_amd import capi
    R = capi
    yield "cfg2_400", dict(cfg=2, F=400), {}
    yield "cfg3_headline", dict(cfg=3), {}
    yield "cfg3_every_gate_factored", dict(cfg=3, F=600), dict(gate_always_factor=1)
    yield "cfg3_outliers", dict(cfg=3, F=500, outlier_frac=0.15), {}
    yield "cfg3_ragged", dict(cfg=3, F=500, track="ragged"), {}
    yield "cfg3_fisheye", dict(cfg=3, F=300, fisheye=True), {}
    yield "cfg3_fp32_stack", dict(cfg=3, F=500), dict(gram_fp32=1)
    yield "cfg3_fp32_stack_outliers", dict(cfg=3, F=300, outlier_frac=0.2, track="ragged"), dict(gram_fp32=1, gate_always_factor=1)
    yield "mono_12_clones", dict(cfg=2, F=120, C=12, K=1), {}
    yield "few_clones", dict(cfg=2, F=60, C=5, K=2), {}
    yield "full_inverse_depth", dict(cfg=2, F=200), dict(feat_rep_msckf=R.REP_GLOBAL_FULL_INVERSE_DEPTH)
    yield "no_calibration_no_fej", dict(cfg=2, F=200), dict(do_calib_camera_pose=0, do_calib_camera_intrinsics=0, do_fej=0)
    yield "imu_intrinsics_state", dict(cfg=3, F=300, imu_intrinsics=True), {}
    yield "tight_chi2", dict(cfg=3, F=400), dict(chi2_multipler=0.7)
    yield "one_feature", dict(cfg=2, F=1), {}
    # the 8-wavefront and block-row shapes (translation unit 1: unchanged code, here as the control)
    yield "cfg4_long_tracks", dict(cfg=4, F=300), {}
    yield "cfg5_block_rows", dict(cfg=5, F=60), {}


STAT_INTS = ("n_used", "n_rows", "D", "n_rows_comp", "status", "n_gate_bound")  # (the ms_* fields are timings)
REPS6 = (0, 1, 2, 3, 4, 5)  # capi.REP_GLOBAL_3D .. capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE
CAND = ("meas_offsets", "uv", "uvn", "clone_idx", "cam_idx", "p_FinG_true")


def put(out, prefix, res):
    """every array and integer of a result dictionary (lists of dictionaries entry by entry); timings stay out"""
    for k, v in res.items():
        if k == "stats":
            for i, st in enumerate(v if isinstance(v, list) else [v]):
                out[f"{prefix}.stats{i}"] = np.array([st[j] for j in STAT_INTS])
        elif isinstance(v, np.ndarray):
            out[f"{prefix}.{k}"] = np.ascontiguousarray(v)
        elif isinstance(v, (int, float, np.integer, np.floating)):
            out[f"{prefix}.{k}"] = np.array([v])
        elif isinstance(v, list) and all(isinstance(t, tuple) for t in v):
            out[f"{prefix}.{k}"] = np.array(v, dtype=np.int64).reshape(-1)


def batch_scenarios(out):
    """The entries that read the resident batch, on seeded states of 30 clones and two cameras."""
    import copy
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    n0 = len(out)
    # ovgpu_slam_update: twelve landmarks of all six representations
    p12 = synth.make_slam_problem(2, L=12, lm_rep=np.array(REPS6 * 2, np.int32), seed=3)
    up = UpdaterMSCKF(opts, device=0)
    up.set_slam_problem(p12)
    res = up.slam_update()
    res.update(up.get_state(P=False))
    put(out, "slam_update", res)
    up.close()
    # ovgpu_slam_update_chunked: three chunks, the middle one empty, options that differ between the chunks; then through the restore-and-chain path
    F = p12.F
    sigma, mult = np.where(np.arange(F) < 5, 1.0, 2.5), np.where(np.arange(F) < 5, 1.0, 0.25)
    for tag, fail in (("chunked", None), ("chunked_restore_and_chain", 1)):
        up = UpdaterMSCKF(opts, device=0)
        up.set_slam_problem(p12)
        up.set_feature_options(sigma_pix=sigma, chi2_multipler=mult)
        if fail is not None:
            up.debug_option("slam_chunked_fail_chunk", fail)
        res = up.slam_update_chunked(p12.lm_index, [0, 5, 5, F])
        res.update(up.get_state(P=False))
        res["fallbacks"] = up.debug_option("slam_chunked_fallbacks")
        put(out, tag, res)
        up.close()
    # three resident landmarks, eight candidate tracks: both delayed initialisations (each followed by ovgpu_reset_state) and mode A of it
    cand = copy.copy(synth.make_slam_problem(2, L=3, lm_rep=np.array([0, 5, 2], np.int32), seed=21))
    tracks = synth.make_problem(2, F=8, seed=22)
    for k in CAND:
        setattr(cand, k, getattr(tracks, k))

    def resident():
        u = UpdaterMSCKF(opts, device=0)
        u.set_slam_state(cand)
        u.set_active_landmarks([])
        u.set_features(cand)
        return u

    for tag, fused in (("delayed_init", False), ("delayed_init_fused", True)):
        up = resident()
        res = up.delayed_init(capi.REP_GLOBAL_3D, fused=fused)
        res["landmarks"] = up.get_landmarks()["value"]
        put(out, tag, res)
        up.reset_state()
        put(out, tag + ".after_reset", up.get_state(P=True))
        up.close()
    for first in (0, 2):
        up = resident()
        for f, d in enumerate(up.init_systems(capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH, first_feature=first)):
            put(out, f"init_systems_from_{first}.f{f}", {k: v for k, v in d.items() if v is not None})
        put(out, f"init_systems_from_{first}.state", up.get_state(P=True))
        up.close()
    # ovgpu_msckf_update_lm: an MSCKF batch over resident landmarks that have no column
    lm = copy.copy(synth.make_slam_problem(2, L=8, lm_rep=np.array(REPS6 + (0, 5), np.int32), seed=3))
    tracks = synth.make_problem(2, F=60, seed=4)
    for k in CAND:
        setattr(lm, k, getattr(tracks, k))
    up = UpdaterMSCKF(opts, device=0)
    up.set_slam_state(lm)
    up.set_active_landmarks([])
    up.set_features(lm)
    put(out, "msckf_update_lm", up.update_lm())
    up.close()
    # (ovgpu_msckf_compress: the `.modeA.` arrays of every shape above)
    print("batch scenarios:", len(out) - n0, "arrays", flush=True)


def fused_scenarios(path, level, big=None):
    """ovgpu_slam_update and ovgpu_slam_update_chunked with "slam_fused" = level: fifteen landmarks of the five 3-dof representations (every batch
    takes k_slam_y<false> from level 1 on), and twelve of all six (k_system_t at level 1, k_slam_y<true> at level 2); on the four-camera rig (30 clones,
    tracks of up to 120 observations) ten of the 3-dof representations and twelve of all six: k_system_t up to level 2, the long shapes of k_slam_y
    (kernels 6 and 7) at level 3.  With `big` ("slam_fused_big", set on every context): also the six-landmark batch of tests/slam_big_shapes.py with tracks
    of 209, 169 and 121 observations — four, three and two passes of the block-row plan — and three short ones, on 3-dof landmarks (kernel 8) and with
    the longest track on a single-depth landmark (kernel 9)."""
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    out = {}

    def context(o):
        u = UpdaterMSCKF(o, device=0)
        u.debug_option("slam_fused", level)
        if big is not None:
            u.debug_option("slam_fused_big", big)
        return u

    for tag, reps, rig in (("3dof", (0, 1, 2, 3, 4) * 3, {}), ("six", REPS6 * 2, {}), ("long_3dof", (0, 1, 2, 3, 4) * 2, dict(C=30, K=4)), ("long_six", REPS6 * 2, dict(C=30, K=4))):
        p = synth.make_slam_problem(2, L=len(reps), lm_rep=np.array(reps, np.int32), seed=3, **rig)
        assert not rig or int(np.diff(p.meas_offsets).max()) >= 63, "the long state holds no track of 63 observations"
        for entry in ("update", "chunked"):
            up = context(opts)
            up.set_slam_problem(p)
            res = up.slam_update() if entry == "update" else up.slam_update_chunked(p.lm_index, [0, 5, 5, p.F])
            res.update(up.get_state(P=False))
            res["kernel"], res["fused_batches"] = up.debug_option("last_feature_kernel"), up.debug_option("slam_fused_batches")
            put(out, f"{tag}.{entry}", res)
            print(tag, entry, "level", level, "kernel", res["kernel"], "fused pipelines", res["fused_batches"], flush=True)
            up.close()
    if big is not None:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import slam_big_shapes as sb
        for kind in ("3dof", "single"):
            p = sb.rig_batch(kind, (209, 169, 121, 12, 9, 3), None)
            assert [sb.n_passes(int(m)) for m in np.diff(p.meas_offsets)[:3]] == [4, 3, 2]
            up = context(capi.default_options(chi2_multipler=1.0, **sb.RIG_A_OPTS))
            up.set_slam_problem(p)
            res = up.slam_update()
            res.update(up.get_state(P=False))
            res["kernel"], res["fused_batches"] = up.debug_option("last_feature_kernel"), up.debug_option("slam_fused_batches")
            put(out, f"big_{kind}.update", res)
            print("big", kind, "level", level, "big", big, "kernel", res["kernel"], "fused pipelines", res["fused_batches"], flush=True)
            up.close()
    np.savez(path, **out)


def init_scenarios(path, level):
    """batch_scenarios' delayed-initialisation state (three resident landmarks, eight candidate tracks, one of them made a gross outlier here) with
    "delayed_init_fused" = level: both entries, each followed by ovgpu_reset_state, and mode A.  Level 2 puts k_init_rows in front of the fused
    step and the gate into its tail; ovgpu_slam_delayed_init and ovgpu_slam_init_systems keep their kernels at every level."""
    import copy
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    out = {}
    cand = copy.copy(synth.make_slam_problem(2, L=3, lm_rep=np.array([0, 5, 2], np.int32), seed=21))
    tracks = synth.make_problem(2, F=8, seed=22)
    a, b = int(tracks.meas_offsets[3]), int(tracks.meas_offsets[4])
    uv = tracks.uv.reshape(-1, 2).copy()
    uv[a:b] += np.float32(15.0) * np.where(np.arange(2 * (b - a)).reshape(-1, 2) % 3 == 0, -1, 1).astype(np.float32)  # (uvn stays: the gate reads uv)
    tracks.uv = np.ascontiguousarray(uv.reshape(-1))
    for k in CAND:
        setattr(cand, k, getattr(tracks, k))

    def resident():
        u = UpdaterMSCKF(opts, device=0)
        u.debug_option("delayed_init_fused", level)
        u.set_slam_state(cand)
        u.set_active_landmarks([])
        u.set_features(cand)
        return u

    for rep in (capi.REP_GLOBAL_3D, capi.REP_ANCHORED_INVERSE_DEPTH_SINGLE):
        for tag, fused in (("delayed_init", False), ("delayed_init_fused", True)):
            up = resident()
            res = up.delayed_init(rep, fused=fused)
            res["landmarks"] = up.get_landmarks()["value"]
            res["steps"] = np.array([up.debug_option("delayed_init_fused_steps"), up.debug_option("delayed_init_chain_steps")])
            put(out, f"rep{rep}.{tag}", res)
            up.reset_state()
            put(out, f"rep{rep}.{tag}.after_reset", up.get_state(P=True))
            print(f"rep {rep}", tag, "level", level, "status", res["feat_status"].tolist(), "steps", res["steps"].tolist(), flush=True)
            up.close()
    up = resident()
    for f, d in enumerate(up.init_systems(capi.REP_ANCHORED_MSCKF_INVERSE_DEPTH)):
        put(out, f"init_systems.f{f}", {k: v for k, v in d.items() if v is not None})
    put(out, "init_systems.state", up.get_state(P=True))
    up.close()
    np.savez(path, **out)


def wide_scenarios(path, level=None):
    """Every update entry at 384 .. 511 columns: ovgpu_msckf_update (448 columns, 70 clones stereo, 60 features; then mode A on the same upload),
    ovgpu_slam_update over all columns (476: 30 clones stereo, 100 landmarks of the six representations, a batch of 25), ovgpu_slam_update_chunked
    (64 clones stereo, twelve landmarks in three chunks: 422 / 422 / 424 columns) and ovgpu_msckf_update_lm (412 columns under eight resident
    landmarks).  Without the switch every one of them takes the Householder route."""
    import copy
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    opts = capi.default_options(chi2_multipler=1.0)
    out = {}

    def ctx():
        u = UpdaterMSCKF(opts, device=0)
        if level is not None:
            u.debug_option("gram_wide", level)
        return u

    def tail(u, res):
        res["route"], res["kernel"], res["gram"] = u.lib.ovgpu_last_update_route(u._ctx), u.debug_option("last_feature_kernel"), u.debug_option("last_gram_kernel")
        return res

    p = synth.make_problem(2, C=70, K=2, F=60, seed=5)
    up = ctx()
    up.set_problem(p)
    put(out, "msckf448", tail(up, up.update()))
    up.reset_state()
    put(out, "msckf448.modeA", up.compress())
    up.close()
    full = synth.make_slam_problem(2, L=100, lm_rep=np.array((REPS6 * 17)[:100], np.int32), seed=3)
    q = full.subset(np.arange(25))
    q.lm_index = np.arange(25, dtype=np.int32)
    up = ctx()
    up.set_slam_problem(q)
    res = up.slam_update(q.lm_index)
    res.update(up.get_state(P=False))
    put(out, "slam476", tail(up, res))
    up.close()
    q = synth.make_slam_problem(2, L=12, lm_rep=np.array(REPS6 * 2, np.int32), seed=41, C=64, K=2)
    up = ctx()
    up.set_slam_problem(q)
    res = up.slam_update_chunked(q.lm_index, [0, 4, 8, 12])
    res.update(up.get_state(P=False))
    put(out, "chunked", tail(up, res))
    up.close()
    lm = copy.copy(synth.make_slam_problem(2, L=8, lm_rep=np.array(REPS6 + (0, 5), np.int32), seed=3, C=64, K=2))
    tracks = synth.make_problem(2, F=40, seed=3, C=64, K=2)
    for k in CAND:
        setattr(lm, k, getattr(tracks, k))
    up = ctx()
    up.set_slam_state(lm)
    up.set_active_landmarks([])
    up.set_features(lm)
    put(out, "msckf_update_lm", tail(up, up.update_lm()))
    up.close()
    for k in sorted(out):
        if k.endswith(".route") or k.endswith(".kernel") or k.endswith(".gram"):
            print(k, out[k].tolist(), flush=True)
    np.savez(path, **out)


def prepare(path):
    """The problems are generated once (CPU work: here, not on the GPU box's clock) and travel as a pickle."""
    import pickle
    from open_vins_amd import synth
    probs = {}
    for name, pk, *_ in shapes():
        pk = dict(pk)
        probs[name] = synth.make_problem(pk.pop("cfg"), **pk)
    with open(path, "wb") as f:
        pickle.dump(probs, f)


def dump(path, problems=None):
    import pickle
    from open_vins_amd import capi, synth
    from open_vins_amd.updater import UpdaterMSCKF
    probs = pickle.load(open(problems, "rb")) if problems else {}
    out = {}
    for name, pk, ok, debug in shapes():
        pk = dict(pk)
        prob = probs[name] if name in probs else synth.make_problem(pk.pop("cfg"), **pk)
        opts = capi.default_options(**{"chi2_multipler": 1.0, **ok})
        up = UpdaterMSCKF(opts, device=0)
        for k, v in debug.items():
            up.debug_option(k, v)
        up.set_problem(prob)
        res = up.update()
        out[f"{name}.kernel"] = np.array([up.debug_option("last_feature_kernel")])
        for k in ("feat_status", "chi2", "chi2_thresh", "p_FinG", "dx", "P", "clone_q_p", "calib_q_p", "intrinsics"):
            if k in res:
                out[f"{name}.{k}"] = np.ascontiguousarray(res[k])
        out[f"{name}.route"] = np.array([up.lib.ovgpu_last_update_route(up._ctx), res["stats"]["n_used"], res["stats"]["n_rows"], res["stats"].get("n_gate_bound", 0)])
        # mode A on the same upload: the compressed system the stock EKFUpdate would get
        up.reset_state()
        ca = up.compress()
        for k in ("H", "r", "col_cov_id"):
            if k in ca:
                out[f"{name}.modeA.{k}"] = np.ascontiguousarray(ca[k])
        up.close()
        print(name, "F", prob.F, "used", res["stats"]["n_used"], "route", out[f"{name}.route"][0], flush=True)
    batch_scenarios(out)
    np.savez(path, **out)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "different output sets"
    bad = []
    for k in A.files:
        x, y = A[k], B[k]
        # (numpy.array_equal on the bytes: NaNs — chi2 of a feature that never reached its gate — compare by bit pattern)
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(np.frombuffer(x.tobytes(), np.uint8), np.frombuffer(y.tobytes(), np.uint8)):
            d = float(np.max(np.abs(x.astype(np.float64) - y.astype(np.float64)))) if x.shape == y.shape else float("nan")
            bad.append((k, d))
    print(f"{len(A.files)} arrays compared, {len(bad)} differ")
    for k, d in bad[:40]:
        print("  DIFFERS", k, "max |a - b| =", d)
    return 1 if bad else 0


if __name__ == "__main__":
    if "--lib" in sys.argv:  # another build of the library (the parent commit's): every scenario above loads it through capi.load()
        from open_vins_amd import capi
        at = sys.argv.index("--lib")
        capi.LIB_PATH = os.path.abspath(sys.argv[at + 1])
        del sys.argv[at:at + 2]
    if sys.argv[1] == "prepare":
        prepare(sys.argv[2])
    elif sys.argv[1] == "fused":
        fused_scenarios(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else None)
    elif sys.argv[1] == "init":
        init_scenarios(sys.argv[2], int(sys.argv[3]))
    elif sys.argv[1] == "wide":
        wide_scenarios(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else None)
    elif sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
