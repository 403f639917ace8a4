"""The catalogue of batches that pin the whitened Gram route of mode B at 384 .. 511 Jacobian columns (ovgpu_debug_option "gram_wide" = 1:
k_gram_blk over four column windows, the fused per-feature kernels over 7 and 8 blocks of 64 columns and 13 to 16 blocks of 32) at its column,
tile, window, block and dispatch edges: tests/test_gram_wide_shapes_cpu.py checks every batch on the oracle alone, tests/test_gpu_gram_wide.py
runs it on the device.

The rules below — which route an update takes, which per-feature kernel the library reports — are restated FROM THEIR DOCUMENTED TERMS
(include/ovgpu.h: "gram_wide", "slam_fused", OVGPU_COMPRESS_GRAM), not from the library.  Snapshots come from synth.make_problem /
make_slam_problem, tracks are cut with track_shapes' helpers.  Column counts: D = 6 C + K (6 pose + 8 intr) + 3 per 3-dof landmark + 1 per
single-depth landmark.  An MSCKF state reaches even counts only; the odd counts and 511 are SLAM states.  States beyond 64 clones take their
window from the 95 s excerpt of the corridor trajectory (synth.load_traj_window).

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import slam_long_shapes as s3
import slam_shapes as ss
import track_shapes as ts
from open_vins_amd import capi

SINGLE = ss.SINGLE
NARROW_MAX_D = 383   # 24 tile columns of [H | r]: the route without the switch
WIDE_MAX_D = 511     # 32 tile columns: with it; also the interface's bound


# --------------------------------------------------------------------------- the rules, restated
def tiles(D):
    """tile columns of [H | r]: 16 columns each, the residual column included"""
    return (D + 1 + 15) // 16


def windows(D):
    """column windows of k_gram_blk: 8 tile columns each"""
    return (tiles(D) + 7) // 8


def fourth_window_tiles(D):
    return max(0, tiles(D) - 24)


def blocks(D, cb):
    """column blocks of the per-feature kernels' sweep: cb = 64, or 32 (k_feat_y_big, the long shapes of k_slam_y)"""
    return (D + cb - 1) // cb


def last_block_columns(D, cb):
    return D - cb * (blocks(D, cb) - 1)


def takes_gram_route(D, wide, compress_route=capi.COMPRESS_GRAM, fp32=0, prior_ok=True, entry="update"):
    """ovgpu_last_update_route == OVGPU_COMPRESS_GRAM: an update (mode B, not a compress entry) of a context on OVGPU_COMPRESS_GRAM whose prior
    block factors, at D <= 383; with "gram_wide" = 1 on a float64 context (gram_fp32 off) at D <= 511."""
    cap = WIDE_MAX_D if (wide >= 1 and not fp32) else NARROW_MAX_D
    return entry == "update" and compress_route != capi.COMPRESS_TSQR and prior_ok and D <= cap


def takes_wide_route(D, wide, **route):
    """... and "gram_wide_updates" counts it: the Gram route at 25 .. 32 tile columns"""
    return takes_gram_route(D, wide, **route) and D > NARROW_MAX_D


def expected_msckf_kernel(m_max, D, wide, shape=0, general=0, **route):
    """"last_feature_kernel" after an MSCKF update: track_shapes.expected_kernel's tile budgets on the Gram route (the fused kernels read the
    prior block's factor), 0 (the general kernel) off it."""
    return ts.expected_kernel(m_max, shape, bool(general)) if takes_gram_route(D, wide, **route) else 0


def expected_slam_kernel(reps, m_max, D, K, C, level, wide, general=0, **route):
    """"last_feature_kernel" after a SLAM update: the rule of "slam_fused" (slam_long_shapes.expected_kernel3) with the route's column bound
    taken from takes_gram_route: 4 / 5 (without / with a single-depth landmark observed) up to 62 observations, 6 / 7 up to 126 at level 3."""
    single = any(int(r) == SINGLE for r in reps)
    bound = s3.BOUND_LONG if level >= 3 else s3.BOUND
    ok = level >= 1 and not general and m_max <= bound and D >= 16 and K * C <= 8192 and takes_gram_route(D, wide, **route)
    if not ok or (single and level < 2):
        return 0
    return (6 if m_max > s3.BOUND else 4) + (1 if single else 0)


def route_terms(options, gram_route=True, entry="update"):
    return dict(compress_route=options.get("compress_route", capi.COMPRESS_GRAM), fp32=options.get("gram_fp32", 0), prior_ok=gram_route, entry=entry)


# --------------------------------------------------------------------------- (a), (c), (d), (f): MSCKF batches
@dataclass
class MCase(ts.Case):
    rejected: int | None = None   # the feature the gate must reject
    lengths: tuple | None = None  # the track lengths the case is built with
    gram_route: bool = True       # False: the prior block does not factor (the Householder repeat)
    entry: str = "update"

    def kernel_at(self, wide):
        return expected_msckf_kernel(self.longest_track, self.D, wide, self.options.get("feature_kernel_shape", 0), self.options.get("no_fast_feature_kernel", 0),
                                     **route_terms(self.options, self.gram_route, self.entry))

    def gram_at(self, wide):
        return takes_gram_route(self.D, wide, **route_terms(self.options, self.gram_route, self.entry))

    def wide_at(self, wide):
        return takes_wide_route(self.D, wide, **route_terms(self.options, self.gram_route, self.entry))


# D = 6 C + 14 K: both sides of every edge an MSCKF state reaches (383 is odd: 382 stands on the narrow side)
MSCKF_STATES = {
    382: dict(C=59, K=2),   # 24 tile columns: the narrow route's last even count
    384: dict(C=57, K=3),   # 25: the switch's first column count, the fourth window's first tile; six full blocks of 64
    386: dict(C=62, K=1),   # the seventh block of 64, two columns of it
    398: dict(C=64, K=1),   # 25 tile columns, the last even count
    400: dict(C=62, K=2),   # 26
    416: dict(C=67, K=1),   # 27
    448: dict(C=70, K=2),   # seven full blocks of 64
    450: dict(C=68, K=3),   # the eighth block
    480: dict(C=73, K=3),   # 31 tile columns, 15 full blocks of 32
    482: dict(C=78, K=1),   # the sixteenth block of 32
    496: dict(C=78, K=2),   # 32 tile columns: the fourth window full
    498: dict(C=76, K=3),
    510: dict(C=78, K=3),   # the last even count
}
MIX_LENGTHS = (40, 33, 25, 17, 16, 9, 8, 5, 3, 2, 1, 0)  # twelve tracks: every tile-row count up to five, a 1-observation and an empty one
MIX_OUTLIER = 3                                           # the 17-observation track
# seeds: chosen on the CPU (tests/test_gram_wide_shapes_cpu.py holds every case to it) so that the oracle uses a feature, rejects the planted
# outlier and nothing else, and leaves no statistic within parity_util.GATE_MARGIN of its threshold.  The default of a group serves all but two.
SEEDS = {"b-399": 700, "b-448": 700}


def msckf_seed(D):
    return SEEDS.get(f"a-{D}", 400 + D)


def msckf_batch(D, seed):
    p = ts.with_lengths(ts._window(MSCKF_STATES[D], len(MIX_LENGTHS), seed), list(MIX_LENGTHS))
    return ts.make_outlier(p, MIX_OUTLIER, 15.0, seed)


# (c) the kernels by track length on four cameras (extrinsics estimated, intrinsics not): D = 6 C + 24
KERNEL_STATES = {384: dict(C=60, K=4, pose=1, intr=0), 510: dict(C=81, K=4, pose=1, intr=0)}
KERNEL_TRACKS = {62: 1, 63: 2, 126: 2, 127: 3}  # longest track -> kernel: <4, 9, 2>, <8, 17, 1> at both ends, k_feat_y_big


def kernel_batch(D, m_long, seed):
    """track_shapes.mixed_batch on the state of D columns: one track of m_long observations, nine short ones (the 32-observation one a gross
    outlier), a 1-observation track and an empty one"""
    p = ts.with_lengths(ts._window(KERNEL_STATES[D], 12, seed), [m_long] + ts.MIXED_SHORT)
    return ts.make_outlier(p, 9, 15.0, seed)


SMALL_LENGTHS = (40, 33, 25, 17, 16, 9, 8, 5)


def small_batch(seed):
    """208 columns (30 clones, stereo): the middle link of the context-hygiene chain — 14 tile columns, the unprojected stack"""
    p = ts.with_lengths(ts._window(ts.SMALL, len(SMALL_LENGTHS), seed), list(SMALL_LENGTHS))
    return ts.make_outlier(p, MIX_OUTLIER, 15.0, seed)


def _msckf_cases():
    out = []
    for D, st in MSCKF_STATES.items():
        out.append(MCase(f"a-{D}", "a", functools.partial(msckf_batch, D, msckf_seed(D)), st, m_max=40, rejected=MIX_OUTLIER, lengths=MIX_LENGTHS))
    for D, st in KERNEL_STATES.items():
        for m in KERNEL_TRACKS:
            out.append(MCase(f"c-{D}-{m}", "c", functools.partial(kernel_batch, D, m, SEEDS.get(f"c-{D}-{m}", 500 + m)), st, m_max=m, rejected=9,
                             lengths=tuple([m] + ts.MIXED_SHORT)))
        out.append(MCase(f"c-{D}-general", "c", functools.partial(kernel_batch, D, 62, SEEDS.get(f"c-{D}-62", 500 + 62)), st, options=dict(no_fast_feature_kernel=1),
                         m_max=62, rejected=9, lengths=tuple([62] + ts.MIXED_SHORT)))
    # (d) what must not move: the switch-off context's bits
    b400 = functools.partial(msckf_batch, 400, msckf_seed(400))
    out.append(MCase("d-tsqr-400", "d", b400, MSCKF_STATES[400], options=dict(compress_route=capi.COMPRESS_TSQR), m_max=40, rejected=MIX_OUTLIER))
    out.append(MCase("d-fp32-400", "d", b400, MSCKF_STATES[400], options=dict(gram_fp32=1), m_max=40, rejected=MIX_OUTLIER))
    out.append(MCase("d-compress-384", "d", functools.partial(msckf_batch, 384, msckf_seed(384)), MSCKF_STATES[384], m_max=40, rejected=MIX_OUTLIER,
                     entry="compress"))
    # ... and what falls back or steps aside at 400 columns
    out.append(MCase("d-semi-definite-400", "d", lambda: ss.semi_definite(b400()), MSCKF_STATES[400], m_max=40, rejected=MIX_OUTLIER, gram_route=False))
    out.append(MCase("d-stepwise-400", "d", b400, MSCKF_STATES[400], options=dict(no_single_launch_cholesky=1), m_max=40, rejected=MIX_OUTLIER))
    # (f) the middle link of the hygiene chain
    out.append(MCase("f-208", "f", functools.partial(small_batch, 600), ts.SMALL, m_max=40, rejected=MIX_OUTLIER, lengths=SMALL_LENGTHS))
    return out


MSCKF_CASES = _msckf_cases()
MSCKF_BY_ID = {c.id: c for c in MSCKF_CASES}
assert len(MSCKF_BY_ID) == len(MSCKF_CASES)
HYGIENE_CHAIN = ("a-510", "f-208", "a-448")

msckf_oracle_run = ts.oracle_run


# --------------------------------------------------------------------------- (b), (d), (e): SLAM batches over all columns
@dataclass
class SCase(s3.Case):
    level: int = 0               # "slam_fused" of the case's switch-on and switch-off contexts alike

    def kernel_wide(self, wide):
        p = self.prob
        return expected_slam_kernel(self.reps_observed, self.longest_track, self.columns, p.K, p.C, self.level, wide, self.options.get("no_fast_feature_kernel", 0),
                                    **route_terms(self.options, self.gram_route, self.entry))

    def gram_at(self, wide):
        return takes_gram_route(self.columns, wide, **route_terms(self.options, self.gram_route, self.entry))

    def wide_at(self, wide):
        return takes_wide_route(self.columns, wide, **route_terms(self.options, self.gram_route, self.entry))


# D = 6 C + 28 (stereo, extrinsics and intrinsics) + 3 a + b: a 3-dof landmarks of the five representations in turn, b single-depth ones
SLAM_STATES = {
    384: dict(C=56, a=6, b=2),    # 25 tile columns; six full blocks of 64, twelve of 32
    385: dict(C=56, a=6, b=3),    # a seventh block of 64 and a thirteenth of 32 of ONE column
    399: dict(C=58, a=7, b=2),    # the 25th tile column full
    400: dict(C=58, a=7, b=3),    # the 26th holds the residual column alone
    401: dict(C=58, a=8, b=1),
    447: dict(C=66, a=7, b=2),    # 28 tile columns full
    448: dict(C=66, a=7, b=3),    # seven full blocks of 64
    449: dict(C=66, a=8, b=1),    # an eighth block of 64 and a fifteenth of 32 of one column
    495: dict(C=74, a=7, b=2),    # 31 tile columns full
    496: dict(C=74, a=7, b=3),    # the 32nd: the fourth window full
    497: dict(C=74, a=8, b=1),
    510: dict(C=76, a=8, b=2),
    511: dict(C=76, a=8, b=3),    # the bound: the eighth block of 64 holds 63 columns, the sixteenth of 32 holds 31
}
SLAM_SEED = 31
SLAM_OUTLIER = 2                  # a 3-dof landmark's track
FUSED_D = {385: 63, 449: 100, 511: 126}  # the column counts that also run fused, and the long track each gets (63 .. 126 observations)


def slam_reps(D):
    st = SLAM_STATES[D]
    reps = (ss.REPS5 * 3)[:st["a"]]
    for i in range(st["b"]):  # the single-depth landmarks spread through the list: positions 1, 4, 7
        reps.insert(min(1 + 3 * i, len(reps)), SINGLE)
    return reps


def slam_batch(D, seed, m_long=None, singles=True):
    """every landmark of the state observed once, tracks of at most 40 observations (widest baseline), one a gross outlier; m_long: the first
    track (a 3-dof landmark's) is exactly that long instead; singles = False: the batch leaves the single-depth landmarks' tracks out — they stay
    resident with their columns"""
    reps = slam_reps(D)
    p = ss.slam(len(reps), reps, seed, C=SLAM_STATES[D]["C"], K=2)
    lens = [min(int(m), 40) for m in np.diff(p.meas_offsets)]
    if m_long is not None:
        lens[0] = m_long
    p = ts.with_lengths(p, lens, patterns=("stride",))
    p = ts.make_outlier(p, SLAM_OUTLIER, 15.0, seed)
    if not singles:
        p = ss.reordered(p, [f for f, r in enumerate(reps) if r != SINGLE])
    return p


def _slam_cases():
    out = []
    for D in SLAM_STATES:
        seed = SEEDS.get(f"b-{D}", SLAM_SEED + D)
        out.append(SCase(f"b-{D}", "b", functools.partial(slam_batch, D, seed), D=D, outliers=True, rejected=SLAM_OUTLIER))
    for D, m in FUSED_D.items():
        seed = SEEDS.get(f"b-{D}", SLAM_SEED + D)
        out.append(SCase(f"b-{D}-fused-single", "bf", functools.partial(slam_batch, D, seed), D=D, outliers=True, rejected=SLAM_OUTLIER, level=3))
        out.append(SCase(f"b-{D}-fused-3dof", "bf", functools.partial(slam_batch, D, seed, None, False), D=D, outliers=True, rejected=SLAM_OUTLIER - 1, level=3))
        out.append(SCase(f"b-{D}-long-single", "bf", functools.partial(slam_batch, D, seed, m), D=D, m_max=m, outliers=True, rejected=SLAM_OUTLIER, level=3))
        out.append(SCase(f"b-{D}-long-3dof", "bf", functools.partial(slam_batch, D, seed, m, False), D=D, m_max=m, outliers=True, rejected=SLAM_OUTLIER - 1, level=3))
    # (d) 383 columns with the switch on (slam_shapes' state: 60 clones, one camera, three landmarks), mode A at 384, a state of 512 columns
    out.append(SCase("d-383", "d", functools.partial(ss.column_batch, 383, 21), D=383))
    out.append(SCase("d-compress-384", "d", functools.partial(slam_batch, 384, SEEDS.get("b-384", SLAM_SEED + 384)), D=384, entry="compress", outliers=True,
                     rejected=SLAM_OUTLIER))
    return out


SLAM_CASES = _slam_cases()
SLAM_BY_ID = {c.id: c for c in SLAM_CASES}
assert len(SLAM_BY_ID) == len(SLAM_CASES)

slam_oracle_run = ss.oracle_run


def over_the_bound():
    """512 columns: 76 clones, stereo, nine 3-dof landmarks and one single-depth one — one column more than any call carries"""
    reps = (ss.REPS5 * 2)[:9] + [SINGLE]
    p = ss.slam(len(reps), reps, SLAM_SEED, C=76, K=2)
    return ts.with_lengths(p, [min(int(m), 12) for m in np.diff(p.meas_offsets)], patterns=("stride",))


# --------------------------------------------------------------------------- (e) chunks
CHUNK_STATE = dict(C=64, K=2)           # 412 columns without a landmark
CHUNK_REPS = [ss.REPS5[0], SINGLE, ss.REPS5[2], ss.REPS5[4], ss.REPS5[1], ss.REPS5[3], SINGLE, ss.REPS5[0], ss.REPS5[2], ss.REPS5[4], ss.REPS5[3], ss.REPS5[1]]
CHUNK_FIRST = [0, 4, 8, 12]             # a chunk's landmarks alone get columns: 412 + 10, + 10, + 12
CHUNK_SEED = 41


def chunk_problem():
    """twelve landmarks (ten 3-dof, two single-depth: 444 columns in all) over 64 clones, tracks of at most 40 observations"""
    p = ss.slam(len(CHUNK_REPS), CHUNK_REPS, SEEDS.get("e", CHUNK_SEED), **CHUNK_STATE)
    return ts.with_lengths(p, [min(int(m), 40) for m in np.diff(p.meas_offsets)], patterns=("stride",))


def chunk_columns():
    dof = np.where(np.asarray(CHUNK_REPS) == SINGLE, 1, 3)
    base = ts.n_columns(CHUNK_STATE["C"], CHUNK_STATE["K"])
    return base + int(dof.sum()), [base + int(dof[a:b].sum()) for a, b in zip(CHUNK_FIRST[:-1], CHUNK_FIRST[1:])]
