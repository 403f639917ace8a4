"""Batches of MIXED track lengths for ovgpu_debug_option "feat_classes" (tests/test_class_shapes_cpu.py checks every one on the oracle alone,
tests/test_gpu_feat_classes.py runs it on the device, tests/test_feat_classes_host.py holds the library's partition header to the rule below).

At level 1 an MSCKF batch laid out for the fast path is served by a per-feature kernel PER LENGTH CLASS: the class of a track is the kernel a batch
whose longest track is that track would get (track_shapes.expected_kernel, restated there from the tile budgets), tracks of 0 or 1 observations
go with the shortest class present, and since the slots are sorted by descending length a class is a contiguous slot range.  expected_partition()
below restates that FROM THE RULE; nothing here is read back from the library.  No class is merged into a neighbour for being small.

A helper module, not a conftest: nothing here is collected.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import track_shapes as ts
from open_vins_amd import capi, synth


def slot_order(lengths):
    """Feature indices by descending track length, equal lengths in batch order (the library's track order, a stable sort)."""
    return np.argsort(-np.asarray(lengths, dtype=np.int64), kind="stable")


def expected_partition(lengths):
    """[(kernel code, first slot, one past the last slot, longest track of the range)], longest class first, from expected_kernel per track.  A batch
    without a track of two observations is one class of the general kernel; an empty batch has no class."""
    lengths = np.asarray(lengths, dtype=np.int64)
    out = []
    for slot, f in enumerate(slot_order(lengths)):
        m = int(lengths[f])
        k = ts.expected_kernel(m) if m >= 2 else (out[-1][0] if out else 0)
        if not out or out[-1][0] != k:
            out.append([k, slot, slot, m])
        out[-1][2] = slot + 1
    return [tuple(r) for r in out]


def class_of_feature(lengths):
    """The kernel code of every feature's class, in batch order."""
    cls = np.zeros(len(lengths), dtype=np.int64)
    order = slot_order(lengths)
    for k, a, b, _ in expected_partition(lengths):
        cls[order[a:b]] = k
    return cls


@dataclass
class Case:
    id: str
    build: object                      # () -> (Problem, planted outliers: feature indices)
    state: dict
    classes: tuple                     # kernel codes, longest class first: what the table in the issue names
    options: dict = field(default_factory=dict)

    @property
    def D(self):
        s = self.state
        return ts.n_columns(s["C"], s["K"], s.get("pose", 1), s.get("intr", 1))

    @functools.cached_property
    def built(self):
        return self.build()

    @property
    def prob(self):
        return self.built[0]

    @property
    def planted(self):
        return self.built[1]

    @property
    def lengths(self):
        return np.diff(self.prob.meas_offsets)

    @property
    def partition(self):
        return expected_partition(self.lengths)

    @property
    def mask(self):
        return sum(1 << k for k, _, _, _ in self.partition)

    @property
    def counts(self):
        n = [0, 0, 0, 0]
        for k, a, b, _ in self.partition:
            n[k] = b - a
        return n

    @property
    def raw(self):
        """ "last_stack_raw" at level 1: the unprojected stack needs one-pass float64 kernels in EVERY class (a block-row or a general class puts the
        whole batch on the projected stack), and a state the regions hold (track_shapes.expected_raw)."""
        ks = [k for k, _, _, _ in self.partition]
        return int(all(k in (1, 2) for k in ks) and ts.expected_raw(self.D, ks[0], 0, self.options.get("gram_fp32", 0)))

    def opts(self, **more):
        s = self.state
        kw = dict(chi2_multipler=1.0, gate_always_factor=1, do_calib_camera_pose=s.get("pose", 1), do_calib_camera_intrinsics=s.get("intr", 1))
        kw.update(self.options)
        kw.update(more)
        return capi.default_options(**kw)


def _lengths_batch(state, lengths, seed, outlier=None, order=None):
    p = ts.with_lengths(ts._window(state, len(lengths), seed), lengths)
    planted = []
    if outlier is not None:
        p = ts.make_outlier(p, outlier, 15.0, seed)
        planted = [outlier]
    if order is not None:
        p = ts.reorder(p, order)
        planted = [order.index(f) for f in planted]
    return p, planted


TWO = [63, 62, 32, 9, 2, 1, 0]
# (seeds: the first of 400, 401, .. at which the oracle alone meets tests/test_class_shapes_cpu.py — an accepted feature in every class, the planted
#  outlier rejected, no statistic within 1e-6 of its threshold)
SEED = {"two": 400, "three": 400, "four": 400, "gap": 400, "singletons": 400, "one-class": 400}


def _ragged_600():
    """synth's ragged tracks (a contiguous sub-window of 5 .. 30 clones per feature, four cameras), one gross outlier planted in each class: the
    longest track of the batch and the longest of the short class.  273 | 327 tracks: on 256 compute units the <8, 17, 1> class has more slots than
    workgroups (256), the <4, 9, 2> class fewer than its 512 — 600 tracks cannot exceed both: `many-short` below does for the short class."""
    p = synth.make_problem(5, C=30, K=4, F=600, track="ragged")
    m = np.diff(p.meas_offsets)
    cls = class_of_feature(m)
    planted = [int(np.flatnonzero(cls == k)[np.argmax(m[cls == k])]) for k in (2, 1)]
    for f in planted:
        p = ts.make_outlier(p, f, 15.0, 0)
    return p, planted


def _many_short():
    """700 ragged tracks of which all but the four longest are cut to 40 .. 62 observations: 696 slots of the <4, 9, 2> class on its 512
    workgroups (two per compute unit of 256), so that workgroups take a SECOND trip of the slot loop from a record pointer that starts at the
    class's first slot — the next-record request of the chains form included — next to a class of four.  An outlier in each class."""
    p = synth.make_problem(5, C=30, K=4, F=700, track="ragged", seed=77)
    m = np.diff(p.meas_offsets)
    keep = set(np.argsort(-m, kind="stable")[:4].tolist())
    assert min(m[f] for f in keep) >= 63
    p = ts.with_lengths(p, [None if (f in keep or m[f] <= 62) else 40 + f % 23 for f in range(p.F)])
    m = np.diff(p.meas_offsets)
    cls = class_of_feature(m)
    planted = [int(np.flatnonzero(cls == k)[np.argmax(m[cls == k])]) for k in (2, 1)]
    for f in planted:
        p = ts.make_outlier(p, f, 15.0, 0)
    return p, planted


def _cases():
    M, L = ts.MID, ts.LARGE
    return [
        Case("two", functools.partial(_lengths_batch, M, TWO, SEED["two"], 2), M, (2, 1)),                       # the 32-observation track is the outlier
        Case("two-rev", functools.partial(_lengths_batch, M, TWO, SEED["two"], 2, [1, 2, 3, 4, 5, 6, 0]), M, (2, 1)),
        Case("three", functools.partial(_lengths_batch, L, [127, 126, 63, 62, 16, 2], SEED["three"], 4), L, (3, 2, 1)),  # class 1 holds three gated tracks: the 16
        Case("four", functools.partial(_lengths_batch, L, [233, 232, 127, 126, 63, 62, 8], SEED["four"]), L, (0, 3, 2, 1)),
        Case("gap", functools.partial(_lengths_batch, L, [127, 62, 9], SEED["gap"]), L, (3, 1)),
        Case("singletons", functools.partial(_lengths_batch, M, [120, 8], SEED["singletons"]), M, (2, 1)),
        Case("one-class", functools.partial(_lengths_batch, M, [60, 40, 9, 2], SEED["one-class"], 1), M, (1,)),  # four gated tracks: the 40
        Case("ragged-600", _ragged_600, M, (2, 1)),
        Case("many-short", _many_short, M, (2, 1)),
    ]


CASES = _cases()
BY_ID = {c.id: c for c in CASES}


def two_without_long():
    """`two` without its 63-observation track, on the same state: the per-feature independence leg."""
    c = BY_ID["two"]
    return ts.reorder(c.prob, list(range(1, c.prob.F)))


def oracle_run(oracle, case, prob=None, **more):
    """(triangulation, update) of the oracle: the reference every leg is held to.  The case's own batch and options are cached on the case."""
    if prob is None and not more:
        if not hasattr(case, "_ref"):
            case._ref = oracle_run(oracle, case, case.prob)
        return case._ref
    v = capi.Views(case.prob if prob is None else prob)
    opts = case.opts(**more)
    tri = oracle.triangulate(opts, v)
    return tri, oracle.msckf_update(opts, v, want_compressed=False, given=tri)
