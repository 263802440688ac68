"""The contract of cc_index_rank_where / cc_index_timeline as a numpy model, and the seeded world both new test files use
(tests/test_index_where_host.py, where the model is held to a brute-force loop, and tests/test_gpu_index_where.py, where the
device is held to the model).

A row filter is a group filter in disguise: every row that does not pass moves to a fresh group G = n_groups that `allowed`
forbids, and `rank_model` / `full_order` of tests/rank_cases.py, unchanged, do the rest on the device's own score matrix.  The
timeline is np.bincount over the ts of `full_order`'s rows."""
import numpy as np

from rank_cases import full_order, rank_model

NO_TS = -(1 << 31)                      # CC_ROW_NO_TS
CLASSES = (0, 2, 7, 63, 64, 255, -1)    # both sides of every 64-bit word of the mask, and "none"
DIM, N, GROUPS, SLOTS = 256, 2 * 4096 + 37, 5, 40


def passing(ts, cls, ts_range=None, classes=None):
    """Bool per row: the row passes the row filter (a row without the attribute never passes a filter on it)."""
    ts, cls = np.asarray(ts, np.int64), np.asarray(cls, np.int64)
    ok = np.ones(len(ts), bool)
    if ts_range is not None:
        lo, hi = ts_range
        ok &= ts != NO_TS
        if lo is not None:
            ok &= ts >= lo
        if hi is not None:
            ok &= ts <= hi
    if classes is not None:
        ok &= (cls >= 0) & np.isin(cls, np.asarray(list(classes), np.int64))
    return ok


def disguise(group, n_groups, ok, allowed=None):
    """-> (group, allowed) in which the rows outside `ok` sit in a group of their own that is not allowed"""
    g = np.where(ok, np.asarray(group), n_groups).astype(np.int64)
    al = np.ones(n_groups, np.uint8) if allowed is None else np.asarray(allowed, np.uint8)[:n_groups]
    al = np.concatenate([al, np.zeros(n_groups + 1 - len(al), np.uint8)])
    return g, al


def where_order(sc, slot, group, n_groups, ts, cls, allowed=None, tracks=True, cut=None, ts_range=None, classes=None):
    """One score vector -> (rows, scores) of every answer of the filtered ranking"""
    g, al = disguise(group, n_groups, passing(ts, cls, ts_range, classes), allowed)
    return full_order(sc, slot, g, al, tracks, cut)


def rank_where_model(sc, slot, group, n_groups, ts, cls, start, count, allowed=None, cut=None, tracks=True, ts_range=None, classes=None):
    """(Q, N) scores -> what EmbeddingIndex.rank(..., ts_range=, classes=) returns"""
    g, al = disguise(group, n_groups, passing(ts, cls, ts_range, classes), allowed)
    return rank_model(sc, slot, g, start, count, al, cut, tracks)


def timeline_model(sc, slot, group, n_groups, ts, cls, t0, bin_seconds, n_bins, allowed=None, cut=None, tracks=True, ts_range=None, classes=None):
    """(Q, N) scores -> what EmbeddingIndex.timeline returns: (counts (Q, n_bins) int64, total (Q,) int64)"""
    sc = np.atleast_2d(np.asarray(sc, np.float32))
    ts = np.asarray(ts, np.int64)
    counts, total = np.zeros((len(sc), n_bins), np.int64), np.zeros(len(sc), np.int64)
    for i, v in enumerate(sc):
        rows, _ = where_order(v, slot, group, n_groups, ts, cls, allowed, tracks, cut, ts_range, classes)
        total[i] = len(rows)
        t = ts[rows]
        b = (t - int(t0)) // int(bin_seconds)                      # int64 floor division
        b = b[(t != NO_TS) & (b >= 0) & (b < n_bins)]
        counts[i] = np.bincount(b, minlength=n_bins)
    return counts, total


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


class Rows:
    """The seeded data: N = 2 * 4096 + 37 rows of 256 (the smallest width the bf16 and i8 storages take), so blocks of 4096 and
    2048 rows and granules of 64 all end in a ragged tail; 5 groups; 40 track slots of which slot 0 owns about 10 % of the rows,
    about 15 % of the rows slot-less; a fifth of the rows copy an earlier embedding (scores tie exactly, across tracks and across
    the edges of a time window, since the copy draws its own slot, ts and class); ts from [-50, 400) with many repeats and about
    5 % "none"; classes from CLASSES."""

    def __init__(self, n=N, seed=7, queries=18):
        rng = np.random.default_rng(seed)
        self.n = n
        E = unit(rng.standard_normal((n, DIM)))
        for i in np.flatnonzero(rng.random(n) < 0.2):
            if i:
                E[i] = E[rng.integers(0, i)]
        self.E = E
        self.q = unit(rng.standard_normal((queries, DIM)))
        self.group = rng.integers(0, GROUPS, n).astype(np.int32)
        u = rng.random(n)
        slot = rng.integers(1, SLOTS, n)
        slot[u < 0.10] = 0
        slot[u > 0.85] = -1
        self.slot = slot.astype(np.int32)
        ts = rng.integers(-50, 400, n)
        ts[rng.random(n) < 0.05] = NO_TS
        self.ts = ts.astype(np.int32)
        self.cls = rng.choice(np.array(CLASSES), n).astype(np.int32)
        if n >= 4096:
            # eight triples of equal, slot-less rows that pass every filter of FILTERS (ts on the edges of the narrow window): even
            # the narrowest ranking, with or without tracks, has runs of equal scores to put a cut and a window edge into
            tied = 11 + np.arange(24) * (n // 24)
            self.E[tied] = self.E[tied[::3]].repeat(3, axis=0)
            self.slot[tied] = -1
            self.group[tied] = np.tile(np.array([0, 2, 3], np.int32), 8)
            self.ts[tied] = np.tile(np.array([100, 250, 177], np.int32), 8)
            self.cls[tied] = np.tile(np.array([64, 255], np.int32), 12)


# the filters the GPU tests run: name -> (ts_range, classes, allowed).  "ts" keeps all but the rows at ts = -50 and those
# without ts, so that a track ranking still has more than 1024 answers; the others are narrow.
FILTERS = {
    "ts": ((-49, 399), None, None),
    "cls": (None, (0, 63, 64, 255), None),
    "both": ((100, 250), (2, 64, 255), None),
    "both+allowed": ((100, 250), (2, 64, 255), np.array([1, 0, 1, 1, 0], np.uint8)),
}
