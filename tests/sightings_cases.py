"""The contract of cc_index_sightings as a numpy model, for tests/test_index_sightings_host.py (where the model is held to a plain double
loop) and tests/test_gpu_index_sightings.py (where the device is held to the model).

Up to 1024 stored rows (the objects) meet every competing row; per object come back the number of pairs at or above `same_at`, the best
pair (largest value, equal values by the lower row) and the matching pairs per group.  The value of a pair is the float64 dot product of
the stored rows (like_cases.stored) rounded to float32, or - where the caller hands in G - the float the device's own cc_index_gram
computes, which makes every comparison of the GPU tests exact.  Against the float64 model the device agrees wherever no pair comes nearer
to a threshold than score_cases.order_free_bound (tests/test_index_sightings_host.py checks that for SAME_AT on distinct_cases.DupWorld),
and on distinct_cases.crafted_rows because every product and partial sum is exact."""
import numpy as np

from clearcam_amd import _lib
from digest_cases import competing                                                        # noqa: F401  (re-exported for the two test files)
from distinct_cases import DIMS, SAME_AT, crafted_rows, threshold_margins, world            # noqa: F401
from like_cases import stored                                                             # noqa: F401
from score_cases import order_free_bound                                                  # noqa: F401
from where_cases import FILTERS, GROUPS                                                   # noqa: F401

MAX_OBJECTS, MAX_GROUPS = _lib.SIGHT_MAX_OBJECTS, _lib.SIGHT_MAX_GROUPS
STORAGES = ("f32", "bf16", "i8")
SMALL_GROUP_COUNTS = 3                                           # fewer than the worlds' GROUPS = 5: matches in groups 3 and 4 are counted in `count` only


def ordered(x):
    """float32 -> uint32 whose order is the ranking keys' total order: -inf < ... < -0 < +0 < ... < +inf"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000)


def pair_values(D, rows, competing_rows):
    """(n, m) float32: the float64 dot products of the stored rows D[rows] with D[competing_rows], rounded once"""
    D = np.asarray(D, np.float64)
    return (D[np.asarray(rows, np.int64)] @ D[np.asarray(competing_rows, np.int64)].T).astype(np.float32)


def sightings_model(D, rows, competing_rows, same_at, skip_self, group, n_group_counts, G=None):
    """D (size, dim) float32: what the index holds, decoded -> what EmbeddingIndex.sightings returns: (count (n,) int32, best_row (n,)
    int32, best_score (n,) f32, group_counts (n, n_group_counts) uint32 or None, total).  G: (n, m) float32 pair values where the caller
    has them (`pair_values`, or the device's own Gram)."""
    rows, comp = np.asarray(rows, np.int64).reshape(-1), np.asarray(competing_rows, np.int64).reshape(-1)
    n, m = len(rows), len(comp)
    G = pair_values(D, rows, comp) if G is None else np.asarray(G, np.float32).reshape(n, m)
    exists = np.ones((n, m), bool) if not skip_self else rows[:, None] != comp[None, :]
    hit = exists & (G >= np.float32(same_at))
    count = hit.sum(axis=1).astype(np.int32)
    # the key of a pair: ordered(value) << 32 | ~row - its maximum is the largest value and, among equal values, the lowest row
    key = (ordered(G) << np.uint64(32)) | ((~comp.astype(np.uint64)) & np.uint64(0xffffffff))[None, :]
    key = np.where(exists, key, np.uint64(0))
    best_row, best_score = np.full(n, -1, np.int32), np.full(n, -np.inf, np.float32)
    if m:
        at = key.argmax(axis=1)
        has = key[np.arange(n), at] != 0
        best_row[has], best_score[has] = comp[at[has]], G[np.arange(n), at][has]
    gc = None
    if n_group_counts:
        g = np.asarray(group, np.int64)[comp]
        gc = np.zeros((n, n_group_counts), np.uint32)
        for k in range(n_group_counts):
            gc[:, k] = (hit & (g == k)[None, :]).sum(axis=1)
    return count, best_row, best_score, gc, m


def ordered_scalar(g):
    u = int(np.float32(g).view(np.uint32))
    return (~u) & 0xffffffff if u & 0x80000000 else u | 0x80000000


def double_loop(D, rows, competing_rows, same_ats, skip_self, group, n_group_counts, values=None):
    """The contract as it is written, pair by pair, for each threshold of `same_ats` -> one answer per threshold (a pair's value is
    computed once and compared with all of them; `values`: a dict that remembers it per (object row, competing row) between calls)"""
    values = {} if values is None else values
    D = np.asarray(D, np.float64)
    ts = [np.float32(t) for t in same_ats]
    n = len(rows)
    count = [np.zeros(n, np.int32) for _ in ts]
    gc = [np.zeros((n, n_group_counts), np.uint32) if n_group_counts else None for _ in ts]
    best_row, best_score = np.full(n, -1, np.int32), np.full(n, -np.inf, np.float32)
    for i, a in enumerate(rows):
        best = None
        for r in competing_rows:
            if skip_self and r == a:
                continue
            g = values.get((int(a), int(r)))
            if g is None:
                g = values[(int(a), int(r))] = np.float32(np.dot(D[a], D[r]))
            for k, t in enumerate(ts):
                if g >= t:
                    count[k][i] += 1
                    if gc[k] is not None and group[r] < n_group_counts:
                        gc[k][i, group[r]] += 1
            key = (ordered_scalar(g), -int(r))
            if best is None or key > best[0]:
                best = (key, r, g)
        if best is not None:
            best_row[i], best_score[i] = best[1], best[2]
    return [(count[k], best_row, best_score, gc[k], len(competing_rows)) for k in range(len(ts))]


def object_sets(w, n, seed=0):
    """The object lists the GPU tests use for a world: `n` row numbers with repeats (every fourth repeats the one before it), among them
    members of big clusters, byte-equal copies and their originals, and rows that the filters of where_cases.FILTERS keep out."""
    rng = np.random.default_rng(1000 * n + seed)
    rows = rng.choice(w.n, n, replace=False)
    _, first, inverse, cnt = np.unique(w.E.view(np.uint32), axis=0, return_index=True, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    copies = np.flatnonzero(first[inverse] != np.arange(w.n))
    if n >= 2:
        rows[0], rows[1] = copies[0], first[inverse[copies[0]]]                            # a copy and its original: the best of each other
    for i in range(3, n, 4):
        rows[i] = rows[i - 1]
    return rows.astype(np.int64)
