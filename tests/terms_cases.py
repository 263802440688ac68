"""The contract of cc_index_rank_terms / cc_index_timeline_terms as a numpy model, and the seeded cases both new test files use
(tests/test_index_terms_host.py, where the model is held to a brute-force loop, and tests/test_gpu_index_terms.py, where the device is
held to the model).

A compound question is a single query whose score vector is a fold of the score matrix of its terms, and a dead row is a row in a
forbidden group: `fold_terms` does the first in float32 arithmetic in the stated order, `where_cases.disguise` the second (as
like_cases.like_model does it), and `rank_cases.rank_model`, unchanged, the rest - on the device's own score matrix
`ix.scores(np.vstack([q, ix.fetch(rows)]))`, so every comparison is exact."""
import numpy as np

from like_cases import N_EVEN, N_ODD, World, dead_rows, ordered  # noqa: F401  (the worlds are like_cases': 8229 and 8224 rows of 256)
from rank_cases import full_order, rank_model
from where_cases import DIM, GROUPS, NO_TS, disguise, passing  # noqa: F401

TERMS_MAX = 64                                                   # CC_TERMS_MAX
ROLES = {"rank": 0, "require": 1, "reject": 2}                   # CC_TERM_RANK / CC_TERM_REQUIRE / CC_TERM_REJECT
COMBINES = {"max": 0, "min": 1, "sum": 2}                        # CC_COMBINE_MAX / CC_COMBINE_MIN / CC_COMBINE_SUM
TERM_COUNTS = (1, 2, 9, 17, 18, 64)                              # both sides of the f32 / bf16 GEMM threshold (17) and of the int8 MFMA one (18)
PATTERNS = ("rank", "require", "reject", "both")                 # RANK terms only, plus one REQUIRE, plus one REJECT, plus one of each


def fold_terms(S, roles, weights, cuts, combine):
    """(T, n) float32 scores -> (v (n,) float32, dead (n,) bool, which (n,) int): the ranking value from the "rank" terms in
    ascending term order, the rows a "require" / "reject" term kills, and the rank term that made v.
    max / min: in the total order of the ranking keys (+0 above -0), which = the lowest-numbered term attaining it.
    sum: v = +0; v = v + w_t * S[t], product and sum each rounded to float32; which = the term with the largest product in key order,
    the lowest-numbered on ties."""
    S = np.atleast_2d(np.ascontiguousarray(S, dtype=np.float32))
    T, n = S.shape
    assert len(roles) == T and combine in COMBINES
    rank = np.array([t for t in range(T) if roles[t] == "rank"], np.int64)
    assert len(rank) >= 1
    dead = np.zeros(n, bool)
    for t in range(T):
        if roles[t] == "require":
            dead |= ~(S[t] >= np.float32(cuts[t]))
        elif roles[t] == "reject":
            dead |= S[t] >= np.float32(cuts[t])
        else:
            assert roles[t] == "rank"
    cols = np.arange(n)
    if combine == "sum":
        v = np.zeros(n, np.float32)
        P = np.empty((len(rank), n), np.float32)
        for i, t in enumerate(rank):
            P[i] = np.float32(weights[t]) * S[t]                 # one rounding
            v = v + P[i]                                         # another one
        assert v.dtype == np.float32
        which = rank[ordered(P).argmax(axis=0)]                  # argmax: the first of equal keys
    else:
        K = ordered(S[rank])
        which = rank[K.argmax(axis=0) if combine == "max" else K.argmin(axis=0)]
        v = S[which, cols]
    return v, dead, which


def excluded(n, rows, roles, n_vec, group, slot, exclude):
    """Bool per row: dead by an exclude mode, which acts on the stored rows that are rank terms (like_cases.dead_rows on those)"""
    if exclude is None:
        return np.zeros(n, bool)
    mine = [int(r) for i, r in enumerate(rows) if roles[n_vec + i] == "rank"]
    assert mine
    return dead_rows(n, mine, group, slot, exclude)


def terms_fold(S, roles, weights, cuts, combine, rows, n_vec, group, slot, exclude):
    """fold_terms plus the exclude mode -> (v, dead, which)"""
    v, dead, which = fold_terms(S, roles, weights, cuts, combine)
    return v, dead | excluded(S.shape[1], rows, roles, n_vec, group, slot, exclude), which


def terms_order(v, dead, slot, group, n_groups, ts, cls, allowed=None, tracks=True, cut=None, ts_range=None, classes=None):
    """-> (rows, scores) of every answer: the dead rows and those the row filter rejects sit in a forbidden group"""
    g, al = disguise(group, n_groups, passing(ts, cls, ts_range, classes) & ~dead, allowed)
    return full_order(v, slot, g, al, tracks, cut)


def terms_model(v, dead, which, slot, group, n_groups, ts, cls, start, count, allowed=None, cut=None, tracks=True, ts_range=None, classes=None):
    """-> what EmbeddingIndex.rank_terms(..., which=True) returns: (idx (1, count), score (1, count), total (1,), which (1, count))"""
    g, al = disguise(group, n_groups, passing(ts, cls, ts_range, classes) & ~dead, allowed)
    idx, sc, total = rank_model(v[None, :], slot, g, start, count, al, cut, tracks)
    wh = np.where(idx >= 0, np.asarray(which)[np.maximum(idx, 0)], -1).astype(np.int32)
    return idx, sc, total, wh


def terms_timeline_model(v, dead, slot, group, n_groups, ts, cls, t0, bin_seconds, n_bins, allowed=None, cut=None, tracks=True, ts_range=None, classes=None):
    """-> what EmbeddingIndex.timeline_terms returns: (counts (1, n_bins) int64, total (1,) int64), from the full order as
    where_cases.timeline_model takes it"""
    rows, _ = terms_order(v, dead, slot, group, n_groups, ts, cls, allowed, tracks, cut, ts_range, classes)
    t = np.asarray(ts, np.int64)[rows]
    b = (t - int(t0)) // int(bin_seconds)
    b = b[(t != NO_TS) & (b >= 0) & (b < n_bins)]
    return np.bincount(b, minlength=n_bins)[None, :].astype(np.int64), np.array([len(rows)], np.int64)


def feasible(T, pattern):
    """A pattern needs its killing terms and at least one rank term"""
    return T >= {"rank": 1, "require": 2, "reject": 2, "both": 3}[pattern]


def plan(world, T, pattern, combine, seed):
    """The terms of one case, without their cuts -> (q (n_vec, DIM) or None, rows int64, roles, weights).  Vectors (the world's
    queries, and crops of the query track with noise) and stored rows (spread over the query track, so that exclude="track" is
    legal) are mixed; for T >= 2 there is at least one of each (T == 1: a vector for an even seed, a stored row for an odd one).
    The REQUIRE term is term 0, a vector, the REJECT term is term T - 1, a stored row; everything else ranks.  Weights (sum): in
    +-[0.2, 1.5], the second rank term's negative."""
    rng = np.random.default_rng(1000 * T + seed)
    n_kill = {"rank": 0, "require": 1, "reject": 1, "both": 2}[pattern]
    assert feasible(T, pattern), "no room for a rank term"
    n_vec = max(T // 3, 1) if T > 1 else 1 - seed % 2
    n_rows = T - n_vec
    q = None
    if n_vec:
        q = world.q[rng.integers(0, len(world.q), n_vec)].copy()
        noisy = world.E[world.track[rng.integers(0, len(world.track), n_vec)]] + 0.7 * rng.standard_normal((n_vec, DIM)).astype(np.float32)
        half = rng.random(n_vec) < 0.5
        q[half] = (noisy / np.linalg.norm(noisy, axis=1, keepdims=True)).astype(np.float32)[half]
    rows = world.query_rows(n_rows).astype(np.int64) if n_rows else np.zeros(0, np.int64)
    roles = ["rank"] * T
    if pattern in ("require", "both"):
        roles[0] = "require"                                     # a vector
    if pattern in ("reject", "both"):
        roles[T - 1] = "reject"                                  # a stored row
    assert roles.count("rank") == T - n_kill
    weights = rng.uniform(0.2, 1.5, T).astype(np.float32)
    ranked = [t for t in range(T) if roles[t] == "rank"]
    if len(ranked) >= 2:
        weights[ranked[1]] = -weights[ranked[1]]
    if combine != "sum":
        weights[:] = 1.0
    return q, rows, roles, [float(x) for x in weights]


def median_cuts(S, roles, competing):
    """One cut per term: for a require / reject term the median of its own scores over the competing rows, so that it kills some of
    them and spares some by construction; None for a rank term"""
    return [None if r == "rank" else float(np.float32(np.median(S[t][competing]))) for t, r in enumerate(roles)]
