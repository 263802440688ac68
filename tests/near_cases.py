"""The contract of cc_index_rank_near / cc_index_timeline_near as a numpy model, and the seeded cases both new test files use
(tests/test_index_near_host.py, where the model is held to a plain double loop, and tests/test_gpu_index_near.py, where the device is
held to the model).

A together question is a single query whose score vector is A's (or the smaller of A's and the partner's B score), and a row without
a partner is a row in a forbidden group: `partner_list` is an ungrouped `rank_cases.full_order` of B among the rows that have a ts,
`near_fold` the join, `where_cases.disguise` the forbidden group (as like_cases.like_model does it), and `rank_cases.rank_model`,
unchanged, the rest - on the device's own score matrix `ix.scores(np.vstack([a, b]))`, so every comparison is exact."""
import numpy as np

from like_cases import N_EVEN, N_ODD, World, ordered  # noqa: F401  (the worlds are like_cases': 8229 and 8224 rows of 256)
from rank_cases import full_order, rank_model
from where_cases import DIM, GROUPS, NO_TS, disguise, passing  # noqa: F401

MAX_PARTNERS, DEFAULT_PARTNERS = 16384, 4096                     # CC_NEAR_MAX_PARTNERS / CC_NEAR_DEFAULT_PARTNERS
VALUES = {"a": 0, "min": 1}                                      # CC_NEAR_VALUE_A / CC_NEAR_VALUE_MIN
CHUNK = 1024                                                     # list entries near_fold_kernel stages into LDS at a time
WITHINS = (0, 1, 7, 500)                                         # the same second, the next one, a few, more than the worlds' whole span of ts
PARTNERS = (1, 5, 1024, 1025, 3000)                              # one entry, a few, one full chunk, one entry into the second chunk, three chunks
INT32_MAX, INT32_MIN = (1 << 31) - 1, -(1 << 31)


def partner_list(Sb, group, n_groups, ts, cls, partners, cut_b=None, allowed=None, b_ts_range=None, b_classes=None):
    """B's score vector -> (the list: rows in ranking order, at most `partners`; the number of rows it would hold without the cap).
    An ungrouped ranking (score descending, equal scores by ascending row) among the allowed rows that pass B's filter and have a ts."""
    ts = np.asarray(ts, np.int64)
    ok = passing(ts, cls, b_ts_range, b_classes) & (ts != NO_TS)
    g, al = disguise(group, n_groups, ok, allowed)
    rows, _ = full_order(Sb, np.full(len(ts), -1, np.int32), g, al, False, cut_b)
    return rows[:int(partners)].astype(np.int64), len(rows)


def near_fold(Sa, Sb, plist, group, slot, ts, within, value="min"):
    """-> (v (n,) float32, dead (n,) bool, partner (n,) int64: the row of each row's partner, -1 none).  Entry p qualifies for row r when
    p != r, same group, r has a ts, |ts[p] - ts[r]| <= within in 64 bits, and not (slot[r] >= 0 and slot[p] == slot[r]); the partner is
    the FIRST qualifying entry in list order.  value "a": v = Sa; "min": the smaller of Sa[r] and Sb[partner] in key order."""
    assert value in VALUES
    Sa, Sb = np.asarray(Sa, np.float32), np.asarray(Sb, np.float32)
    n = len(Sa)
    group, slot, t = np.asarray(group, np.int64), np.asarray(slot, np.int64), np.asarray(ts, np.int64)
    P = np.asarray(plist, np.int64)
    partner = np.full(n, -1, np.int64)
    for g in np.unique(group[P]):                                # one (entries, rows) matrix per group: a pair of two groups never qualifies
        Pg, R = P[group[P] == g], np.flatnonzero((group == g) & (t != NO_TS))   # the entries stay in list order
        q = np.abs(t[Pg][:, None] - t[R][None, :]) <= int(within)
        q &= Pg[:, None] != R[None, :]
        q &= ~((slot[R][None, :] >= 0) & (slot[Pg][:, None] == slot[R][None, :]))
        hit = q.any(axis=0)
        partner[R[hit]] = Pg[q.argmax(axis=0)[hit]]              # argmax: the first True
    dead = partner < 0
    v = Sa.copy()
    if value == "min":
        sb = Sb[np.maximum(partner, 0)]
        take = ~dead & (ordered(sb) < ordered(Sa))
        v[take] = sb[take]
    return v, dead, partner


def list_position(plist, partner):
    """The place in the list of each row's partner, -1 where it has none"""
    at = np.full(int(max(np.max(plist, initial=-1), np.max(partner, initial=-1))) + 2, -1, np.int64)
    at[np.asarray(plist, np.int64)] = np.arange(len(plist))
    return np.where(partner >= 0, at[np.maximum(partner, 0)], -1)


def near_order(v, dead, slot, group, n_groups, ts, cls, allowed=None, tracks=True, cut=None, ts_range=None, classes=None):
    """-> (rows, scores) of every answer: the dead rows and those A's row filter rejects sit in a forbidden group"""
    g, al = disguise(group, n_groups, passing(ts, cls, ts_range, classes) & ~dead, allowed)
    return full_order(v, slot, g, al, tracks, cut)


def near_page(v, dead, partner, Sb, n_partners, slot, group, n_groups, ts, cls, start, count, allowed=None, cut=None, tracks=True, ts_range=None,
              classes=None):
    """One window of the ranking behind a fold (`near_fold`'s v, dead, partner) -> what EmbeddingIndex.rank_near returns"""
    g, al = disguise(group, n_groups, passing(ts, cls, ts_range, classes) & ~dead, allowed)
    idx, sc, total = rank_model(v[None, :], slot, g, start, count, al, cut, tracks)
    pr = np.where(idx >= 0, partner[np.maximum(idx, 0)], -1).astype(np.int32)
    ps = np.where(idx >= 0, np.asarray(Sb, np.float32)[np.maximum(pr, 0)], np.float32(-np.inf)).astype(np.float32)
    return idx, sc, total, pr, ps, n_partners


def near_model(Sa, Sb, slot, group, n_groups, ts, cls, within, start, count, partners=DEFAULT_PARTNERS, cut_b=None, value="min", allowed=None,
               cut=None, tracks=True, ts_range=None, classes=None, b_ts_range=None, b_classes=None):
    """-> what EmbeddingIndex.rank_near returns: (idx (1, count), score (1, count), total (1,), partner (1, count), partner_score
    (1, count), n_partners)"""
    plist, n_partners = partner_list(Sb, group, n_groups, ts, cls, partners, cut_b, allowed, b_ts_range, b_classes)
    v, dead, partner = near_fold(Sa, Sb, plist, group, slot, ts, within, value)
    return near_page(v, dead, partner, Sb, n_partners, slot, group, n_groups, ts, cls, start, count, allowed, cut, tracks, ts_range, classes)


def near_timeline_model(Sa, Sb, slot, group, n_groups, ts, cls, within, t0, bin_seconds, n_bins, partners=DEFAULT_PARTNERS, cut_b=None, value="min",
                        allowed=None, cut=None, tracks=True, ts_range=None, classes=None, b_ts_range=None, b_classes=None):
    """-> what EmbeddingIndex.timeline_near returns: (counts (1, n_bins) int64, total (1,) int64, n_partners), from the full order as
    where_cases.timeline_model takes it"""
    plist, n_partners = partner_list(Sb, group, n_groups, ts, cls, partners, cut_b, allowed, b_ts_range, b_classes)
    v, dead, _ = near_fold(Sa, Sb, plist, group, slot, ts, within, value)
    rows, _ = near_order(v, dead, slot, group, n_groups, ts, cls, allowed, tracks, cut, ts_range, classes)
    t = np.asarray(ts, np.int64)[rows]
    b = (t - int(t0)) // int(bin_seconds)
    b = b[(t != NO_TS) & (b >= 0) & (b < n_bins)]
    return np.bincount(b, minlength=n_bins)[None, :].astype(np.int64), np.array([len(rows)], np.int64), n_partners


def case_table():
    """[(within, partners)]: every pair of the two lists"""
    return [(w, p) for w in WITHINS for p in PARTNERS]
