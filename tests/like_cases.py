"""The contract of cc_index_fetch_rows / cc_index_rank_like as a numpy model, and the seeded worlds both new test files use
(tests/test_index_like_host.py, where the model is held to a brute-force loop, and tests/test_gpu_index_like.py, where the device is
held to the model).

A query by stored rows is a single query whose score vector is the row-wise maximum of the score matrix of the query rows, and an
excluded row is a row in a forbidden group: `fold` does the first, `where_cases.disguise` the second, and `rank_cases.rank_model`,
unchanged, the rest - on the device's own score matrix `ix.scores(ix.fetch(rows))`, so every comparison is exact."""
import numpy as np

import score_cases
from i8_cases import decode, quantise
from rank_cases import full_order, rank_model
from where_cases import DIM, GROUPS, Rows, disguise, passing

MAX_ROWS = 64                                                    # CC_LIKE_MAX_ROWS
N_ODD, N_EVEN = 2 * 4096 + 37, 2 * 4096 + 32                     # 8229: score rows unaligned, no GEMM route; 8224 = 8 * 1028: every route opens
SET_SIZES = (2, 9, 17, 18, 64)                                   # both sides of the f32 / bf16 GEMM threshold (17) and of the int8 MFMA one (18)


def stored(E, storage):
    """What an index of `storage` holds of E, decoded to float32: score_cases.stored for f32 / bf16, the int8 rule for i8"""
    if storage == "i8":
        return decode(*quantise(E))
    return score_cases.stored(E, storage)


def expected_path(storage, dim, n, Q):
    """score_cases.expected_path plus the int8 rule: the MFMA kernel (2) from 18 queries on, dim % 256 == 0 and dim <= 4096"""
    if storage == "i8":
        return 2 if (Q >= 18 and dim % 256 == 0 and dim <= 4096 and n >= 1) else 0
    return score_cases.expected_path(storage, dim, n, Q)


def ordered(x):
    """float32 -> uint32, monotone in the total order of the ranking keys: -0 below +0"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def fold(S):
    """(Q, n) float32 -> (n,) float32: per row the maximum in the order of `ordered`"""
    S = np.atleast_2d(np.ascontiguousarray(S, dtype=np.float32))
    return S[ordered(S).argmax(axis=0), np.arange(S.shape[1])]


def dead_rows(n, rows, group, slot, exclude):
    """Bool per row: the row is excluded.  "rows": the query rows; "track": every row of the query rows' group and slot."""
    d = np.zeros(n, bool)
    rows = np.asarray(rows, np.int64)
    if exclude == "rows":
        d[rows] = True
    elif exclude == "track":
        assert (group[rows] == group[rows[0]]).all() and (slot[rows] == slot[rows[0]]).all() and slot[rows[0]] >= 0
        d = (np.asarray(group) == group[rows[0]]) & (np.asarray(slot) == slot[rows[0]])
    else:
        assert exclude is None
    return d


def like_order(S, slot, group, n_groups, ts, cls, rows, allowed=None, tracks=True, cut=None, exclude=None, ts_range=None, classes=None):
    """(Q, n) scores of the query rows -> (rows, scores) of every answer"""
    ok = passing(ts, cls, ts_range, classes) & ~dead_rows(len(slot), rows, group, slot, exclude)
    g, al = disguise(group, n_groups, ok, allowed)
    return full_order(fold(S), slot, g, al, tracks, cut)


def like_model(S, slot, group, n_groups, ts, cls, rows, start, count, allowed=None, cut=None, tracks=True, exclude=None, ts_range=None, classes=None):
    """(Q, n) scores of the query rows -> what EmbeddingIndex.rank_like returns: (idx (1, count), score (1, count), total (1,))"""
    ok = passing(ts, cls, ts_range, classes) & ~dead_rows(len(slot), rows, group, slot, exclude)
    g, al = disguise(group, n_groups, ok, allowed)
    return rank_model(fold(S)[None, :], slot, g, start, count, al, cut, tracks)


def pick_rows(row, members):
    """The picking rule of ObjectFinder.similar(whole_track=True), restated: up to 64 members, all of them; more, the clicked row
    plus the others (in row order) at positions linspace(0, m - 2, 63) rounded.  Ascending."""
    members = sorted(set(int(r) for r in members))
    assert row in members
    if len(members) <= MAX_ROWS:
        return members
    others = [r for r in members if r != row]
    at = [int(p) for p in np.linspace(0, len(members) - 2, MAX_ROWS - 1).round()]
    return sorted([others[p] for p in at] + [int(row)])


class World(Rows):
    """where_cases.Rows with a query track: slot 0 (a tenth of the rows) in the group of slot 0's FIRST row, so that excluding the
    track kills the row that would place slot 0 among equal scores, while slot 0 goes on answering from the other groups."""

    def __init__(self, n):
        super().__init__(n=n)
        self.qslot = 0
        self.qgroup = int(self.group[np.flatnonzero(self.slot == 0)[0]])
        self.track = np.flatnonzero((self.slot == self.qslot) & (self.group == self.qgroup))

    def copies_outside(self):
        """[(row of the query track, a byte-equal row outside it)], computed once"""
        if not hasattr(self, "_copies"):
            b = self.E.view(np.uint32)
            inside = set(self.track.tolist())
            self._copies = []
            for r in self.track:
                same = np.flatnonzero((b == b[r]).all(axis=1))
                self._copies += [(int(r), int(c)) for c in same if int(c) not in inside]
        return self._copies

    def query_rows(self, k):
        """k rows of the query track, spread over it, in ascending order"""
        return self.track[np.linspace(0, len(self.track) - 1, k).round().astype(int)]
