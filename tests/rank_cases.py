"""The contract of cc_index_rank / EmbeddingIndex.rank as a numpy model, shared by tests/test_index_rank_host.py (where it IS
the index) and tests/test_gpu_index_rank.py (where the device is held to it).

It is the full order that tests/test_gpu_index_tracks.py::expected builds before its `[:k]` - per slot the best allowed row (equal
scores: the lower row), slot-less rows as they are, descending by score and then by first appearance (a track: its first allowed
row; a slot-less row: N + row) - plus what ranking adds: without tracks every allowed row answers for itself at position = row;
only answers with score >= cut (float32) exist; a window [start, start + count) of that order with -1/-inf padding; and total,
the number of answers."""
import numpy as np


def allowed_rows(n, group, allowed):
    if allowed is None:
        return np.arange(n)
    al = np.asarray(allowed)
    return np.flatnonzero((group < len(al)) & (al[np.minimum(group, len(al) - 1)] != 0))


def full_order(sc, slot, group, allowed=None, tracks=True, cut=None):
    """One score vector -> (rows, scores) of every answer, in the order of the contract."""
    sc = np.asarray(sc, np.float32)
    n = len(sc)
    rows = allowed_rows(n, group, allowed)
    if tracks:
        tr, loose = rows[slot[rows] >= 0], rows[slot[rows] < 0]
        o = tr[np.lexsort((tr, -sc[tr], slot[tr]))]              # by slot, then score descending, then row: the first of a slot is its best
        lead = np.r_[True, slot[o][1:] != slot[o][:-1]] if len(o) else np.zeros(0, bool)
        best = o[lead]
        first = np.full(int(max(slot.max(initial=-1), 0)) + 2, n, np.int64)
        np.minimum.at(first, slot[tr], tr)
        ans = np.concatenate([best, loose]).astype(np.int64)
        pos = np.concatenate([first[slot[best]], n + loose]).astype(np.int64)
    else:
        ans = pos = rows.astype(np.int64)
    if cut is not None:
        keep = ~(sc[ans] < np.float32(cut))
        ans, pos = ans[keep], pos[keep]
    order = np.lexsort((pos, -sc[ans]))
    return ans[order], sc[ans[order]]


def window(ans, s, start, count):
    """-> (idx (count,) int32, score (count,) f32, total) of a full order"""
    idx = np.full(count, -1, np.int32); out = np.full(count, -np.inf, np.float32)
    part = slice(start, start + count)
    m = len(ans[part])
    idx[:m] = ans[part]; out[:m] = s[part]
    return idx, out, len(ans)


def rank_model(sc, slot, group, start, count, allowed=None, cut=None, tracks=True):
    """(Q, N) scores -> what EmbeddingIndex.rank returns"""
    sc = np.atleast_2d(np.asarray(sc, np.float32))
    res = [window(*full_order(v, slot, group, allowed, tracks, cut), start, count) for v in sc]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int64)


def run_bounds(s, min_len=2):
    """(first, last + 1) of every run of at least min_len equal values in a descending score list"""
    s = np.asarray(s)
    edge = np.flatnonzero(np.r_[True, s[1:] != s[:-1], True])
    return [(int(a), int(b)) for a, b in zip(edge[:-1], edge[1:]) if b - a >= min_len]
