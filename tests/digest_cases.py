"""The contract of cc_index_digest as a numpy model, for tests/test_index_digest_host.py (where the model is held to a plain double
loop) and tests/test_gpu_index_digest.py (where the device is held to the model).

A digest is leader clustering in row order: walking the competing rows in ascending row number, a row joins the first-created leader
it is at least `same_at` similar to, else it becomes a leader while fewer than `cap` exist, else it is left over.  The similarity is
the float64 dot product of the stored rows (like_cases.stored), rounded to float32 and compared in float32.  The device compares the
float cc_index_gram computes instead, which lies within score_cases.order_free_bound of the float64 value: the two agree wherever no
pair of stored rows comes nearer to a threshold than that, which tests/test_index_digest_host.py checks for SAME_AT on the worlds used
here (distinct_cases.DupWorld; its clusters meet at LEVELS, 0.01 and more from every threshold).  distinct_cases.crafted_rows gives
rows whose products are exact in every order, for thresholds that ARE a pair's value.

The model walks as the device does - a new leader claims the unclaimed matching rows behind it - which is the sequential rule because
leaders are created in row order: a row's first-created matching leader is the first one that could claim it."""
import numpy as np

from clearcam_amd import _lib
from distinct_cases import DIMS, SAME_AT, crafted_rows, threshold_margins, world            # noqa: F401  (re-exported for the two test files)
from like_cases import stored                                                             # noqa: F401
from score_cases import order_free_bound                                                  # noqa: F401
from where_cases import FILTERS, GROUPS, NO_TS, passing                                    # noqa: F401

MAX_LEADERS = _lib.DIGEST_MAX_LEADERS                            # CC_DIGEST_MAX_LEADERS: 1024
STORAGES = ("f32", "bf16", "i8")
NOT_COMPETING, LEFT_OVER = -1, -2                                # owner of a row outside the selection / of a left-over row


def similarities(D, rows, block=1024):
    """(m, m) float32: the float64 dot products of the stored rows D[rows], rounded once"""
    A = np.asarray(D, np.float64)[np.asarray(rows, np.int64)]
    S = np.empty((len(A), len(A)), np.float32)
    for a in range(0, len(A), block):
        S[a:a + block] = A[a:a + block] @ A.T
    return S


def leaders_of(S, same_at, cap):
    """(m, m) float32 similarities of the competing rows in walk order -> owner (m,) int64: the position of each row's leader (its own
    for a leader), LEFT_OVER for a left-over row."""
    m = len(S)
    t = np.float32(same_at)
    owner = np.full(m, LEFT_OVER, np.int64)
    claimed = np.zeros(m, bool)
    made = 0
    for j in range(m):
        if claimed[j]:
            continue
        if made == cap:
            continue                                             # left over: owns nothing, claims nothing
        made += 1
        hit = (S[j] >= t) & ~claimed
        hit[:j] = False
        hit[j] = True                                            # a leader owns itself whatever its norm
        owner[hit] = j
        claimed |= hit
    return owner


def summarise(competing, owner_pos, n, ts, by, start, count):
    """The walk's answer -> what EmbeddingIndex.digest(..., owners=True) returns"""
    competing = np.asarray(competing, np.int64)
    ts = np.full(n, NO_TS, np.int64) if ts is None else np.asarray(ts, np.int64)
    owner = np.full(n, NOT_COMPETING, np.int32)
    member = owner_pos >= 0
    owner[competing[~member]] = LEFT_OVER
    owner[competing[member]] = competing[owner_pos[member]]
    lead = np.flatnonzero(owner_pos == np.arange(len(competing)))
    cnt = np.bincount(owner_pos[member], minlength=len(competing))[lead] if len(competing) else np.zeros(0, np.int64)
    first, last = np.full(len(lead), NO_TS, np.int64), np.full(len(lead), NO_TS, np.int64)
    for k, p in enumerate(lead):
        t = ts[competing[owner_pos == p]]
        t = t[t != NO_TS]
        if len(t):
            first[k], last[k] = t.min(), t.max()
    order = np.lexsort((competing[lead], -cnt)) if by == "count" else np.arange(len(lead))
    win = order[start:start + count]
    rows, counts = np.full(count, -1, np.int32), np.zeros(count, np.int32)
    t0, t1 = np.full(count, NO_TS, np.int32), np.full(count, NO_TS, np.int32)
    rows[:len(win)], counts[:len(win)], t0[:len(win)], t1[:len(win)] = competing[lead[win]], cnt[win], first[win], last[win]
    totals = np.array([len(lead), len(competing), int((~member).sum())], np.int64)
    return rows, counts, t0, t1, totals, owner


def digest_model(D, competing_rows, same_at, cap, by, start, count, ts=None, S=None):
    """D (n, dim) float32: what the index holds, decoded; competing_rows ascending -> (rows, counts, ts_first, ts_last (count,) int32,
    totals (3,) int64, owner (n,) int32).  S: `similarities(D, competing_rows)` where the caller has it already."""
    competing = np.asarray(competing_rows, np.int64)
    assert (np.diff(competing) > 0).all()
    S = similarities(D, competing) if S is None else S
    return summarise(competing, leaders_of(S, same_at, cap), len(D), ts, by, start, count)


def double_loop(D, competing_rows, same_at, cap):
    """The contract as it is written, row by row and leader by leader -> owner positions as leaders_of returns them"""
    D = np.asarray(D, np.float64)
    t = np.float32(same_at)
    leaders, owner = [], []
    for j, r in enumerate(competing_rows):
        mine = LEFT_OVER
        for p in leaders:
            if np.float32(np.dot(D[competing_rows[p]], D[r])) >= t:
                mine = p
                break
        else:
            if len(leaders) < cap:
                leaders.append(j)
                mine = j
        owner.append(mine)
    return np.asarray(owner, np.int64)


def competing(w, name=None):
    """The rows of world `w` that compete under filter `name` of where_cases.FILTERS (None: all) -> (rows, digest keyword arguments)"""
    if name is None:
        return np.arange(w.n), {}
    ts_range, classes, allowed = FILTERS[name]
    ok = passing(w.ts, w.cls, ts_range, classes)
    if allowed is not None:
        ok &= allowed[w.group].astype(bool)
    kw = {k: v for k, v in (("ts_range", ts_range), ("classes", classes), ("allowed", allowed)) if v is not None}
    return np.flatnonzero(ok), kw


_S = {}


def world_similarities(dim, storage):
    """similarities of the whole world, remembered for the last (dim, storage) only: 270 MB"""
    if (dim, storage) not in _S:
        _S.clear()
        w = world(dim)
        _S[(dim, storage)] = similarities(stored(w.E, storage), np.arange(w.n))
    return _S[(dim, storage)]
