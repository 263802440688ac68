"""The day digest on the host: the model of tests/digest_cases.py held to a plain double loop, its invariants, the condition on the
inputs that makes the GPU comparison exact, and that the worlds reach both sides of the leader cap.  No GPU."""
import numpy as np
import pytest

from digest_cases import (DIMS, FILTERS, LEFT_OVER, MAX_LEADERS, NO_TS, NOT_COMPETING, SAME_AT, STORAGES, competing, digest_model, double_loop,
                          leaders_of, similarities, stored, threshold_margins, world, world_similarities)

BY = ("count", "first")


def test_the_abi_knows_the_entry_point():
    from clearcam_amd import _lib
    assert "cc_index_digest" in _lib.SYMBOLS and _lib.DIGEST_MAX_LEADERS == MAX_LEADERS == 1024
    assert (_lib.DIGEST_BY_COUNT, _lib.DIGEST_BY_FIRST) == (0, 1)


@pytest.mark.parametrize("dim", DIMS)
def test_the_model_is_the_double_loop(dim):
    w = world(dim)
    D = stored(w.E, "f32")
    rng = np.random.default_rng(dim)
    picks = [np.arange(150), np.arange(100, 260), np.sort(rng.choice(w.n, 170, replace=False)), np.arange(1), np.arange(0)]
    for rows in picks:
        S = similarities(D, rows)
        for same_at in SAME_AT + (np.inf, -np.inf, 0.0):
            for cap in (1, 7, MAX_LEADERS):
                assert np.array_equal(leaders_of(S, same_at, cap), double_loop(D, rows, same_at, cap)), (dim, len(rows), same_at, cap)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_no_pair_of_stored_rows_comes_near_a_threshold_of_the_digest(dim, storage):
    """Re-asserts test_no_pair_of_stored_rows_comes_near_a_threshold of tests/test_index_distinct_host.py for the thresholds used here:
    the device compares a float32 chain, the model the rounded float64 value, and they agree while no pair lies nearer to a threshold
    than the order of a float32 summation can move it."""
    margins, bound = threshold_margins(stored(world(dim).E, storage), SAME_AT)
    assert bound < 1e-4
    for same_at, m in zip(SAME_AT, margins):
        assert m > 10 * bound, (dim, storage, same_at, m, bound)


def check_invariants(w, rows, got, cap):
    r, c, t0, t1, totals, owner = got
    leaders, n_comp, left = (int(v) for v in totals)
    assert n_comp == len(rows) and leaders <= cap and (left == 0 or leaders == cap)
    assert (owner == NOT_COMPETING).sum() == w.n - n_comp and (owner == LEFT_OVER).sum() == left
    mem = owner >= 0
    assert set(np.flatnonzero(mem).tolist()) | set(np.flatnonzero(owner == LEFT_OVER).tolist()) == set(rows.tolist())
    lead = np.flatnonzero(mem & (owner == np.arange(w.n)))
    assert len(lead) == leaders and np.isin(owner[mem], lead).all()                    # every owner is a leader
    assert (owner[mem] <= np.flatnonzero(mem)).all()                                   # ... and stands before its members
    k = r >= 0
    assert k.sum() == leaders and c[k].sum() == n_comp - left                          # asked for every leader: the counts add up
    assert np.array_equal(np.sort(r[k]), lead)
    for row, cnt, a, b in zip(r[k], c[k], t0[k], t1[k]):
        t = w.ts[owner == row]
        t = t[t != NO_TS]
        assert cnt == (owner == row).sum() and (a, b) == ((t.min(), t.max()) if len(t) else (NO_TS, NO_TS))


@pytest.mark.parametrize("storage", ("f32", "i8"))
def test_the_worlds_reach_both_sides_of_the_cap(storage):
    """Whole world and the filters at the three thresholds, dim 768: below the cap with nothing left over, and at the cap with rows
    left over; the orders agree on everything but the order."""
    w = world(768)
    S, D = world_similarities(768, storage), stored(w.E, storage)
    seen = {}
    for name in (None, "ts", "both+allowed"):
        rows, _ = competing(w, name)
        Ss = S[np.ix_(rows, rows)]
        for same_at in SAME_AT:
            got = digest_model(D, rows, same_at, MAX_LEADERS, "count", 0, MAX_LEADERS, ts=w.ts, S=Ss)
            check_invariants(w, rows, got, MAX_LEADERS)
            first = digest_model(D, rows, same_at, MAX_LEADERS, "first", 0, MAX_LEADERS, ts=w.ts, S=Ss)
            assert np.array_equal(first[4], got[4]) and np.array_equal(first[5], got[5])
            k = int(got[4][0])
            assert (np.diff(first[0][:k]) > 0).all() and np.array_equal(np.sort(got[0][:k]), first[0][:k])
            assert (np.diff(got[1][:k]) <= 0).all() and (got[1][k:] == 0).all() and (got[0][k:] == -1).all()
            ties = np.flatnonzero(np.diff(got[1][:k]) == 0)
            assert len(ties) and (got[0][ties] < got[0][ties + 1]).all()               # equal counts: the lower leader row first
            seen[(name, same_at)] = got[4]
    whole = [seen[(None, t)] for t in SAME_AT]                                         # SAME_AT descends: 0.95, 0.92, 0.90
    assert whole[2][0] < MAX_LEADERS and whole[2][2] == 0 and whole[2][0] > 0          # 0.90: below the cap, nothing left over
    assert whole[1][0] == MAX_LEADERS and whole[1][2] > 0                              # 0.92: the cap, rows left over
    assert whole[0][0] == MAX_LEADERS and whole[0][2] > whole[1][2]                    # 0.95: more of them
    ts_ = [seen[("ts", t)] for t in SAME_AT]
    assert ts_[2][0] < MAX_LEADERS and ts_[2][2] == 0 and ts_[1][0] == ts_[0][0] == MAX_LEADERS and 0 < ts_[1][2] < ts_[0][2]
    narrow = [seen[("both+allowed", t)] for t in SAME_AT]
    assert all(0 < v[0] < MAX_LEADERS and v[2] == 0 for v in narrow) and narrow[0][0] > narrow[1][0] > narrow[2][0]


def test_small_indices_and_small_caps():
    """The first n rows of the world as an index of their own: around the word boundary below the cap, and around the piece boundary
    with a cap of 64 that is reached inside the first piece."""
    w = world(768)
    D = stored(w.E, "f32")
    for n in (63, 64, 65):
        got = digest_model(D[:n], np.arange(n), 0.90, MAX_LEADERS, "count", 0, n, ts=w.ts[:n])
        assert 0 < got[4][0] <= n and got[4][2] == 0
    for n in (1023, 1024, 1025):
        got = digest_model(D[:n], np.arange(n), 0.95, 64, "count", 0, 64, ts=w.ts[:n])
        assert got[4][0] == 64 and got[4][2] > 0 and got[4][2] == (got[5] == LEFT_OVER).sum()
        assert np.flatnonzero(got[5] == LEFT_OVER)[0] < 1024                              # the cap is reached in the middle of a piece
    got = digest_model(stored(world(256).E, "f32"), np.arange(world(256).n), 0.90, MAX_LEADERS, "count", 0, 10)
    assert 0 < got[4][0] < MAX_LEADERS and got[4][2] == 0


def test_windows_and_padding():
    w = world(256)
    D = stored(w.E, "f32")
    rows = np.arange(500)
    S = similarities(D, rows)
    full = digest_model(D[:500], rows, 0.92, MAX_LEADERS, "count", 0, MAX_LEADERS, ts=w.ts[:500], S=S)
    k = int(full[4][0])
    for by in BY:
        full = digest_model(D[:500], rows, 0.92, MAX_LEADERS, by, 0, MAX_LEADERS, ts=w.ts[:500], S=S)
        for start, count in ((0, 1), (k // 2, 3), (k - 1, 1), (k - 1, 4), (k, 2), (0, k + 5)):
            got = digest_model(D[:500], rows, 0.92, MAX_LEADERS, by, start, count, ts=w.ts[:500], S=S)
            for a, b, pad in zip(got[:4], full[:4], (-1, 0, NO_TS, NO_TS)):
                want = np.concatenate([b[start:start + count][:max(k - start, 0)], np.full(count, pad, np.int32)])[:count]
                assert np.array_equal(a, want), (by, start, count)
