"""Query by stored rows on the CPU: the numpy model of tests/like_cases.py against a brute-force loop, the track-row picking rule,
`_RowTable.row_of`, and the preconditions the GPU tests (tests/test_gpu_index_like.py) rely on, checked with numpy scores of the
stored rows."""
import numpy as np
import pytest

from clearcam_amd import _lib
from clearcam_amd import objects as O
from like_cases import MAX_ROWS, N_EVEN, N_ODD, SET_SIZES, World, dead_rows, expected_path, fold, like_model, like_order, ordered, pick_rows, stored
from where_cases import DIM, GROUPS, NO_TS, Rows


def brute(S, slot, group, ts, cls, rows, allowed, tracks, cut, exclude, ts_range, classes):
    """The contract in words, row by row -> [(row, score)] in order"""
    n = S.shape[1]
    key = lambda x: ordered(np.float32(x)).item()                                   # noqa: E731
    best, first, loose = {}, {}, []
    v = [max((S[q][r] for q in range(S.shape[0])), key=key) for r in range(n)]
    for r in range(n):
        if exclude == "rows" and r in rows:
            continue
        if exclude == "track" and group[r] == group[rows[0]] and slot[r] == slot[rows[0]]:
            continue
        if allowed is not None and not (group[r] < len(allowed) and allowed[group[r]]):
            continue
        if ts_range is not None and (ts[r] == NO_TS or ts[r] < ts_range[0] or ts[r] > ts_range[1]):
            continue
        if classes is not None and (cls[r] < 0 or cls[r] not in classes):
            continue
        t = slot[r]
        if tracks and t >= 0:
            first.setdefault(t, r)
            if t not in best or v[r] > v[best[t]]:
                best[t] = r
        else:
            loose.append(r)
    ans = [(v[r], first[t], r) for t, r in best.items()] + [(v[r], (n + r) if tracks else r, r) for r in loose]
    if cut is not None:
        ans = [a for a in ans if not a[0] < np.float32(cut)]
    ans.sort(key=lambda a: (-a[0], a[1]))
    return [(r, s) for s, _, r in ans]


def test_fold_takes_the_maximum_in_key_order():
    S = np.array([[-0.0, 0.0, 1.0, -2.0, -0.0], [0.0, -0.0, -1.0, -3.0, -0.0]], np.float32)
    v = fold(S)
    assert v.tolist() == [0.0, 0.0, 1.0, -2.0, 0.0] and np.signbit(v).tolist() == [False, False, False, True, True]
    assert np.array_equal(fold(S[:1]), S[0]) and np.array_equal(np.signbit(fold(S[:1])), np.signbit(S[0]))
    rng = np.random.default_rng(1)
    R = rng.standard_normal((7, 300)).astype(np.float32)
    assert np.array_equal(fold(R), R.max(axis=0))


@pytest.mark.parametrize("tracks", [True, False])
def test_model_equals_the_brute_force_loop(tracks):
    w = Rows(n=60, seed=3, queries=2)
    w.E[7] = w.E[3]; w.E[40] = w.E[3]                                               # ties across tracks, whatever the seed drew
    track = np.flatnonzero((w.slot == w.slot[3]) & (w.group == w.group[3]))
    assert w.slot[3] >= 0 and len(track) >= 1
    allowed = np.array([1, 1, 0, 1, 1], np.uint8)
    for rows in ([3], [3, 3], track.tolist(), [50, 3, 17]):
        S = (w.E[rows] @ w.E.T).astype(np.float32)
        one_track = len({(w.group[r], w.slot[r]) for r in rows}) == 1 and w.slot[rows[0]] >= 0
        for exclude in (None, "rows") + (("track",) if one_track else ()):
            for al in (None, allowed):
                for cut, ts_range, classes in ((None, None, None), (float(np.median(fold(S))), None, None), (None, (0, 300), (0, 2, 64, 255))):
                    want = brute(S, w.slot, w.group, w.ts, w.cls, rows, al, tracks, cut, exclude, ts_range, classes)
                    got, s = like_order(S, w.slot, w.group, GROUPS, w.ts, w.cls, rows, al, tracks, cut, exclude, ts_range, classes)
                    what = (rows, exclude, al is None, cut, ts_range)
                    assert got.tolist() == [r for r, _ in want] and s.tolist() == [x for _, x in want], what
                    idx, out, total = like_model(S, w.slot, w.group, GROUPS, w.ts, w.cls, rows, 2, 9, al, cut, tracks, exclude, ts_range, classes)
                    assert idx.shape == out.shape == (1, 9) and total.shape == (1,) and total[0] == len(want), what
                    assert idx[0].tolist() == ([r for r, _ in want][2:11] + [-1] * 9)[:9], what
                    if exclude:
                        assert not set(got.tolist()) & set(np.flatnonzero(dead_rows(60, rows, w.group, w.slot, exclude)).tolist())


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 66, 127, 1000])
def test_the_picking_rule(m):
    rng = np.random.default_rng(m)
    members = np.sort(rng.choice(5000, m, replace=False))
    for clicked in {int(members[0]), int(members[-1]), int(members[m // 2]), int(members[m // 3])}:
        got = O.pick_track_rows(clicked, rng.permutation(members))
        assert got.dtype == np.int64 and got.tolist() == pick_rows(clicked, members.tolist())
        assert len(got) == min(m, MAX_ROWS) and clicked in got and (np.diff(got) > 0).all() and set(got.tolist()) <= set(members.tolist())
        assert np.array_equal(got, O.pick_track_rows(clicked, members))              # the same on every call
        if m > MAX_ROWS:                                                            # ... and it spans the track
            assert got[0] in members[:2] and got[-1] in members[-2:]
    with pytest.raises(ValueError):
        O.pick_track_rows(5001, members)
    assert MAX_ROWS == _lib.LIKE_MAX_ROWS == 64


FOLDER = "data/cameras/front/objects/2026-01-01"


def test_row_of_follows_extend_and_remove():
    t = O._RowTable()
    a = [f"{FOLDER}/{i}.0_{i % 3}_2.jpg" for i in range(6)]
    t.extend(a[:4]); t.extend(a[4:])
    assert [t.row_of(p) for p in a] == list(range(6))
    with pytest.raises(KeyError):
        t.row_of(f"{FOLDER}/nothing.jpg")
    t.extend([a[1], f"{FOLDER}/9.0_1_2.jpg"])                                       # a path stored twice names its last row
    assert t.row_of(a[1]) == 6 and t.row_of(f"{FOLDER}/9.0_1_2.jpg") == 7 and len(t.row) == 7
    mask = np.zeros(8, bool); mask[[0, 6]] = True                                    # the later copy goes: the earlier row answers again
    assert t.remove(mask) == 2
    assert t.paths == a[1:] + [f"{FOLDER}/9.0_1_2.jpg"]
    assert [t.row_of(p) for p in t.paths] == list(range(6))
    with pytest.raises(KeyError):
        t.row_of(a[0])
    t.extend([a[0]])
    assert t.row_of(a[0]) == 6 and all(t.paths[r] == p for p, r in t.row.items())


def test_the_storage_and_route_rules_cover_int8():
    E = Rows(n=40, seed=5).E
    assert np.array_equal(stored(E, "f32"), E) and not np.array_equal(stored(E, "bf16"), E) and not np.array_equal(stored(E, "i8"), E)
    assert np.abs(stored(E, "i8") - E).max() < 1.0 / 127 and np.abs(stored(E, "bf16") - E).max() < 2.0 ** -8
    taken = {s: {expected_path(s, DIM, n, Q) for n in (N_ODD, N_EVEN) for Q in SET_SIZES} for s in ("f32", "bf16", "i8")}
    assert taken == {"f32": {0, 1}, "bf16": {0, 1}, "i8": {0, 2}}
    assert [expected_path("f32", DIM, N_EVEN, Q) for Q in SET_SIZES] == [0, 0, 1, 1, 1] == [expected_path("bf16", DIM, N_EVEN, Q) for Q in SET_SIZES]
    assert [expected_path("i8", DIM, N_ODD, Q) for Q in SET_SIZES] == [0, 0, 0, 2, 2]
    assert not any(expected_path(s, DIM, N_ODD, Q) for s in ("f32", "bf16") for Q in SET_SIZES)


@pytest.mark.parametrize("n", [N_ODD, N_EVEN])
def test_the_worlds_hold_what_the_gpu_tests_need(n):
    w = World(n)
    assert (n == N_ODD and n % 4 == 1) or (n == N_EVEN and n % 8 == 0)
    assert 10 <= len(w.track) <= 200 and len(w.track) >= MAX_ROWS                  # the query track: enough rows for the largest set
    assert w.track[0] == np.flatnonzero(w.slot == w.qslot)[0]                        # its first row is the first row of its slot
    assert ((w.slot == w.qslot) & (w.group != w.qgroup)).sum() > 100               # the slot also lives in other groups
    copies = w.copies_outside()
    assert copies and any(w.slot[c] != w.qslot for _, c in copies)                  # a crop of the track has a copy in another track
    for storage in ("f32", "bf16", "i8"):
        D = stored(w.E, storage)
        for k in SET_SIZES:
            rows = w.query_rows(k)
            assert len(set(rows.tolist())) == k and (np.diff(rows) > 0).all()
            S = (D[rows] @ D.T).astype(np.float32)
            for exclude in ("rows", "track"):
                ans, _ = like_order(S, w.slot, w.group, GROUPS, w.ts, w.cls, rows, None, True, None, exclude)
                assert len(ans) > 1130, (storage, k, exclude)                        # a window at 1030 is real
                assert (w.slot[ans] == w.qslot).sum() == 1                           # the slot still answers, from another group
