"""Query by stored rows on the GPU: cc_index_fetch_rows / cc_index_rank_like through EmbeddingIndex.fetch / rank_like /
rank_like_device and ObjectFinder.similar.

The expected answers are the numpy model of tests/like_cases.py (the row-wise maximum in key order, excluded rows as a forbidden
group, then the unchanged model of tests/rank_cases.py) applied to the index's own `ix.scores(ix.fetch(rows))`.  Every comparison
is exact: integer keys and f32 maxima, no tolerance.  The worlds are like_cases.World: 8229 rows of 256 (odd: the score rows are
unaligned, no GEMM route) and 8224 (a multiple of 8: the f32 / bf16 GEMM from 17 query rows, the int8 MFMA kernel from 18)."""
import ctypes as C
import os

import numpy as np
import pytest

from like_cases import DIM, GROUPS, N_EVEN, N_ODD, SET_SIZES, World, expected_path, fold, like_model, like_order, stored
from rank_cases import run_bounds
from where_cases import FILTERS, unit

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "bf16", "i8")
NO_FILTER = (None, None, None)


class GpuWorld(World):
    def __init__(self, n):
        super().__init__(n)
        self._ix = {}

    def index(self, storage):
        from clearcam_amd.objects import EmbeddingIndex
        if storage not in self._ix:
            ix = self._ix[storage] = EmbeddingIndex(DIM, self.n, storage=storage)
            ix.add(self.E, self.group, self.slot, ts=self.ts, classes=self.cls)
        return self._ix[storage]

    def model(self, S, rows, start, count, name=None, cut=None, tracks=True, exclude=None):
        ts_range, classes, allowed = FILTERS[name] if name else NO_FILTER
        return like_model(S, self.slot, self.group, GROUPS, self.ts, self.cls, rows, start, count, allowed, cut, tracks, exclude, ts_range, classes)

    def order(self, S, rows, name=None, cut=None, tracks=True, exclude=None):
        ts_range, classes, allowed = FILTERS[name] if name else NO_FILTER
        return like_order(S, self.slot, self.group, GROUPS, self.ts, self.cls, rows, allowed, tracks, cut, exclude, ts_range, classes)


@pytest.fixture(scope="module")
def worlds():
    return {N_ODD: GpuWorld(N_ODD), N_EVEN: GpuWorld(N_EVEN)}


def filter_kw(name):
    ts_range, classes, allowed = FILTERS[name] if name else NO_FILTER
    return dict(ts_range=ts_range, classes=classes, allowed=allowed)


def same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int64, what
    assert got[0].shape == want[0].shape == got[1].shape and got[2].shape == want[2].shape, what
    assert np.array_equal(got[2], want[2]), (what, "total", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, "score")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_fetch_returns_the_stored_rows_bit_for_bit(worlds, storage):
    import torch
    from clearcam_amd import _lib
    from clearcam_amd.objects import EmbeddingIndex
    w = worlds[N_ODD]
    n, ix, D = w.n, w.index(storage), stored(w.E, storage)
    rng = np.random.default_rng(2)
    many = np.r_[n - 1, 0, rng.integers(0, n, 61), 0, n - 1]                        # 65 rows: unsorted, the first and the last row, repeats
    for rows in ([0], [n - 1], [5, 5, 5], [n - 1, 17, 0, 17], many):
        got = ix.fetch(rows)
        assert got.dtype == np.float32 and got.shape == (len(rows), DIM)
        assert np.array_equal(bits(got), bits(D[np.asarray(rows)])), (storage, len(rows))
        dev = ix.fetch(np.asarray(rows), device_out=True)
        torch.cuda.synchronize()
        assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(bits(dev.cpu().numpy()), bits(got))
    # an out-of-range number: an error, and the output buffer is untouched, on the host and on the device
    L = _lib.lib()
    for bad in ([n], [-1], [3, n, 4], [2 ** 40]):
        ids = np.asarray(bad, np.int64)
        out = np.full((len(bad), DIM), 7.0, np.float32)
        assert L.cc_index_fetch_rows(ix._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), len(bad), _lib.ptr(out), 0, None) == -22 and L.cc_last_error()
        assert (out == 7.0).all()
        dout = torch.full((len(bad), DIM), 7.0, dtype=torch.float32, device="cuda")
        assert L.cc_index_fetch_rows(ix._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), len(bad), _lib.ptr(dout), 1, None) == -22
        torch.cuda.synchronize()
        assert bool((dout == 7.0).all())
        with pytest.raises(_lib.CCError):
            ix.fetch(bad)
    with pytest.raises(_lib.CCError):
        ix.fetch([])
    assert np.array_equal(bits(ix.fetch([1])), bits(D[[1]]))                        # and the index goes on answering
    # after growth past the initial capacity, and after removal (rows renumbered)
    small = EmbeddingIndex(DIM, 1024, storage=storage)
    for a, b in ((0, 1000), (1000, 3000)):
        small.add(w.E[a:b], w.group[a:b], w.slot[a:b])
    assert small.capacity >= 3000 > 1024
    pick = np.r_[2999, 0, 1024, 1023, rng.integers(0, 3000, 30)]
    assert np.array_equal(bits(small.fetch(pick)), bits(D[pick]))
    mask = rng.random(3000) < 0.3
    mask[:70] = False; mask[100:300] = True; mask[2999] = False
    keep = np.flatnonzero(~mask)
    assert small.remove(mask) == int(mask.sum())
    pick = np.r_[len(keep) - 1, 0, 99, 100, rng.integers(0, len(keep), 30)]
    assert np.array_equal(bits(small.fetch(pick)), bits(D[keep[pick]]))
    with pytest.raises(_lib.CCError):
        small.fetch([len(keep)])
    small.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def tied_cut(s):
    runs = run_bounds(s)
    assert runs, "no equal scores among the answers"
    return float(s[runs[len(runs) // 2][0]])


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("tracks", [True, False])
def test_one_row_is_rank_of_the_fetched_row(worlds, storage, tracks):
    w = worlds[N_ODD]
    ix = w.index(storage)
    r = int(w.track[3])
    q = ix.fetch([r])
    for name in (None,) + tuple(FILTERS):
        kw = filter_kw(name)
        _, s, total = ix.rank(q, 0, w.n, min_score=None, tracks=tracks, **kw)
        s = s[0, :int(total[0])]
        assert len(s) > 40
        for cut in (None, tied_cut(s)):
            left = len(s) if cut is None else int((s >= np.float32(cut)).sum())
            for start, count in ((0, 50), (1030, 100), (max(left - 5, 0), 20)):
                got = ix.rank_like([r], start, count, min_score=cut, tracks=tracks, **kw)
                assert ix.last_scores_path() == 0
                same(got, ix.rank(q, start, count, min_score=cut, tracks=tracks, **kw), (storage, name, tracks, cut, start))
                assert got[2][0] == left
    idx, s, total = ix.rank_like([r], 0, 3, tracks=False)
    assert idx[0, 0] == r or bits(w.E[idx[0, 0]]).tolist() == bits(w.E[r]).tolist()  # the crop itself (or an equal one before it) comes first


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_sets_equal_the_model_on_every_route(worlds, storage):
    taken = set()
    for n, w in worlds.items():
        ix = w.index(storage)
        for k in SET_SIZES:
            rows = w.query_rows(k)
            path = expected_path(storage, DIM, n, k)
            got = {}
            for tracks, start, count, name in ((True, 0, 50, None), (True, 1030, 100, None), (False, 0, 50, None), (True, 5, 40, "both+allowed"), (False, 1030, 100, "ts")):
                got[(tracks, start, count, name)] = ix.rank_like(rows, start, count, tracks=tracks, **filter_kw(name))
                assert ix.last_scores_path() == path, (storage, n, k)
            S = ix.scores(ix.fetch(rows))
            assert ix.last_scores_path() == path and S.shape == (k, n)
            taken.add(path)
            for (tracks, start, count, name), res in got.items():
                same(res, w.model(S, rows, start, count, name, None, tracks), (storage, n, k, tracks, start, name))
            v = fold(S)
            assert (v >= S).all() and (v == S.max(axis=0)).all()
    assert taken == {"f32": {0, 1}, "bf16": {0, 1}, "i8": {0, 2}}[storage]


def test_sets_on_the_device_with_a_cut(worlds):
    import torch
    w = worlds[N_EVEN]
    ix = w.index("f32")
    rows = w.query_rows(17)
    S = ix.scores(ix.fetch(rows))
    _, s = w.order(S, rows, "ts", None, True, "track")
    cut = tied_cut(s)
    want = w.model(S, rows, 20, 200, "ts", cut, True, "track")
    same(ix.rank_like(rows, 20, 200, min_score=cut, exclude="track", **filter_kw("ts")), want, "host")
    di, ds, dt = ix.rank_like_device(rows, 20, 200, min_score=cut, exclude="track", **filter_kw("ts"))
    torch.cuda.synchronize()
    assert di.is_cuda and ds.is_cuda
    same((di.cpu().numpy(), ds.cpu().numpy(), dt), want, "rank_like_device")
    di, ds, dt = ix.rank_like_device(rows, 20, 200, min_score=cut, exclude="track", with_total=False, **filter_kw("ts"))
    torch.cuda.synchronize()
    assert dt is None and np.array_equal(di.cpu().numpy(), want[0])


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_exclusion_equals_the_model(worlds, storage):
    for n, w in worlds.items():
        ix = w.index(storage)
        r, c = next((r, c) for r, c in w.copies_outside() if w.slot[c] != w.qslot)   # a crop of the query track with a copy in another track
        for k in (1, 9) + ((18, 19) if n == N_EVEN else ()):                        # 18 / 19: at least 17 / 18 distinct rows, the GEMM and MFMA routes
            rows = np.unique(np.r_[w.query_rows(k)[:k - 1], r]) if k > 1 else np.array([r])
            S = ix.scores(ix.fetch(rows))
            v = fold(S)
            at = int(np.flatnonzero(rows == r)[0])
            for exclude in ("rows", "track"):
                dead = set(rows.tolist()) if exclude == "rows" else set(w.track.tolist())
                for tracks in (True, False):
                    got = ix.rank_like(rows, 0, n, tracks=tracks, exclude=exclude)
                    same(got, w.model(S, rows, 0, n, None, None, tracks, exclude), (storage, n, k, exclude, tracks))
                    ans = got[0][0, :int(got[2][0])]
                    assert not set(ans.tolist()) & dead and (ans >= 0).all()
                    if not tracks:
                        # the copy answers, and with the excluded crop's own score: equal rows score equally under every query
                        assert bits(v)[c] == bits(v)[r] and bits(S[at, c]) == bits(S[at, r])
                        assert got[1][0, ans.tolist().index(c)] == v[r]
                        assert got[2][0] == n - len(dead)
                    elif exclude == "track":
                        # the slot of the dead track still answers from its other groups
                        mine = ans[w.slot[ans] == w.qslot]
                        assert len(mine) == 1 and w.group[mine[0]] != w.qgroup
                for name in ("ts", "both+allowed"):
                    same(ix.rank_like(rows, 1030 if name == "ts" else 3, 60, exclude=exclude, **filter_kw(name)),
                         w.model(S, rows, 1030 if name == "ts" else 3, 60, name, None, True, exclude), (storage, n, k, exclude, name))


@pytest.mark.parametrize("storage", STORAGES)
def test_a_track_that_lost_its_first_row_is_placed_by_its_first_competing_row(storage):
    """Slot 0: row 0 (group 1, the clicked track) and row 2 (group 2).  Slot 1: row 1, byte-equal to row 2.  With the clicked track dead
    the two slots tie, and slot 1 (first competing row 1) comes before slot 0 (first competing row 2, not the dead row 0)."""
    from clearcam_amd._lib import CCError
    from clearcam_amd.objects import EmbeddingIndex
    rng = np.random.default_rng(4)
    E = unit(rng.standard_normal((6, DIM)))
    E[2] = E[1]
    slot, group = np.array([0, 1, 0, -1, -1, 2], np.int32), np.array([1, 2, 2, 1, 2, 1], np.int32)
    ix = EmbeddingIndex(DIM, 8, storage=storage)
    ix.add(E, group, slot)
    S = ix.scores(ix.fetch([0]))
    none = np.full(6, -(1 << 31), np.int32), np.full(6, -1, np.int32)
    idx, s, total = ix.rank_like([0], 0, 6, exclude="track")
    same((idx, s, total), like_model(S, slot, group, 3, *none, [0], 0, 6, None, None, True, "track"), "model")
    a, b = idx[0].tolist().index(1), idx[0].tolist().index(2)
    assert total[0] == 5 and b == a + 1 and s[0, a] == s[0, b] and 0 not in idx[0]
    idx, s, total = ix.rank_like([0], 0, 6)                                          # nothing excluded: slot 0 is placed by row 0 and answers with it
    assert total[0] == 5 and idx[0, 0] == 0
    # "track" needs query rows of one group and one slot >= 0
    for rows in ([3], [0, 2], [0, 5], [0, 3]):
        with pytest.raises(CCError, match="-22"):
            ix.rank_like(rows, 0, 6, exclude="track")
        assert ix.rank_like(rows, 0, 6, exclude="rows")[2][0] > 0                    # "rows" takes them
    same(ix.rank_like([0], 0, 6, exclude="track"), like_model(S, slot, group, 3, *none, [0], 0, 6, None, None, True, "track"), "after the errors")
    ix.close()


def small_world(n):
    """n rows in 3 groups: rows 3, 7, 11, ... (64 of them) are slot 0 of group 1, the query track; rows 7 and 11 of it are byte-equal,
    so two query rows score every row alike; row 2 (slot 5, group 2) is a copy of row 3, row 1 is slot 0 in group 2 (the slot goes on
    answering with the track dead); the rest: slots 1 .. 8, every seventh row slot-less."""
    rng = np.random.default_rng(n)
    E = unit(rng.standard_normal((n, DIM)))
    track = 3 + 4 * np.arange(64)
    slot = (1 + np.arange(n) % 8).astype(np.int32)
    slot[::7] = -1
    group = (1 + rng.integers(0, 3, n)).astype(np.int32)
    slot[track], group[track] = 0, 1
    E[11], E[2] = E[7], E[3]
    slot[2], group[2], slot[1], group[1] = 5, 2, 0, 2
    return E, slot, group, track


@pytest.mark.parametrize("n", [260, 261])                                           # four rows per thread / one row per thread
def test_the_fold_of_a_set_is_the_compound_fold_at_its_edges(n):
    """rank_like runs the fold of rank_terms (every row a RANK term, MAX): sets of 1, 3, 4, 5 and 64 rows (the one-row case, both sides
    of the fold's four-term step, the most a call takes), with nothing, the rows and the track excluded, tracks on and off, against
    the model on the device's own scores and against rank_terms of the same rows, bit for bit."""
    from clearcam_amd.objects import EmbeddingIndex
    E, slot, group, track = small_world(n)
    ix = EmbeddingIndex(DIM, n, storage="f32")                                      # the fold does not depend on the storage
    ix.add(E, group, slot)
    none = np.full(n, -(1 << 31), np.int32), np.full(n, -1, np.int32)
    for k in (1, 3, 4, 5, 64):
        rows = track[:k] if k > 1 else track[1:2]                                   # from 3 rows on: rows 7 and 11, the equal pair, are in
        S = ix.scores(ix.fetch(rows))
        assert S.shape == (k, n) and (k < 3 or np.array_equal(bits(S[1]), bits(S[2])))
        for exclude in (None, "rows", "track"):
            for tracks in (True, False):
                what = (n, k, exclude, tracks)
                want = like_model(S, slot, group, 4, *none, rows, 0, n, None, None, tracks, exclude)
                got = ix.rank_like(rows, 0, n, tracks=tracks, exclude=exclude)
                same(got, want, what)
                same(ix.rank_terms(rows=rows, start=0, count=n, tracks=tracks, exclude=exclude), got, what + ("rank_terms",))
                same(ix.rank_like(rows, 5, 40, tracks=tracks, exclude=exclude), like_model(S, slot, group, 4, *none, rows, 5, 40, None, None, tracks, exclude), what + ("page",))
                ans = got[0][0, :int(got[2][0])]
                dead = set() if exclude is None else set(rows.tolist()) if exclude == "rows" else set(track.tolist())
                assert not set(ans.tolist()) & dead
                if not tracks:
                    assert got[2][0] == n - len(dead)
                    if k > 1:
                        assert 2 in ans                                             # the copy of an excluded crop still answers
        if k == 1:
            q = ix.fetch(rows)
            for tracks in (True, False):
                same(ix.rank_like(rows, 0, n, tracks=tracks), ix.rank(q, 0, n, tracks=tracks), (n, "one row is rank of the fetched row", tracks))
    ix.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_the_order_of_the_set_changes_nothing(worlds, storage):
    w = worlds[N_ODD]
    ix = w.index(storage)
    rows = w.query_rows(8)
    rng = np.random.default_rng(6)
    for exclude, tracks, start, count in ((None, True, 0, 300), ("track", True, 1030, 100), ("rows", False, 0, 300)):
        want = ix.rank_like(rows, start, count, tracks=tracks, exclude=exclude)
        for _ in range(3):
            same(ix.rank_like(rng.permutation(rows), start, count, tracks=tracks, exclude=exclude), want, (storage, exclude))
        same(ix.rank_like(np.r_[rows[::-1], rows[:5]], start, count, tracks=tracks, exclude=exclude), want, (storage, exclude, "repeats"))
        assert ix.last_scores_path() == 0


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_index_answering(worlds):
    from clearcam_amd import _lib
    w = worlds[N_ODD]
    ix, n = w.index("f32"), w.n
    L = _lib.lib()
    good = w.query_rows(9)
    idx, s, total = np.empty((1, 10), np.int32), np.empty((1, 10), np.float32), np.zeros(1, np.int64)
    where = ix.row_filter(*FILTERS["both"][:2])
    window = _lib.RowFilter()
    window.use_ts, window.ts_min, window.ts_max = 1, 5, 4

    def call(rows=good, n_rows=None, start=1, cut=-np.inf, flags=1 | _lib.LIKE_EXCLUDE_TRACK, where=where, count=10):
        ids = np.ascontiguousarray(rows, dtype=np.int64)
        return L.cc_index_rank_like(ix._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), len(ids) if n_rows is None else n_rows, start, count, cut, flags, None, 0,
                                    C.byref(where), _lib.ptr(idx), _lib.ptr(s), _lib.ptr(total), 0, None)

    S = ix.scores(ix.fetch(good))
    want = w.model(S, good, 1, 10, "both", None, True, "track")
    slotless = int(np.flatnonzero(w.slot < 0)[0])
    other = int(np.flatnonzero((w.slot == w.qslot) & (w.group != w.qgroup))[0])
    bad = {"no rows": lambda: call(n_rows=0), "65 rows": lambda: call(rows=np.resize(good, 65)), "a row past the end": lambda: call(rows=[3, n]),
           "a negative row": lambda: call(rows=[-1]), "unknown flag": lambda: call(flags=1 | 8), "unknown flag 16": lambda: call(flags=16),
           "track of a slot-less row": lambda: call(rows=[slotless]), "track of two groups": lambda: call(rows=[int(good[0]), other]),
           "NaN cut": lambda: call(cut=float("nan")), "start -1": lambda: call(start=-1), "count 0": lambda: call(count=0), "empty window": lambda: call(where=window)}
    for what, f in bad.items():
        idx[:] = 99; s[:] = 99.0
        assert f() == -22, what
        assert L.cc_last_error() and (idx == 99).all() and (s == 99.0).all(), what
        assert len(ix) == n
        assert call() == 0
        same((idx, s, total), want, what)
    assert call(rows=np.resize(good, 64), flags=1) == 0                             # 64 rows are fine
    with pytest.raises(ValueError):
        ix.rank_like(good, 0, 10, exclude="all")
    with pytest.raises(TypeError):
        ix.rank_like([0.5], 0, 10)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
CAMS, DAYS = ("back", "front"), ("2026-01-01", "2026-01-02")


def finder_spec():
    """(camera, day) -> [(name, vector)]: 4 folders x 60 crops around six directions (cosines inside a cluster about 0.8, so a cut of
    0.21 keeps a cluster), ten track ids shared across folders, every ninth crop a snapshot without '_', three classes, a tenth of
    the crops copies of an earlier one."""
    rng = np.random.default_rng(31)
    centres = unit(rng.standard_normal((6, 768)))
    out = {}
    for cam in CAMS:
        for day in DAYS:
            crops = []
            for i in range(60):
                v = unit(centres[int(rng.integers(0, 6))] + 0.5 * unit(rng.standard_normal(768)))
                if i and rng.random() < 0.1:
                    v = crops[int(rng.integers(0, i))][1]
                name = f"snap{i}.jpg" if i % 9 == 4 else f"{1000 + 7 * i}.5_{int(rng.integers(0, 10))}_{(0, 2, 7)[int(rng.integers(0, 3))]}.jpg"
                crops.append((name, v))
            out[(cam, day)] = list({n: (n, v) for n, v in crops}.values())
    return out


def build_finder(root, folders, storage):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    for (cam, day), crops in folders.items():
        d = os.path.join(root, cam, "objects", day)
        if not os.path.exists(os.path.join(d, "embeddings.idx")):
            EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    f = ObjectFinder(root)
    f.index_storage = storage
    f.attach_store(capacity=64)
    return f


@pytest.mark.parametrize("storage", STORAGES)
def test_object_finder_similar_is_search_page_with_the_stored_embedding(tmp_path, storage):
    root = str(tmp_path / "cameras")
    folders = finder_spec()
    f = build_finder(root, folders, storage)
    rng = np.random.default_rng(8)
    added = {}
    for cam, tid in (("front", 3), ("back", 77)):                                   # crops that arrive later, through add_embedding
        p = os.path.join(root, cam, "objects", DAYS[1], f"5000.5_{tid}_2.jpg")
        added[p] = unit(folders[(cam, DAYS[1])][0][1] + 0.3 * unit(rng.standard_normal(768)))
        f.add_embedding(p, added[p])
    index, table = f._dev["store"]
    assert index.storage == storage and len(table.paths) == len(index) == sum(len(c) for c in folders.values()) + 2
    clicked = list(added) + [table.paths[0], table.paths[100], next(p for p in table.paths if "snap" in p)]
    searches = (dict(), dict(cam_name="front"), dict(timestamp=DAYS[0], min_score=0.21), dict(cam_name="back", timestamp=DAYS[1], start=3, count=7, min_score=0.21),
                dict(ts_range=(1000, 1300), classes=(0, 2), min_score=0.21), dict(classes=(7,), start=2, count=1000), dict(start=4, count=5))
    for path in clicked:
        row = table.row_of(path)
        q = added[path] if (storage == "f32" and path in added) else index.fetch([row])[0]
        if storage == "f32":
            assert np.array_equal(index.fetch([row])[0], q)
        for kw in searches:
            got = f.similar(path, **kw)
            assert got == f.search_page(text_embedding=q, **kw), (storage, path, kw)
            assert got[1] > 0
        assert path not in dict(f.similar(path, exclude="rows", count=1000)[0])
        url = "/" + os.path.relpath(path, root).replace(os.sep, "/")               # the endpoint's form: '/<cam>/objects/<day>/<file>'
        assert url.count("/") == 4 and f.similar(url, count=5) == f.similar(path, count=5)
    with pytest.raises(KeyError):
        f.similar(os.path.join(root, "front", "objects", DAYS[0], "nothing.jpg"))
    with pytest.raises(ValueError):
        f.similar(clicked[0], exclude="everything")
    # the face index goes through the same call: 512-d rows, built from the dict
    faces = [p for p in table.paths if "snap" not in p][:40]
    fe = unit(unit(rng.standard_normal(512)) + 0.5 * unit(rng.standard_normal((40, 512))))       # one face: cosines about 0.8
    f.add_face_embeddings(faces, fe)
    got = f.similar(faces[7], is_face=True, min_score=0.21, count=20)
    findex, ftable = f._dev["face"]
    assert findex.dim == 512 and got == f.search_page(text_embedding=findex.fetch([ftable.row_of(faces[7])])[0], is_face=True, min_score=0.21, count=20)
    assert got[1] > 1 and got[0][0][1] > 0.9


@pytest.mark.parametrize("storage", STORAGES)
def test_a_whole_track_finds_what_one_crop_of_it_misses(tmp_path, storage):
    """Camera A holds a track with two nearly orthogonal views v1 and v2.  Camera B holds a crop close to v2 and a distractor that
    scores higher against v1.  Clicking the v1 crop ranks B's crop below the distractor and below 0.21; the whole track, with the
    track itself excluded, puts B's crop first."""
    def e(*pairs):
        v = np.zeros(768)
        for i, x in pairs:
            v[i] = x
        return unit(v)
    rng = np.random.default_rng(12)
    noise = [unit(np.r_[np.zeros(8), rng.standard_normal(760)]) for _ in range(40)]   # orthogonal to everything planted
    a, b = ("A", DAYS[0]), ("B", DAYS[0])
    folders = {a: [("100.5_5_2.jpg", e((0, 1.0))), ("200.5_5_2.jpg", e((0, 0.05), (1, 1.0)))] + [(f"{300 + i}.5_{6 + i % 3}_2.jpg", noise[i]) for i in range(20)],
               b: [("400.5_9_2.jpg", e((0, 0.04), (1, 0.95), (2, 0.3))), ("500.5_8_2.jpg", e((0, 0.15), (3, 1.0))), ("600.5_5_2.jpg", e((0, 0.1), (4, 1.0)))] +
                  [(f"{700 + i}.5_{6 + i % 3}_2.jpg", noise[20 + i]) for i in range(20)]}
    root = str(tmp_path / "cameras")
    f = build_finder(root, folders, storage)
    name = lambda key, i: os.path.join(root, key[0], "objects", key[1], folders[key][i][0])   # noqa: E731
    v1, v2, close, distractor = name(a, 0), name(a, 1), name(b, 0), name(b, 1)
    one, total = f.similar(v1, count=100)
    paths = [p for p, _ in one]
    assert paths[0] == v1 and paths.index(distractor) < paths.index(close)
    assert dict(one)[close] < 0.21 and dict(one)[distractor] < 0.21
    assert close not in [p for p, _ in f.similar(v1, min_score=0.21)[0]]
    res, total = f.similar(v1, whole_track=True, exclude="track", min_score=0.21)
    assert res[0][0] == close and res[0][1] > 0.9 and v1 not in dict(res) and v2 not in dict(res) and total == len(res)
    everything, total = f.similar(v1, whole_track=True, exclude="track", count=1000)
    assert v1 not in dict(everything) and v2 not in dict(everything) and total == len(everything)
    assert name(b, 2) in dict(everything)                                           # track id 5 goes on answering, from camera B
    assert [p for p, _ in f.similar(v2, whole_track=True, exclude="track", min_score=0.21)[0]] == [p for p, _ in res]   # whichever crop of it was clicked
    kept = f.similar(v1, whole_track=True, min_score=0.21)[0]                       # nothing excluded: the track's best crop leads
    assert kept[0][0] in (v1, v2) and kept[0][1] > 0.99 and kept[1][0] == close
