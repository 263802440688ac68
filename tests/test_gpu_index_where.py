"""Row filters (time window, object class) and the timeline on the GPU: cc_index_add_described / cc_index_row_info /
cc_index_rank_where / cc_index_timeline through EmbeddingIndex and ObjectFinder.

The expected answers are the numpy model of tests/where_cases.py (a row filter as a forbidden group in front of the unchanged
model of tests/rank_cases.py) applied to the index's own score matrix `ix.scores(q)`: idx, score, total and the bin counts must be
EQUAL to it (integer keys and integer sums: no tolerance).  The world is where_cases.Rows: 2 * 4096 + 37 rows of 256."""
import os

import numpy as np
import pytest

from rank_cases import run_bounds
from where_cases import CLASSES, DIM, FILTERS, GROUPS, N, NO_TS, Rows, passing, rank_where_model, timeline_model, unit, where_order

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "bf16", "i8")


class World(Rows):
    def __init__(self):
        super().__init__()
        self._ix, self._sc = {}, {}

    def index(self, storage):
        from clearcam_amd.objects import EmbeddingIndex
        if storage not in self._ix:
            ix = self._ix[storage] = EmbeddingIndex(DIM, N, storage=storage)
            ix.add(self.E, self.group, self.slot, ts=self.ts, classes=self.cls)
        return self._ix[storage]

    def scores(self, storage, Q=3):
        if storage not in self._sc:
            self._sc[storage] = self.index(storage).scores(self.q[:3])
        return self._sc[storage][:Q]

    def model(self, sc, start, count, name, cut=None, tracks=True, rows=None):
        ts_range, classes, allowed = FILTERS[name]
        r = slice(None) if rows is None else rows
        return rank_where_model(sc, self.slot[r], self.group[r], GROUPS, self.ts[r], self.cls[r], start, count, allowed, cut, tracks, ts_range, classes)


@pytest.fixture(scope="module")
def world():
    return World()


def same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int64, what
    assert got[0].shape == want[0].shape == got[1].shape and got[2].shape == want[2].shape, what
    assert np.array_equal(got[2], want[2]), (what, "total", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[1], want[1]), (what, "score")


def tied_cut(s):
    """A score that occurs at least twice among the answers, from the middle of the order: a cut inside a run of equal scores"""
    runs = run_bounds(s)
    assert runs, "no equal scores among the answers"
    return float(s[runs[len(runs) // 2][0]])


def filter_kw(name):
    ts_range, classes, allowed = FILTERS[name]
    return dict(ts_range=ts_range, classes=classes, allowed=allowed)


def test_the_world_reaches_every_edge(world):
    assert N % 4096 and N % 2048 and N % 64 and N > 2 * 4096
    assert (world.ts == NO_TS).mean() > 0.03 and (world.ts == -50).any() and (world.ts == -49).any() and (world.ts == 399).any()
    assert (world.ts == 100).any() and (world.ts == 250).any() and (world.ts < 0).any()
    assert set(np.unique(world.cls).tolist()) == set(CLASSES)
    assert 0.07 < (world.slot == 0).mean() < 0.13 and 0.12 < (world.slot == -1).mean() < 0.18
    ans, _ = where_order(world.scores("f32", 1)[0], world.slot, world.group, GROUPS, world.ts, world.cls, None, True, None, *FILTERS["ts"][:2])
    assert len(ans) > 1130                                             # the window at 1030 lies inside the track order of the "ts" filter


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("tracks", [True, False])
def test_filtered_rank_equals_the_model(world, storage, tracks):
    ix, sc = world.index(storage), world.scores(storage)
    for name in FILTERS:
        kw = filter_kw(name)
        ans, s = where_order(sc[0], world.slot, world.group, GROUPS, world.ts, world.cls, kw["allowed"], tracks, None, kw["ts_range"], kw["classes"])
        assert 40 < len(ans) < N
        for cut in (None, tied_cut(s)):
            total = len(ans) if cut is None else int((s >= np.float32(cut)).sum())
            for start, count in ((0, 50), (1030, 100), (max(total - 5, 0), 20), (total + 3, 10)):
                same(ix.rank(world.q[:3], start, count, min_score=cut, tracks=tracks, **kw), world.model(sc, start, count, name, cut, tracks),
                     (storage, name, tracks, cut, start))
            same(ix.rank(world.q[:1], 0, 50, min_score=cut, tracks=tracks, **kw), world.model(sc[:1], 0, 50, name, cut, tracks), (storage, name, "Q = 1"))
            if cut is not None:                                        # the cut keeps the whole run of equal scores
                got = ix.rank(world.q[:1], total - 2, 4, min_score=cut, tracks=tracks, **kw)
                assert got[2][0] == total and got[1][0, 0] == got[1][0, 1] == np.float32(cut) and got[0][0, 2] == -1


@pytest.mark.parametrize("storage", STORAGES)
def test_filtered_rank_equals_an_index_of_the_passing_rows(world, storage):
    from clearcam_amd.objects import EmbeddingIndex
    ix = world.index(storage)
    for name in ("ts", "both+allowed"):
        kw = filter_kw(name)
        rows = np.flatnonzero(passing(world.ts, world.cls, kw["ts_range"], kw["classes"]))
        small = EmbeddingIndex(DIM, len(rows), storage=storage)
        small.add(world.E[rows], world.group[rows], world.slot[rows])
        for tracks, start, count in ((True, 0, 100), (True, 1030, 100), (False, 0, 1500), (False, 1020, 40)):
            idx, s, total = small.rank(world.q[:3], start, count, kw["allowed"], None, tracks)
            back = np.where(idx >= 0, rows[np.maximum(idx, 0)], -1).astype(np.int32)
            same(ix.rank(world.q[:3], start, count, tracks=tracks, **kw), (back, s, total), (storage, name, tracks, start))
        small.close()


def test_no_filter_is_rank(world):
    import ctypes as C
    import torch
    from clearcam_amd import _lib
    ix = world.index("f32")
    al = FILTERS["both+allowed"][2]
    L = _lib.lib()
    q = np.ascontiguousarray(world.q[:3])
    for allowed, tracks, start, count, cut in ((None, True, 0, 100, None), (al, True, 1000, 300, 0.02), (al, False, 4090, 1100, None)):
        want = ix.rank(q, start, count, allowed, cut, tracks)
        idx, s, total = np.empty((3, count), np.int32), np.empty((3, count), np.float32), np.zeros(3, np.int64)
        assert L.cc_index_rank_where(ix._h, _lib.ptr(q), 3, start, count, float(ix.cut_f32(cut)), int(tracks), _lib.ptr(allowed), 0 if allowed is None else len(allowed),
                                     None, _lib.ptr(idx), _lib.ptr(s), _lib.ptr(total), 0, None) == 0
        same((idx, s, total), want, "where = NULL")
        empty = _lib.RowFilter()                                       # use_ts = use_cls = 0: a filter that filters nothing
        assert L.cc_index_rank_where(ix._h, _lib.ptr(q), 3, start, count, float(ix.cut_f32(cut)), int(tracks), _lib.ptr(allowed), 0 if allowed is None else len(allowed),
                                     C.byref(empty), _lib.ptr(idx), _lib.ptr(s), _lib.ptr(total), 0, None) == 0
        same((idx, s, total), want, "an empty filter")
        di, ds, dt = ix.rank_device(q, start, count, allowed, cut, tracks)
        torch.cuda.synchronize()
        same((di.cpu().numpy(), ds.cpu().numpy(), dt), want, "rank_device")
    kw = filter_kw("both+allowed")
    want = ix.rank(q, 20, 200, min_score=0.01, **kw)
    di, ds, dt = ix.rank_device(q, 20, 200, min_score=0.01, **kw)
    torch.cuda.synchronize()
    assert di.is_cuda and ds.is_cuda
    same((di.cpu().numpy(), ds.cpu().numpy(), dt), want, "rank_device with a filter")


def removal_mask():
    mask = np.random.default_rng(9).random(N) < 0.3                    # thins every granule ...
    mask[:320] = False                                                 # ... but the first five, which stay where they are,
    mask[640:1280] = True                                              # ten that go entirely,
    mask[4096 - 70:4096 + 70] = True                                   # and a hole across the 4096-row block boundary
    return mask


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("slab_rows", [-1, 256])
def test_attributes_follow_their_rows_through_removal(world, storage, slab_rows):
    from clearcam_amd import _lib
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(DIM, N, storage=storage)
    ix.add(world.E, world.group, world.slot, ts=world.ts, classes=world.cls)
    mask = removal_mask()
    keep = np.flatnonzero(~mask)
    _lib.check(_lib.lib().cc_dev_set(b"index_slab_rows", slab_rows))   # 256: bounced slabs at this size
    try:
        assert ix.remove(mask) == int(mask.sum()) and len(ix) == len(keep)
    finally:
        _lib.check(_lib.lib().cc_dev_set(b"index_slab_rows", -1))
    ts, cls = ix.row_info()
    assert np.array_equal(ts, world.ts[keep]) and np.array_equal(cls, world.cls[keep])
    sc = ix.scores(world.q[:3])
    assert np.array_equal(sc, world.scores(storage)[:, keep])         # and the rows are the survivors
    for name in ("ts", "both", "both+allowed"):
        for tracks, start, count in ((True, 0, 60), (True, 900, 300), (False, 1000, 1100)):
            same(ix.rank(world.q[:3], start, count, tracks=tracks, **filter_kw(name)), world.model(sc, start, count, name, None, tracks, keep), (storage, name, tracks, start))
    ix.close()


@pytest.mark.parametrize("storage", STORAGES)
def test_attributes_follow_their_rows_through_growth(world, storage):
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(DIM, 1024, storage=storage)
    for a, b in ((0, 1000), (1000, 4100), (4100, N)):                   # the second and the third call outgrow the matrix
        ix.add(world.E[a:b], world.group[a:b], world.slot[a:b], ts=world.ts[a:b], classes=world.cls[a:b])
    assert len(ix) == N and ix.capacity >= N
    ts, cls = ix.row_info()
    assert np.array_equal(ts, world.ts) and np.array_equal(cls, world.cls)
    sc = ix.scores(world.q[:3])
    assert np.array_equal(sc, world.scores(storage))
    for name in ("ts", "both+allowed"):
        for tracks, start, count in ((True, 0, 60), (False, 1000, 1100)):
            same(ix.rank(world.q[:3], start, count, tracks=tracks, **filter_kw(name)), world.model(sc, start, count, name, None, tracks), (storage, name, tracks))
    ix.close()


def test_rows_of_the_older_add_calls_pass_no_filter(world):
    from clearcam_amd import _lib
    from clearcam_amd.objects import EmbeddingIndex
    from rank_cases import rank_model
    L = _lib.lib()
    ix = EmbeddingIndex(DIM, 64)
    n = 300
    E, g, t = np.ascontiguousarray(world.E[:n]), np.ascontiguousarray(world.group[:n]), np.ascontiguousarray(world.slot[:n])
    _lib.check(L.cc_index_add_tracked(ix._h, _lib.ptr(E[:100]), 100, 0, _lib.ptr(g[:100]), _lib.ptr(t[:100])))
    _lib.check(L.cc_index_add_grouped(ix._h, _lib.ptr(E[100:200]), 100, 0, _lib.ptr(g[100:200])))
    _lib.check(L.cc_index_add(ix._h, _lib.ptr(E[200:]), 100, 0))
    ix.add(E[:7], g[:7], t[:7])                                         # and `add` without ts / classes
    ts, cls = ix.row_info()
    assert len(ts) == n + 7 and (ts == NO_TS).all() and (cls == -1).all()
    slot = np.r_[t[:100], np.full(200, -1, np.int32), t[:7]]
    group = np.r_[g[:200], np.zeros(100, np.int32), g[:7]]
    sc = ix.scores(world.q[:2])
    for tracks in (True, False):
        same(ix.rank(world.q[:2], 0, 400, tracks=tracks), rank_model(sc, slot, group, 0, 400, None, None, tracks), "no filter")
        for kw in (dict(ts_range=(None, None)), dict(classes=range(256)), dict(ts_range=(-50, 400), classes=(0, 2))):
            idx, s, total = ix.rank(world.q[:2], 0, 10, tracks=tracks, **kw)
            assert (idx == -1).all() and np.isneginf(s).all() and (total == 0).all(), kw
            counts, total = ix.timeline(world.q[:2], -50, 10, 50, tracks=tracks, **kw)
            assert not counts.any() and (total == 0).all()
        counts, total = ix.timeline(world.q[:2], -50, 10, 50, tracks=tracks)
        assert not counts.any() and np.array_equal(total, ix.rank(world.q[:2], 0, 1, tracks=tracks)[2])   # answers without ts: in total only
    ix.close()


# (t0, bin_seconds, n_bins): every answer with a ts in ONE bin; a day of hours in small; one bin per second, most of them empty;
# bins that leave answers out on both sides, with a negative t0 inside the data
BINS = ((-50, 450, 1), (-50, 19, 24), (-2000, 1, 4096), (-7, 5, 24))


@pytest.mark.parametrize("storage", STORAGES)
def test_timeline_equals_the_model(world, storage):
    ix, sc = world.index(storage), world.scores(storage)
    for name in (None, "ts", "both+allowed"):
        ts_range, classes, allowed = FILTERS[name] if name else (None, None, None)
        for tracks in (True, False):
            ans, s = where_order(sc[0], world.slot, world.group, GROUPS, world.ts, world.cls, allowed, tracks, None, ts_range, classes)
            for cut in (None, tied_cut(s)):
                rank_total = ix.rank(world.q[:3], 0, 1, allowed, cut, tracks, ts_range, classes)[2]
                for t0, bin_seconds, n_bins in BINS:
                    counts, total = ix.timeline(world.q[:3], t0, bin_seconds, n_bins, allowed, cut, tracks, ts_range, classes)
                    want = timeline_model(sc, world.slot, world.group, GROUPS, world.ts, world.cls, t0, bin_seconds, n_bins, allowed, cut, tracks, ts_range, classes)
                    what = (storage, name, tracks, cut, n_bins)
                    assert counts.dtype == np.int64 and counts.shape == (3, n_bins) and total.dtype == np.int64, what
                    assert np.array_equal(total, want[1]) and np.array_equal(total, rank_total), what
                    assert np.array_equal(counts, want[0]), what
                    assert (counts.sum(axis=1) <= total).all()
                    if n_bins == 1 and name is None:                   # contention: one bin takes every answer that has a ts
                        assert (counts[:, 0] < total).all() and (counts[:, 0] > 0.9 * total).all(), what
                    if n_bins == 1 and name is not None:               # ... and behind a time window every answer has one
                        assert np.array_equal(counts[:, 0], total), what
    one = ix.timeline(world.q[:1], -50, 19, 24, ts_range=(100, 250), classes=(2, 64, 255))
    assert np.array_equal(one[0][0], ix.timeline(world.q[:3], -50, 19, 24, ts_range=(100, 250), classes=(2, 64, 255))[0][0])


def test_timeline_time_of_a_track_is_its_best_passing_crop():
    """Two crops of one track: the first one in the window scores lower than the second.  The track's answer is counted at the
    second crop's ts, not at its first passing row's; a better crop outside the window does not count at all."""
    from clearcam_amd.objects import EmbeddingIndex
    q = np.zeros((1, DIM), np.float32); q[0, 0] = 1.0
    E = np.zeros((4, DIM), np.float32)
    E[:, 0] = (0.9, 0.2, 0.5, 0.1)
    ix = EmbeddingIndex(DIM, 8)
    ix.add(E, None, np.array([0, 0, 0, -1], np.int32), ts=np.array([500, 10, 30, NO_TS], np.int32), classes=np.array([1, 1, 1, 1], np.int32))
    counts, total = ix.timeline(q, 0, 10, 5, ts_range=(0, 100))
    assert total[0] == 1 and counts[0].tolist() == [0, 0, 0, 1, 0]
    counts, total = ix.timeline(q, 0, 10, 5)
    assert total[0] == 2 and counts[0].tolist() == [0, 0, 0, 0, 0]      # the track at ts 500 is past the bins, the slot-less row has no ts
    counts, total = ix.timeline(q, 0, 10, 5, tracks=False)
    assert total[0] == 4 and counts[0].tolist() == [0, 1, 0, 1, 0]
    ix.close()


def test_timeline_bin_arithmetic():
    from clearcam_amd.objects import EmbeddingIndex
    rng = np.random.default_rng(3)
    ts = np.array([2**31 - 1, -2**31 + 1, 0, 59, 60, -1, -60, -61, 119, 120, NO_TS, 2**31 - 1, -2**31 + 2**20, -2**31 + 2**20 + 1], np.int64)
    n = len(ts)
    ix = EmbeddingIndex(DIM, n)
    ix.add(unit(rng.standard_normal((n, DIM))), ts=ts, classes=np.zeros(n, np.int32))
    assert np.array_equal(ix.row_info()[0], ts.astype(np.int32))
    q = unit(rng.standard_normal((1, DIM)))

    def want(t0, bs, nb):
        b = (ts[ts != NO_TS] - t0) // bs
        return np.bincount(b[(b >= 0) & (b < nb)], minlength=nb)

    # a difference of 2^32 - 2: the last of 4096 bins of 2^20 s; in 32 bits it would wrap to -2
    counts, total = ix.timeline(q, -2**31 + 1, 2**20, 4096, tracks=False)
    assert total[0] == n and counts[0, 4095] == 2 and counts[0, 0] == 2 and counts[0, 1] == 1 and np.array_equal(counts[0], want(-2**31 + 1, 2**20, 4096))
    # t0 negative, ts exactly on the edges of the bins: -60 opens bin 0, -1 closes it, 0 opens bin 1, 60 bin 2, 120 is past three bins, -61 before them
    counts, total = ix.timeline(q, -60, 60, 3, tracks=False)
    assert counts[0].tolist() == [2, 2, 2] == want(-60, 60, 3).tolist() and total[0] == n
    for t0, bs, nb in ((2**31 - 1, 1, 1), (-2**31, 2**31 - 1, 3), (0, 2**31 - 1, 2), (-61, 1, 200)):
        counts, total = ix.timeline(q, t0, bs, nb, tracks=False)
        assert np.array_equal(counts[0], want(t0, bs, nb)) and total[0] == n, (t0, bs, nb)
    ix.close()


def test_timeline_of_a_batch_on_the_mfma_path(world):
    ix = world.index("i8")
    q = world.q[:18]
    kw = dict(ts_range=(100, 250), classes=(2, 64, 255))
    counts, total = ix.timeline(q, -50, 19, 24, **kw)
    assert ix.last_scores_path() == 2
    sc = ix.scores(q)
    assert ix.last_scores_path() == 2
    want = timeline_model(sc, world.slot, world.group, GROUPS, world.ts, world.cls, -50, 19, 24, None, None, True, **kw)
    assert np.array_equal(counts, want[0]) and np.array_equal(total, want[1])
    same(ix.rank(q, 5, 40, **kw), rank_where_model(sc, world.slot, world.group, GROUPS, world.ts, world.cls, 5, 40, **kw), "rank of 18 queries")


def test_errors_leave_the_index_answering(world):
    import ctypes as C
    from clearcam_amd import _lib
    ix, sc = world.index("f32"), world.scores("f32", 1)
    L = _lib.lib()
    q = np.ascontiguousarray(world.q[:1])
    idx, s, total = np.empty((1, 10), np.int32), np.empty((1, 10), np.float32), np.zeros(1, np.int64)
    counts = np.zeros((1, 24), np.uint32)
    good = ix.row_filter(*FILTERS["both"][:2])

    def rank(where=good, start=1, cut=-np.inf, flags=1):
        return L.cc_index_rank_where(ix._h, _lib.ptr(q), 1, start, 10, cut, flags, None, 0, C.byref(where), _lib.ptr(idx), _lib.ptr(s), _lib.ptr(total), 0, None)

    def timeline(where=good, bin_seconds=19, n_bins=24, cut=-np.inf, flags=1):
        return L.cc_index_timeline(ix._h, _lib.ptr(q), 1, cut, flags, None, 0, C.byref(where), -50, bin_seconds, n_bins, _lib.ptr(counts), _lib.ptr(total), 0, None)

    window, no_class = _lib.RowFilter(), _lib.RowFilter()
    window.use_ts, window.ts_min, window.ts_max = 1, 5, 4
    no_class.use_cls = 1
    too_big = np.array([3, 256], np.int32)
    bad = {"empty window": lambda: rank(window), "empty class set": lambda: rank(no_class), "NaN cut": lambda: rank(cut=float("nan")),
           "start -1": lambda: rank(start=-1), "unknown flag": lambda: rank(flags=2),
           "timeline: empty window": lambda: timeline(window), "timeline: empty class set": lambda: timeline(no_class),
           "timeline: bin_seconds 0": lambda: timeline(bin_seconds=0), "timeline: bin_seconds -5": lambda: timeline(bin_seconds=-5),
           "timeline: n_bins 0": lambda: timeline(n_bins=0), "timeline: n_bins 4097": lambda: timeline(n_bins=4097),
           "timeline: NaN cut": lambda: timeline(cut=float("nan")), "timeline: unknown flag": lambda: timeline(flags=4),
           "class 256": lambda: L.cc_index_add_described(ix._h, _lib.ptr(world.E[:2]), 2, 0, None, None, None, _lib.ptr(too_big)),
           "class -2": lambda: L.cc_index_add_described(ix._h, _lib.ptr(world.E[:2]), 2, 0, None, None, None, _lib.ptr(np.array([-2, 0], np.int32))),
           "row_info past the end": lambda: L.cc_index_row_info(ix._h, N - 1, 2, _lib.ptr(idx), None),
           "row_info before the start": lambda: L.cc_index_row_info(ix._h, -1, 1, _lib.ptr(idx), None)}
    want = world.model(sc, 1, 10, "both")
    want_t = timeline_model(sc, world.slot, world.group, GROUPS, world.ts, world.cls, -50, 19, 24, None, None, True, *FILTERS["both"][:2])
    for what, call in bad.items():
        assert call() == -22, what
        assert L.cc_last_error()
        assert len(ix) == N, what
        assert rank() == 0
        same((idx, s, total), want, what)
        assert timeline() == 0 and np.array_equal(counts.astype(np.int64), want_t[0]) and total[0] == want_t[1][0], what
    with pytest.raises(ValueError):
        ix.rank(q, 0, 10, ts_range=(5, 4))
    with pytest.raises(ValueError):
        ix.timeline(q, 0, 10, 5, classes=[])
    with pytest.raises(_lib.CCError):
        ix.timeline(q, 0, 0, 5)
    with pytest.raises(ValueError):
        ix.add(world.E[:2], classes=[0, 256])
    assert np.array_equal(ix.row_info()[1], world.cls)


# ---- ObjectFinder on a small attached store: two cameras, two days -------------------------------------------------------------
CAMS, DAYS, PER = ("back", "front"), ("2026-01-01", "2026-01-02"), 120


def store_spec(bad_name=False):
    """(camera, day) -> [(name, vector)]: scores are the first component alone (the query is e0), a fifth of them copied (ties);
    ts in [0, 86400), forty track ids shared across folders, every ninth crop a snapshot without '_', classes from CLASSES."""
    rng = np.random.default_rng(23)
    out = {}
    for cam in CAMS:
        for day in DAYS:
            crops, vals = [], rng.random(PER).astype(np.float32)
            for i in range(PER):
                if i and rng.random() < 0.2:
                    vals[i] = vals[rng.integers(0, i)]
                v = np.zeros(768, np.float32); v[0] = vals[i]; v[1 + i] = rng.random()
                c = CLASSES[int(rng.integers(0, 6))]
                name = f"snap{i}.jpg" if i % 9 == 4 else f"{int(rng.integers(0, 86400))}.5_{int(rng.integers(0, 40))}_{c}.jpg"
                crops.append((name, v))
            out[(cam, day)] = list({n: (n, v) for n, v in crops}.values())       # a name only once per folder
    if bad_name:
        out[("front", DAYS[1])].append(("50000.5_x_2.jpg", np.eye(1, 768, 0, dtype=np.float32)[0] * 0.99))
    return out


def attach(root, folders):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    for (cam, day), crops in folders.items():
        d = os.path.join(root, cam, "objects", day)
        EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    f = ObjectFinder(root)
    f.attach_store(capacity=64)
    return f


def host_answer(f, q, cam, day, ts_range, classes, grouped):
    """`ObjectFinder._rank` on the host over the passing rows' scores: the whole filtered order"""
    index, table = f._dev["store"]
    allowed = table.allowed(cam, day)
    ok = passing(table.ts, table.cls, ts_range, classes)
    rows = [r for r in range(len(table.paths)) if allowed[table.group[r]] and ok[r]]
    scores = index.scores(q)[0]
    return f._rank(table, rows, [float(scores[r]) for r in rows], grouped)


SEARCHES = ((None, None, (20000, 70000), None), ("front", None, None, (0, 2, 255)), (None, DAYS[1], (3600 * 8, 3600 * 16), (2, 7, 63, 64)),
            ("back", DAYS[0], (0, 86399), (0, 2, 7, 63, 64, 255)))


@pytest.mark.parametrize("bad_name", [False, True])
def test_object_finder_pages_search_and_timeline_with_row_filters(tmp_path, monkeypatch, bad_name):
    from clearcam_amd.objects import EmbeddingIndex
    f = attach(str(tmp_path / "cameras"), store_spec(bad_name))
    q = np.zeros(768, np.float32); q[0] = 1.0
    index, table = f._dev["store"]
    ts, cls = index.row_info()
    assert np.array_equal(ts, np.asarray(table.ts, np.int32)) and np.array_equal(cls, np.asarray(table.cls, np.int32)) and (ts == NO_TS).any()
    calls = {"rank": 0, "timeline": 0, "scores": 0}
    for name in calls:
        def counted(ix, *a, _fn=getattr(EmbeddingIndex, name), _name=name, **kw):
            calls[_name] += 1
            return _fn(ix, *a, **kw)
        monkeypatch.setattr(EmbeddingIndex, name, counted)
    for cam, day, ts_range, classes in SEARCHES:
        fallback = bad_name and cam != "back" and day != DAYS[0]       # the unparsable name sits in front / the second day
        before = dict(calls)
        full = host_answer(f, q, cam, day, ts_range, classes, grouped=True)
        calls.update(before)
        cut = full[len(full) // 2][1]                                  # the median answer's score: about half of them stay
        kept = [r for r in full if not r[1] < cut]
        assert len(full) > 12 and 3 < len(kept) < len(full)
        for start, count in ((0, 5), (3, 1000), (len(kept), 4)):
            assert f.search_page(start=start, count=count, cam_name=cam, timestamp=day, text_embedding=q, min_score=cut, ts_range=ts_range, classes=classes) == \
                (kept[start:start + count], len(kept)), (cam, day, start)
        assert f.search_page(start=0, count=10**6, cam_name=cam, timestamp=day, text_embedding=q, ts_range=ts_range, classes=classes) == (full, len(full))
        for k in (7, 2000):
            assert f.search(top_k=k, cam_name=cam, timestamp=day, text_embedding=q, ts_range=ts_range, classes=classes) == full[:k]
        counts, total = f.timeline(text_embedding=q, cam_name=cam, timestamp=day, min_score=cut, ts_range=ts_range, classes=classes)
        assert total == len(kept) and counts.shape == (24,) and counts.sum() == total            # every ts lies inside the day
        by_hour = np.bincount([table.name_attrs(p)[0] // 3600 for p, _ in kept], minlength=24)
        assert np.array_equal(counts, by_hour)
        counts, total = f.timeline(text_embedding=q, t0=3600 * 6, bin_seconds=1800, n_bins=10, cam_name=cam, timestamp=day, min_score=None, ts_range=ts_range, classes=classes)
        half_hours = np.array([(table.name_attrs(p)[0] - 3600 * 6) // 1800 for p, _ in full])
        assert total == len(full) and np.array_equal(counts, np.bincount(half_hours[(half_hours >= 0) & (half_hours < 10)], minlength=10))
        assert 0 < counts.sum() < total
        if fallback:
            assert calls["rank"] == before["rank"] and calls["timeline"] == before["timeline"] and calls["scores"] > before["scores"], (cam, day)
        else:
            assert calls["rank"] == before["rank"] + 6 and calls["timeline"] == before["timeline"] + 2 and calls["scores"] == before["scores"], (cam, day)
    # without a row filter nothing changed: the unparsable name still raises like the reference
    if bad_name:
        with pytest.raises(ValueError):
            f.search(top_k=5, text_embedding=q)
    else:
        assert f.search(top_k=5, text_embedding=q) == host_answer(f, q, None, None, None, None, True)[:5]
