"""Compound search on the GPU: cc_index_rank_terms / cc_index_timeline_terms through EmbeddingIndex.rank_terms / rank_terms_device /
timeline_terms and ObjectFinder.compound / compound_timeline.

The expected answers are the numpy model of tests/terms_cases.py (the fold by roles in float32 arithmetic, dead rows as a forbidden
group, then the unchanged model of tests/rank_cases.py) applied to the index's own `ix.scores(np.vstack([q, ix.fetch(rows)]))`.
Every comparison is exact: integer keys and f32 bits, no tolerance.  The worlds are like_cases.World: 8229 rows of 256 (odd: the
scalar fold, unaligned score rows, no GEMM route) and 8224 (the vector fold; the f32 / bf16 GEMM from 17 terms, the int8 MFMA kernel
from 18)."""
import ctypes as C
import os

import numpy as np
import pytest

from like_cases import expected_path, fold
from rank_cases import run_bounds
from terms_cases import (COMBINES, DIM, GROUPS, N_EVEN, N_ODD, PATTERNS, TERM_COUNTS, World, feasible, fold_terms, median_cuts, ordered, passing, plan, terms_fold,
                         terms_model, terms_order, terms_timeline_model)
from where_cases import FILTERS, SLOTS, unit

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

    def competing(self, name):
        ts_range, classes, allowed = FILTERS[name] if name else NO_FILTER
        ok = passing(self.ts, self.cls, ts_range, classes)
        if allowed is not None:
            ok &= allowed[self.group] != 0
        return np.flatnonzero(ok)

    def cols(self):
        return self.slot, self.group, GROUPS, self.ts, self.cls


@pytest.fixture(scope="module")
def worlds():
    return {N_ODD: GpuWorld(N_ODD), N_EVEN: GpuWorld(N_EVEN)}


def filter_kw(name):
    ts_range, classes, allowed = FILTERS[name] if name else NO_FILTER
    return dict(ts_range=ts_range, classes=classes, allowed=allowed)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int64, what
    assert got[0].shape == want[0].shape == got[1].shape and got[2].shape == want[2].shape, what
    assert np.array_equal(got[2], want[2]), (what, "total", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "score")
    if len(want) > 3:
        assert got[3].dtype == np.int32 and got[3].shape == want[3].shape and np.array_equal(got[3], want[3]), (what, "which")


def term_scores(ix, q, rows):
    """The device's own (T, n) score matrix of the terms, the vectors first"""
    parts = ([] if q is None else [q]) + ([ix.fetch(rows)] if len(rows) else [])
    return ix.scores(np.vstack(parts))


def tied_cut(s):
    runs = run_bounds(s)
    assert runs, "no equal scores among the answers"
    return float(s[runs[len(runs) // 2][0]])


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("tracks", [True, False])
def test_one_vector_rank_term_is_rank(worlds, storage, tracks):
    for n, w in worlds.items():
        ix = w.index(storage)
        q = w.q[3:4]
        for name in (None, "ts", "both+allowed"):
            kw = filter_kw(name)
            _, s, total = ix.rank(q, 0, w.n, tracks=tracks, **kw)
            s = s[0, :int(total[0])]
            assert len(s) > 40
            for cut in (None, tied_cut(s)):
                left = len(s) if cut is None else int((s >= np.float32(cut)).sum())
                for start, count in ((0, 50), (1030, 100)):
                    want = ix.rank(q, start, count, min_score=cut, tracks=tracks, **kw)
                    for combine in ("max", "min", "sum"):                              # one term with weight 1: every rule is the identity
                        got = ix.rank_terms(q=q, combine=combine, start=start, count=count, min_score=cut, tracks=tracks, **kw)
                        assert ix.last_scores_path() == 0
                        same(got, want, (storage, n, name, tracks, cut, start, combine))
                    assert got[2][0] == left
        got = ix.rank_terms(q=q, start=0, count=50, tracks=tracks, which=True)
        assert len(got) == 4 and (got[3][got[0] >= 0] == 0).all() and (got[3][got[0] < 0] == -1).all()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_stored_rank_rows_with_max_are_rank_like(worlds, storage):
    for n, w in worlds.items():
        ix = w.index(storage)
        for k in (1, 9, 18):
            rows = w.query_rows(k)
            S = ix.scores(ix.fetch(rows))
            v = fold(S)
            for exclude in (None, "rows", "track"):
                for tracks, start, count in ((True, 0, 50), (False, 1030, 100), (True, 0, n)):
                    got = ix.rank_terms(rows=rows, start=start, count=count, tracks=tracks, exclude=exclude, which=True)
                    assert ix.last_scores_path() == expected_path(storage, DIM, n, k)
                    same(got[:3], ix.rank_like(rows, start, count, tracks=tracks, exclude=exclude), (storage, n, k, exclude, tracks, start))
                    idx, wh = got[0][0], got[3][0]
                    real = idx >= 0
                    assert real.any() and (wh[~real] == -1).all()
                    at = ordered(S[:, idx[real]]) == ordered(v[idx[real]])[None, :]     # the terms that attain the maximum, per answer
                    assert np.array_equal(wh[real], at.argmax(axis=0)) and at[wh[real], np.arange(real.sum())].all()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
CONFIGS = ((True, None, False), (False, None, True), (True, "cls", False), (False, "ts", True))   # tracks, a FILTERS entry, min_score on a tie
EXCLUDES = (None, "rows", "track")


def run_case(w, ix, storage, T, pattern, combine, seed, tracks, name, tie, exclude):
    """One case of terms_cases.plan on the device and in the model -> the route its scores took"""
    import torch
    q, rows, roles, weights = plan(w, T, pattern, combine, seed)
    n_vec = 0 if q is None else len(q)
    if not any(r == "rank" for r in roles[n_vec:]):
        exclude = None                                                              # an exclude mode needs a stored row that ranks
    S = term_scores(ix, q, rows)
    path = ix.last_scores_path()
    assert path == expected_path(storage, DIM, w.n, T) and S.shape == (T, w.n)
    competing = w.competing(name)
    cuts = median_cuts(S, roles, competing)
    v, dead, which = terms_fold(S, roles, weights, cuts, combine, rows, n_vec, w.group, w.slot, exclude)
    what = (storage, w.n, T, pattern, combine, tracks, name, exclude)
    if pattern != "rank":
        killed = fold_terms(S, roles, weights, cuts, combine)[1][competing]
        assert killed.any() and not killed.all(), what                             # the terms kill some competing rows and spare some
    kw = filter_kw(name)
    ans, s = terms_order(v, dead, *w.cols(), kw["allowed"], tracks, None, kw["ts_range"], kw["classes"])
    assert len(ans) >= 40, what
    cut = tied_cut(s) if tie else None
    left = len(s) if cut is None else int((s >= np.float32(cut)).sum())
    ask = dict(q=q, rows=rows, roles=roles, weights=weights, cuts=cuts, combine=combine, min_score=cut, tracks=tracks, exclude=exclude, which=True, **kw)
    for start, count in ((0, 50), (1030, 100), (max(left - 5, 0), 20)):
        want = terms_model(v, dead, which, *w.cols(), start, count, kw["allowed"], cut, tracks, kw["ts_range"], kw["classes"])
        assert want[2][0] == left
        got = ix.rank_terms(start=start, count=count, **ask)
        assert ix.last_scores_path() == path, what
        same(got, want, what + (start,))
        if start == 0:
            di, ds, dt, dw = ix.rank_terms_device(start=start, count=count, **ask)
            torch.cuda.synchronize()
            assert di.is_cuda and ds.is_cuda and dw.is_cuda
            same((di.cpu().numpy(), ds.cpu().numpy(), dt, dw.cpu().numpy()), want, what + ("device",))
    return path


@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_equals_the_model(worlds, storage):
    taken, k = set(), 0
    for n, w in worlds.items():
        ix = w.index(storage)
        for T in TERM_COUNTS:
            for pattern in PATTERNS:
                if not feasible(T, pattern):
                    continue
                for combine in sorted(COMBINES):
                    tracks, name, tie = CONFIGS[k % len(CONFIGS)]
                    taken.add(run_case(w, ix, storage, T, pattern, combine, k % 2, tracks, name, tie, EXCLUDES[(k // 2) % 3]))
                    k += 1
    assert taken == {"f32": {0, 1}, "bf16": {0, 1}, "i8": {0, 2}}[storage]


def test_device_results_without_a_total(worlds):
    import torch
    w = worlds[N_EVEN]
    ix = w.index("f32")
    q, rows, roles, weights = plan(w, 17, "both", "sum", 0)
    S = term_scores(ix, q, rows)
    cuts = median_cuts(S, roles, np.arange(w.n))
    v, dead, which = terms_fold(S, roles, weights, cuts, "sum", rows, len(q), w.group, w.slot, "track")
    want = terms_model(v, dead, which, *w.cols(), 20, 200)
    ask = dict(q=torch.as_tensor(q).cuda(), rows=rows, roles=roles, weights=weights, cuts=cuts, combine="sum", exclude="track", start=20, count=200)
    di, ds, dt = ix.rank_terms_device(with_total=False, **ask)                     # vectors that are on the device already, nothing waited for
    torch.cuda.synchronize()
    assert dt is None and np.array_equal(di.cpu().numpy(), want[0]) and np.array_equal(bits(ds.cpu().numpy()), bits(want[1]))
    same(ix.rank_terms(which=True, **ask), want, "device vectors, host results")
    big = ix.rank_terms(which=True, **dict(ask, start=0, count=140000))             # past the pinned block: the results come down by copies
    want = terms_model(v, dead, which, *w.cols(), 0, 140000)
    same(big, want, "a large host result")


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_dead_rows_shape_tracks(worlds, storage):
    for n, w in worlds.items():
        ix = w.index(storage)
        q = w.q[5:6]
        # a REJECT term made of the first row of slot 0's track, cut at its self-score: that row and its byte-equal copies die
        r0 = int(w.track[0])
        assert r0 == np.flatnonzero(w.slot == w.qslot)[0]
        S = term_scores(ix, q, [r0])
        roles, cuts = ["rank", "reject"], [None, float(S[1, r0])]
        v, dead, which = fold_terms(S, roles, None, cuts, "max")
        same_bytes = (w.E.view(np.uint32) == w.E.view(np.uint32)[r0]).all(axis=1)
        assert dead[r0] and np.array_equal(dead, same_bytes) and 1 <= dead.sum() < 20
        for tracks in (True, False):
            got = ix.rank_terms(q=q, rows=[r0], roles=roles, cuts=cuts, start=0, count=n, tracks=tracks, which=True)
            same(got, terms_model(v, dead, which, *w.cols(), 0, n, tracks=tracks), (storage, n, "reject the first row", tracks))
        ans = got[0][0, :int(got[2][0])]                                               # without tracks: every surviving row answers
        assert not set(ans.tolist()) & set(np.flatnonzero(dead).tolist()) and len(ans) == n - dead.sum()
        got = ix.rank_terms(q=q, rows=[r0], roles=roles, cuts=cuts, start=0, count=n, which=True)
        ans = got[0][0, :int(got[2][0])]
        mine = ans[w.slot[ans] == w.qslot]
        survivors = np.flatnonzero((w.slot == w.qslot) & ~dead)
        assert len(mine) == 1 and mine[0] != r0 and not dead[mine[0]]                  # the track answers with its best SURVIVING crop ...
        assert v[mine[0]] == v[survivors].max()
        tied = ans[bits(v[ans]) == bits(v[mine[0]])]                                    # ... and among equal scores stands where its first surviving row puts it
        first_of = {int(a): (int(np.flatnonzero((w.slot == w.slot[a]) & ~dead)[0]) if w.slot[a] >= 0 else n + int(a)) for a in tied}
        assert [first_of[int(a)] for a in tied] == sorted(first_of.values())
        # a byte-equal copy outside the track is rejected with the crop, while an EXCLUDED crop's copy competes
        r, c = next((r, c) for r, c in w.copies_outside() if w.slot[c] != w.qslot)
        S = term_scores(ix, q, [r])
        roles, cuts = ["rank", "reject"], [None, float(S[1, r])]
        assert bits(S[1, c]) == bits(S[1, r])
        v, dead, which = fold_terms(S, roles, None, cuts, "max")
        got = ix.rank_terms(q=q, rows=[r], roles=roles, cuts=cuts, start=0, count=n, tracks=False)
        same(got, terms_model(v, dead, which, *w.cols(), 0, n, tracks=False)[:3], (storage, n, "reject a crop with a copy"))
        ans = got[0][0, :int(got[2][0])].tolist()
        assert r not in ans and c not in ans
        got = ix.rank_terms(rows=[r], start=0, count=n, tracks=False, exclude="rows")
        ans = got[0][0, :int(got[2][0])].tolist()
        assert r not in ans and c in ans and got[2][0] == n - 1
        # a REQUIRE term that no row of a track passes removes the track: total drops by one
        S = term_scores(ix, w.q[6:8], [])
        slot = next(t for t in range(1, SLOTS) if not ((S[1] == S[1][w.slot == t].max()) & (w.slot != t)).any())
        top = np.float32(S[1][w.slot == slot].max())
        totals = []
        for cut in (top, np.nextafter(top, np.float32(np.inf))):
            roles, cuts = ["rank", "require"], [None, float(cut)]
            v, dead, which = fold_terms(S, roles, None, cuts, "max")
            got = ix.rank_terms(q=w.q[6:8], roles=roles, cuts=cuts, start=0, count=2000, which=True)
            same(got, terms_model(v, dead, which, *w.cols(), 0, 2000), (storage, n, "require", float(cut)))
            totals.append(int(got[2][0]))
            assert (slot in w.slot[got[0][0][got[0][0] >= 0]]) == (cut == top)
        assert totals[1] == totals[0] - 1 and totals[1] >= 1


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_timeline_terms_counts_what_rank_terms_ranks(worlds, storage):
    k = 0
    for n, w in worlds.items():
        ix = w.index(storage)
        for T in (9, 18):                                                           # below and above the GEMM / MFMA threshold
            for pattern in PATTERNS:
                combine = sorted(COMBINES)[k % 3]
                tracks, name, _ = CONFIGS[k % len(CONFIGS)]
                q, rows, roles, weights = plan(w, T, pattern, combine, k % 2)
                exclude = EXCLUDES[k % 3] if any(r == "rank" for r in roles[len(q):]) else None
                k += 1
                S = term_scores(ix, q, rows)
                path = ix.last_scores_path()
                cuts = median_cuts(S, roles, w.competing(name))
                v, dead, which = terms_fold(S, roles, weights, cuts, combine, rows, len(q), w.group, w.slot, exclude)
                kw = filter_kw(name)
                what = (storage, n, T, pattern, combine, tracks, name, exclude)
                for cut in (None, float(np.median(v))):
                    ask = dict(q=q, rows=rows, roles=roles, weights=weights, cuts=cuts, combine=combine, min_score=cut, tracks=tracks, exclude=exclude, **kw)
                    counts, total = ix.timeline_terms(-50, 30, 12, **ask)
                    assert ix.last_scores_path() == path == expected_path(storage, DIM, n, T)
                    want = terms_timeline_model(v, dead, *w.cols(), -50, 30, 12, kw["allowed"], cut, tracks, kw["ts_range"], kw["classes"])
                    assert counts.dtype == np.int64 and counts.shape == (1, 12) and np.array_equal(counts, want[0]), what
                    assert np.array_equal(total, want[1]) and total[0] == ix.rank_terms(start=0, count=1, **ask)[2][0] and total[0] >= 40, what
                    assert 0 < counts.sum() < total[0], what                           # some answers lie outside the bins or carry no ts


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_index_answering(worlds):
    import torch
    from clearcam_amd import _lib
    w = worlds[N_ODD]
    ix, n = w.index("f32"), w.n
    L = _lib.lib()
    q = np.ascontiguousarray(w.q[:2])
    good_rows = w.query_rows(3)
    good_terms = [(0, 1.0, 0.0), (1, 1.0, 0.05), (0, -0.5, 0.0), (0, 1.0, 0.0), (2, 1.0, 0.4)]
    where = ix.row_filter(*FILTERS["both"][:2])
    window = _lib.RowFilter()
    window.use_ts, window.ts_min, window.ts_max = 1, 5, 4
    empty = _lib.RowFilter()
    empty.use_cls = 1
    idx, s, wh, total = np.empty((1, 10), np.int32), np.empty((1, 10), np.float32), np.empty((1, 10), np.int32), np.zeros(1, np.int64)
    counts = np.empty((1, 12), np.uint32)
    dq = torch.as_tensor(q).cuda()
    didx, dwh = (torch.full((1, 10), 99, dtype=torch.int32, device="cuda") for _ in range(2))
    ds = torch.full((1, 10), 99.0, dtype=torch.float32, device="cuda")
    dcounts = torch.full((1, 12), 99, dtype=torch.int32, device="cuda")
    al = np.ones(GROUPS, np.uint8)
    NULL = object()

    def args(q=q, n_vec=None, rows=good_rows, n_rows=None, terms=good_terms, combine=2, flags=1 | _lib.LIKE_EXCLUDE_TRACK, cut=-np.inf, where=where,
             allowed=None, n_groups=0):
        ids = np.ascontiguousarray([] if rows is NULL else rows, dtype=np.int64)
        tt = (_lib.Term * max(len(terms), 1))(*[_lib.Term(*t) for t in terms])
        keep.extend([ids, tt])
        head = (ix._h, None if q is NULL else _lib.ptr(q), (0 if q is NULL else len(q)) if n_vec is None else n_vec,
                None if rows is NULL else ids.ctypes.data_as(C.POINTER(C.c_int64)), len(ids) if n_rows is None else n_rows, tt, combine)
        return head, (cut, flags, _lib.ptr(allowed) if allowed is not None else None, n_groups, C.byref(where) if where is not None else None)

    keep = []

    def call(start=1, count=10, device=False, **kw):
        if device and "q" not in kw:
            kw["q"] = dq
        head, mid = args(**kw)
        out = (_lib.ptr(didx), _lib.ptr(ds), _lib.ptr(dwh), None, 1, None) if device else (_lib.ptr(idx), _lib.ptr(s), _lib.ptr(wh), _lib.ptr(total), 0, None)
        return L.cc_index_rank_terms(*head, start, count, *mid, *out)

    def line(t0=-50, bin_seconds=30, n_bins=12, device=False, **kw):
        if device and "q" not in kw:
            kw["q"] = dq
        head, mid = args(**kw)
        out = (_lib.ptr(dcounts), None, 1, None) if device else (_lib.ptr(counts), _lib.ptr(total), 0, None)
        return L.cc_index_timeline_terms(*head, *mid, t0, bin_seconds, n_bins, *out)

    roles = ["rank", "require", "rank", "rank", "reject"]
    S = term_scores(ix, q, good_rows)
    v, dead, which = terms_fold(S, roles, [t[1] for t in good_terms], [t[2] for t in good_terms], "sum", good_rows, 2, w.group, w.slot, "track")
    ts_range, classes, _ = FILTERS["both"]
    want = terms_model(v, dead, which, *w.cols(), 1, 10, None, None, True, ts_range, classes)
    want_line = terms_timeline_model(v, dead, *w.cols(), -50, 30, 12, None, None, True, ts_range, classes)
    assert want[2][0] >= 10 and dead.any()
    plain = ix.rank(w.q[:1], 0, 20)
    slotless = int(np.flatnonzero(w.slot < 0)[0])
    other = int(np.flatnonzero((w.slot == w.qslot) & (w.group != w.qgroup))[0])
    t5 = lambda **role_of: [tuple(role_of.get(f"t{i}", t)) for i, t in enumerate(good_terms)]   # noqa: E731
    both = {  # what both calls refuse
        "no terms": dict(q=NULL, rows=NULL, terms=[]), "65 terms": dict(q=np.resize(q, (33, DIM)), rows=np.resize(good_rows, 32), terms=[(0, 1.0, 0.0)] * 65),
        "a negative n_vec": dict(n_vec=-1), "a negative n_rows": dict(n_rows=-1), "n_vec + n_rows overflows": dict(n_vec=2 ** 31 - 1, n_rows=2 ** 31 - 1),
        "null q": dict(q=NULL, n_vec=2), "null rows": dict(rows=NULL, n_rows=3),
        "no RANK term": dict(terms=[(1, 1.0, 0.1), (2, 1.0, 0.1), (1, 1.0, 0.1), (2, 1.0, 0.1), (2, 1.0, 0.1)], flags=1),
        "role 3": dict(terms=t5(t1=(3, 1.0, 0.0))), "role -1": dict(terms=t5(t4=(-1, 1.0, 0.0))), "combine 3": dict(combine=3), "combine -1": dict(combine=-1),
        "an infinite weight under SUM": dict(terms=t5(t2=(0, np.inf, 0.0))), "a NaN weight under SUM": dict(terms=t5(t0=(0, np.nan, 0.0))),
        "a NaN cut on REQUIRE": dict(terms=t5(t1=(1, 1.0, np.nan))), "a NaN cut on REJECT": dict(terms=t5(t4=(2, 1.0, np.nan))),
        "a row past the end": dict(rows=[int(good_rows[0]), n, int(good_rows[2])]), "a negative row": dict(rows=[-1, int(good_rows[1]), int(good_rows[2])]),
        "exclude without a stored RANK row": dict(terms=[(0, 1.0, 0.0), (0, 1.0, 0.0), (2, 1.0, 0.5), (1, 1.0, 0.0), (2, 1.0, 0.5)]),
        "exclude rows, vectors only": dict(rows=NULL, terms=good_terms[:2], flags=1 | _lib.LIKE_EXCLUDE_ROWS),
        "track of a slot-less row": dict(rows=[int(good_rows[0]), slotless, int(good_rows[2])]), "track of two groups": dict(rows=[int(good_rows[0]), other, int(good_rows[2])]),
        "unknown flag 8": dict(flags=1 | 8), "unknown flag 16": dict(flags=16), "NaN min_score": dict(cut=float("nan")),
        "a bad group count": dict(allowed=al, n_groups=0), "an empty window": dict(where=window), "an empty class set": dict(where=empty),
    }
    cases = [(what, call, kw) for what, kw in both.items()] + [(what, line, kw) for what, kw in both.items()]
    cases += [("start -1", call, dict(start=-1)), ("count 0", call, dict(count=0)), ("bin_seconds 0", line, dict(bin_seconds=0)), ("no bins", line, dict(n_bins=0)),
              ("4097 bins", line, dict(n_bins=4097))]
    for what, f, kw in cases:
        idx[:] = 99; s[:] = 99.0; wh[:] = 99; counts[:] = 99
        assert f(**kw) == -22, what
        assert L.cc_last_error(), what
        assert (idx == 99).all() and (s == 99.0).all() and (wh == 99).all() and (counts == 99).all(), what
        assert f(device=True, **kw) == -22, (what, "device")
        assert len(ix) == n
    torch.cuda.synchronize()
    assert bool((didx == 99).all()) and bool((ds == 99.0).all()) and bool((dwh == 99).all()) and bool((dcounts == 99).all())
    got = ix.rank(w.q[:1], 0, 20)                                                      # a plain rank answers as it did before the failed calls
    assert all(np.array_equal(a, b) for a, b in zip(got, plain))
    assert call() == 0
    same((idx, s, total, wh), want, "after the errors")
    assert line() == 0 and np.array_equal(counts.astype(np.int64), want_line[0]) and total[0] == want_line[1][0]
    # what is NOT an error: weights that MAX / MIN never read, 64 terms, a null which
    assert call(terms=t5(t2=(0, np.inf, 0.0)), combine=0) == 0 and call(terms=t5(t2=(0, np.nan, 0.0)), combine=1) == 0
    assert call(q=np.resize(q, (32, DIM)), rows=np.resize(good_rows, 32), terms=[(0, 1.0, 0.0)] * 64, flags=1) == 0
    with pytest.raises(ValueError):
        ix.rank_terms(q=q, roles=["rank", "must"])
    with pytest.raises(ValueError):
        ix.rank_terms(q=q, combine="mean")
    with pytest.raises(ValueError):
        ix.rank_terms(q=q, exclude="all")
    with pytest.raises(ValueError):
        ix.rank_terms(q=q, roles=["rank"])
    with pytest.raises(TypeError):
        ix.rank_terms(rows=[0.5])
    with pytest.raises(_lib.CCError, match="-22"):
        ix.rank_terms()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_calls_repeat_and_leave_their_neighbours_alone(worlds, storage):
    w = worlds[N_EVEN]
    ix = w.index(storage)
    rows = w.query_rows(9)

    def neighbours():
        return (ix.rank(w.q[:3], 5, 300, min_score=0.0, **filter_kw("ts")) + ix.rank_like(rows, 1030, 100, exclude="track") +
                ix.rank_like(rows[:1], 0, 50) + ix.digest(0.9, 0, 200, ts_range=(100, 250)))

    before = neighbours()
    for T, pattern, combine in ((18, "both", "sum"), (9, "reject", "min"), (2, "require", "max")):
        q, r, roles, weights = plan(w, T, pattern, combine, 1)
        S = term_scores(ix, q, r)
        ask = dict(q=q, rows=r, roles=roles, weights=weights, cuts=median_cuts(S, roles, np.arange(w.n)), combine=combine, which=True)
        a = ix.rank_terms(start=0, count=300, exclude="rows" if pattern != "require" else None, **ask)
        b = ix.rank_terms(start=0, count=300, exclude="rows" if pattern != "require" else None, **ask)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[2][0] > 40
        after = neighbours()
        assert len(before) == len(after) and all(x.tobytes() == y.tobytes() for x, y in zip(before, after)), (storage, T)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
CAMS, DAY = ("back", "front", "gate"), "2026-01-01"


def finder_spec():
    """camera -> [(name, vector)]: 3 folders x 100 crops around six directions (cosines inside a cluster about 0.8), ten track ids
    shared across folders, every ninth crop a snapshot without '_', three classes, a tenth of the crops copies of an earlier one."""
    rng = np.random.default_rng(41)
    centres = unit(rng.standard_normal((6, 768)))
    out = {}
    for cam in CAMS:
        crops = []
        for i in range(100):
            v = unit(centres[int(rng.integers(0, 6))] + 0.5 * unit(rng.standard_normal(768)))
            if i and rng.random() < 0.1:
                v = crops[int(rng.integers(0, i))][1]
            name = f"snap{i}.jpg" if i % 9 == 4 else f"{1000 + 7 * i}.5_{int(rng.integers(0, 10))}_{(0, 2, 7)[int(rng.integers(0, 3))]}.jpg"
            crops.append((name, v))
        out[cam] = list({n: (n, v) for n, v in crops}.values())
    return out, centres


def build_finder(root, folders, storage):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    for cam, crops in folders.items():
        d = os.path.join(root, cam, "objects", DAY)
        EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    f = ObjectFinder(root)
    f.index_storage = storage
    f.attach_store(capacity=64)
    return f


@pytest.mark.parametrize("storage", STORAGES)
def test_object_finder_compound(tmp_path, storage):
    from clearcam_amd.objects import Term
    root = str(tmp_path / "cameras")
    folders, centres = finder_spec()
    f = build_finder(root, folders, storage)
    index, table = f._dev["store"]
    n = len(table.paths)
    assert index.storage == storage and n == len(index) == sum(len(c) for c in folders.values()) and n >= 280
    slot, group = table.slots(), np.asarray(table.group, np.int32)
    ts, cls = table.attrs()
    clicked = next(p for p in table.paths if "snap" not in p and "/front/" in p)
    other = next(p for p in table.paths if "snap" not in p and "/back/" in p)
    e0, e1 = centres[0], unit(centres[1] + 0.3 * centres[2])

    def expect(terms, combine, start, count, min_score=None, cam_name=None, ts_range=None, classes=None, exclude=None, **_):
        vec_at = [i for i, t in enumerate(terms) if t.path is None]
        row_at = [i for i, t in enumerate(terms) if t.path is not None]
        order = vec_at + row_at
        q = np.stack([np.asarray(terms[i].embedding, np.float32) for i in vec_at]) if vec_at else None
        rows = np.array([table.row_of(terms[i].path) for i in row_at], np.int64)
        S = term_scores(index, q, rows)
        roles = [terms[i].role for i in order]
        v, dead, which = terms_fold(S, roles, [terms[i].weight for i in order], [terms[i].cut for i in order], combine, rows, len(vec_at), group, slot, exclude)
        allowed = table.allowed(cam_name, None)
        tracks = any(table.truthy[g] for g in np.flatnonzero(allowed))
        cut = None if min_score is None else float(index.cut_f32(min_score))
        cols = (slot, group, len(table.dirs), ts, cls)
        idx, sc, total, wh = terms_model(v, dead, which, *cols, start, count, allowed, cut, tracks, ts_range, classes)
        res = [(table.paths[r], float(x), order[t]) for r, x, t in zip(idx[0].tolist(), sc[0], wh[0].tolist()) if r >= 0]
        counts, _ = terms_timeline_model(v, dead, *cols, 1000, 100, 8, allowed, cut, tracks, ts_range, classes)
        return res, int(total[0]), counts[0]

    s_clicked = index.scores(index.fetch([table.row_of(clicked)]))[0]
    questions = (
        (dict(terms=[Term(embedding=e0)], combine="max"), dict()),
        (dict(terms=[Term(path=clicked, role="reject", cut=float(np.sort(s_clicked)[-30])), Term(embedding=e0), Term(embedding=e1)], combine="max"), dict(count=40)),
        (dict(terms=[Term(embedding=e0, weight=1.0), Term(path=clicked, weight=0.5), Term(embedding=e1, weight=-0.7)], combine="sum"),
         dict(start=3, count=25, exclude="track", cam_name="front")),
        (dict(terms=[Term(embedding=e1, role="require", cut=0.1), Term(path=clicked), Term(path=other)], combine="min"), dict(min_score=-0.02, count=300)),
        (dict(terms=[Term(path=other), Term(embedding=e0, role="require", cut=0.0), Term(path=clicked, role="reject", cut=0.6)], combine="max"),
         dict(ts_range=(1000, 1500), classes=(0, 2), exclude="rows")),
    )
    for ask, page in questions:
        kw = dict(start=0, count=100)
        kw.update(page)
        res, total, hist = expect(**ask, **kw)
        assert total >= 5, ask
        got = f.compound(explain=True, **ask, **kw)
        assert got == (res, total), (storage, kw)
        assert f.compound(**ask, **kw) == ([r[:2] for r in res], total)
        tl = {k: v for k, v in kw.items() if k not in ("start", "count")}
        counts, t = f.compound_timeline(t0=1000, bin_seconds=100, n_bins=8, **ask, **tl)
        assert t == total and counts.dtype == np.int64 and np.array_equal(counts, hist), (storage, kw)
    # the rejected crop, and every crop that looks like it, left the second question's answers
    res, _ = f.compound(count=1000, **questions[1][0])
    gone = {table.paths[r] for r in np.flatnonzero(s_clicked >= np.float32(questions[1][0]["terms"][0].cut))}
    assert clicked in gone and len(gone) >= 30 and not gone & {p for p, _ in res}
    # distinct= thins the compound ranking on the device, behind rank_terms_device
    ask = questions[2][0]
    calls = []
    real = index.distinct_device
    index.distinct_device = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        got = f.compound(distinct=0.7, distinct_depth=128, start=1, count=20, explain=True, **ask)
    finally:
        del index.distinct_device
    assert calls == [1]
    full = expect(start=0, count=128, **ask)[0]
    oi, os_, od, total = index.distinct(np.array([table.row_of(p) for p, _, _ in full], np.int32), np.array([x for _, x, _ in full], np.float32), 0.7, 1, 20)
    term_of = {p: t for p, _, t in full}
    assert got == ([(table.paths[r], float(x), int(d), term_of[table.paths[r]]) for r, x, d in zip(oi[0].tolist(), os_[0], od[0].tolist()) if r >= 0], int(total[0]))
    assert 0 < got[1] < len(full) and any(d > 0 for _, _, d, _ in got[0])
    # what is wrong with the question is said before any GPU work
    index.rank_terms = index.rank_terms_device = index.timeline_terms = None
    try:
        for bad, err in (([Term(text="a van", embedding=e0)], ValueError), ([Term(embedding=e0, role="must")], ValueError), ([Term()], ValueError),
                         ([Term(embedding=e0), Term(path=os.path.join(root, "front", "objects", DAY, "nothing.jpg"))], KeyError),
                         ([Term(embedding=e0[:512])], ValueError), ([Term(embedding=e0, role="reject", cut=0.3)], ValueError)):
            with pytest.raises(err):
                f.compound(bad)
            with pytest.raises(err):
                f.compound_timeline(bad)
        with pytest.raises(ValueError):
            f.compound([Term(embedding=e0)], count=0)
        with pytest.raises(ValueError):
            f.compound([Term(embedding=e0)], distinct=float("nan"))
    finally:
        del index.rank_terms, index.rank_terms_device, index.timeline_terms
    url = "/" + os.path.relpath(clicked, root).replace(os.sep, "/")                   # the endpoint's form of a stored crop
    assert f.compound([Term(path=url), Term(embedding=e0)], count=5) == f.compound([Term(path=clicked), Term(embedding=e0)], count=5)
    # a folder with a name the reference raises on: the call says which folder, and the other folders go on answering
    bad_name = os.path.join(root, "gate", "objects", DAY, "12.5_x_2.jpg")
    f.add_embedding(bad_name, e1)
    with pytest.raises(ValueError, match="gate"):
        f.compound([Term(embedding=e0)])
    with pytest.raises(ValueError, match="gate"):
        f.compound_timeline([Term(embedding=e0)], cam_name="gate")
    assert f.compound([Term(embedding=e0)], cam_name="front")[1] > 0
