"""Together on the GPU: cc_index_rank_near / cc_index_timeline_near through EmbeddingIndex.rank_near / rank_near_device / timeline_near
and ObjectFinder.together / together_timeline.

The expected answers are the numpy model of tests/near_cases.py (the partner list as an ungrouped ranking of B, the join row by list
entry, dead rows as a forbidden group, then the unchanged model of tests/rank_cases.py) applied to the index's own
`ix.scores(np.vstack([a, b]))`.  Every comparison is exact: integer arrays equal and f32 compared as bits, no tolerance.  The worlds are
like_cases.World, 8229 and 8224 rows of 256; the case table (near_cases.case_table) is checked for what it exercises on the CPU
(tests/test_index_near_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from near_cases import (CHUNK, DIM, GROUPS, INT32_MAX, INT32_MIN, MAX_PARTNERS, N_EVEN, N_ODD, NO_TS, World, case_table, list_position, near_fold, near_model,
                        near_order, near_page, near_timeline_model, partner_list, passing)
from rank_cases import run_bounds
from where_cases import FILTERS, unit

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "bf16", "i8")
NO_FILTER = (None, None, None)
B_CLASSES = (0, 2, 64, 255)


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
    """(idx, score, total, partner, partner_score, n_partners) of the device against the model's"""
    assert got[0].dtype == got[3].dtype == np.int32 and got[1].dtype == got[4].dtype == np.float32 and got[2].dtype == np.int64, what
    assert got[0].shape == got[1].shape == got[3].shape == got[4].shape == want[0].shape and got[2].shape == want[2].shape == (1,), what
    assert got[5] == want[5] and isinstance(got[5], int), (what, "n_partners", got[5], want[5])
    assert np.array_equal(got[2], want[2]), (what, "total", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "score")
    assert np.array_equal(got[3], want[3]), (what, "partner")
    assert np.array_equal(bits(got[4]), bits(want[4])), (what, "partner_score")


def side_scores(ix, a, b):
    """The device's own (2, n) score matrix of the two sides (an int: a stored row, as the index decodes it)"""
    vec = [ix.fetch([x])[0] if isinstance(x, int) else np.asarray(x, np.float32) for x in (a, b)]
    S = ix.scores(np.vstack(vec))
    assert ix.last_scores_path() == 0
    return S[0], S[1]


def tied_cut(s):
    """A cut inside a run of equal scores of a descending list (the middle run); without a run, the middle score"""
    runs = run_bounds(s)
    return float(s[runs[len(runs) // 2][0]]) if runs else float(s[len(s) // 2])


# 1 ---------------------------------------------------------------------------------------------------------------------------------
SIDES = ("vectors", "a stored", "b stored")
A_FILTERS = (None, "ts", "both+allowed")


def run_case(w, ix, k, within, partners):
    """Case k of the table on the device and in the model; the other arguments rotate with k so that every one takes every value"""
    value = ("a", "min")[k % 2]
    tracks = (k // 2) % 2 == 0
    name = A_FILTERS[k % 3]
    b_classes = B_CLASSES if k % 4 == 1 else None
    tie_b, tie_a = k % 5 == 2, k % 3 == 1
    side = SIDES[(k // 3) % 3]
    a, b = w.q[0], w.q[1]
    if side == "a stored":
        a = int(w.query_rows(3)[1])
    elif side == "b stored":
        b = int(w.query_rows(3)[2])
    Sa, Sb = side_scores(ix, a, b)
    kw = filter_kw(name)
    what = (ix.storage, w.n, within, partners, value, tracks, name, b_classes is not None, tie_b, tie_a, side)
    cut_b = None
    if tie_b:
        full, _ = partner_list(Sb, w.group, GROUPS, w.ts, w.cls, w.n, None, kw["allowed"], None, b_classes)
        cut_b = tied_cut(Sb[full])
    plist, n_partners = partner_list(Sb, w.group, GROUPS, w.ts, w.cls, partners, cut_b, kw["allowed"], None, b_classes)
    v, dead, partner = near_fold(Sa, Sb, plist, w.group, w.slot, w.ts, within, value)
    ans, s = near_order(v, dead, *w.cols(), kw["allowed"], tracks, None, kw["ts_range"], kw["classes"])
    cut = tied_cut(s) if tie_a and len(s) else None
    ask = dict(a=a, b=b, within=within, partners=partners, cut_b=cut_b, value=value, min_score=cut, tracks=tracks, b_classes=b_classes, **kw)
    for start, count in ((0, 50), (1030, 100)):
        want = near_page(v, dead, partner, Sb, n_partners, *w.cols(), start, count, kw["allowed"], cut, tracks, kw["ts_range"], kw["classes"])
        same(ix.rank_near(start=start, count=count, **ask), want, what + (start,))
    return list_position(plist, partner), dead


@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_equals_the_model_over_the_case_table(worlds, storage):
    deepest, seen = 0, {"dead": False, "living": False}
    for n, w in worlds.items():
        ix = w.index(storage)
        for k, (within, partners) in enumerate(case_table()):
            pos, dead = run_case(w, ix, k + (n == N_EVEN), within, partners)         # the second world shifts the rotation by one
            deepest = max(deepest, int(pos.max(initial=-1)))
            seen["dead"] |= bool(dead[w.ts != NO_TS].any()); seen["living"] |= bool((~dead).any())
    assert deepest >= 2 * CHUNK and all(seen.values())                               # partners were found in the third chunk of a list


def test_a_page_past_the_pinned_block(worlds):
    """A host result too large for the pinned block comes down by copies, partner and partner_score with it"""
    w = worlds[N_ODD]
    ix = w.index("f32")
    Sa, Sb = side_scores(ix, w.q[0], w.q[1])
    want = near_model(Sa, Sb, *w.cols(), 7, 0, 140000, 1025, None, "min", None, None, False)
    same(ix.rank_near(w.q[0], w.q[1], 7, 0, 140000, partners=1025, tracks=False), want, "a large host result")
    assert want[2][0] > 7000


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_a_crop_of_the_same_track_is_nobodys_partner(worlds, storage):
    w = worlds[N_ODD]
    ix, n = w.index(storage), w.n
    q = w.q[2]
    Sa, Sb = side_scores(ix, q, q)
    assert np.array_equal(bits(Sa), bits(Sb))
    got = ix.rank_near(q, q, 500, 0, n, partners=3000, value="a", tracks=False)
    same(got, near_model(Sa, Sb, *w.cols(), 500, 0, n, 3000, None, "a", None, None, False), (storage, "b is a"))
    idx, pr = got[0][0, :int(got[2][0])], got[3][0, :int(got[2][0])]
    assert len(idx) > 7000 and (pr >= 0).all() and (idx >= 0).all()
    assert (pr != idx).all()                                                         # no answer is its own partner, though it tops B's list for itself
    assert (w.group[pr] == w.group[idx]).all() and (np.abs(w.ts[pr].astype(np.int64) - w.ts[idx]) <= 500).all()
    assert not ((w.slot[idx] >= 0) & (w.slot[pr] == w.slot[idx])).any()               # nor a crop of its own track in its own folder
    # slot-less rows may pair with each other: both sides are one stored slot-less crop, which tops B's list and is everybody's partner
    # in its group but its own
    r = int(np.flatnonzero((w.slot < 0) & (w.ts != NO_TS))[3])
    Ra, Rb = side_scores(ix, r, r)
    got = ix.rank_near(r, r, 500, 0, n, partners=3000, value="a", tracks=False)
    same(got, near_model(Ra, Rb, *w.cols(), 500, 0, n, 3000, None, "a", None, None, False), (storage, "a slot-less stored row"))
    loose_idx, loose_pr = got[0][0, :int(got[2][0])], got[3][0, :int(got[2][0])]
    assert ((w.slot[loose_idx] < 0) & (w.slot[loose_pr] < 0)).any() and (loose_pr != loose_idx).all() and r in loose_idx and r in loose_pr
    # without the rule the best-scoring row of a row's own track would often be the first qualifying entry
    plist, _ = partner_list(Sb, w.group, GROUPS, w.ts, w.cls, 3000)
    _, _, loose = near_fold(Sa, Sb, plist, w.group, np.full(n, -1, np.int32), w.ts, 500, "a")
    assert ((w.slot[idx] >= 0) & (w.slot[loose[idx]] == w.slot[idx])).any()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_time_differences_are_taken_in_64_bits(storage):
    from clearcam_amd.objects import EmbeddingIndex
    rng = np.random.default_rng(11)
    n = 70
    E, q = unit(rng.standard_normal((n, DIM))), unit(rng.standard_normal((2, DIM)))
    ts = np.zeros(n, np.int32)
    ts[0], ts[1] = INT32_MAX, INT32_MIN + 1
    ts[[5, 33, 69]] = NO_TS
    group, slot, cls = np.ones(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    ix = EmbeddingIndex(DIM, n, storage=storage)
    ix.add(E, group, slot, ts=ts, classes=cls)
    Sa, Sb = side_scores(ix, q[0], q[1])
    cols = (slot, group, 2, ts, cls)
    at_zero = np.flatnonzero(ts == 0)
    for within in (INT32_MAX, 0):
        for b_ts_range in (None, (INT32_MAX, INT32_MAX), (INT32_MIN + 1, INT32_MIN + 1)):
            got = ix.rank_near(q[0], q[1], within, 0, n, partners=n, value="a", tracks=False, b_ts_range=b_ts_range)
            want = near_model(Sa, Sb, *cols, within, 0, n, n, None, "a", None, None, False, None, None, b_ts_range)
            same(got, want, (storage, within, b_ts_range))
            idx, pr = got[0][0, :int(got[2][0])], got[3][0, :int(got[2][0])]
            assert not set(idx.tolist()) & {5, 33, 69} and not set(pr.tolist()) & {5, 33, 69}   # rows without a ts never pair
            assert got[5] == (n - 3 if b_ts_range is None else 1)
            if within == 0:                                                          # only the rows at 0 have company in their second
                assert sorted(idx.tolist()) == (at_zero.tolist() if b_ts_range is None else [])
            elif b_ts_range is None:                                                 # the ends pair with the rows at 0 ...
                assert sorted(idx.tolist()) == sorted(at_zero.tolist() + [0, 1]) and ts[pr[idx == 0][0]] == 0 and ts[pr[idx == 1][0]] == 0
            else:                                                                    # ... but not with each other: 2^32 - 2 seconds, not 2
                assert sorted(idx.tolist()) == at_zero.tolist() and set(pr.tolist()) == {0 if b_ts_range[0] == INT32_MAX else 1}
    ix.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_n_partners_tells_a_truncated_list(worlds, storage):
    w = worlds[N_EVEN]
    ix = w.index(storage)
    Sa, Sb = side_scores(ix, w.q[0], w.q[1])
    for name, b_classes in ((None, None), ("both+allowed", B_CLASSES), ("ts", (7,))):
        kw = filter_kw(name)
        ok = passing(w.ts, w.cls, None, b_classes) & (w.ts != NO_TS)
        if kw["allowed"] is not None:
            ok &= kw["allowed"][w.group] != 0
        got = ix.rank_near(w.q[0], w.q[1], 7, 0, 60, partners=5, b_classes=b_classes, **kw)
        assert got[5] == int(ok.sum()) > 500, (storage, name)
        want = near_model(Sa, Sb, *w.cols(), 7, 0, 60, 5, None, "min", kw["allowed"], None, True, kw["ts_range"], kw["classes"], None, b_classes)
        same(got, want, (storage, name))
        assert len(set(got[3][0][got[3][0] >= 0].tolist())) <= 5


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_an_empty_list_answers_nothing(worlds, storage):
    w = worlds[N_ODD]
    ix = w.index(storage)
    for tracks in (True, False):
        idx, sc, total, pr, ps, n_partners = ix.rank_near(w.q[0], w.q[1], 500, 0, 40, cut_b=2.0, tracks=tracks)
        assert total.tolist() == [0] and n_partners == 0
        assert (idx == -1).all() and np.isneginf(sc).all() and (pr == -1).all() and np.isneginf(ps).all()
        counts, total, n_partners = ix.timeline_near(w.q[0], w.q[1], 500, -50, 30, 15, cut_b=2.0, tracks=tracks)
        assert counts.shape == (1, 15) and not counts.any() and total.tolist() == [0] and n_partners == 0


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_timeline_near_counts_what_rank_near_ranks(worlds, storage):
    for n, w in worlds.items():
        ix = w.index(storage)
        for k, (within, partners) in enumerate(((1, 1025), (7, 5), (0, 3000), (500, 1024))):
            value, tracks, name = ("a", "min")[k % 2], k < 2, A_FILTERS[k % 3]
            a, b = (w.q[0], int(w.query_rows(3)[0])) if k == 2 else (w.q[0], w.q[1])
            Sa, Sb = side_scores(ix, a, b)
            kw = filter_kw(name)
            v = near_fold(Sa, Sb, partner_list(Sb, w.group, GROUPS, w.ts, w.cls, partners, None, kw["allowed"])[0], w.group, w.slot, w.ts, within, value)[0]
            for cut in (None, float(np.median(v))):
                ask = dict(a=a, b=b, within=within, partners=partners, value=value, min_score=cut, tracks=tracks, **kw)
                counts, total, n_partners = ix.timeline_near(t0=-50, bin_seconds=30, n_bins=12, **ask)
                want = near_timeline_model(Sa, Sb, *w.cols(), within, -50, 30, 12, partners, None, value, kw["allowed"], cut, tracks, kw["ts_range"], kw["classes"])
                what = (storage, n, within, partners, value, tracks, name, cut)
                assert counts.dtype == np.int64 and counts.shape == (1, 12) and np.array_equal(counts, want[0]), what
                assert np.array_equal(total, want[1]) and n_partners == want[2], what
                page = ix.rank_near(start=0, count=1, **ask)
                assert total[0] == page[2][0] and n_partners == page[5] and 0 < counts.sum() <= total[0], what


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_form_and_its_neighbours(worlds, storage):
    import torch
    w = worlds[N_EVEN]
    ix = w.index(storage)
    rows = w.query_rows(9)

    def neighbours():
        return (ix.rank(w.q[:3], 5, 300, min_score=0.0, **filter_kw("ts")) + ix.rank_like(rows, 1030, 100, exclude="track") +
                ix.rank_terms(q=w.q[:2], rows=rows[:2], roles=["rank", "require", "rank", "reject"], cuts=[None, 0.0, None, 0.5], start=0, count=200, which=True))

    before = neighbours()
    side = torch.cuda.Stream()
    for a, b, within, partners, value, tracks in ((w.q[0], w.q[1], 1, 1025, "min", True), (int(rows[3]), w.q[1], 7, 3000, "a", False),
                                                  (w.q[0], int(rows[5]), 500, 5, "min", True)):
        ask = dict(a=a, b=b, within=within, partners=partners, value=value, tracks=tracks, b_classes=B_CLASSES, **filter_kw("ts"))
        host = ix.rank_near(start=3, count=200, **ask)
        assert host[2][0] > 40 and ix.rank_near(start=3, count=200, **ask)[0].tobytes() == host[0].tobytes()
        with torch.cuda.stream(side):
            dev = ix.rank_near_device(start=3, count=200, **ask)
            quiet = ix.rank_near_device(start=3, count=200, with_total=False, **ask)
        side.synchronize()
        assert all(t.is_cuda for t in (dev[0], dev[1], dev[3], dev[4])) and quiet[2] is None and quiet[5] is None
        same((dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2], dev[3].cpu().numpy(), dev[4].cpu().numpy(), dev[5]), host, (storage, within, "device"))
        same((quiet[0].cpu().numpy(), quiet[1].cpu().numpy(), host[2], quiet[3].cpu().numpy(), quiet[4].cpu().numpy(), host[5]), host, (storage, within, "no total"))
        after = neighbours()                       # score row 0, the dead bytes and the list are the call's own scratch
        assert len(before) == len(after) and all(x.tobytes() == y.tobytes() for x, y in zip(before, after)), (storage, within)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_index_answering(worlds):
    import torch
    from clearcam_amd import _lib
    w = worlds[N_ODD]
    ix, n = w.index("f32"), w.n
    L = _lib.lib()
    qa, qb = np.ascontiguousarray(w.q[0]), np.ascontiguousarray(w.q[1])
    where = ix.row_filter(*FILTERS["both"][:2])
    window = _lib.RowFilter()
    window.use_ts, window.ts_min, window.ts_max = 1, 5, 4
    empty = _lib.RowFilter()
    empty.use_cls = 1
    idx, pr = np.empty((1, 10), np.int32), np.empty((1, 10), np.int32)
    s, ps = np.empty((1, 10), np.float32), np.empty((1, 10), np.float32)
    total, n_partners = np.zeros(1, np.int64), np.zeros(1, np.int64)
    counts = np.empty((1, 12), np.uint32)
    dqa, dqb = torch.as_tensor(qa).cuda(), torch.as_tensor(qb).cuda()
    didx, dpr = (torch.full((1, 10), 99, dtype=torch.int32, device="cuda") for _ in range(2))
    ds, dps = (torch.full((1, 10), 99.0, dtype=torch.float32, device="cuda") for _ in range(2))
    dcounts = torch.full((1, 12), 99, dtype=torch.int32, device="cuda")
    al = np.ones(GROUPS, np.uint8)
    NULL = object()

    def question(device, a=None, row_a=-1, b=None, row_b=-1, within=7, partners=1025, cut_b=-np.inf, value=1, cut=-np.inf, flags=1, allowed=None, n_groups=0,
                 where_a=where, where_b=None):
        a = (dqa if device else qa) if a is None else a
        b = (dqb if device else qb) if b is None else b
        head = (ix._h, None if a is NULL else _lib.ptr(a), row_a, None if b is NULL else _lib.ptr(b), row_b, within, partners, cut_b, value)
        return head, (cut, flags, _lib.ptr(allowed) if allowed is not None else None, n_groups, C.byref(where_a) if where_a is not None else None,
                      C.byref(where_b) if where_b is not None else None)

    def call(start=1, count=10, device=False, **kw):
        head, mid = question(device, **kw)
        out = (_lib.ptr(didx), _lib.ptr(ds), _lib.ptr(dpr), _lib.ptr(dps), None, None, 1, None) if device else \
              (_lib.ptr(idx), _lib.ptr(s), _lib.ptr(pr), _lib.ptr(ps), _lib.ptr(total), _lib.ptr(n_partners), 0, None)
        return L.cc_index_rank_near(*head, start, count, *mid, *out)

    def line(t0=-50, bin_seconds=30, n_bins=12, device=False, **kw):
        head, mid = question(device, **kw)
        out = (_lib.ptr(dcounts), None, None, 1, None) if device else (_lib.ptr(counts), _lib.ptr(total), _lib.ptr(n_partners), 0, None)
        return L.cc_index_timeline_near(*head, *mid, t0, bin_seconds, n_bins, *out)

    Sa, Sb = side_scores(ix, qa, qb)
    ts_range, classes, _ = FILTERS["both"]
    want = near_model(Sa, Sb, *w.cols(), 7, 1, 10, 1025, None, "min", None, None, True, ts_range, classes)
    want_line = near_timeline_model(Sa, Sb, *w.cols(), 7, -50, 30, 12, 1025, None, "min", None, None, True, ts_range, classes)
    assert want[2][0] >= 10
    plain = ix.rank(w.q[:1], 0, 20)
    both = {  # what both calls refuse
        "a: vector and row": dict(row_a=3), "b: vector and row": dict(row_b=0), "a: neither": dict(a=NULL), "b: neither": dict(b=NULL),
        "a: a row past the end": dict(a=NULL, row_a=n), "b: a row past the end": dict(b=NULL, row_b=n + 5), "a: a negative row": dict(a=NULL, row_a=-7),
        "within -1": dict(within=-1), "within INT32_MIN": dict(within=INT32_MIN), "no partners": dict(partners=0), "negative partners": dict(partners=-3),
        "too many partners": dict(partners=MAX_PARTNERS + 1), "a NaN cut_b": dict(cut_b=float("nan")), "value 2": dict(value=2), "value -1": dict(value=-1),
        "unknown flag 2": dict(flags=1 | 2), "unknown flag 16": dict(flags=16), "NaN min_score": dict(cut=float("nan")),
        "a bad group count": dict(allowed=al, n_groups=0), "an empty window for a": dict(where_a=window), "an empty class set for a": dict(where_a=empty),
        "an empty window for b": dict(where_b=window), "an empty class set for b": dict(where_b=empty),
    }
    cases = [(what, call, kw) for what, kw in both.items()] + [(what, line, kw) for what, kw in both.items()]
    cases += [("start -1", call, dict(start=-1)), ("count 0", call, dict(count=0)), ("bin_seconds 0", line, dict(bin_seconds=0)), ("no bins", line, dict(n_bins=0)),
              ("4097 bins", line, dict(n_bins=4097))]
    for what, f, kw in cases:
        idx[:] = 99; s[:] = 99.0; pr[:] = 99; ps[:] = 99.0; counts[:] = 99; total[:] = 99; n_partners[:] = 99
        assert f(**kw) == -22, what
        assert L.cc_last_error(), what
        assert (idx == 99).all() and (s == 99.0).all() and (pr == 99).all() and (ps == 99.0).all() and (counts == 99).all(), what
        assert total[0] == 99 and n_partners[0] == 99, what
        assert f(device=True, **kw) == -22, (what, "device")
        assert len(ix) == n
    torch.cuda.synchronize()
    assert bool((didx == 99).all()) and bool((ds == 99.0).all()) and bool((dpr == 99).all()) and bool((dps == 99.0).all()) and bool((dcounts == 99).all())
    got = ix.rank(w.q[:1], 0, 20)                                                      # a plain rank answers as it did before the failed calls
    assert all(np.array_equal(x, y) for x, y in zip(got, plain))
    assert call() == 0
    same((idx, s, total, pr, ps, int(n_partners[0])), want, "after the errors")
    assert line() == 0 and np.array_equal(counts.astype(np.int64), want_line[0]) and total[0] == want_line[1][0] and n_partners[0] == want_line[2]
    # what is NOT an error: the limits themselves, null partner outputs, a null n_partners
    assert call(within=INT32_MAX, partners=MAX_PARTNERS) == 0 and call(within=0, partners=1) == 0
    head, mid = question(False)
    assert L.cc_index_rank_near(*head, 1, 10, *mid, _lib.ptr(idx), _lib.ptr(s), None, None, _lib.ptr(total), None, 0, None) == 0
    assert np.array_equal(idx, want[0]) and total[0] == want[2][0]
    # the Python layer passes the library's verdict on, and names what it can see itself
    for kw in (dict(within=-1), dict(partners=0), dict(partners=MAX_PARTNERS + 1), dict(cut_b=float("nan")), dict(min_score=float("nan")), dict(count=0),
               dict(start=-1), dict(ts_range=None, b=n)):
        with pytest.raises(_lib.CCError, match="-22"):
            ix.rank_near(**{**dict(a=qa, b=qb, within=7), **kw})
    with pytest.raises(_lib.CCError, match="-22"):
        ix.timeline_near(qa, -1, 7, 0, 60, 10)
    with pytest.raises(ValueError):
        ix.rank_near(qa, qb, 7, value="max")
    with pytest.raises(ValueError):
        ix.rank_near(qa, w.q[:2], 7)
    got = ix.rank(w.q[:1], 0, 20)
    assert all(np.array_equal(x, y) for x, y in zip(got, plain))


# 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_object_finder_together(tmp_path, storage):
    from clearcam_amd.objects import Term
    from test_gpu_index_terms import build_finder, finder_spec
    root = str(tmp_path / "cameras")
    folders, centres = finder_spec()
    f = build_finder(root, folders, storage)
    index, table = f._dev["store"]
    n = len(table.paths)
    assert index.storage == storage and n == len(index) >= 280
    slot, group = table.slots(), np.asarray(table.group, np.int32)
    ts, cls = table.attrs()
    clicked = next(p for p in table.paths if "snap" not in p and "/front/" in p)
    e0, e1 = centres[0], unit(centres[1] + 0.3 * centres[2])

    def expect(a, b, within, start, count, min_score, min_partner, value="min", cam_name=None, ts_range=None, classes=None, with_classes=None, partners=4096):
        sides = [table.row_of(x) if isinstance(x, str) else x for x in (a, b)]
        Sa, Sb = side_scores(index, *sides)
        allowed = table.allowed(cam_name, None)
        tracks = any(table.truthy[g] for g in np.flatnonzero(allowed))
        cols = (slot, group, len(table.dirs), ts, cls)
        cuts = [float(index.cut_f32(c)) for c in (min_score, min_partner)]
        idx, sc, total, pr, ps, n_partners = near_model(Sa, Sb, *cols, within, start, count, partners, cuts[1], value, allowed, cuts[0], tracks, ts_range,
                                                        classes, None, with_classes)
        res = [(table.paths[r], float(x), table.paths[p], float(y), int(ts[p]) - int(ts[r])) for r, x, p, y in zip(idx[0].tolist(), sc[0], pr[0].tolist(), ps[0])
               if r >= 0]
        counts, _, _ = near_timeline_model(Sa, Sb, *cols, within, 1000, 100, 8, partners, cuts[1], value, allowed, cuts[0], tracks, ts_range, classes, None,
                                           with_classes)
        return res, {"total": int(total[0]), "partners": min(n_partners, partners), "partners_left": max(n_partners - partners, 0)}, counts[0]

    questions = (
        dict(a=e0, b=e1, within=30, start=0, count=100, min_score=-1.0, min_partner=0.0),
        dict(a=e0, b=clicked, within=60, start=2, count=30, min_score=0.0, min_partner=0.1, value="a", cam_name="front"),
        dict(a=clicked, b=e1, within=15, start=0, count=50, min_score=-1.0, min_partner=-1.0, partners=7, with_classes=(0, 2)),
        dict(a=e1, b=e0, within=200, start=0, count=300, min_score=-1.0, min_partner=0.2, ts_range=(1000, 1500), classes=(0, 2)),
    )
    for ask in questions:
        res, info, hist = expect(**ask)
        assert info["total"] >= 5 and len(res) >= 3, ask
        got = f.together(**ask)
        assert got == (res, info), (storage, {k: v for k, v in ask.items() if k not in ("a", "b")})
        assert all(abs(dt) <= ask["within"] and p != q for p, _, q, _, dt in got[0])
        tl = {k: v for k, v in ask.items() if k not in ("start", "count")}
        counts, t = f.together_timeline(t0=1000, bin_seconds=100, n_bins=8, **tl)
        assert t == info["total"] and counts.dtype == np.int64 and np.array_equal(counts, hist), storage
    assert expect(**questions[2])[1]["partners_left"] > 0 and expect(**questions[2])[1]["partners"] == 7
    # a Term names its source itself; the endpoint's form of a stored crop is the crop
    url = "/" + os.path.relpath(clicked, root).replace(os.sep, "/")
    assert f.together(Term(embedding=e0), Term(path=url), within=60, min_score=0.0, min_partner=0.1) == f.together(e0, clicked, within=60, min_score=0.0, min_partner=0.1)
    # what is wrong with the question is said before any GPU work
    index.rank_near = index.timeline_near = None
    try:
        for bad, err in (((e0, os.path.join(root, "front", "objects", day_of(clicked), "nothing.jpg")), KeyError), ((e0[:512], e1), ValueError),
                         ((Term(text="a van", embedding=e0), e1), ValueError), ((e0, Term()), ValueError)):
            with pytest.raises(err):
                f.together(*bad)
            with pytest.raises(err):
                f.together_timeline(*bad)
        for kw in (dict(count=0), dict(within=-1), dict(value="max"), dict(partners=0), dict(min_partner=float("nan"))):
            with pytest.raises(ValueError):
                f.together(e0, e1, **kw)
    finally:
        del index.rank_near, index.timeline_near
    assert f.together(e0, e1, cam_name="nowhere") == ([], {"total": 0, "partners": 0, "partners_left": 0})


def day_of(path):
    return os.path.basename(os.path.dirname(path))
