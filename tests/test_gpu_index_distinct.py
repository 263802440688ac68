"""Distinct answers on the GPU: cc_index_gram / cc_index_distinct through EmbeddingIndex.gram / distinct / distinct_device and
ObjectFinder.search_page / similar with `distinct`.

`gram` is held to float64 (score_cases.order_free_bound of the stored rows), to bitwise symmetry and to depending on a pair's two rows
alone.  `distinct` is held to the numpy model of tests/distinct_cases.py run on the index's own `ix.gram(list)`: every comparison is
exact, idx, score, dups and total.  The worlds are distinct_cases.DupWorld: 8229 rows of 768 and of 256 in clusters, with byte-equal
copies and chains; tests/test_index_distinct_host.py holds the model to a double loop and checks that no pair of stored rows comes
near a threshold used here."""
import ctypes as C
import os

import numpy as np
import pytest

from distinct_cases import DEPTHS, DIMS, MAX_DEPTH, MAX_Q, SAME_AT, crafted_rows, distinct_model, exact, mask_rule, order_free_bound, world
from like_cases import stored
from where_cases import FILTERS, unit

pytestmark = pytest.mark.gpu

STORAGES = ("f32", "bf16", "i8")
_indices = {}


def index(dim, storage):
    from clearcam_amd.objects import EmbeddingIndex
    if (dim, storage) not in _indices:
        w = world(dim)
        ix = _indices[(dim, storage)] = EmbeddingIndex(dim, w.n, storage=storage)
        ix.add(w.E, w.group, w.slot, ts=w.ts, classes=w.cls)
    return _indices[(dim, storage)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gram_of(ix):
    """rows -> ix.gram(rows), remembered per list"""
    seen = {}

    def G_of(rows):
        key = np.asarray(rows, np.int64).tobytes()
        if key not in seen:
            seen[key] = ix.gram(rows)
        return seen[key]
    return G_of


def same(got, want, what):
    assert got[0].dtype == np.int32 and got[2].dtype == np.int32 and got[3].dtype == np.int64, what
    assert got[0].shape == want[0].shape == got[2].shape and got[3].shape == want[3].shape, what
    assert np.array_equal(got[3], want[3]), (what, "total", got[3], want[3])
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(got[2], want[2]), (what, "dups")
    if want[1] is None:
        assert got[1] is None, what
    else:
        assert got[1].dtype == np.float32 and np.array_equal(bits(got[1]), bits(want[1])), (what, "score")


def queries(w, Q, seed=3):
    """Q queries, each a stored row with fresh noise: the head of its ranking is that row's cluster"""
    rng = np.random.default_rng(seed)
    return unit(w.E[rng.choice(w.n, Q, replace=False)] + 0.2 * unit(rng.standard_normal((Q, w.dim))))


def windows(depth, total):
    """(start, count): the head, the middle, the last kept entry and past it; one answer and more than there are"""
    return sorted({(0, depth), (0, 1), (total // 2, 3), (max(total - 1, 0), 1), (max(total - 1, 0), 4), (total, 2), (0, depth + 5)})


def check_lists(ix, w, idx, sc, same_at, what, G_of=None):
    G_of = G_of or gram_of(ix)
    depth = idx.shape[1]
    full = distinct_model(idx, sc, G_of, same_at, 0, depth, w.n)
    for start, count in windows(depth, int(full[3][0])):
        want = distinct_model(idx, sc, G_of, same_at, start, count, w.n)
        same(ix.distinct(idx, sc, same_at, start, count), want, (what, start, count))
    want = distinct_model(idx, None, G_of, same_at, 0, depth, w.n)
    same(ix.distinct(idx, None, same_at), want, (what, "no score"))
    return full


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_gram_against_float64_and_symmetric_bit_for_bit(storage, dim):
    import torch
    from clearcam_amd import _lib
    w, ix = world(dim), index(dim, storage)
    D = stored(w.E, storage)
    rng = np.random.default_rng(5)
    for n in (1, 2, 17, 64, 65, 1024):
        rows = rng.integers(0, w.n, n)
        rows[0] = w.n - 1                                                      # the last row of the index
        if n > 2:
            rows[n // 2] = rows[1]; rows[-1] = w.n - 1                          # repeats
        got = ix.gram(rows)
        assert got.dtype == np.float32 and got.shape == (n, n)
        ex, bound = exact(D[rows], D[rows]), order_free_bound(D[rows], D[rows])
        assert (np.abs(got.astype(np.float64) - ex) <= bound).all(), (storage, dim, n, float((np.abs(got - ex) / bound).max()))
        assert np.array_equal(bits(got), bits(got.T)), (storage, dim, n)
        dev = ix.gram(rows, device_out=True)
        torch.cuda.synchronize()
        assert dev.is_cuda and np.array_equal(bits(dev.cpu().numpy()), bits(got))
    L = _lib.lib()
    for bad in ([w.n], [-1], [3, w.n, 4], [2 ** 40], list(range(MAX_DEPTH + 1))):
        ids = np.asarray(bad, np.int64)
        out = np.full((len(bad), len(bad)), 7.0, np.float32)
        assert L.cc_index_gram(ix._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), len(bad), _lib.ptr(out), 0, None) == -22 and L.cc_last_error()
        assert (out == 7.0).all()
    with pytest.raises(_lib.CCError):
        ix.gram([])
    assert ix.gram([1]).shape == (1, 1)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_a_pair_depends_on_its_two_rows_alone(storage):
    w, ix = world(768), index(768, storage)
    b = w.E.view(np.uint32)
    x = next(r for r in range(w.n - 1, 0, -1) if (b[:r] == b[r]).all(axis=1).any())          # a row that copies an earlier one
    copy = int(np.flatnonzero((b[:x] == b[x]).all(axis=1))[0])
    y = w.chains[0][1]
    pair = ix.gram([x, y])
    rng = np.random.default_rng(9)
    for first in (x, copy):
        rows = rng.integers(0, w.n, 1024)
        rows[1000], rows[3] = first, y
        G = ix.gram(rows)
        assert bits(G[1000, 3]) == bits(pair[0, 1]) == bits(G[3, 1000]) == bits(pair[1, 0]), (storage, first)
        assert bits(G[1000, 1000]) == bits(pair[0, 0]) and bits(G[3, 3]) == bits(pair[1, 1])
    assert pair[0, 1] != 0


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_distinct_equals_the_model_on_the_index_own_gram(storage):
    w, ix = world(768), index(768, storage)
    G_of = gram_of(ix)
    q3 = queries(w, 3)
    ts_range, classes, allowed = FILTERS["ts"]
    dropped = 0
    for k, depth in enumerate(DEPTHS):
        same_at = SAME_AT[k % len(SAME_AT)]
        idx, sc, _ = ix.rank(q3, 0, depth, tracks=False)
        full = check_lists(ix, w, idx, sc, same_at, (storage, "rank", depth), G_of)
        dropped += int(((idx >= 0).sum(axis=1) - full[3]).sum())
        idx, sc, _ = ix.rank(q3, 0, depth, allowed, tracks=bool(k & 1), ts_range=ts_range, classes=classes)
        check_lists(ix, w, idx, sc, same_at, (storage, "rank_where", depth), G_of)
        track = np.flatnonzero((w.slot == 0) & (w.group == w.group[np.flatnonzero(w.slot == 0)[0]]))[:9]      # rows of one folder and one track
        idx, sc, _ = ix.rank_like(track, 0, depth, tracks=False, exclude="track")
        check_lists(ix, w, idx, sc, same_at, (storage, "rank_like", depth), G_of)
    assert dropped > 100                                                       # the lists were full of near-duplicates
    idx, sc, _ = ix.rank(q3[:1], 0, 129, tracks=False)
    check_lists(ix, w, idx, sc, SAME_AT[0], (storage, "Q 1"), G_of)


@pytest.mark.parametrize("storage", STORAGES)
def test_sixty_four_lists_at_full_depth(storage):
    w, ix = world(256), index(256, storage)
    idx, sc, _ = ix.rank(queries(w, MAX_Q), 0, MAX_DEPTH, tracks=False)
    G_of = gram_of(ix)
    for start, count in ((0, MAX_DEPTH), (40, 100)):
        same(ix.distinct(idx, sc, SAME_AT[1], start, count), distinct_model(idx, sc, G_of, SAME_AT[1], start, count, w.n), (storage, start, count))
    idx, sc, _ = ix.rank(queries(w, MAX_Q, seed=4), 0, 65, tracks=True)
    same(ix.distinct(idx, sc, SAME_AT[2]), distinct_model(idx, sc, gram_of(ix), SAME_AT[2], 0, 65, w.n), (storage, "depth 65"))


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_edges_of_the_threshold_and_bad_entries(storage):
    w, ix = world(768), index(768, storage)
    G_of = gram_of(ix)
    a, b, c = w.chains[1]
    v = ix.gram([a, b])[0, 1]
    up = np.nextafter(v, np.float32(np.inf))
    oi, os_, od, total = ix.distinct([a, b], [0.5, 0.25], same_at=v)          # an actual value drops the pair
    assert oi.tolist() == [[a, -1]] and od.tolist() == [[1, 0]] and total.tolist() == [1] and os_[0, 0] == 0.5 and os_[0, 1] == -np.inf
    oi, os_, od, total = ix.distinct([a, b], [0.5, 0.25], same_at=up)         # the next float32 above it keeps it
    assert oi.tolist() == [[a, b]] and od.tolist() == [[0, 0]] and total.tolist() == [2] and os_.tolist() == [[0.5, 0.25]]
    idx, sc, _ = ix.rank(queries(w, 2, seed=6), 0, 200, tracks=False)
    G = G_of(idx[0])
    near = np.sort(np.unique(G[np.triu_indices(200, 1)]))[-40]                 # a similarity inside the list, among the largest
    for t in (near, np.nextafter(near, np.float32(np.inf))):
        same(ix.distinct(idx, sc, t), distinct_model(idx, sc, G_of, t, 0, 200, w.n), (storage, "a value of G", t))
    # bad entries: -1 in the middle, entries >= size, an all-absent list
    holes = idx.copy()
    holes[:, 5:9] = -1; holes[0, 50] = w.n; holes[0, 51] = 2 ** 31 - 1; holes[1, 0] = -7
    for t in (SAME_AT[0], np.inf, -np.inf):
        same(ix.distinct(holes, sc, t), distinct_model(holes, sc, G_of, t, 0, 200, w.n), (storage, "holes", t))
    present = ((holes >= 0) & (holes < w.n)).sum(axis=1)
    oi, os_, od, total = ix.distinct(holes, sc, np.inf)                        # +inf: the input with its absent entries squeezed out
    for q in range(2):
        ok = (holes[q] >= 0) & (holes[q] < w.n)
        assert oi[q, :present[q]].tolist() == holes[q, ok].tolist() and (oi[q, present[q]:] == -1).all() and total[q] == present[q] and not od.any()
        assert np.array_equal(os_[q, :present[q]], sc[q, ok]) and (os_[q, present[q]:] == -np.inf).all()
    oi, os_, od, total = ix.distinct(holes, sc, -np.inf)                       # -inf: the first present entry alone
    assert total.tolist() == [1, 1] and oi[:, 0].tolist() == [holes[0, 0], holes[1, 1]] and od[:, 0].tolist() == (present - 1).tolist()
    assert (oi[:, 1:] == -1).all() and not od[:, 1:].any()
    gone = np.stack([np.full(70, -1), np.full(70, w.n)]).astype(np.int32)
    oi, os_, od, total = ix.distinct(gone, np.ones((2, 70), np.float32), SAME_AT[0], 0, 5)
    assert total.tolist() == [0, 0] and (oi == -1).all() and (os_ == -np.inf).all() and not od.any()
    # one row number repeated: G of a row with itself, an ordinary pair
    rep = np.full((1, 130), a, np.int32)
    for t in (SAME_AT[0], np.inf):
        same(ix.distinct(rep, None, t), distinct_model(rep, None, G_of, t, 0, 130, w.n), (storage, "one row repeated", t))
    assert ix.distinct(rep, None, SAME_AT[0])[2][0, 0] == 129


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_crafted_exact_rows_sit_on_the_threshold_as_ge_says(storage, dim):
    from clearcam_amd.objects import EmbeddingIndex
    E, same_at = crafted_rows(dim)
    ix = EmbeddingIndex(dim, 16, storage=storage)
    ix.add(np.concatenate([E, world(dim).E[:5]]))
    G = ix.gram([0, 1, 2, 3])
    assert np.array_equal(G.astype(np.float64), E.astype(np.float64) @ E.astype(np.float64).T)    # exact, whatever the order
    assert G[0, 1] == same_at and G[0, 2] == np.nextafter(same_at, np.float32(0)) and G[0, 3] == np.nextafter(same_at, np.float32(2))
    oi, _, od, total = ix.distinct([0, 1, 2, 3], None, same_at)
    assert oi.tolist() == [[0, 2, -1, -1]] and od.tolist() == [[2, 0, 0, 0]] and total.tolist() == [2]     # equal: dropped; below: kept; above: dropped
    oi, _, od, total = ix.distinct([2, 7, 0, 3, 1], None, same_at)             # in another order, with a stranger between them
    assert oi.tolist() == [[2, 7, 0, -1, -1]] and od.tolist() == [[0, 0, 2, 0, 0]] and total.tolist() == [3]
    ix.close()


@pytest.mark.parametrize("storage", STORAGES)
def test_a_chain_comes_back_by_the_greedy_rule(storage):
    w, ix = world(768), index(768, storage)
    for (a, b, c), t in zip(w.chains, SAME_AT * 3):
        G = ix.gram([a, b, c])
        assert mask_rule(G, t).tolist() == [True, False, False]                  # the detector's rule would drop c as well
        oi, _, od, total = ix.distinct([a, b, c], None, t)
        assert oi.tolist() == [[a, c, -1]] and od.tolist() == [[1, 0, 0]] and total.tolist() == [2], (storage, a, t)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_form_equals_the_host_form(storage):
    import torch
    w, ix = world(768), index(768, storage)
    q = queries(w, 3, seed=8)
    for depth, start, count in ((300, 0, None), (1024, 10, 100)):
        di, ds, _ = ix.rank_device(q, 0, depth, tracks=False, with_total=False)
        hi, hs, _ = ix.rank(q, 0, depth, tracks=False)
        want = ix.distinct(hi, hs, SAME_AT[0], start, count)
        quiet = ix.distinct_device(di, ds, SAME_AT[0], start, count, with_total=False)
        asked = ix.distinct_device(di, ds, SAME_AT[0], start, count)
        torch.cuda.synchronize()
        assert quiet[3] is None and all(t.is_cuda for t in quiet[:3])
        for got in (quiet, asked):
            same((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), want[3] if got[3] is None else got[3]), want, (storage, depth))
        bare = ix.distinct_device(di, None, SAME_AT[0], start, count)
        assert bare[1] is None and np.array_equal(bare[0].cpu().numpy(), want[0]) and np.array_equal(bare[3], want[3])
    li, ls, _ = ix.rank_like_device([w.chains[2][0]], 0, 64, tracks=False)
    got = ix.distinct_device(li, ls, SAME_AT[2])
    hi, hs, _ = ix.rank_like([w.chains[2][0]], 0, 64, tracks=False)
    same((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), got[3]), distinct_model(hi, hs, gram_of(ix), SAME_AT[2], 0, 64, w.n), storage)


@pytest.mark.parametrize("storage", STORAGES)
def test_the_first_call_on_a_fresh_handle_reads_only_bits_it_wrote(storage):
    """A fresh handle thins a long list first (every bit the walk reads comes from that call's Gram epilogue), then shorter lists with
    another threshold over the stale bit matrix of the long one, then more lists than before (the scratch grows)."""
    import torch
    from clearcam_amd.objects import EmbeddingIndex
    w = world(256)
    fresh = EmbeddingIndex(256, w.n, storage=storage)
    fresh.add(w.E, w.group, w.slot, ts=w.ts, classes=w.cls)
    G_of = gram_of(index(256, storage))                                        # the same rows in another handle: the same bits
    hi, hs, _ = index(256, storage).rank(queries(w, 5, seed=11), 0, MAX_DEPTH, tracks=False)
    for lists, depth, t in ((slice(0, 1), MAX_DEPTH, SAME_AT[2]), (slice(1, 2), 70, SAME_AT[0]), (slice(0, 5), 700, SAME_AT[1]), (slice(2, 3), 65, np.float32(-np.inf))):
        idx, sc = np.ascontiguousarray(hi[lists, :depth]), np.ascontiguousarray(hs[lists, :depth])
        got = fresh.distinct_device(torch.as_tensor(idx).cuda(), torch.as_tensor(sc).cuda(), t)
        same((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy(), got[3]), distinct_model(idx, sc, G_of, t, 0, depth, w.n), (storage, depth))
    fresh.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_index_answering():
    from clearcam_amd import _lib
    w, ix = world(768), index(768, "f32")
    L = _lib.lib()
    idx, sc, _ = ix.rank(queries(w, 2), 0, 100, tracks=False)

    def call(Q=2, depth=100, same_at=0.9, start=0, count=100, total=True):
        oi, os_, od = np.full((2, 100), 7, np.int32), np.full((2, 100), 7, np.float32), np.full((2, 100), 7, np.int32)
        tot = np.full(2, 7, np.int64)
        rc = L.cc_index_distinct(ix._h, _lib.ptr(idx), _lib.ptr(sc), Q, depth, same_at, start, count, _lib.ptr(oi), _lib.ptr(os_), _lib.ptr(od),
                                 _lib.ptr(tot) if total else None, 0, None)
        return rc, (oi == 7).all() and (os_ == 7).all() and (od == 7).all() and (tot == 7).all()
    bad = {"NaN same_at": dict(same_at=float("nan")), "depth 0": dict(depth=0), "depth 1025": dict(depth=MAX_DEPTH + 1), "Q 0": dict(Q=0),
           "Q 65": dict(Q=MAX_Q + 1), "start -1": dict(start=-1), "count 0": dict(count=0), "count -3": dict(count=-3)}
    for what, kw in bad.items():
        rc, untouched = call(**kw)
        assert rc == -22 and untouched and L.cc_last_error(), what
    rc, untouched = call()
    assert rc == 0 and not untouched
    for f in (lambda: ix.distinct(idx, sc, float("nan")), lambda: ix.distinct(np.zeros((1, MAX_DEPTH + 1), np.int32)), lambda: ix.distinct(idx, sc, 0.9, -1),
              lambda: ix.distinct(idx, sc, 0.9, 0, 0), lambda: ix.distinct(np.zeros((MAX_Q + 1, 4), np.int32))):
        with pytest.raises(_lib.CCError):
            f()
    again = ix.rank(queries(w, 2), 0, 100, tracks=False)
    assert np.array_equal(again[0], idx) and np.array_equal(bits(again[1]), bits(sc))
    same(ix.distinct(idx, sc, SAME_AT[0]), distinct_model(idx, sc, gram_of(ix), SAME_AT[0], 0, 100, w.n), "after the errors")


# 7 ---------------------------------------------------------------------------------------------------------------------------------
CAMS, DAYS = ("back", "front"), ("2026-01-01", "2026-01-02", "2026-01-03")
VAN_TRACKS = 9


def van_spec(bad_name=False):
    """(camera, day) -> [(name, vector)]: 6 folders x 30 crops of unrelated things (random directions: nothing alike) and one van, seen
    under VAN_TRACKS track ids spread over the folders, two crops per track, all within cosine 0.97 of one another."""
    rng = np.random.default_rng(17)
    van = unit(rng.standard_normal(768))
    out = {(cam, day): [(f"{1000 + 13 * i}.5_{500 + 40 * k + i}_{(0, 2, 7)[i % 3]}.jpg", unit(rng.standard_normal(768))) for i in range(30)]
           for k, (cam, day) in enumerate((c, d) for c in CAMS for d in DAYS)}
    keys = list(out)
    for t in range(VAN_TRACKS):
        for shot in range(2):
            v = unit(van + 0.08 * unit(rng.standard_normal(768)))
            out[keys[t % len(keys)]].append((f"{5000 + 100 * t + shot}.5_{100 + t}_2.jpg", v))
    if bad_name:
        out[("front", DAYS[1])].append(("50000.5_x_2.jpg", unit(rng.standard_normal(768))))
    return van, out


def attach(root, folders, storage):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    for (cam, day), crops in folders.items():
        d = os.path.join(root, cam, "objects", day)
        EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    f = ObjectFinder(root)
    f.index_storage = storage
    f.attach_store(capacity=64)
    return f


def thinned(index, table, plain, same_at, depth, start, count):
    """The model over a plain page's first `depth` answers -> what the call with `distinct` returns"""
    head = plain[:depth]
    rows = np.array([[table.row_of(p) for p, _ in head]], np.int64)
    sc = np.array([[v for _, v in head]], np.float32)
    oi, os_, od, total = distinct_model(rows, sc, gram_of(index), same_at, start, min(count, len(head)), len(table.paths))
    return [(table.paths[r], float(v), int(d)) for r, v, d in zip(oi[0], os_[0], od[0]) if r >= 0], int(total[0])


@pytest.mark.parametrize("storage", STORAGES)
def test_object_finder_pages_without_near_duplicates(tmp_path, storage):
    van, folders = van_spec()
    f = attach(str(tmp_path / "cameras"), folders, storage)
    index, table = f._dev["store"]
    assert index.storage == storage
    plain, n_plain = f.search_page(text_embedding=van, count=1000)
    assert f.search_page(text_embedding=van, count=1000, distinct=None) == (plain, n_plain)          # None: exactly today's call
    assert [("_1" in os.path.basename(p)) and v > 0.9 for p, v in plain[:VAN_TRACKS]] == [True] * VAN_TRACKS   # the first page today: the van, nine times
    got, total = f.search_page(text_embedding=van, count=1000, distinct=0.9)
    assert got[0][:2] == plain[0] and got[0][2] == VAN_TRACKS - 1                   # once, with its other tracks folded into it
    assert all(d == 0 for _, _, d in got[1:]) and total == len(got) == n_plain - (VAN_TRACKS - 1)
    for kw in (dict(), dict(start=1, count=5), dict(start=0, count=3, distinct_depth=20), dict(cam_name="front", min_score=-0.05), dict(classes=(2,), timestamp=DAYS[0])):
        depth = kw.get("distinct_depth", 1024)
        base = {k: v for k, v in kw.items() if k not in ("start", "count", "distinct_depth")}
        plain, _ = f.search_page(text_embedding=van, count=1000, **base)
        want = thinned(index, table, plain, 0.9, depth, kw.get("start", 0), kw.get("count", 100))
        assert f.search_page(text_embedding=van, distinct=0.9, **kw) == want, (storage, kw)
    # more like one crop of the van, the whole track asking and standing aside: its other tracks answer once
    clicked = next(p for p in table.paths if os.path.basename(p).startswith("5000.5_100_"))
    plain, _ = f.similar(clicked, whole_track=True, exclude="track", count=1000)
    assert f.similar(clicked, whole_track=True, exclude="track", count=1000, distinct=None)[0] == plain
    got, total = f.similar(clicked, whole_track=True, exclude="track", count=1000, distinct=0.9)
    assert (got, total) == thinned(index, table, plain, 0.9, 1024, 0, 1000)
    assert got[0][:2] == plain[0] and got[0][2] == VAN_TRACKS - 2 and "_100_" not in got[0][0]
    for bad in (dict(distinct=float("nan")), dict(distinct=0.9, distinct_depth=0), dict(distinct=0.9, distinct_depth=1025)):
        with pytest.raises(ValueError):
            f.search_page(text_embedding=van, **bad)
        with pytest.raises(ValueError):
            f.similar(clicked, **bad)


def test_object_finder_thins_the_host_ranked_list_too(tmp_path, monkeypatch):
    from clearcam_amd.objects import EmbeddingIndex
    van, folders = van_spec(bad_name=True)
    f = attach(str(tmp_path / "cameras"), folders, "f32")
    index, table = f._dev["store"]
    calls = {"distinct": 0, "distinct_device": 0}
    for name in calls:
        def counted(ix, *a, _fn=getattr(EmbeddingIndex, name), _name=name, **kw):
            calls[_name] += 1
            return _fn(ix, *a, **kw)
        monkeypatch.setattr(EmbeddingIndex, name, counted)
    with pytest.raises(ValueError):
        f.search_page(text_embedding=van, distinct=0.9)                        # the unparsable name still raises like the reference
    kw = dict(text_embedding=van, classes=(2,))                                # a row filter hides it: ranked on the host
    plain, _ = f.search_page(count=1000, **kw)
    got = f.search_page(count=1000, distinct=0.9, **kw)
    assert calls == {"distinct": 1, "distinct_device": 0}
    assert got == thinned(index, table, plain, 0.9, 1024, 0, 1000) and got[0][0][2] == VAN_TRACKS - 1
    assert f.search_page(start=2, count=4, distinct=0.9, distinct_depth=15, **kw) == thinned(index, table, plain, 0.9, 15, 2, 4)
    clicked = next(p for p in table.paths if os.path.basename(p).startswith("5000.5_100_"))
    plain, _ = f.similar(clicked, whole_track=True, exclude="track", count=1000, classes=(2,))
    got = f.similar(clicked, whole_track=True, exclude="track", count=1000, classes=(2,), distinct=0.9)
    assert got == thinned(index, table, plain, 0.9, 1024, 0, 1000) and got[0][0][2] == VAN_TRACKS - 2
    assert calls == {"distinct": 3, "distinct_device": 0}
