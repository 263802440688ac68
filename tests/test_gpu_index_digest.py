"""Day digest on the GPU: cc_index_digest through EmbeddingIndex.digest / digest_device and ObjectFinder.digest.

The device is held to the numpy model of tests/digest_cases.py, element for element: rows, counts, ts_first / ts_last, totals and owner.
The model compares rounded float64 dot products of the stored rows, the device the float cc_index_gram computes; the two agree because no
pair of stored rows of the worlds comes near a threshold used here (tests/test_index_digest_host.py), and on distinct_cases.crafted_rows
because every product and partial sum is exact.  The worlds are distinct_cases.DupWorld: 8229 rows of 768 and of 256, nine pieces."""
import ctypes as C
import os

import numpy as np
import pytest

from digest_cases import (DIMS, FILTERS, LEFT_OVER, MAX_LEADERS, NO_TS, NOT_COMPETING, SAME_AT, STORAGES, competing, crafted_rows, digest_model,
                          similarities, stored, world, world_similarities)
from where_cases import unit

pytestmark = pytest.mark.gpu

BY = ("count", "first")
_indices = {}


def index(dim, storage):
    from clearcam_amd.objects import EmbeddingIndex
    if (dim, storage) not in _indices:
        w = world(dim)
        ix = _indices[(dim, storage)] = EmbeddingIndex(dim, w.n, storage=storage)
        ix.add(w.E, w.group, w.slot, ts=w.ts, classes=w.cls)
    return _indices[(dim, storage)]


def index_of(E, storage, **kw):
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(E.shape[1], len(E), storage=storage)
    ix.add(E, **kw)
    return ix


def same(got, want, what):
    names = ("rows", "counts", "ts_first", "ts_last", "totals", "owner")
    assert len(got) == len(want), what
    for name, g, x in zip(names, got, want):
        assert g.dtype == (np.int64 if name == "totals" else np.int32) and g.shape == x.shape, (what, name, g.dtype, g.shape, x.shape)
        assert np.array_equal(g, x), (what, name, np.flatnonzero(g != x)[:8], g[g != x][:8], x[g != x][:8])


def windows(k):
    """(start, count): the head, the middle, the last leader and past it, and more than there are"""
    return sorted({(0, 1), (k // 2, 3), (max(k - 1, 0), 1), (max(k - 1, 0), 4), (k, 2), (0, k + 5)})


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_equals_the_model(storage, dim):
    w, ix = world(dim), index(dim, storage)
    S, D = world_similarities(dim, storage), stored(w.E, storage)
    for name in (None,) + tuple(FILTERS):
        rows, kw = competing(w, name)
        Ss = S[np.ix_(rows, rows)]
        for same_at in SAME_AT:
            for by in BY:
                want = digest_model(D, rows, same_at, MAX_LEADERS, by, 0, MAX_LEADERS, ts=w.ts, S=Ss)
                same(ix.digest(same_at, by=by, owners=True, **kw), want, (storage, dim, name, same_at, by))
        for by in BY:
            for start, count in windows(int(want[4][0])):
                want_w = digest_model(D, rows, SAME_AT[-1], MAX_LEADERS, by, start, count, ts=w.ts, S=Ss)
                same(ix.digest(SAME_AT[-1], start, count, by=by, **kw), want_w[:5], (storage, dim, name, by, start, count))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_piece_boundaries_and_caps(storage):
    w = world(768)
    S = world_similarities(768, storage)
    for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049):
        ix = index_of(w.E[:n], storage, ts=w.ts[:n])
        D = stored(w.E[:n], storage)
        for cap in (1, 63, 64, 65, 1024):
            for same_at in (0.95, 0.90):
                want = digest_model(D, np.arange(n), same_at, cap, "count", 0, cap, ts=w.ts[:n], S=S[:n, :n])
                same(ix.digest(same_at, max_leaders=cap, owners=True), want, (storage, n, cap, same_at))
        if n >= 1023:
            assert want[4][0] > 65                                                 # at 0.90 the smaller caps were reached inside a piece
        ix.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_in_a_chain_the_middle_joins_the_first_and_the_last_leads(storage):
    w = world(768)
    at = np.array([r for c in w.chains for r in c])
    ix = index_of(w.E[at], storage, groups=np.repeat(np.arange(len(w.chains)), 3).astype(np.int32))
    for k in range(len(w.chains)):
        allowed = np.zeros(len(w.chains), np.uint8)
        allowed[k] = 1
        for same_at in SAME_AT:
            rows, counts, _, _, totals, owner = ix.digest(same_at, count=3, allowed=allowed, owners=True)
            assert rows.tolist() == [3 * k, 3 * k + 2, -1] and counts.tolist() == [2, 1, 0] and totals.tolist() == [2, 3, 0], (storage, k, same_at)
            want = np.full(len(at), NOT_COMPETING, np.int32)
            want[3 * k:3 * k + 3] = (3 * k, 3 * k, 3 * k + 2)
            assert np.array_equal(owner, want)
    ix.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_a_threshold_that_is_a_pairs_value(storage, dim):
    """A, B=, B-, B+ with A.B= == same_at, A.B- one ulp below, A.B+ one ulp above, every product exact: equal joins, below leads, above joins"""
    E, same_at = crafted_rows(dim)
    for order in ((0, 1, 2, 3), (2, 0, 3, 1), (3, 2, 1, 0), (1, 3, 0, 2)):
        P = E[list(order)]
        ix = index_of(P, storage)
        want = digest_model(stored(P, storage), np.arange(4), same_at, MAX_LEADERS, "first", 0, 4)
        got = ix.digest(float(same_at), count=4, by="first", owners=True)
        same(got, want, (storage, dim, order))
        if order == (0, 1, 2, 3):
            assert got[5].tolist() == [0, 0, 2, 0] and got[0].tolist() == [0, 2, -1, -1] and got[1].tolist() == [3, 1, 0, 0]
        ix.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_thresholds_empty_selections_and_rows_without_ts(storage):
    w, ix = world(768), index(768, storage)
    n = w.n
    rows, counts, t0, t1, totals, owner = ix.digest(np.inf, count=MAX_LEADERS + 3, owners=True)
    assert totals.tolist() == [MAX_LEADERS, n, n - MAX_LEADERS]                    # every row a leader up to the cap
    assert np.array_equal(rows[:MAX_LEADERS], np.arange(MAX_LEADERS)) and (counts[:MAX_LEADERS] == 1).all() and (rows[MAX_LEADERS:] == -1).all()
    assert np.array_equal(t0[:MAX_LEADERS], w.ts[:MAX_LEADERS]) and np.array_equal(t1[:MAX_LEADERS], w.ts[:MAX_LEADERS])
    assert np.array_equal(owner[:MAX_LEADERS], np.arange(MAX_LEADERS)) and (owner[MAX_LEADERS:] == LEFT_OVER).all()
    has = w.ts[w.ts != NO_TS]
    got = ix.digest(-np.inf, count=2, owners=True)                                 # one leader owns all
    assert [g.tolist() for g in got[:5]] == [[0, -1], [n, 0], [has.min(), NO_TS], [has.max(), NO_TS], [1, n, 0]] and (got[5] == 0).all()
    got = ix.digest(0.9, count=3, allowed=np.zeros(5, np.uint8), owners=True)      # nothing competes
    assert [g.tolist() for g in got[:5]] == [[-1] * 3, [0] * 3, [NO_TS] * 3, [NO_TS] * 3, [0, 0, 0]] and (got[5] == NOT_COMPETING).all()
    # byte-equal copies join the leader of their original (0.90: nothing is left over)
    owner = ix.digest(0.90, owners=True)[5]
    _, first, inverse = np.unique(w.E.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    original = first[inverse.reshape(-1)]
    assert (original != np.arange(n)).sum() > 500 and np.array_equal(owner, owner[original])
    one = index_of(w.E[:1], storage)                                               # an index of one row, without ts
    got = one.digest(0.9, count=2, owners=True)
    assert [g.tolist() for g in got] == [[0, -1], [1, 0], [NO_TS, NO_TS], [NO_TS, NO_TS], [1, 1, 0], [0]]
    one.close()
    bare = index_of(w.E[:200], storage)                                            # no row has a ts
    got = bare.digest(0.9)
    assert got[4][0] > 0 and (got[2] == NO_TS).all() and (got[3] == NO_TS).all()
    bare.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_form_equals_the_host_form(storage):
    import torch
    ix = index(768, storage)
    _, kw = competing(world(768), "both+allowed")
    for args in (dict(same_at=0.92), dict(same_at=0.90, start=5, count=40, by="first", **kw), dict(same_at=0.95, max_leaders=100, count=120)):
        want = ix.digest(owners=True, **args)
        got = ix.digest_device(owners=True, **args)
        assert all(t.is_cuda and t.dtype == torch.int32 for t in got[:4] + got[5:]) and isinstance(got[4], np.ndarray)
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() if hasattr(t, "cpu") else t for t in got), want, (storage, args))
        got = ix.digest_device(with_total=False, **args)
        assert len(got) == 5 and got[4] is None and all(t.is_cuda for t in got[:4])
        torch.cuda.synchronize()
        same(tuple(t.cpu().numpy() for t in got[:4]), want[:4], (storage, args, "no total"))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_a_fresh_handle_and_stale_scratch():
    w = world(768)
    other = index(768, "bf16")
    ix = index_of(w.E, "bf16", groups=w.group, tracks=w.slot, ts=w.ts, classes=w.cls)
    S, D = world_similarities(768, "bf16"), stored(w.E, "bf16")
    same(ix.digest(0.92, owners=True), digest_model(D, np.arange(w.n), 0.92, MAX_LEADERS, "count", 0, MAX_LEADERS, ts=w.ts, S=S), "long")
    rows, kw = competing(w, "both+allowed")                                        # shorter, another threshold: over the stale scratch
    want = digest_model(D, rows, 0.95, 70, "first", 0, 70, ts=w.ts, S=S[np.ix_(rows, rows)])
    same(ix.digest(0.95, max_leaders=70, by="first", owners=True, **kw), want, "short")
    q = unit(w.E[[5, 900]] + 0.2 * unit(np.random.default_rng(1).standard_normal((2, 768))))
    a, b = ix.rank(q, 0, 100, tracks=False), other.rank(q, 0, 100, tracks=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2])
    da, db = ix.distinct(a[0], a[1], 0.9), other.distinct(b[0], b[1], 0.9)
    assert all(np.array_equal(x, y) for x, y in zip(da, db))
    ix.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_leave_the_index_answering():
    from clearcam_amd import _lib
    w, ix = world(768), index(768, "f32")
    L = _lib.lib()
    q = unit(w.E[[7, 4000]] + 0.2 * unit(np.random.default_rng(2).standard_normal((2, 768))))
    before = ix.rank(q, 0, 100, tracks=False)
    thinned = ix.distinct(before[0], before[1], 0.9)
    al = np.ones(5, np.uint8)

    def call(same_at=0.9, cap=MAX_LEADERS, order=0, allowed=None, n_groups=0, where=None, start=0, count=10, out_row=True):
        outs = [np.full(10, 7, np.int32) for _ in range(4)]
        owner, totals = np.full(w.n, 7, np.int32), np.full(3, 7, np.int64)
        rc = L.cc_index_digest(ix._h, same_at, cap, order, _lib.ptr(allowed), n_groups, C.byref(where) if where is not None else None, start, count,
                               _lib.ptr(outs[0]) if out_row else None, _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(outs[3]), _lib.ptr(owner),
                               _lib.ptr(totals), 0, None)
        return rc, all((o == 7).all() for o in outs + [owner, totals])
    empty_window, no_class = _lib.RowFilter(), _lib.RowFilter()
    empty_window.use_ts, empty_window.ts_min, empty_window.ts_max = 1, 5, 4
    no_class.use_cls = 1
    bad = {"NaN same_at": dict(same_at=float("nan")), "cap 0": dict(cap=0), "cap 1025": dict(cap=MAX_LEADERS + 1), "order 2": dict(order=2),
           "order -1": dict(order=-1), "start -1": dict(start=-1), "count 0": dict(count=0), "count -3": dict(count=-3), "no out_row": dict(out_row=False),
           "n_groups 0": dict(allowed=al, n_groups=0), "n_groups -1": dict(allowed=al, n_groups=-1), "n_groups 2^24 + 1": dict(allowed=al, n_groups=(1 << 24) + 1),
           "empty window": dict(where=empty_window), "empty class set": dict(where=no_class)}
    for what, kw in bad.items():
        rc, untouched = call(**kw)
        assert rc == -22 and untouched and L.cc_last_error(), what
    rc, untouched = call(allowed=al, n_groups=5)
    assert rc == 0 and not untouched
    for f in (lambda: ix.digest(float("nan")), lambda: ix.digest(0.9, max_leaders=0), lambda: ix.digest(0.9, -1), lambda: ix.digest(0.9, 0, 0),
              lambda: ix.digest_device(0.9, max_leaders=MAX_LEADERS + 1)):
        with pytest.raises(_lib.CCError):
            f()
    for f in (lambda: ix.digest(0.9, by="score"), lambda: ix.digest(0.9, ts_range=(5, 4)), lambda: ix.digest(0.9, classes=[])):
        with pytest.raises(ValueError):
            f()
    again = ix.rank(q, 0, 100, tracks=False)
    assert np.array_equal(again[0], before[0]) and np.array_equal(bits(again[1]), bits(before[1])) and np.array_equal(again[2], before[2])
    assert all(np.array_equal(x, y) for x, y in zip(ix.distinct(again[0], again[1], 0.9), thinned))


# 9 ---------------------------------------------------------------------------------------------------------------------------------
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


def finder_model(index, table, same_at, start, count, by, cam=None, day=None, ts_range=None, classes=None):
    """The model over the rows of the table that compete -> what ObjectFinder.digest returns"""
    from clearcam_amd.objects import row_filter
    n = len(table.paths)
    ok = table.allowed(cam, day)[np.asarray(table.group)].astype(bool) & table.passing(row_filter(ts_range, classes))
    r, c, t0, t1, totals, _ = digest_model(index.fetch(np.arange(n)), np.flatnonzero(ok), same_at, MAX_LEADERS, by, start, count, ts=np.asarray(table.ts))
    entries = [(table.paths[i], int(k), None if a == NO_TS else int(a), None if b == NO_TS else int(b)) for i, k, a, b in zip(r, c, t0, t1) if i >= 0]
    return entries, {"objects": int(totals[0]), "crops": int(totals[1]), "left_over": int(totals[2])}


@pytest.mark.parametrize("storage", STORAGES)
def test_object_finder_digests_the_folders(tmp_path, storage):
    _, folders = van_spec()
    f = attach(str(tmp_path / "cameras"), folders, storage)
    index, table = f._dev["store"]
    n = len(table.paths)
    got, info = f.digest(count=1000)
    assert info == {"objects": n - 2 * VAN_TRACKS + 1, "crops": n, "left_over": 0} and len(got) == info["objects"]
    van_rows = [r for r, p in enumerate(table.paths) if os.path.basename(p).split("_")[1] in {str(100 + t) for t in range(VAN_TRACKS)}]
    seen = [int(float(os.path.basename(table.paths[r]).split("_")[0])) for r in van_rows]
    assert got[0] == (table.paths[van_rows[0]], 2 * VAN_TRACKS, min(seen), max(seen)) == (got[0][0], 18, 5000, 5801)   # the van: once
    assert all(c == 1 and a == b == int(float(os.path.basename(p).split("_")[0])) for p, c, a, b in got[1:])
    for kw in (dict(), dict(start=1, count=5), dict(by="first", count=1000), dict(cam_name="front"), dict(timestamp=DAYS[1], count=1000),
               dict(cam_name="back", timestamp=DAYS[0], classes=(2,), same_at=0.99), dict(ts_range=(1100, 5300), classes=(2, 7), by="first")):
        want = finder_model(index, table, kw.get("same_at", 0.9), kw.get("start", 0), kw.get("count", 100), kw.get("by", "count"), kw.get("cam_name"),
                            kw.get("timestamp"), kw.get("ts_range"), kw.get("classes"))
        assert f.digest(**kw) == want, (storage, kw)
    assert f.digest(cam_name="nowhere") == ([], {"objects": 0, "crops": 0, "left_over": 0})
    for bad in (dict(same_at=float("nan")), dict(start=-1), dict(count=0), dict(by="score"), dict(ts_range=(5, 4))):
        with pytest.raises(ValueError):
            f.digest(**bad)


def test_object_finder_digests_faces_and_raises_on_unparsable_names(tmp_path):
    from clearcam_amd.objects import ObjectFinder
    rng = np.random.default_rng(23)
    base = str(tmp_path / "cameras")
    f = ObjectFinder(base)
    who = unit(rng.standard_normal((4, 512)))
    faces = {f"{base}/front/faces/{DAYS[0]}/{100 + 7 * i}.0_{i}_0.jpg": unit(who[i % 4] + 0.05 * unit(rng.standard_normal(512)))[None] for i in range(40)}
    f.face_embeddings = faces
    got, info = f.digest(is_face=True, same_at=0.9)
    findex, ftable = f._index_and_table(True)
    assert findex.dim == 512 and info == {"objects": 4, "crops": 40, "left_over": 0}
    assert (got, info) == finder_model(findex, ftable, 0.9, 0, 100, "count")
    assert [c for _, c, _, _ in got] == [10] * 4 and got[0][2:] == (100, 100 + 7 * 36)
    _, folders = van_spec(bad_name=True)
    g = attach(str(tmp_path / "second" / "cameras"), folders, "f32")
    with pytest.raises(ValueError):
        g.digest()                                                                 # the unparsable name competes: raises like `search`
    with pytest.raises(ValueError):
        g.digest(cam_name="front", timestamp=DAYS[1])
    index, table = g._dev["store"]
    assert g.digest(cam_name="back") == finder_model(index, table, 0.9, 0, 100, "count", cam="back")   # its folder is not asked for
    assert g.digest(ts_range=(0, 40000)) == finder_model(index, table, 0.9, 0, 100, "count", ts_range=(0, 40000))   # a row filter hides it
