"""Seen before on the GPU: cc_index_sightings through EmbeddingIndex.sightings / sightings_device and ObjectFinder.seen_before.

Most tests hold the device to the model of tests/sightings_cases.py run on the device's OWN pair values - `ix.gram` over chunks of the
objects plus up to 512 competing rows - so every output must be equal, best_score bit for bit: a pair's value may not depend on the tile,
the side, the kernel or the rest of the launch.  One test per storage holds 1024 objects to the float64 model instead; no pair of stored
rows comes near a threshold used there (tests/test_index_sightings_host.py).  The worlds are distinct_cases.DupWorld, 8229 rows."""
import ctypes as C
import os

import numpy as np
import pytest

from sightings_cases import (DIMS, GROUPS, MAX_GROUPS, MAX_OBJECTS, SAME_AT, SMALL_GROUP_COUNTS, STORAGES, competing, crafted_rows, object_sets,
                             order_free_bound, pair_values, sightings_model, stored, world)
from where_cases import unit

pytestmark = pytest.mark.gpu

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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_pairs(ix, rows, comp):
    """(n, m) float32: element [i][j] of `ix.gram` over (rows[i], comp[j]), from calls of at most 512 objects plus 512 competing rows"""
    rows, comp = np.asarray(rows, np.int64), np.asarray(comp, np.int64)
    G = np.empty((len(rows), len(comp)), np.float32)
    for a in range(0, len(rows), 512):
        for b in range(0, len(comp), 512):
            ra, cb = rows[a:a + 512], comp[b:b + 512]
            G[a:a + 512, b:b + 512] = ix.gram(np.concatenate([ra, cb]))[:len(ra), len(ra):]
    return G


def same(got, want, what):
    assert len(got) == len(want) == 5, what
    for name, g, x, dt in zip(("count", "best_row", "best_score", "group_counts"), got, want, (np.int32, np.int32, np.float32, np.uint32)):
        if x is None:
            assert g is None, (what, name)
            continue
        assert g.dtype == dt and g.shape == x.shape, (what, name, g.dtype, g.shape, x.shape)
        a, b = (bits(g), bits(x)) if name == "best_score" else (g, x)
        assert np.array_equal(a, b), (what, name, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:8], g[a != b][:8], x[a != b][:8])
    assert got[4] == want[4], (what, "total", got[4], want[4])


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_every_output_equals_the_model_on_the_devices_own_gram(storage, dim):
    w, ix = world(dim), index(dim, storage)
    D = stored(w.E, storage)
    rows65 = object_sets(w, 65)
    G65 = device_pairs(ix, rows65, np.arange(w.n))
    ties = 0
    for n in (1, 2, 63, 64, 65):
        rows = rows65[:n]
        for name in (None, "ts", "both+allowed"):
            comp, kw = competing(w, name)
            G = G65[:n][:, comp]
            for skip_self in (False, True):
                for same_at, ngc in ((SAME_AT[-1], GROUPS), (SAME_AT[0], 0)):
                    want = sightings_model(D, rows, comp, same_at, skip_self, w.group, ngc, G=G)
                    got = ix.sightings(rows, same_at, skip_self=skip_self, group_counts=ngc, **kw)
                    same(got, want, (storage, dim, n, name, skip_self, same_at))
            for i in (0, n - 1):                                                        # the best score is the Gram value of that very pair
                if got[1][i] >= 0:
                    assert bits(got[2][i]) == bits(ix.gram([rows[i], got[1][i]])[0, 1]), (storage, dim, n, name, i)
            plain = ix.sightings(rows, SAME_AT[0], **kw)
            top = bits(G) == bits(plain[2])[:, None]
            for i in np.flatnonzero(top.sum(axis=1) > 1):                              # a copy and its original: ties resolve to the lowest row
                assert plain[1][i] == comp[top[i]].min()
                ties += 1
    assert ties > 0


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_1024_objects_against_the_float64_model(storage):
    w, ix = world(768), index(768, storage)
    D = stored(w.E, storage).astype(np.float64)
    rows = object_sets(w, MAX_OBJECTS)
    comp = np.arange(w.n)
    exact = D[rows] @ D.T
    bound = order_free_bound(D[rows], D)
    for same_at, skip_self in ((SAME_AT[0], False), (SAME_AT[1], True), (SAME_AT[2], False)):
        want = sightings_model(D, rows, comp, same_at, skip_self, w.group, GROUPS, G=exact.astype(np.float32))
        got = ix.sightings(rows, same_at, skip_self=skip_self, group_counts=GROUPS)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]) and got[4] == w.n, (storage, same_at)
        assert (got[3].sum(axis=1) == got[0]).all() and (same_at != SAME_AT[2] or got[0].max() >= 40)
        alive = np.where(rows[:, None] != comp[None, :], exact, -np.inf) if skip_self else exact
        i = np.arange(len(rows))
        assert (got[1] >= 0).all()
        assert (np.abs(got[2].astype(np.float64) - exact[i, got[1]]) <= bound[i, got[1]]).all(), (storage, same_at)
        assert (alive[i, got[1]] >= alive.max(axis=1) - 2 * bound.max(axis=1)).all(), (storage, same_at)
        if skip_self:
            assert (got[1] != rows).all()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_small_indices_and_an_empty_competing_set(storage):
    w = world(768)
    for m in (1, 63, 64, 65, 129, 1025):
        group = (np.arange(m) // 200).astype(np.int32)                                 # folders are contiguous: strips of one group and mixed ones, group 5 past the counts
        ix = index_of(w.E[:m], storage, groups=group, ts=w.ts[:m], classes=w.cls[:m])
        D = stored(w.E[:m], storage)
        rows = np.unique(np.array([0, m - 1, m // 2, min(m - 1, 64), min(m - 1, 127), min(m - 1, 128)]))[::-1].copy()
        G = device_pairs(ix, rows, np.arange(m))
        for skip_self in (False, True):
            want = sightings_model(D, rows, np.arange(m), SAME_AT[-1], skip_self, group, GROUPS, G=G)
            same(ix.sightings(rows, SAME_AT[-1], skip_self=skip_self, group_counts=GROUPS), want, (storage, m, skip_self))
        if m == 1:
            assert [g.tolist() for g in ix.sightings([0], 0.9, skip_self=True)[:3]] == [[0], [-1], [-np.inf]]
        ix.close()
    ix = index(768, storage)
    rows = object_sets(w, 70)
    for kw in (dict(allowed=np.zeros(5, np.uint8)), dict(ts_range=(100000, 100001))):  # everything forbidden
        c, br, bs, gc, total = ix.sightings(rows, -np.inf, group_counts=GROUPS, **kw)
        assert total == 0 and not c.any() and (br == -1).all() and (bs == -np.inf).all() and not gc.any() and gc.shape == (70, GROUPS)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_a_threshold_that_is_a_pairs_value(storage, dim):
    """A, B=, B-, B+ with A.B= == same_at, A.B- one ulp below, A.B+ one ulp above, every product exact, among filler far below: B= and
    B+ count, B- does not, A itself only without skip_self"""
    E4, same_at = crafted_rows(dim)
    rng = np.random.default_rng(3)
    E = (0.25 * unit(rng.standard_normal((300, dim)))).astype(np.float32)
    at = np.array([201, 7, 150, 299])                                                  # A, B=, B-, B+: three strips
    E[at] = E4
    ix = index_of(E, storage, groups=(np.arange(300) % 3).astype(np.int32))
    for skip_self, n_hit in ((False, 3), (True, 2)):
        c, br, bs, gc, total = ix.sightings([201, 7], float(same_at), skip_self=skip_self, group_counts=3)
        assert c[0] == n_hit and total == 300, (storage, dim, skip_self, c)
        want = np.bincount(at[[0, 1, 3]][(0 if not skip_self else 1):] % 3, minlength=3)
        assert gc[0].tolist() == want.tolist()
        assert br[0] == (299 if skip_self else 201) and (not skip_self or bs[0] == np.nextafter(same_at, np.float32(2)))
        G = device_pairs(ix, [201, 7], np.arange(300))
        same((c, br, bs, gc, total), sightings_model(None, [201, 7], np.arange(300), same_at, skip_self, np.arange(300) % 3, 3, G=G), (storage, dim))
    ix.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_group_counts_narrower_than_the_groups(storage):
    w, ix = world(768), index(768, storage)
    rows = object_sets(w, 65)
    full = ix.sightings(rows, SAME_AT[-1], group_counts=GROUPS)
    assert (full[3].sum(axis=1) == full[0]).all() and full[0].max() >= 40
    small = ix.sightings(rows, SAME_AT[-1], group_counts=SMALL_GROUP_COUNTS)
    assert np.array_equal(small[3], full[3][:, :SMALL_GROUP_COUNTS]) and (small[3].sum(axis=1) <= small[0]).all() and (small[3].sum(axis=1) < small[0]).any()
    wide = ix.sightings(rows, SAME_AT[-1], group_counts=MAX_GROUPS)
    assert np.array_equal(wide[3][:, :GROUPS], full[3]) and not wide[3][:, GROUPS:].any()
    none = ix.sightings(rows, SAME_AT[-1])
    assert none[3] is None
    for got in (small, wide, none):
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], full[:3])) and got[4] == full[4] == w.n


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_the_device_form_twice_and_an_unchanged_index(storage):
    import torch
    w, ix = world(768), index(768, storage)
    q = unit(w.E[[5]] + 0.2 * unit(np.random.default_rng(1).standard_normal((1, 768))))
    before = ix.scores(q).copy()
    _, kw = competing(w, "both+allowed")
    for n, args in ((65, dict(same_at=0.92, group_counts=GROUPS)), (200, dict(same_at=0.90, skip_self=True, **kw)), (3, dict(same_at=0.95, group_counts=2, **kw))):
        rows = object_sets(w, n)
        want = ix.sightings(rows, **args)
        got = ix.sightings_device(rows, **args)
        assert all(t is None or t.is_cuda for t in got[:4]) and got[4] == want[4]
        again = ix.sightings_device(rows, with_total=False, **args)                    # nothing is waited for
        assert again[4] is None
        torch.cuda.synchronize()
        for g in (got, again):
            host = tuple(None if t is None else t.cpu().numpy() for t in g[:4])
            host = host[:3] + (None if host[3] is None else host[3].view(np.uint32),)
            same(host + (want[4],), want, (storage, n, args))
        twice = ix.sightings(rows, **args)
        assert all(a is None and b is None or a.tobytes() == b.tobytes() for a, b in zip(twice[:4], want[:4]))
    assert np.array_equal(bits(ix.scores(q)), bits(before))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", STORAGES)
def test_consistency_with_the_digest(storage):
    w, ix = world(768), index(768, storage)
    for name in (None, "both+allowed"):
        _, kw = competing(w, name)
        rows, counts, _, _, totals, owner = ix.digest(SAME_AT[-1], by="first", owners=True, **kw)
        k = int(totals[0])
        assert 0 < k < 1024 and totals[2] == 0                                         # below the cap
        lead = rows[:k]
        c, br, bs, gc, total = ix.sightings(lead, SAME_AT[-1], group_counts=GROUPS, **kw)
        assert total == totals[1] and (c >= counts[:k]).all() and (name is not None or (c > counts[:k]).any())
        assert (br >= 0).all() and np.array_equal(gc.sum(axis=1), c)
        # a leader's members all match it (that is why they joined); equality wherever no row matches two leaders
        comp = np.flatnonzero(owner >= 0)
        G = device_pairs(ix, lead, comp)
        hits = G >= np.float32(SAME_AT[-1])
        shared = hits[:, hits.sum(axis=0) > 1].any(axis=1)
        assert (~shared).any() and np.array_equal(c[~shared], counts[:k][~shared])


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing_and_leave_the_index_answering():
    from clearcam_amd import _lib
    w, ix = world(768), index(768, "f32")
    L = _lib.lib()
    q = unit(w.E[[7]] + 0.2 * unit(np.random.default_rng(2).standard_normal((1, 768))))
    before = ix.scores(q).copy()
    al = np.ones(5, np.uint8)
    ok_rows = np.array([3, 1, 3], np.int64)

    def call(rows=ok_rows, n=None, same_at=0.9, flags=0, allowed=None, n_groups=0, where=None, out_count=True, gc=False, ngc=0):
        outs = [np.full(8, 7, np.int32), np.full(8, 7, np.int32), np.full(8, 7, np.float32), np.full((8, 4), 7, np.uint32)]
        total = np.full(1, 7, np.int64)
        rc = L.cc_index_sightings(ix._h, rows.ctypes.data_as(C.POINTER(C.c_int64)) if rows is not None else None, len(rows) if n is None else n, same_at, flags,
                                  _lib.ptr(allowed), n_groups, C.byref(where) if where is not None else None, _lib.ptr(outs[0]) if out_count else None,
                                  _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(outs[3]) if gc else None, ngc, _lib.ptr(total), 0, None)
        return rc, all((o == 7).all() for o in outs + [total])
    empty_window, no_class = _lib.RowFilter(), _lib.RowFilter()
    empty_window.use_ts, empty_window.ts_min, empty_window.ts_max = 1, 5, 4
    no_class.use_cls = 1
    many = np.zeros(MAX_OBJECTS + 1, np.int64)
    bad = {"NaN same_at": dict(same_at=float("nan")), "n 0": dict(n=0), "n -1": dict(n=-1), "n 1025": dict(rows=many), "row -1": dict(rows=np.array([3, -1], np.int64)),
           "row size": dict(rows=np.array([w.n, 0], np.int64)), "flag 2": dict(flags=2), "flag -1": dict(flags=-1), "no out_count": dict(out_count=False),
           "no rows": dict(rows=None, n=2), "counts without width": dict(gc=True, ngc=0), "width without counts": dict(gc=False, ngc=3),
           "width 4097": dict(gc=True, ngc=MAX_GROUPS + 1), "width -1": dict(gc=True, ngc=-1),
           "n_groups 0": dict(allowed=al, n_groups=0), "n_groups -1": dict(allowed=al, n_groups=-1), "n_groups 2^24 + 1": dict(allowed=al, n_groups=(1 << 24) + 1),
           "empty window": dict(where=empty_window), "empty class set": dict(where=no_class)}
    for what, kw in bad.items():
        rc, untouched = call(**kw)
        assert rc == -22 and untouched and L.cc_last_error(), what
    rc, untouched = call(allowed=al, n_groups=5, gc=True, ngc=4, flags=1)
    assert rc == 0 and not untouched
    for f in (lambda: ix.sightings([0], float("nan")), lambda: ix.sightings([]), lambda: ix.sightings(np.zeros(1025, np.int64)), lambda: ix.sightings([w.n]),
              lambda: ix.sightings([0], group_counts=MAX_GROUPS + 1), lambda: ix.sightings_device([-1])):
        with pytest.raises(_lib.CCError):
            f()
    for f in (lambda: ix.sightings([0], ts_range=(5, 4)), lambda: ix.sightings([0], classes=[])):
        with pytest.raises(ValueError):
            f()
    assert np.array_equal(bits(ix.scores(q)), bits(before))


# 9 ---------------------------------------------------------------------------------------------------------------------------------
CAMS, DAYS = ("back", "front", "gate"), ("2026-01-01", "2026-01-02", "2026-01-03")


def yard_spec(dim=768):
    """(camera, day) -> [(name, vector)]: 9 folders x 20 crops of unrelated things, a van seen today (front, DAYS[2]) and before on
    DAYS[0] at back and gate and on DAYS[1] at back, and a stranger seen today only."""
    rng = np.random.default_rng(29)
    van, stranger = unit(rng.standard_normal(dim)), unit(rng.standard_normal(dim))
    out = {(cam, day): [(f"{1000 + 13 * i}.5_{500 + 40 * k + i}_{(0, 2, 7)[i % 3]}.jpg", unit(rng.standard_normal(dim))) for i in range(20)]
           for k, (cam, day) in enumerate((c, d) for c in CAMS for d in DAYS)}
    near = lambda v: unit(v + 0.08 * unit(rng.standard_normal(dim)))                   # noqa: E731
    for shot in range(3):
        out[("front", DAYS[2])].append((f"{5000 + shot}.5_100_2.jpg", near(van)))
        out[("front", DAYS[2])].append((f"{7000 + shot}.5_101_0.jpg", near(stranger)))
    for (cam, day), shots in ((("back", DAYS[0]), 2), (("gate", DAYS[0]), 1), (("back", DAYS[1]), 4)):
        for shot in range(shots):
            out[(cam, day)].append((f"{6000 + shot}.5_102_2.jpg", near(van)))
    return out


def check_yard(f, index, table, is_face):
    got, info = f.seen_before(cam_name="front", timestamp=DAYS[2], count=1000, is_face=is_face)
    assert info == {"objects": 22, "new": 21, "crops": 26, "left_over": 0, "history_crops": len(table.paths) - 26}
    assert len(got) == 22 and [e[4] == 0 for e in got] == [True] * 21 + [False]
    stranger, van = got[0], got[-1]
    assert "_101_0.jpg" in stranger[0] and stranger[1:8] == (3, 7000, 7002, 0, 0, [], None)
    assert stranger[8] is not None and f"/front/objects/{DAYS[2]}/" not in stranger[8] and stranger[9] < 0.5
    assert "_100_2.jpg" in van[0] and van[1:8] == (3, 5000, 5002, 7, 2, ["back", "gate"], DAYS[1])
    assert "_102_2.jpg" in van[8] and van[9] > 0.9
    row = table.row[van[0]]
    assert index.gram([row, table.row[van[8]]])[0, 1] == np.float32(van[9])
    only_gate, _ = f.seen_before(cam_name="front", timestamp=DAYS[2], count=1000, history_cam="gate", is_face=is_face)
    assert only_gate[-1][4:8] == (1, 1, ["gate"], DAYS[0])


@pytest.mark.parametrize("storage", STORAGES)
def test_object_finder_tells_the_seen_from_the_new(tmp_path, storage):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    root = str(tmp_path / "cameras")
    for (cam, day), crops in yard_spec().items():
        d = os.path.join(root, cam, "objects", day)
        EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    f = ObjectFinder(root)
    f.index_storage = storage
    f.attach_store(capacity=64)
    index, table = f._dev["store"]
    check_yard(f, index, table, False)


def test_object_finder_tells_seen_faces_from_new_ones(tmp_path):
    from clearcam_amd.objects import ObjectFinder
    base = str(tmp_path / "cameras")
    f = ObjectFinder(base)
    f.face_embeddings = {f"{base}/{cam}/objects/{day}/{name}": v[None] for (cam, day), crops in yard_spec(512).items() for name, v in crops}
    index, table = f._index_and_table(True)
    assert index.dim == 512
    check_yard(f, index, table, True)
