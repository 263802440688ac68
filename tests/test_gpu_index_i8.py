"""EmbeddingIndex(storage="i8") on the GPU: int8 codes with one f32 scale per 32 elements (include/clearcam_hip.h, CC_INDEX_I8).

The stored bytes are held, bit for bit, to the numpy restatement of tests/i8_cases.py; the scores to the decoded rows (2e-6, the bar
of the bf16 mode) and to the exact rows (the derived bound of `score_bound`); every search to the model of tests/rank_cases.py fed
with the index's own scores; removal and growth to a fresh index of the survivors; ObjectFinder to its own answers on f32 rows."""
import ctypes as C
import os

import numpy as np
import pytest

from i8_cases import crafted_rows, decode, quantise, score_bound, unit
from rank_cases import rank_model
from test_gpu_index_remove import assert_same_answers, fresh, slab_rows

pytestmark = pytest.mark.gpu


def i8_index(dim, capacity):
    from clearcam_amd.objects import EmbeddingIndex
    return EmbeddingIndex(dim, capacity, storage="i8")


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dim", [256, 768])
def test_stored_rows_equal_the_restatement_bit_for_bit(dim, on_device):
    """37 rows (the crafted ones and random ones of several magnitudes) appended in pieces of 1, 8 and 28 into an index of capacity
    4, which grows twice.  A one-hot query makes every sum exact, so scores(eye) IS the decoded matrix."""
    import torch
    crafted, _ = crafted_rows(dim)
    rng = np.random.default_rng(7)
    rand = rng.standard_normal((30, dim)).astype(np.float32) * (10.0 ** rng.integers(-3, 3, (30, 1))).astype(np.float32)
    E = np.concatenate([crafted[:1], rand[:8], crafted[1:], rand[8:]])
    assert len(E) == 37
    ix = i8_index(dim, 4)
    for a, b in ((0, 1), (1, 9), (9, 37)):
        ix.add(torch.from_numpy(E[a:b]).cuda() if on_device else E[a:b])
    assert len(ix) == 37 and ix.capacity == 64
    storage = C.c_int()
    from clearcam_amd import _lib
    _lib.check(_lib.lib().cc_index_info(ix._h, None, C.byref(storage), None))
    assert storage.value == 8
    want = decode(*quantise(E))
    got = ix.scores(np.eye(dim, dtype=np.float32))
    assert got.shape == (dim, 37)
    assert np.array_equal(got, want.T), np.argwhere(got != want.T)[:8]
    ix.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit_rows():
    rng = np.random.default_rng(11)
    E = unit(rng.standard_normal((1000, 768)))
    Q = unit(rng.standard_normal((17, 768)))
    codes, scales = quantise(E)
    return E, Q, decode(codes, scales), scales


@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 33, 1000])
def test_scores_are_those_of_the_decoded_rows_however_the_batch_is_split(unit_rows, n):
    E, Q, D, scales = unit_rows
    ix = i8_index(768, n)
    ix.add(E[:n])
    single = np.concatenate([ix.scores(Q[i]) for i in range(17)])                  # one query per call
    dec = Q.astype(np.float64) @ D[:n].astype(np.float64).T
    exact = Q.astype(np.float64) @ E[:n].astype(np.float64).T
    assert np.abs(single - dec).max() <= 2e-6
    assert (np.abs(single - exact) <= score_bound(Q, scales[:n]) + 2e-6).all()
    for nq in list(range(1, 10)) + [17]:
        got = ix.scores(Q[:nq])
        assert got.shape == (nq, n) and np.array_equal(got, single[:nq]), nq
    got = ix.scores(Q[3:12])                                                        # the same queries at other places of a batch
    assert np.array_equal(got, single[3:12])
    ix.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
class RankWorld:
    N, DIM = 17000, 256

    def __init__(self):
        rng = np.random.default_rng(12)
        n = self.N
        u = unit(rng.standard_normal(self.DIM))
        E = unit(rng.standard_normal((n, self.DIM)))
        hot = rng.choice(n, 1500, replace=False)
        E[hot] = unit(u + 0.08 * rng.standard_normal((1500, self.DIM)))              # a crowd near the queries: ranks are decided among neighbours
        for r in rng.choice(np.arange(1, n), 600, replace=False):                    # byte-for-byte copies of EARLIER rows: exact ties
            E[r] = E[rng.integers(0, r)]
        E[hot[1]] = E[hot[2]] = E[hot[0]]
        self.E = E
        self.group = rng.integers(0, 5, n).astype(np.int32)
        self.slot = rng.integers(0, 400, n).astype(np.int32)
        self.slot[rng.random(n) < 0.1] = -1
        self.allowed = np.array([1, 0, 1, 0, 1], np.uint8)
        self.q = unit(u + 0.05 * rng.standard_normal((3, self.DIM)))
        self.ix = i8_index(self.DIM, 1024)                                          # grows on the way to 17 000
        for a in range(0, n, 6000):
            self.ix.add(E[a:a + 6000], self.group[a:a + 6000], self.slot[a:a + 6000])
        self.sc = self.ix.scores(self.q)


@pytest.fixture(scope="module")
def rank_world():
    w = RankWorld()
    yield w
    w.ix.close()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "ids")
    assert np.array_equal(got[1], want[1]), (what, "scores")
    if len(want) > 2 and len(got) > 2:
        assert np.array_equal(got[2], want[2]), (what, "total")


def test_search_ranks_what_scores_says(rank_world):
    w = rank_world
    assert len(w.ix) == w.N and np.array_equal(w.sc, w.ix.scores(w.q))               # the scan is deterministic
    top = np.sort(w.sc, axis=1)[:, ::-1]
    assert (top[:, :1024] == np.roll(top, 1, axis=1)[:, :1024]).any()                # exact ties among the answers
    for al in (None, w.allowed):
        for k in (1, 100, 1024):
            same(w.ix.search(w.q, k, al), rank_model(w.sc, w.slot, w.group, 0, k, al, None, tracks=False)[:2], ("search", k, al is not None))
        for k in (10, 1024):
            same(w.ix.search_tracks(w.q, k, al), rank_model(w.sc, w.slot, w.group, 0, k, al, None, tracks=True)[:2], ("search_tracks", k, al is not None))


@pytest.mark.parametrize("window", [(0, 10), (1000, 100), (1023, 2), (16380, 10)])
def test_rank_pages_what_scores_says(rank_world, window):
    from clearcam_amd.objects import EmbeddingIndex
    w = rank_world
    start, count = window
    for al in (None, w.allowed):
        for tracks in (True, False):
            for cut in (None, 0.0, float(np.sort(w.sc[0])[-1200])):                   # no cut, half of the rows, a cut on a stored score
                want = rank_model(w.sc, w.slot, w.group, start, count, al, None if cut is None else EmbeddingIndex.cut_f32(cut), tracks)
                same(w.ix.rank(w.q, start, count, al, cut, tracks), want, ("rank", window, al is not None, tracks, cut))
    full = w.ix.rank(w.q, start, count, None, None, False)
    assert (full[2] == w.N).all() and (full[0][:, 0] >= 0).all()                      # every window lies inside the plain order


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_removal_and_growth_keep_the_bytes():
    rng = np.random.default_rng(13)
    n, dim = 5000, 256
    E = unit(rng.standard_normal((n + 300, dim)))
    for r in rng.choice(np.arange(1, n), 500, replace=False):
        E[r] = E[rng.integers(0, r)]
    group = rng.integers(0, 8, n + 300).astype(np.int32)
    slot = rng.integers(-1, 120, n + 300).astype(np.int32)
    q = unit(E[:3] + 0.2 * rng.standard_normal((3, dim)))
    allowed = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
    rows = np.arange(n)
    drop = (rows % 3 == 0) | ((rows >= 2100) & (rows < 2800))
    with slab_rows(256):                                                            # slabs of 256 rows: bounced ones first, direct ones after 64 removed rows
        ix = i8_index(dim, n)
        ix.add(E[:n], group[:n], slot[:n])
        cap = ix.capacity
        assert ix.remove(drop) == int(drop.sum()) and ix.capacity == cap
        live = np.flatnonzero(~drop)
        ref = fresh(E[live], group[live], slot[live], "i8", dim)
        assert_same_answers(ix, ref, q, allowed, "removal")
        assert np.array_equal(ix.scores(np.eye(dim, dtype=np.float32)[:40]), decode(*quantise(E[live])).T[:40])    # scales moved with their codes
        ref.close()
        more = np.arange(n, n + 300)
        ix.add(E[more], group[more], slot[more])
        live = np.concatenate([live, more])
        ref = fresh(E[live], group[live], slot[live], "i8", dim)
        assert_same_answers(ix, ref, q, allowed, "removal, then 300 rows")
        ref.close(); ix.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_close_to_the_f32_index():
    """The inputs of test_gpu_clip.py::test_bf16_index_scores_within_1e_3.  On these the restatement reads 9.2e-4 max, 1.9e-4 rms
    and 19-20 of 20 on the host; the asserted bars are the derived bound and the bf16 test's overlap."""
    from clearcam_amd.objects import EmbeddingIndex
    rng = np.random.default_rng(22)
    E = rng.standard_normal((40000, 768)).astype(np.float32); E /= np.linalg.norm(E, axis=1, keepdims=True)
    Q = rng.standard_normal((11, 768)).astype(np.float32); Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    a, b = EmbeddingIndex(768, 40000), i8_index(768, 1000)
    a.add(E); b.add(E[:25000]); b.add(E[25000:])
    sa, sb = a.scores(Q), b.scores(Q)
    err = np.abs(sa.astype(np.float64) - sb)
    bound = score_bound(Q, quantise(E)[1])
    print(f"i8 against f32: max {err.max():.3g}, rms {np.sqrt((err ** 2).mean()):.3g}, largest bound {bound.max():.3g}")
    assert (err <= bound + 2e-6).all()
    ia, _ = a.search(Q, 20); ib, scb = b.search(Q, 20)
    for r in range(11):
        assert len(set(ia[r]) & set(ib[r])) >= 17
        assert (np.diff(scb[r]) <= 0).all()
    a.close(); b.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
CAMS, DAYS, LEVELS = ("back", "front", "yard"), ("2026-01-01", "2026-01-02"), 50
FILTERS = ((None, None), ("back", None), (None, DAYS[1]), ("yard", DAYS[0]))


def finder_spec():
    """6 folders x 50 crops.  Fifty vectors whose cosines with the query lie 0.03 apart (0.765 .. -0.705, so that the endpoint's cut of
    0.21 falls half way between two of them, 0.015 from either); every folder holds each of them once, in an order of its own, so the
    copies of one vector are exact ties in either storage and everything else is further apart than twice the int8 bound: both
    storages must return the same paths in the same order, and cut the list at the same place."""
    rng = np.random.default_rng(14)
    q = unit(rng.standard_normal(768))
    r = rng.standard_normal((LEVELS, 768))
    r -= np.outer(r @ q.astype(np.float64), q)
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    cos = 0.765 - 0.03 * np.arange(LEVELS)
    V = unit(cos[:, None] * q + np.sqrt(1 - cos ** 2)[:, None] * r)
    folders, t = {}, 1000
    for cam in CAMS:
        for day in DAYS:
            crops = []
            for i, level in enumerate(rng.permutation(LEVELS)):
                t += 1
                name = f"{t}.0_{int(rng.integers(0, 12))}_2.jpg" if i % 9 else f"snap{t}.jpg"
                crops.append((name, V[level]))
            folders[(cam, day)] = crops
    return folders, q, V


def finder_answers(f, q):
    out = {}
    for cam, day in FILTERS:
        for k in (10, 300):
            out[("search", cam, day, k)] = f.search(top_k=k, cam_name=cam, timestamp=day, text_embedding=q)
        for start, count, cut in ((0, 10, None), (7, 20, None), (0, 300, 0.21), (3, 5, 0.21)):
            res, total = f.search_page(start=start, count=count, cam_name=cam, timestamp=day, text_embedding=q, min_score=cut)
            out[("page", cam, day, start, count, cut)] = res
            out[("total", cam, day, start, count, cut)] = total
    return out


def compare_finders(a, b, q, bound):
    """a: f32 rows, b: int8 rows"""
    fa, fb = finder_answers(a, q), finder_answers(b, q)
    assert fa.keys() == fb.keys()
    seen = 0
    for key in fa:
        if key[0] == "total":
            assert fa[key] == fb[key], key
            continue
        assert [p for p, _ in fa[key]] == [p for p, _ in fb[key]], key
        assert all(abs(x - y) <= bound + 2e-6 for (_, x), (_, y) in zip(fa[key], fb[key])), key
        seen += len(fa[key])
    assert seen > 100 and len(fa[("search", None, None, 300)]) >= 12


def test_object_finder_on_int8_rows(tmp_path):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    folders, q, V = finder_spec()
    bound = float(score_bound(q, quantise(V)[1]).max())
    assert 0.03 > 2 * bound and 0.015 > bound                                      # the spacing is more than twice the bound, the cut more than one away
    root = str(tmp_path / "cameras")
    for (cam, day), crops in folders.items():
        d = os.path.join(root, cam, "objects", day)
        EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    # through attach_store
    finders = {}
    for storage in ("f32", "i8"):
        f = ObjectFinder(root)
        f.index_storage = storage
        assert f.attach_store(capacity=64) == 6 * LEVELS
        assert f._dev["store"][0].storage == storage
        finders[storage] = f
    compare_finders(finders["f32"], finders["i8"], q, bound)
    # through the dict the reference exposes (_device_index -> _new_index)
    plain = {}
    for storage in ("f32", "i8"):
        f = ObjectFinder(root)
        f.index_storage = storage
        f._load_all_embeddings()
        assert len(f.image_embeddings) == 6 * LEVELS
        plain[storage] = f
    compare_finders(plain["f32"], plain["i8"], q, bound)
    assert plain["i8"]._dev["image"][0].storage == "i8"


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    from clearcam_amd import _lib
    from clearcam_amd._lib import CCError
    from clearcam_amd.objects import EmbeddingIndex
    with pytest.raises(CCError, match=r"dim % 256"):
        EmbeddingIndex(260, 16, storage="i8")
    h = C.c_void_p()
    assert _lib.lib().cc_index_create_ex(C.byref(h), 256, 16, 0, 3) == -22 and not h.value
    assert "storage" in _lib.lib().cc_last_error().decode()
    with pytest.raises(KeyError):
        EmbeddingIndex(256, 16, storage="int8")
    ix = i8_index(256, 16)                                                          # the library answers afterwards
    E = unit(np.random.default_rng(15).standard_normal((5, 256)))
    ix.add(E)
    with pytest.raises(ValueError):
        ix.add(np.zeros((2, 768), np.float32))
    idx, sc = ix.search(E[3], 2)
    assert idx[0, 0] == 3 and abs(sc[0, 0] - 1.0) <= 2e-2 and len(ix) == 5
    ix.close()
