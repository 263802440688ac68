"""cc_index_add_tracked / cc_index_search_tracks on the GPU: best crop per track slot, slot-less rows kept, top-k, in one call.

The expected answer is the reference's rule (models/objects.py:378-390) applied in numpy to the index's own score vector
`ix.scores(q)`: per slot the best allowed row (equal scores: the lower row), slot-less rows as they are, ordered by score
descending and then by first appearance (a track: its first allowed row; a slot-less row: N + row).  idx and score must be EQUAL
to it - integer keys, no tolerance; the f32 scores themselves are held to q @ E.T within 1e-6 like test_index_scores_and_topk_exact.

The world (40 000 x 256, three 16 384-row selection chunks and twenty 2 048-row reduction blocks): one track of 6 000 rows spread
over all of them that outscores everything, 300 ordinary tracks, 5 % slot-less rows, 20 % exact duplicates of earlier rows (inside
a track and across tracks: ties decide the order), the last rows appended through the plain add (slot -1), 8 groups."""
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, N_GROUPS, DOMINANT, PLAIN_TAIL = 40000, 256, 8, 6000, 1500
PIECES = (0, 10000, 16384, 16391, 30000, N - PLAIN_TAIL, N)            # appends: past the initial capacity, across chunk boundaries


class World:
    def __init__(self):
        rng = np.random.default_rng(21)
        unit = lambda a: (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)
        u = unit(rng.standard_normal(DIM))
        E = unit(rng.standard_normal((N, DIM)))
        slot = rng.integers(1, 301, N).astype(np.int32)
        slot[rng.random(N) < 0.05] = -1
        dom = rng.choice(N - PLAIN_TAIL, DOMINANT, replace=False)
        slot[dom] = 0
        E[dom] = unit(u + 0.02 * rng.standard_normal((DOMINANT, DIM)))          # cosine ~0.95 with u: above every other row for every query
        dup = np.flatnonzero(rng.random(N) < 0.20); dup = dup[dup > 0]
        origin = np.arange(N)
        for r in dup:                                                           # copies of EARLIER rows (chains allowed), whatever their track
            src = rng.integers(0, r)
            E[r], origin[r] = E[src], origin[src]
        for r in dom[1:3]:                                                      # ties inside the dominant track, for certain
            E[r], origin[r] = E[dom[0]], origin[dom[0]]
        self.hot = np.isin(origin, dom)                                         # the dominant track's vectors, wherever they were copied to
        slot[N - PLAIN_TAIL:] = -1                                              # these go in through add() without tracks
        self.E, self.slot, self.dom = E, slot, dom
        self.group = rng.integers(0, N_GROUPS, N).astype(np.int32)
        self.q = unit(u + 0.03 * rng.standard_normal((20, DIM)))
        self._ix, self._sc = {}, {}

    def index(self, storage):
        from clearcam_amd.objects import EmbeddingIndex
        if storage not in self._ix:
            ix = EmbeddingIndex(DIM, 1000, storage=storage)
            for a, b in zip(PIECES[:-2], PIECES[1:-1]):
                ix.add(self.E[a:b], self.group[a:b], self.slot[a:b])
            ix.add(self.E[PIECES[-2]:], self.group[PIECES[-2]:])
            assert len(ix) == N and ix.capacity >= N
            self._ix[storage] = ix
        return self._ix[storage]

    def scores(self, storage, Q):
        if (storage, Q) not in self._sc:
            self._sc[(storage, Q)] = self.index(storage).scores(self.q[:Q])
        return self._sc[(storage, Q)]

    def filters(self, sc0):
        """name -> allowed bytes (None: no filter); sc0: the scores of query 0"""
        best_dom = self.dom[np.lexsort((self.dom, -sc0[self.dom]))[0]]
        no_best = np.ones(N_GROUPS, np.uint8); no_best[self.group[best_dom]] = 0
        first_row = int(np.flatnonzero(self.slot == self.slot[self.slot > 0][0])[0])
        no_first = np.ones(N_GROUPS, np.uint8); no_first[self.group[first_row]] = 0
        return {"none": None, "without the dominant track's best row": no_best, "without a track's first row": no_first,
                "short bitmap": np.ones(5, np.uint8), "nothing": np.zeros(N_GROUPS, np.uint8)}


def expected(sc, slot, group, allowed, k):
    """The reference rule on one score vector -> (idx (k,), score (k,)) with -1/-inf padding."""
    n = len(sc)
    ok = np.ones(n, bool) if allowed is None else (group < len(allowed)) & (np.asarray(allowed)[np.minimum(group, len(allowed) - 1)] != 0)
    rows = np.flatnonzero(ok)
    tr, loose = rows[slot[rows] >= 0], rows[slot[rows] < 0]
    o = tr[np.lexsort((tr, -sc[tr], slot[tr]))]                   # by slot, then score descending, then row: the first of a slot is its best
    lead = np.r_[True, slot[o][1:] != slot[o][:-1]] if len(o) else np.zeros(0, bool)
    best = o[lead]
    first = np.full(int(slot.max()) + 2, n, np.int64)
    np.minimum.at(first, slot[tr], tr)
    ans = np.concatenate([best, loose]).astype(np.int64)
    pos = np.concatenate([first[slot[best]], n + loose])
    order = np.lexsort((pos, -sc[ans]))[:k]
    idx = np.full(k, -1, np.int32); s = np.full(k, -np.inf, np.float32)
    idx[:len(order)] = ans[order]; s[:len(order)] = sc[ans[order]]
    return idx, s


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("Q", [1, 3, 20])
def test_search_tracks_equals_the_reference_rule(world, storage, Q):
    ix, sc = world.index(storage), world.scores(storage, Q)
    if storage == "f32":
        assert np.abs(sc - world.q[:Q] @ world.E.T).max() < 1e-6
    assert sc[:, world.hot].min() > 0.7 and sc[:, ~world.hot].max() < 0.5      # the dominant track (and the copies of its crops) on top
    for name, allowed in world.filters(world.scores(storage, 1)[0]).items():
        want = [expected(sc[i], world.slot, world.group, allowed, 1024) for i in range(Q)]
        for k in (1, 10, 1024):
            idx, s = ix.search_tracks(world.q[:Q], k, allowed)
            assert idx.shape == s.shape == (Q, k) and idx.dtype == np.int32 and s.dtype == np.float32
            for i in range(Q):
                assert np.array_equal(idx[i], want[i][0][:k]), (name, k, i)
                assert np.array_equal(s[i], want[i][1][:k]), (name, k, i)
        if name == "nothing":
            assert (idx == -1).all() and np.isneginf(s).all()
    i1, s1 = ix.search_tracks(world.q[:Q], 10)
    assert np.array_equal(ix.search_tracks(world.q[:Q], 10)[0], i1)            # integer max / min: the same answer every time


def test_fewer_answers_than_k_and_empty_index(world):
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(DIM, 4)
    idx, s = ix.search_tracks(world.q[:2], 7)
    assert (idx == -1).all() and np.isneginf(s).all()                           # empty index
    rows = world.dom[:3].tolist() + [int(np.flatnonzero(world.slot == 5)[0]), int(np.flatnonzero(world.slot == -1)[0])]
    ix.add(world.E[rows], None, [0, 0, 0, 1, -1])                               # past the capacity of 4
    sc = ix.scores(world.q[:2])
    idx, s = ix.search_tracks(world.q[:2], 7)
    for i in range(2):
        wi, ws = expected(sc[i], np.array([0, 0, 0, 1, -1], np.int32), np.zeros(5, np.int32), None, 7)
        assert np.array_equal(idx[i], wi) and np.array_equal(s[i], ws)
    assert (idx[:, 3:] == -1).all() and np.isneginf(s[:, 3:]).all() and (idx[:, :3] >= 0).all()
    with pytest.raises(Exception):
        ix.search_tracks(world.q[:1], 1025)
    with pytest.raises(ValueError):
        ix.add(world.E[:2], None, [0, 1 << 24])
    with pytest.raises(ValueError):
        ix.add(world.E[:2], None, [0])


def test_device_result_equals_host_result(world):
    import torch
    ix = world.index("f32")
    allowed = world.filters(world.scores("f32", 1)[0])["without a track's first row"]
    for al in (None, allowed):
        idx, s = ix.search_tracks(world.q[:3], 50, al)
        di, ds = ix.search_tracks_device(world.q[:3], 50, al)
        assert di.is_cuda and ds.is_cuda
        torch.cuda.synchronize()
        assert np.array_equal(di.cpu().numpy(), idx) and np.array_equal(ds.cpu().numpy(), s)
    di, ds = ix.search_tracks_device(torch.as_tensor(world.q[:3]).cuda(), 50)
    assert np.array_equal(di.cpu().numpy(), ix.search_tracks(world.q[:3], 50)[0])


def test_row_searches_do_not_see_the_slots(world):
    from clearcam_amd.objects import EmbeddingIndex
    ix = world.index("f32")
    plain = EmbeddingIndex(DIM, N)
    plain.add(world.E, world.group)
    allowed = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
    ix.search_tracks(world.q[:3], 10, allowed)                                  # a track search in between leaves nothing behind
    for k in (1, 100, 1024):
        for al in (None, allowed):
            a, b = ix.search(world.q[:5], k, al), plain.search(world.q[:5], k, al)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(ix.scores(world.q[:5]), plain.scores(world.q[:5]))
    a, b = ix.search_device(world.q[:2], 10), plain.search_device(world.q[:2], 10)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy())


class Counted:
    """Counts the calls of EmbeddingIndex.scores / search / search_tracks made while it is active."""

    def __init__(self, monkeypatch):
        from clearcam_amd.objects import EmbeddingIndex
        self.n = {"scores": 0, "search": 0, "search_tracks": 0}
        for name in self.n:
            monkeypatch.setattr(EmbeddingIndex, name, self._wrap(name, getattr(EmbeddingIndex, name)))

    def _wrap(self, name, fn):
        def counted(ix, *a, **kw):
            self.n[name] += 1
            return fn(ix, *a, **kw)
        return counted


def test_object_finder_dominant_track_is_one_call(monkeypatch):
    """The world of tests/test_search_host.py::test_candidate_growth_and_full_fallback: 2 500 crops of one track above 300 others.
    Every component but one of a crop meets a zero of the query, so device and reference scores are the same floats."""
    from clearcam_amd.objects import ObjectFinder
    from oracle.clip_oracle import search_reference
    rng = np.random.default_rng(11)
    dim = 16
    q = np.zeros(dim, np.float32); q[0] = 1.0
    emb = {}
    for i in range(2500):
        v = np.zeros(dim, np.float32); v[0] = 0.9 + 0.09 * rng.random(); v[1] = rng.random() * 0.1
        emb[f"data/cameras/front/objects/2026-01-01/{i}.0_7_2.jpg"] = v.reshape(1, -1)
    for i in range(300):
        v = np.zeros(dim, np.float32); v[0] = 0.5 * rng.random(); v[2] = 0.3
        emb[f"data/cameras/front/objects/2026-01-01/{9000 + i}.0_{100 + i}_2.jpg"] = v.reshape(1, -1)
    f = ObjectFinder("nowhere")
    f.image_embeddings = emb
    c = Counted(monkeypatch)
    got = f.search(top_k=10, text_embedding=q)
    assert got == search_reference(emb, q, 10)
    assert c.n == {"scores": 0, "search": 0, "search_tracks": 1}
    assert f.search(top_k=400, text_embedding=q) == search_reference(emb, q, 400)       # 301 answers
    assert c.n == {"scores": 0, "search": 0, "search_tracks": 2}


def test_store_backed_search_after_appends(tmp_path, monkeypatch):
    from clearcam_amd.objects import ObjectFinder
    from oracle.clip_oracle import search_reference
    rng = np.random.default_rng(12)
    unit = lambda a: (a / np.linalg.norm(a)).astype(np.float32)
    base = tmp_path / "cameras"
    crops = {}
    for cam, day in (("front", "2026-01-01"), ("back", "2026-01-02")):
        d = base / cam / "objects" / day
        os.makedirs(d)
        here = {f"{d}/{1000 + i}.0_{i % 9 - 2}_2.jpg" if i % 7 else f"{d}/snap{i}.jpg": unit(rng.standard_normal(768))[None] for i in range(120)}
        with open(d / "embeddings.pkl", "wb") as fh:
            pickle.dump({"embeddings": here}, fh)
        crops.update(here)
    f = ObjectFinder(str(base))
    assert f.attach_store(capacity=64) == 240
    q = unit(rng.standard_normal(768))
    d = base / "front" / "objects" / "2026-01-01"
    for i in range(900):                                                        # past the attached matrix's capacity (1024 rows)
        p = f"{d}/{5000 + i}.0_{i % 50}_2.jpg" if i % 11 else f"{d}/late{i}.jpg"
        e = unit(rng.standard_normal(768) + (3.0 if i % 50 == 3 else 0.0) * q)[None]   # track 3 keeps scoring on top
        f.add_embedding(p, e)
        crops[p] = e
    assert len(f._dev["store"][0]) == 1140
    c = Counted(monkeypatch)
    for cam, ts, k in ((None, None, 10), ("front", None, 30), (None, "2026-01-02", 1024), ("back", "2026-01-01", 5)):
        got, want = f.search(top_k=k, cam_name=cam, timestamp=ts, text_embedding=q), search_reference(crops, q, k, cam, ts)
        assert [p for p, _ in got] == [p for p, _ in want], (cam, ts, k)
        assert np.allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-6)
    assert c.n == {"scores": 0, "search": 0, "search_tracks": 3}                 # ("back", "2026-01-01") allows no folder: no call
