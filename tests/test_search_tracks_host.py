"""``ObjectFinder.search`` over an index that reduces per track itself (``EmbeddingIndex.search_tracks``), on the CPU.

The device matrix is replaced by a numpy double that keeps the contract of cc_index_add_tracked / cc_index_search_tracks: among
the allowed rows every track slot answers once with its best row (equal scores: the lower row), rows of slot -1 answer for
themselves, descending by score, equal scores by first appearance with the slot-less rows last, -1/-inf padding.  What is tested
here is the host side: the slots `_RowTable` hands out, that a grouped search is ONE `search_tracks` call with no widening and no
score download, and that every other case still takes the candidate-list path.  Expected answers come from the restatement of
models/objects.py:356-390 in tests/test_search_host.py."""
import ctypes

import numpy as np
import pytest

from clearcam_amd import objects as O
from test_search_host import FakeIndex, make_world, reference_search


class FakeTrackIndex(FakeIndex):
    def __init__(self, dim=768, capacity=1024, device=0, storage="f32"):
        super().__init__(dim, capacity, device, storage)
        self.tracks, self.track_searches, self.score_calls = np.zeros(0, np.int32), [], 0

    def add(self, emb, groups=None, tracks=None):
        n0 = len(self.rows)
        super().add(emb, groups)
        n = len(self.rows) - n0
        self.tracks = np.concatenate([self.tracks, np.full(n, -1, np.int32) if tracks is None else np.asarray(tracks, np.int32)])
        assert len(self.tracks) == len(self.rows)

    def _scores(self, q):
        # one (1,dim) @ (dim,1) product per row, as the reference evaluates them: bit-equal scores, so ties fall the same way
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        return np.array([[(r.reshape(1, -1) @ v.reshape(-1, 1)).item() for r in self.rows] for v in q], np.float32).reshape(len(q), len(self.rows))

    def scores(self, q):
        self.score_calls += 1
        return super().scores(q)

    def search_tracks(self, q, k, allowed=None):
        s = self._scores(q)
        self.track_searches.append(k)
        idx = np.full((s.shape[0], k), -1, np.int32); sc = np.full((s.shape[0], k), -np.inf, np.float32)
        for i in range(s.shape[0]):
            best, loose = {}, []
            for r in range(len(self.rows)):
                if allowed is not None and not (self.groups[r] < len(allowed) and allowed[self.groups[r]]):
                    continue
                t = int(self.tracks[r])
                if t < 0:
                    loose.append((r, s[i][r]))
                elif t not in best or s[i][r] > best[t][1]:
                    best[t] = (r, s[i][r])
            res = sorted(list(best.values()) + loose, key=lambda x: x[1], reverse=True)[:k]
            idx[i, :len(res)] = [r for r, _ in res]; sc[i, :len(res)] = [v for _, v in res]
        return idx, sc


@pytest.fixture(autouse=True)
def fake_index(monkeypatch):
    monkeypatch.setattr(O, "EmbeddingIndex", FakeTrackIndex)


def finder_with(emb):
    f = O.ObjectFinder("nowhere")
    f.image_embeddings = emb
    return f


def calls(f):
    ix = f._dev["image"][0]
    return len(ix.track_searches), len(ix.searches), ix.score_calls


def grouped_and_live(emb, cam, ts):
    """(some allowed *.jpg crop has a truthy track id, some *.jpg crop is allowed at all): the reference's two branch conditions"""
    live = grouped = False
    for p in emb:
        if cam and f"/cameras/{cam}/" not in p:
            continue
        if ts and f"/objects/{ts}/" not in p and "/objects/video/" not in p:
            continue
        fn = p.rsplit("/", 1)[1]
        if fn.lower().endswith(".jpg"):
            live = True
            grouped = grouped or ("_" in fn and bool(O.event_img_info(fn.split(".jpg")[0])["object_id"]))
    return grouped, live


@pytest.mark.parametrize("seed,dup,neg", [(0, 0.05, False), (1, 0.05, False), (2, 0.05, True), (100, 0.5, True), (101, 0.5, True), (102, 0.5, True)])
def test_grouped_search_is_one_search_tracks_call_and_equals_the_reference(seed, dup, neg):
    rng = np.random.default_rng(seed)
    dim = 16
    emb = make_world(rng, 1200, dim, n_ids=25, dup=dup, neg_ids=neg)
    emb = {p: v for p, v in emb.items() if not p.endswith(".JPG")}         # names the reference raises on: tests/test_search_host.py
    f = finder_with(emb)
    for _ in range(14):
        q = rng.standard_normal(dim).astype(np.float32)
        cam = [None, "front", "back", "nope"][rng.integers(4)]
        ts = [None, "2026-01-01", "2026-01-02", "1999-01-01"][rng.integers(4)]
        k = int(rng.choice([1, 2, 5, 10, 30, 200, 1024]))
        want = reference_search(emb, q, k, cam, ts)
        before = calls(f) if "image" in f._dev else (0, 0, 0)
        got = f.search(top_k=k, cam_name=cam, timestamp=ts, text_embedding=q)
        assert [p for p, _ in got] == [p for p, _ in want], (seed, k, cam, ts)
        assert [s for _, s in got] == [s for _, s in want]
        grouped, live = grouped_and_live(emb, cam, ts)
        if live:
            assert grouped                                                  # every folder of these worlds holds track ids
        after = calls(f)
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == ((1, 0, 0) if live else (0, 0, 0))
        if live:
            assert f._dev["image"][0].track_searches[-1] == k               # asked for top_k answers, not for a wider candidate list


def test_dominant_track_needs_no_widening():
    """The world of test_search_host.py::test_candidate_growth_and_full_fallback: there three searches and the whole score vector."""
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
    f = finder_with(emb)
    got = f.search(top_k=10, text_embedding=q)
    assert got == reference_search(emb, q, 10)
    assert calls(f) == (1, 0, 0)


def test_other_cases_keep_the_candidate_list_path(monkeypatch):
    rng = np.random.default_rng(7)
    dim = 16
    base = "data/cameras/front/objects/2026-01-01"
    vec = lambda: rng.standard_normal((1, dim)).astype(np.float32)
    q = rng.standard_normal(dim).astype(np.float32)
    # no truthy track id among the allowed crops (id 0 and id-less names only): the reference does not group, neither do we
    flat = {f"{base}/{1000 + i}.0_0_2.jpg" if i % 2 else f"{base}/snap{i}.jpg": vec() for i in range(300)}
    f = finder_with(flat)
    assert [p for p, _ in f.search(top_k=7, text_embedding=q)] == [p for p, _ in reference_search(flat, q, 7)]
    assert calls(f)[0] == 0 and calls(f)[1] >= 1
    # top_k above the kernel's limit
    world = {f"{base}/{1000 + i}.0_{i % 1500}_2.jpg": vec() for i in range(3000)}
    f = finder_with(world)
    assert [p for p, _ in f.search(top_k=1100, text_embedding=q)] == [p for p, _ in reference_search(world, q, 1100)]
    assert calls(f)[0] == 0
    assert [p for p, _ in f.search(top_k=1024, text_embedding=q)] == [p for p, _ in reference_search(world, q, 1024)]
    assert calls(f)[0] == 1
    # unparsable names: the reference raises, and so do we, through the exact loop
    bad = {f"{base}/12.0_x_1.jpg": vec(), f"{base}/1.0_2_3.jpg": vec()}
    f = finder_with(bad)
    with pytest.raises(ValueError):
        f.search(text_embedding=q)
    assert calls(f)[0] == 0
    # an index object without search_tracks (its add() takes no tracks either)
    monkeypatch.setattr(O, "EmbeddingIndex", FakeIndex)
    small = dict(list(world.items())[:400])
    f = finder_with(small)
    assert [p for p, _ in f.search(top_k=10, text_embedding=q)] == [p for p, _ in reference_search(small, q, 10)]
    assert not hasattr(f._dev["image"][0], "search_tracks") and f._dev["image"][0].searches


def test_store_backed_path_passes_slots(tmp_path):
    import os
    import pickle
    rng = np.random.default_rng(5)
    day = tmp_path / "cameras" / "front" / "objects" / "2026-01-01"
    os.makedirs(day)
    crops = {f"{day}/{i}.0_{i % 6}_2.jpg": rng.standard_normal((1, 768)).astype(np.float32) for i in range(30)}
    with open(day / "embeddings.pkl", "wb") as fh:
        pickle.dump({"embeddings": crops}, fh)
    f = O.ObjectFinder(str(tmp_path / "cameras"))
    assert f.attach_store() == 30
    index, table = f._dev["store"]
    assert index.tracks.tolist() == table.slot == [i % 6 for i in range(30)]
    q = rng.standard_normal(768).astype(np.float32)
    new = {str(day / "99.0_3_2.jpg"): (q * 10).reshape(1, -1), str(day / "snap.jpg"): (q * 5).reshape(1, -1), str(day / "100.0_-4_2.jpg"): (q * 2).reshape(1, -1)}
    for p, e in new.items():
        f.add_embedding(p, e)
        crops[p] = e
    assert index.tracks.tolist()[30:] == [3, -1, 6]
    got = f.search(top_k=8, text_embedding=q)
    assert [p for p, _ in got] == [p for p, _ in reference_search(crops, q, 8)]
    assert len(index.track_searches) == 1 and not index.searches


def test_row_table_slots():
    t = O._RowTable()
    d = "data/cameras/a/objects/d"
    groups = t.extend([f"{d}/1.0_5_1.jpg", f"{d}/2.0_0_1.jpg", f"{d}/snap.jpg", f"{d}/3.0_-3_1.jpg", f"{d}/4.0_5_1.jpg", f"{d}/5.0_9_1.png",
                       "data/cameras/b/objects/d/6.0_0_1.jpg"])
    assert groups.dtype == np.int32 and groups.tolist() == [1, 1, 1, 1, 1, 0, 2]      # extend() still returns the groups; *.png -> group 0
    assert t.slot == [0, 1, -1, 2, 0, -1, 1]                                          # id 0 and negative ids are ids; no '_' / not *.jpg: none
    assert t.slot_of == {5: 0, 0: 1, -3: 2}
    more = t.extend([f"{d}/7.0_-3_1.jpg", f"{d}/8.0_11_1.jpg"])
    assert more.tolist() == [1, 1] and t.slot[7:] == [2, 3]
    assert t.slots(7).dtype == np.int32 and t.slots(7).tolist() == [2, 3] and t.slots().tolist() == t.slot


def test_library_exports_the_track_calls(lib_path):
    L = ctypes.CDLL(lib_path)
    assert hasattr(L, "cc_index_add_tracked") and hasattr(L, "cc_index_search_tracks")
