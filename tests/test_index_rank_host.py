"""``ObjectFinder.search`` / ``search_page`` over an index that ranks the whole order itself (``EmbeddingIndex.rank``), on the CPU.

The device matrix is replaced by `FakeRankIndex`: tests/test_search_tracks_host.py::FakeTrackIndex plus `rank`, answered by the numpy
model of the contract in tests/rank_cases.py.  What is tested here is the host side: that the two cases which used to leave the
device (top_k > 1024; no truthy track id among the allowed crops) are ONE `rank` call with no `search` / `scores` call and no more
than one slot per row, that `search_page` is the slice of the filtered reference list with its length as `total`, and that the
caller's double cut becomes the float32 that keeps the same results.  Expected answers come from `reference_search`."""
import ctypes
import os
import re

import numpy as np
import pytest

from clearcam_amd import _lib
from clearcam_amd import objects as O
from rank_cases import rank_model
from test_search_host import reference_search
from test_search_tracks_host import FakeTrackIndex

REAL = O.EmbeddingIndex                                # the real shim (replaced by the numpy double while a test runs)
cut_f32 = REAL.cut_f32
BASE = "data/cameras/front/objects/2026-01-01"
DIM = 16


class FakeRankIndex(FakeTrackIndex):
    def __init__(self, dim=768, capacity=1024, device=0, storage="f32"):
        super().__init__(dim, capacity, device, storage)
        self.ranks = []

    def rank(self, q, start, count, allowed=None, min_score=None, tracks=True):
        self.ranks.append({"start": start, "count": count, "min_score": min_score, "tracks": tracks})
        return rank_model(self._scores(q), self.tracks, self.groups, start, count, allowed, cut_f32(min_score), tracks)


@pytest.fixture(autouse=True)
def fake_index(monkeypatch):
    monkeypatch.setattr(O, "EmbeddingIndex", FakeRankIndex)


def finder_with(emb):
    f = O.ObjectFinder("nowhere")
    f.image_embeddings = emb
    return f


def index_of(f):
    return f._dev["image"][0]


def other_calls(f):
    ix = index_of(f)
    return len(ix.track_searches), len(ix.searches), ix.score_calls


def grouped_world(rng, n=3000, ids=1437, dup=0.2):
    """n crops of `ids` tracks (id 0 among them), every 13th an id-less snapshot, a fifth exact copies of earlier vectors (ties)"""
    vecs = rng.standard_normal((n, DIM)).astype(np.float32)
    for i in range(1, n):
        if rng.random() < dup:
            vecs[i] = vecs[rng.integers(0, i)]
    return {(f"{BASE}/snap{i}.jpg" if i % 13 == 5 else f"{BASE}/{1000 + i}.0_{i % ids}_2.jpg"): vecs[i].reshape(1, DIM).copy() for i in range(n)}


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(31)
    emb = grouped_world(rng)
    q = rng.standard_normal(DIM).astype(np.float32)
    return emb, q, reference_search(emb, q, 10**9)


@pytest.mark.parametrize("top_k", [1100, 10**9])
def test_deep_search_is_one_rank_call(world, top_k):
    emb, q, everything = world
    f = finder_with(emb)
    got = f.search(top_k=top_k, text_embedding=q)
    assert got == everything[:top_k] and len(got) == min(top_k, len(everything)) > 1024
    ix = index_of(f)
    assert len(ix.ranks) == 1 and other_calls(f) == (0, 0, 0)
    r = ix.ranks[0]
    assert r["tracks"] is True and r["start"] == 0 and r["min_score"] is None
    assert r["count"] == min(top_k, len(emb)) <= len(ix)                     # "everything" asks for no more than one slot per row
    assert f.search(top_k=1024, text_embedding=q) == everything[:1024]      # the first page still takes the search_tracks pass
    assert len(ix.ranks) == 1 and other_calls(f) == (1, 0, 0)


def test_filtered_deep_search(world):
    emb, q, _ = world
    more = dict(emb)
    rng = np.random.default_rng(32)
    for i in range(1300):
        more[f"data/cameras/back/objects/2026-01-02/{5000 + i}.0_{i}_2.jpg"] = rng.standard_normal((1, DIM)).astype(np.float32)
    f = finder_with(more)
    for cam, ts in (("back", None), (None, "2026-01-01"), ("back", "2026-01-01")):
        assert f.search(top_k=1200, cam_name=cam, timestamp=ts, text_embedding=q) == reference_search(more, q, 1200, cam, ts), (cam, ts)
    assert len(index_of(f).ranks) == 2 and other_calls(f) == (0, 0, 0)      # ("back", "2026-01-01") allows no folder: no call


@pytest.mark.parametrize("top_k", [7, 1024, 5000])
def test_ungrouped_world_is_one_rank_call_without_tracks(top_k):
    rng = np.random.default_rng(33)
    vec = lambda: rng.standard_normal((1, DIM)).astype(np.float32)
    flat = {f"{BASE}/{1000 + i}.0_0_2.jpg" if i % 2 else f"{BASE}/snap{i}.jpg": vec() for i in range(1500)}
    keys = list(flat)
    for i in range(10, 1500, 7):
        flat[keys[i]] = flat[keys[i - 9]].copy()                             # ties between id-0 crops and snapshots: row order decides
    q = rng.standard_normal(DIM).astype(np.float32)
    f = finder_with(flat)
    assert f.search(top_k=top_k, text_embedding=q) == reference_search(flat, q, top_k)
    ix = index_of(f)
    assert other_calls(f) == (0, 0, 0) and len(ix.ranks) == 1
    assert ix.ranks[0]["tracks"] is False and ix.ranks[0]["count"] == min(top_k, 1500)


def filtered(everything, t):
    return [r for r in everything if t is None or not r[1] < t]


def test_search_page_equals_the_filtered_slices(world):
    emb, q, everything = world
    f = finder_with(emb)
    scores = [s for _, s in everything]
    runs = [v for v in set(scores) if scores.count(v) >= 2 and v > np.median(scores)]
    assert runs                                                               # duplicate crops without a track id: equal answers
    cases = [(None, "no cut"), (float(np.median(scores)), "a cut"), (max(runs), "a cut inside a run of equal scores"), (1e9, "above everything")]
    for t, what in cases:
        want = filtered(everything, t)
        last = len(want) // 100 * 100
        for start, count in ((0, 100), (1000, 100), (last, 100), (0, 2000), (len(want), 5), (123, 1)):
            got, total = f.search_page(start=start, count=count, text_embedding=q, min_score=t)
            assert got == want[start:start + count], (what, start, count)
            assert total == len(want), (what, start, count)
        if what == "a cut inside a run of equal scores":
            assert scores.count(want[-1][1]) >= 2 and want[-1][1] == t and everything[len(want)][1] < t
            assert sum(1 for _, s in want if s == t) == scores.count(t)      # the whole run is kept and counted
    ix = index_of(f)
    assert other_calls(f) == (0, 0, 0) and len(ix.ranks) == 4 * 6
    assert all(r["count"] <= len(ix) for r in ix.ranks)
    assert len(everything) > 1100 and 0 < len(filtered(everything, cases[1][0])) % 100   # page 10 exists; the last page is partial


def test_search_page_filters_ungrouped_faces_and_empty_cases(world):
    emb, q, _ = world
    rng = np.random.default_rng(34)
    faces = {f"data/cameras/front/faces/2026-01-01/{i}.0_{i % 40}_0.jpg": rng.standard_normal((1, 512)).astype(np.float32) for i in range(300)}
    f = finder_with(emb)
    f.face_embeddings = faces
    qf = rng.standard_normal(512).astype(np.float32)
    want = filtered(reference_search(faces, qf, 10**9), 0.5)
    assert f.search_page(start=10, count=20, text_embedding=qf, is_face=True, min_score=0.5) == (want[10:30], len(want))
    assert f._dev["face"][0].dim == 512 and len(f._dev["face"][0].ranks) == 1
    assert f.search_page(text_embedding=q, cam_name="nope") == ([], 0)
    assert O.ObjectFinder("nowhere").search_page(text_embedding=q) == ([], 0)
    with pytest.raises(ValueError):
        f.search_page(start=-1, text_embedding=q)
    with pytest.raises(ValueError):
        f.search_page(count=0, text_embedding=q)
    with pytest.raises(ValueError):
        f.search_page(text_embedding=q, min_score=float("nan"))


def test_the_cut_is_rounded_up_to_float32(world):
    emb, q, everything = world
    f = finder_with(emb)
    scores = np.array([s for _, s in everything], np.float32)
    v = scores[len(scores) // 3]                                              # a float32 score that occurs
    below = np.nextafter(v, np.float32(-np.inf))
    cuts = {"equal to a score": float(v),
            "between two adjacent float32, nearer the lower": float(below) + 0.25 * (float(v) - float(below)),
            "between two adjacent float32, nearer the upper": float(below) + 0.75 * (float(v) - float(below)),
            "just above a score": float(v) * (1 + 1e-12) if v > 0 else float(v) * (1 - 1e-12)}
    for what, t in cuts.items():
        c = cut_f32(t)
        assert c.dtype == np.float32 and float(c) >= t and float(np.nextafter(c, np.float32(-np.inf))) < t, what
        want = [r for r in everything if not r[1] < t]                        # the reference's test, in double
        got, total = f.search_page(start=0, count=len(everything), text_embedding=q, min_score=t)
        assert got == want and total == len(want), what
        assert np.array_equal(scores >= c, np.array([not float(s) < t for s in scores])), what
    assert float(cut_f32(cuts["equal to a score"])) == float(v) and float(cut_f32(cuts["just above a score"])) > float(v)
    assert cut_f32(None) == -np.inf and cut_f32(-np.inf) == -np.inf and cut_f32(1e39) == np.inf
    assert cut_f32(-1e39) == np.finfo(np.float32).min and cut_f32(0.21) == np.nextafter(np.float32(0.21), np.float32(1)) and float(np.float32(0.21)) < 0.21


def test_unparsable_names_still_raise_through_the_exact_loop():
    rng = np.random.default_rng(35)
    vec = lambda: rng.standard_normal((1, DIM)).astype(np.float32)
    bad = {f"{BASE}/12.0_x_1.jpg": vec(), f"{BASE}/1.0_2_3.jpg": vec()}
    q = rng.standard_normal(DIM).astype(np.float32)
    f = finder_with(bad)
    for call in (lambda: f.search(text_embedding=q), lambda: f.search(top_k=5000, text_embedding=q), lambda: f.search_page(text_embedding=q)):
        with pytest.raises(ValueError):
            call()
    assert index_of(f).ranks == [] and other_calls(f)[0] == 0


def test_an_index_without_rank_keeps_the_candidate_list_path(monkeypatch, world):
    emb, q, everything = world
    monkeypatch.setattr(O, "EmbeddingIndex", FakeTrackIndex)
    f = finder_with(emb)
    paths = lambda res: [p for p, _ in res]                                  # this double's matrix product rounds unlike the reference's
    assert paths(f.search(top_k=1100, text_embedding=q)) == paths(everything[:1100])
    assert other_calls(f)[0] == 0 and other_calls(f)[1] >= 1
    want = filtered(everything, 0.0)
    got, total = f.search_page(start=200, count=50, text_embedding=q, min_score=0.0)
    assert paths(got) == paths(want[200:250]) and total == len(want)


def test_header_declares_the_call_and_the_binding_knows_it(lib_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"\s+", " ", open(os.path.join(root, "include", "clearcam_hip.h")).read())
    assert "#define CC_RANK_TRACKS 1" in src
    assert ("int cc_index_rank(cc_index* h, const float* q, int Q, int64_t start, int64_t count, float min_score, int flags, "
            "const uint8_t* allowed, int n_groups, int32_t* idx, float* score, int64_t* total, int on_device, void* stream);") in src
    assert "cc_index_rank" in _lib.SYMBOLS
    assert hasattr(ctypes.CDLL(lib_path), "cc_index_rank")
    assert callable(REAL.rank) and callable(REAL.rank_device)
