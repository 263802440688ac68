"""Track rankings past 1024 track slots on the GPU: track_reduce_kernel's collision path, its flush by tag, and the (Q, T) layout of
best[] behind it at T of two million and at 2^24, through every call that answers one crop per track.

Every other track test has fewer slots than the reduction's table has entries, so no entry ever meets two slots.  The world of
tests/slot_cases.py has them in every block (tests/test_slot_cases_host.py shows that each ranking asked here would see a flush by
bucket, a merge into the owner and dropped colliders).  The expected answers are the existing numpy models, unchanged, applied to the
index's own `ix.scores(...)`: idx, score, total and counts must be EQUAL to them - integer keys, no tolerance.  Every call runs twice
and must return the same bytes: the integer max and min hide the order in which rows arrive."""
import numpy as np
import pytest

import near_cases
import slot_cases as S
import terms_cases
from like_cases import like_model
from rank_cases import full_order, rank_model
from where_cases import DIM, FILTERS, rank_where_model, timeline_model

pytestmark = pytest.mark.gpu


class GpuWorld(S.World):
    def __init__(self):
        super().__init__()
        self._ix, self._sc = {}, {}

    def index(self, storage):
        from clearcam_amd.objects import EmbeddingIndex
        if storage not in self._ix:
            ix = self._ix[storage] = EmbeddingIndex(DIM, self.n, storage=storage)
            ix.add(self.E, self.group, self.slot, ts=self.ts, classes=self.cls)
        return self._ix[storage]

    def scores(self, storage, Q):
        if (storage, Q) not in self._sc:                               # of these Q queries: a larger batch may take another scoring kernel
            self._sc[(storage, Q)] = self.index(storage).scores(self.q[:Q])
        return self._sc[(storage, Q)]


@pytest.fixture(scope="module")
def world():
    return GpuWorld()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def twice(call):
    """The call's result, after a second run of it returned the same bytes"""
    a, b = call(), call()
    for x, y in zip(a, b):
        assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y
    return a


def same(got, want, what):
    """(idx, score[, total]) of the device against the model's"""
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == got[1].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), (what, "idx")
    assert np.array_equal(bits(got[1]), bits(want[1])), (what, "score")
    if len(got) > 2:
        assert got[2].dtype == np.int64 and np.array_equal(got[2], want[2]), (what, "total", got[2], want[2])


def check_search_tracks(ix, q, sc, slot, group, allowed, k, what):
    got = twice(lambda: ix.search_tracks(q, k, allowed))
    same(got, rank_model(sc, slot, group, 0, k, allowed, None, True)[:2], what)
    return got


def check_rank(ix, q, sc, slot, group, start, count, what, allowed=None, cut=None):
    got = twice(lambda: ix.rank(q, start, count, allowed, cut, True))
    same(got, rank_model(sc, slot, group, start, count, allowed, cut, True), what)
    return got


# ---- search_tracks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 3, 20])
def test_search_tracks_equals_the_reference_rule(world, Q):
    w = world
    ix, sc = w.index("f32"), w.scores("f32", Q)
    assert np.abs(sc - w.q[:Q] @ w.E.T).max() < 1e-6
    for name, allowed in S.search_filters(w).items():
        for k in (100, 1024):
            idx, s = check_search_tracks(ix, w.q[:Q], sc, w.slot, w.group, allowed, k, (name, Q, k))
            assert idx.shape == (Q, k)
            if name == "nothing":
                assert (idx == -1).all() and np.isneginf(s).all()
            else:
                assert (idx >= 0).all()                                # more than 1024 tracks answer


@pytest.mark.parametrize("storage", ["bf16", "i8"])
def test_search_tracks_of_the_other_storages(world, storage):
    w = world
    ix, sc = w.index(storage), w.scores(storage, 3)
    for name, allowed in S.search_filters(w).items():
        for k in (100, 1024):
            check_search_tracks(ix, w.q[:3], sc, w.slot, w.group, allowed, k, (storage, name, k))


def test_device_result_equals_host_result(world):
    import torch
    w = world
    ix = w.index("f32")
    for allowed in (None, S.first_row_filter(w)[0]):
        for k in (100, 1024):
            idx, s = ix.search_tracks(w.q[:3], k, allowed)
            di, ds = ix.search_tracks_device(w.q[:3], k, allowed)
            assert di.is_cuda and ds.is_cuda
            torch.cuda.synchronize()
            assert np.array_equal(di.cpu().numpy(), idx) and np.array_equal(bits(ds.cpu().numpy()), bits(s))


# ---- rank -----------------------------------------------------------------------------------------------------------------------------
def test_rank_at_every_window(world):
    w = world
    ix, sc = w.index("f32"), w.scores("f32", S.RANK_Q)
    rows, s = full_order(sc[0], w.slot, w.group, None, True, None)
    assert len(rows) > 2500
    for start, count, cut in S.rank_windows(s):
        got = check_rank(ix, w.q[:S.RANK_Q], sc, w.slot, w.group, start, count, (start, count, cut), None, cut)
        assert (got[0][0] >= 0).any()
        if cut is not None:                                            # the cut keeps the whole run of equal scores, and nothing below
            left = int(got[2][0])
            at = left - 1 - start
            assert got[1][0, at] == got[1][0, at - 1] == np.float32(cut) and got[0][0, at + 1] == -1 and left < len(rows)
    one = twice(lambda: ix.rank(w.q[:1], 1100, 300))
    same(one, rank_model(sc[:1], w.slot, w.group, 1100, 300), "Q = 1")


def test_row_rankings_do_not_see_the_slots(world):
    from clearcam_amd.objects import EmbeddingIndex
    w = world
    ix = w.index("f32")
    plain = EmbeddingIndex(DIM, w.n)
    plain.add(w.E, w.group, ts=w.ts, classes=w.cls)
    allowed = FILTERS["both+allowed"][2]
    ix.search_tracks(w.q[:3], 100)                                     # a track search in between leaves nothing behind
    for start, count in ((0, 1024), (3000, 500), (w.n - 10, 20)):
        for al in (None, allowed):
            a, b = ix.rank(w.q[:3], start, count, al, None, False), plain.rank(w.q[:3], start, count, al, None, False)
            same(a, b, (start, count, "rank"))
    for k in (100, 1024):
        a, b = ix.search(w.q[:3], k), plain.search(w.q[:3], k)
        same(a, b, (k, "search"))
    plain.close()


@pytest.mark.parametrize("name", list(FILTERS))
def test_filtered_rank_and_timeline(world, name):
    w = world
    ix, sc = w.index("f32"), w.scores("f32", S.RANK_Q)
    ts_range, classes, allowed = FILTERS[name]
    lost_first, lost_best = S.filter_losses(w, sc[0], name)
    assert lost_first >= 3 and lost_best >= 3                          # colliders that fail the filter would have placed / answered for a track
    g, al = S.where_groups(w, name)
    rows, s = full_order(sc[0], w.slot, g, al, True, None)
    assert len(rows) > 400
    q = w.q[:S.RANK_Q]
    for start, count, cut in S.filtered_windows(s):
        got = twice(lambda: ix.rank(q, start, count, allowed, cut, True, ts_range, classes))
        same(got, rank_where_model(sc, *w.cols(), start, count, allowed, cut, True, ts_range, classes), (name, start, cut))
    for min_score in (None, S.tied_cut(s)):
        counts, total = twice(lambda: ix.timeline(q, *S.TIMELINE_BINS, allowed, min_score, True, ts_range, classes))
        want = timeline_model(sc, *w.cols(), *S.TIMELINE_BINS, allowed, min_score, True, ts_range, classes)
        assert np.array_equal(counts, want[0]) and np.array_equal(total, want[1]), (name, min_score)
        assert np.array_equal(total, ix.rank(q, 0, 1, allowed, min_score, True, ts_range, classes)[2])


def test_timeline_without_a_filter(world):
    w = world
    ix, sc = w.index("f32"), w.scores("f32", S.RANK_Q)
    counts, total = twice(lambda: ix.timeline(w.q[:S.RANK_Q], *S.TIMELINE_BINS))
    want = timeline_model(sc, *w.cols(), *S.TIMELINE_BINS)
    assert np.array_equal(counts, want[0]) and np.array_equal(total, want[1]) and (total > 2500).all()


# ---- the rankings behind a fold -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["f32", "bf16", "i8"])
def test_rank_like_without_the_query_track(world, storage):
    w = world
    ix = w.index(storage)
    rows, Sm, v, _, _ = S.like_question(w, ix)
    assert w.qslot >= S.TABLE
    for start, count in S.LIKE_WINDOWS:
        got = twice(lambda: ix.rank_like(rows, start, count, exclude="track"))
        same(got, like_model(Sm, *w.cols(), rows, start, count, None, None, True, "track"), (storage, start))
    idx, _, total = ix.rank_like(rows, 0, w.n, exclude="track")
    ans = idx[0, :int(total[0])]
    assert not np.isin(ans, w.track).any() and (ans >= 0).all()
    mine = ans[w.slot[ans] == w.qslot]
    assert len(mine) == 1 and w.group[mine[0]] != w.qgroup             # the dead track's slot answers from its other group
    assert (w.slot[ans] == S.MATE).sum() == 1                          # and its bucket mate keeps answering
    kept = twice(lambda: ix.rank_like(rows, 0, 1024))                  # nothing excluded
    same(kept, like_model(Sm, *w.cols(), rows, 0, 1024), (storage, "no exclusion"))


def test_rank_terms_of_a_compound(world):
    w = world
    ix = w.index("f32")
    ask, v, dead, which, _, _ = S.terms_question(w, ix)
    start, count = S.TERMS["window"]
    got = twice(lambda: ix.rank_terms(start=start, count=count, which=True, **ask))
    want = terms_cases.terms_model(v, dead, which, *w.cols(), start, count)
    same(got[:3], want[:3], "rank_terms")
    assert np.array_equal(got[3], want[3]) and 400 < got[2][0] < 1024 and dead.any()     # every answer is in the window, padding behind
    counts, total = twice(lambda: ix.timeline_terms(*S.TIMELINE_BINS, **ask))
    want = terms_cases.terms_timeline_model(v, dead, *w.cols(), *S.TIMELINE_BINS)
    assert np.array_equal(counts, want[0]) and np.array_equal(total, want[1]) and total[0] == got[2][0]


def test_rank_near_and_its_timeline(world):
    w = world
    ix = w.index("f32")
    ask, Sa, Sb, v, dead, _, _ = S.near_question(w, ix)
    start, count = S.NEAR["window"]
    got = twice(lambda: ix.rank_near(start=start, count=count, **ask))
    want = near_cases.near_model(Sa, Sb, *w.cols(), S.NEAR["within"], start, count, partners=S.NEAR["partners"], value=S.NEAR["value"])
    same(got[:3], want[:3], "rank_near")
    assert np.array_equal(got[3], want[3]) and np.array_equal(bits(got[4]), bits(want[4])) and got[5] == want[5]
    assert got[2][0] > 1024 and dead.any()
    counts, total, n_partners = twice(lambda: ix.timeline_near(t0=S.NEAR["bins"][0], bin_seconds=S.NEAR["bins"][1], n_bins=S.NEAR["bins"][2], **ask))
    want = near_cases.near_timeline_model(Sa, Sb, *w.cols(), S.NEAR["within"], *S.NEAR["bins"], partners=S.NEAR["partners"], value=S.NEAR["value"])
    assert np.array_equal(counts, want[0]) and np.array_equal(total, want[1]) and n_partners == want[2] and total[0] == got[2][0]


# ---- growth, removal, the top of the range --------------------------------------------------------------------------------------------
def test_growth_across_the_table_size():
    """3000 rows with slots below 300, then 3000 whose slots reach past 1024 and share buckets with the old ones, asked with more
    queries than before: best[] and first[] are made again, larger, and cleared."""
    from clearcam_amd.objects import EmbeddingIndex
    w = S.GrowthWorld()
    ix = EmbeddingIndex(DIM, 1000)
    for n, Q in zip((3000, 6000), S.GROWTH_Q):
        ix.add(w.E[n - 3000:n], w.group[n - 3000:n], w.slot[n - 3000:n])
        assert len(ix) == n
        q = w.q[:Q]
        sc = ix.scores(q)
        assert sc.shape == (Q, n)
        for k in S.GROWTH_KS:
            check_search_tracks(ix, q, sc, w.slot[:n], w.group[:n], None, k, (n, k))
        for start, count in S.GROWTH_WINDOWS:
            check_rank(ix, q, sc, w.slot[:n], w.group[:n], start, count, (n, start))
    q = w.q[:1]                                                        # and fewer queries again, in the buffers of eight
    check_search_tracks(ix, q, ix.scores(q), w.slot, w.group, None, 1024, "Q = 1 after Q = 8")
    ix.close()


def test_removal_of_groups_and_of_best_rows(world):
    """remove_groups of the group that holds every row of some forty colliding slots, then remove(rows) of the best rows of the planted
    slots and of the fifty leading tracks: the searches equal the model on the surviving rows.  Slots are stable: T does not shrink."""
    from clearcam_amd.objects import EmbeddingIndex
    w = world
    g = S.removal_groups(w)
    ix = EmbeddingIndex(DIM, w.n)
    ix.add(w.E, g, w.slot, ts=w.ts, classes=w.cls)
    q = w.q[:S.REMOVAL_Q]
    drop = np.zeros(S.GONE_GROUP + 1, np.uint8); drop[S.GONE_GROUP] = 1
    keep = np.flatnonzero(g != S.GONE_GROUP)
    assert ix.remove_groups(drop) == w.n - len(keep) and len(ix) == len(keep)
    for round_ in range(2):
        slot, group = w.slot[keep], g[keep]
        sc = ix.scores(q)
        assert np.array_equal(bits(sc), bits(w.scores("f32", S.REMOVAL_Q)[:, keep]))
        for k in S.REMOVAL_KS:
            check_search_tracks(ix, q, sc, slot, group, None, k, (round_, k))
        for start, count in S.REMOVAL_WINDOWS:
            check_rank(ix, q, sc, slot, group, start, count, (round_, start))
        if round_ == 0:
            rows = S.second_removal(sc[0], slot)
            assert len(rows) >= 50 and ix.remove(rows) == len(rows)
            keep = np.delete(keep, rows)
    ix.close()


def test_the_top_of_the_slot_range():
    """Slots up to 2^24 - 1: T = 2^24, best[] is 128 MB for the one query"""
    from clearcam_amd.objects import EmbeddingIndex
    w = S.TopWorld()
    ix = EmbeddingIndex(DIM, w.n)
    ix.add(w.E, w.group, w.slot)
    sc = ix.scores(w.q)
    assert sc.shape == (1, w.n) and w.slot.max() == (1 << 24) - 1
    for k in S.TOP_KS:
        check_search_tracks(ix, w.q, sc, w.slot, w.group, None, k, ("top", k))
    for start, count in S.TOP_WINDOWS:
        got = check_rank(ix, w.q, sc, w.slot, w.group, start, count, ("top", start))
    assert got[2][0] == 7 + (w.slot < 0).sum()
    ix.close()


# ---- ObjectFinder ---------------------------------------------------------------------------------------------------------------------
def finder_crops():
    """3000 crops of dim 16 in dict order = row order.  Ids 1 .. 1100 appear once each first, so id i takes slot i - 1; then ids j and
    j + 1024 (slots 1024 apart) alternate, and every eleventh crop is one of the dominant track, id 5000 (slot 1100), whose crops
    score above all others.  Every component but one of a crop meets a zero of the query, so device and reference scores are the
    same floats (tests/test_gpu_index_tracks.py::test_object_finder_dominant_track_is_one_call)."""
    rng = np.random.default_rng(17)
    dim = 16
    emb = {}
    for i in range(3000):
        v = np.zeros(dim, np.float32)
        if i < 1100:
            oid = 1 + i
        elif i % 11 == 0:
            oid = 5000
        else:
            j = 1 + (i // 2) % 70
            oid = j if i % 2 else j + 1024
        if oid == 5000:
            v[0] = 0.9 + 0.09 * rng.random(); v[1] = rng.random() * 0.1
        else:
            v[0] = 0.8 * rng.random(); v[2] = 0.3
        emb[f"data/cameras/front/objects/2026-01-01/{10000 + i}.0_{oid}_2.jpg"] = v.reshape(1, -1)
    return emb


def test_object_finder_past_1024_track_ids_is_one_call(monkeypatch):
    from clearcam_amd.objects import EmbeddingIndex, ObjectFinder
    from oracle.clip_oracle import search_reference
    emb = finder_crops()
    q = np.zeros(16, np.float32); q[0] = 1.0
    f = ObjectFinder("nowhere")
    f.image_embeddings = emb
    calls = {"scores": 0, "search": 0, "search_tracks": 0}
    for name in calls:
        def counted(ix, *a, _fn=getattr(EmbeddingIndex, name), _name=name, **kw):
            calls[_name] += 1
            return _fn(ix, *a, **kw)
        monkeypatch.setattr(EmbeddingIndex, name, counted)
    for n, k in enumerate((10, 1024), 1):
        got = f.search(top_k=k, text_embedding=q)
        assert got == search_reference(emb, q, k) and len(got) == k
        assert calls == {"scores": 0, "search": 0, "search_tracks": n}
    assert got[0][0].split("_")[-2] == "5000"
    table = f._dev["image"][1]
    slot = np.asarray(table.slot)
    assert len(slot) == 3000 and slot.max() == 1100 and table.slot_of[5000] == 1100 and table.slot_of[1025] == 1024
    for pick in S.PICKS:                                               # the table's slots collide in both blocks
        hit = S.colliders(slot, pick)
        assert hit[:S.BLOCK].sum() > 400 and hit[S.BLOCK:].sum() > 400
