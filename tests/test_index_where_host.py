"""Row filters and the timeline on the CPU: the numpy model of tests/where_cases.py against a brute-force loop, the ts / class
columns of `_RowTable`, the Python-side argument checks, and `ObjectFinder`'s host fallback with a row filter (an index that
cannot rank)."""
import os

import numpy as np
import pytest

from clearcam_amd import _lib
from clearcam_amd import objects as O
from where_cases import CLASSES, GROUPS, NO_TS, Rows, passing, rank_where_model, timeline_model, where_order


def brute(sc, slot, group, ts, cls, allowed, tracks, cut, ts_range, classes):
    """The contract in words, row by row -> [(row, score)] in order"""
    n = len(sc)
    best, first, loose = {}, {}, []
    for r in range(n):
        if allowed is not None and not (group[r] < len(allowed) and allowed[group[r]]):
            continue
        if ts_range is not None and (ts[r] == NO_TS or ts[r] < ts_range[0] or ts[r] > ts_range[1]):
            continue
        if classes is not None and (cls[r] < 0 or cls[r] not in classes):
            continue
        t = slot[r]
        if tracks and t >= 0:
            first.setdefault(t, r)
            if t not in best or sc[r] > sc[best[t]]:
                best[t] = r
        else:
            loose.append(r)
    ans = [(sc[r], first[t], r) for t, r in best.items()] + [(sc[r], (n + r) if tracks else r, r) for r in loose]
    if cut is not None:
        ans = [a for a in ans if not a[0] < np.float32(cut)]
    ans.sort(key=lambda a: (-a[0], a[1]))
    return [(r, s) for s, _, r in ans]


def small():
    w = Rows(n=200, seed=3, queries=2)
    sc = (w.E @ w.q.T).T.astype(np.float32)
    return w, sc


CASES = [dict(ts_range=None, classes=None), dict(ts_range=(0, 200), classes=None), dict(ts_range=None, classes=(0, 64, 255)),
         dict(ts_range=(-50, 120), classes=(2, 63))]


@pytest.mark.parametrize("tracks", [True, False])
def test_model_equals_the_brute_force_loop(tracks):
    w, sc = small()
    allowed = np.array([1, 1, 0, 1, 1], np.uint8)
    assert (w.ts == NO_TS).any() and (w.cls == -1).any() and (w.slot == -1).any()
    for case in CASES:
        for al in (None, allowed):
            for cut in (None, float(np.median(sc[0]))):
                want = brute(sc[0], w.slot, w.group, w.ts, w.cls, al, tracks, cut, case["ts_range"], case["classes"])
                rows, s = where_order(sc[0], w.slot, w.group, GROUPS, w.ts, w.cls, al, tracks, cut, **case)
                assert rows.tolist() == [r for r, _ in want] and s.tolist() == [v for _, v in want], (case, al is None, cut)
                idx, out, total = rank_where_model(sc, w.slot, w.group, GROUPS, w.ts, w.cls, 3, 10, al, cut, tracks, **case)
                assert total[0] == len(want) and idx[0].tolist() == ([r for r, _ in want][3:13] + [-1] * 10)[:10]
                # the timeline: bins of 37 s from -20 on, 9 bins: answers before -20, at 313 and later, and without ts are not counted
                counts, tot = timeline_model(sc, w.slot, w.group, GROUPS, w.ts, w.cls, -20, 37, 9, al, cut, tracks, **case)
                loop = np.zeros(9, np.int64)
                for r, _ in want:
                    if w.ts[r] != NO_TS and 0 <= (int(w.ts[r]) + 20) // 37 < 9:
                        loop[(int(w.ts[r]) + 20) // 37] += 1
                assert tot[0] == len(want) and counts[0].tolist() == loop.tolist() and counts[0].sum() <= tot[0]


def test_a_row_without_the_attribute_never_passes():
    ts, cls = np.array([NO_TS, 5, 5]), np.array([3, -1, 3])
    assert passing(ts, cls).tolist() == [True, True, True]
    assert passing(ts, cls, ts_range=(None, None)).tolist() == [False, True, True]
    assert passing(ts, cls, classes=(3,)).tolist() == [True, False, True]
    assert passing(ts, cls, (5, 5), (3,)).tolist() == [False, False, True]


FOLDER = "data/cameras/front/objects/2026-01-01"


def test_row_table_parses_ts_and_class():
    names = {"12.5_3_0.jpg": (12, 0), "-4.9_3_2.jpg": (-4, 2), "snapshot.jpg": (NO_TS, -1), "abc_3_2.jpg": (NO_TS, -1), "7.0_x_2.jpg": (NO_TS, -1),
             "100.0_3_256.jpg": (100, -1), "100.0_3_-2.jpg": (100, -1), "3000000000.0_1_5.jpg": (NO_TS, 5), "-2147483648.0_1_5.jpg": (NO_TS, 5),
             "2147483647.0_1_255.jpg": (2147483647, 255), "1e400_1_1.jpg": (NO_TS, -1), "5.0_1_2.png": (NO_TS, -1), "5.0_1": (NO_TS, -1)}
    t = O._RowTable()
    t.extend([f"{FOLDER}/{n}" for n in names])
    assert list(zip(t.ts, t.cls)) == list(names.values())
    assert [O._RowTable.name_attrs(n) for n in names] == list(names.values())
    assert _lib.ROW_NO_TS == NO_TS
    ts, c = t.attrs(1)
    assert ts.dtype == np.int32 and c.dtype == np.int32 and ts.tolist() == t.ts[1:] and c.tolist() == t.cls[1:]


def test_extend_and_remove_keep_ts_and_class_in_step():
    rng = np.random.default_rng(5)
    t = O._RowTable()
    paths = []
    for i in range(60):
        name = f"snap{i}.jpg" if i % 7 == 0 else f"{int(rng.integers(-5, 90))}.5_{int(rng.integers(0, 6))}_{CLASSES[i % 6]}.jpg"
        paths.append(f"data/cameras/{'front' if i % 2 else 'back'}/objects/2026-01-0{1 + i % 3}/{i}_{name}" if i % 11 == 5 else
                     f"data/cameras/{'front' if i % 2 else 'back'}/objects/2026-01-0{1 + i % 3}/{name}")
    t.extend(paths[:25]); t.extend(paths[25:])
    want = [O._RowTable.name_attrs(p) for p in paths]
    assert list(zip(t.ts, t.cls)) == want and len({w for w in want}) > 20
    mask = rng.random(60) < 0.4
    assert t.remove(mask) == int(mask.sum())
    keep = np.flatnonzero(~mask)
    assert t.paths == [paths[r] for r in keep] and list(zip(t.ts, t.cls)) == [want[r] for r in keep]
    assert len(t.ts) == len(t.cls) == len(t.slot) == len(t.group) == len(t.paths)
    f = O.EmbeddingIndex.row_filter((0, 40), (0, 2))
    assert t.passing(f).tolist() == passing(t.ts, t.cls, (0, 40), (0, 2)).tolist() and t.passing(None).all()
    t.extend(paths[:3])
    assert list(zip(t.ts, t.cls))[-3:] == want[:3]


def test_python_side_argument_checks():
    rf = O.EmbeddingIndex.row_filter
    assert rf() is None and rf(None, None) is None
    f = rf((3, 3), [0, 63, 64, 255])
    assert (f.use_ts, f.ts_min, f.ts_max, f.use_cls) == (1, 3, 3, 1)
    assert list(f.cls_mask) == [1 | 1 << 63, 1, 0, 1 << 63]
    f = rf((None, 9))
    assert (f.use_ts, f.ts_min, f.ts_max, f.use_cls, list(f.cls_mask)) == (1, -(1 << 31), 9, 0, [0, 0, 0, 0])
    f = rf(None, np.array([7, 7, 2]))
    assert (f.use_ts, f.use_cls, list(f.cls_mask)) == (0, 1, [1 << 7 | 1 << 2, 0, 0, 0])
    for bad in (dict(ts_range=(5, 4)), dict(classes=[]), dict(classes=[256]), dict(classes=[-1]), dict(ts_range=(1 << 31, None))):
        with pytest.raises(ValueError):
            rf(**bad)
    finder = O.ObjectFinder("nowhere")
    for call in (finder.search, finder.search_page, finder.timeline):
        with pytest.raises(ValueError):
            call(text_embedding=np.zeros(8, np.float32), ts_range=(5, 4))
        with pytest.raises(ValueError):
            call(text_embedding=np.zeros(8, np.float32), classes=())
    for bad in (dict(bin_seconds=0), dict(n_bins=0), dict(n_bins=4097)):
        with pytest.raises(ValueError):
            finder.timeline(text_embedding=np.zeros(8, np.float32), **bad)


def test_host_fallback_filters_like_the_reference_on_the_passing_crops(monkeypatch):
    """An index that cannot rank (the numpy double of tests/test_search_host.py): `search` with a row filter takes the host path
    over the passing rows and equals the reference's search over a dict that holds only the passing crops."""
    from test_search_host import FakeIndex, reference_search
    monkeypatch.setattr(O, "EmbeddingIndex", FakeIndex)
    rng = np.random.default_rng(11)
    dim, emb = 16, {}
    for i in range(400):
        name = f"snap{i}.jpg" if i % 13 == 4 else f"{int(rng.integers(0, 300))}.0_{int(rng.integers(0, 25))}_{CLASSES[int(rng.integers(0, 6))]}.jpg"
        v = np.zeros(dim, np.float32); v[0] = rng.random(); v[1 + i % (dim - 1)] = rng.random()      # one non-zero product: the same float however it is summed
        emb[f"data/cameras/{'front' if i % 3 else 'back'}/objects/2026-01-0{1 + i % 2}/{i}/{name}"] = v.reshape(1, -1)
    q = np.zeros(dim, np.float32); q[0] = 1.0
    f = O.ObjectFinder("nowhere")
    f.image_embeddings = emb
    for ts_range, classes in (((50, 200), None), (None, (0, 64)), ((50, 200), (2, 255))):
        ok = {p: e for p, e in emb.items() if passing(*[np.array([a]) for a in O._RowTable.name_attrs(p)], ts_range, classes)[0]}
        assert 10 < len(ok) < len(emb)
        for cam, k in ((None, 10), ("front", 500)):
            want = reference_search(ok, q, k, cam)
            assert want and f.search(top_k=k, cam_name=cam, text_embedding=q, ts_range=ts_range, classes=classes) == want
        everything = reference_search(ok, q, 10**9, "back")
        kept = [r for r in everything if not r[1] < 0.1]
        assert f.search_page(start=2, count=5, cam_name="back", text_embedding=q, min_score=0.1, ts_range=ts_range, classes=classes) == (kept[2:7], len(kept))
        counts, total = f.timeline(text_embedding=q, t0=0, bin_seconds=60, n_bins=4, cam_name="back", min_score=0.1, ts_range=ts_range, classes=classes)
        loop = np.zeros(4, np.int64)
        for p, _ in kept:
            b = O.event_img_info(os.path.basename(p).split(".jpg")[0])["ts"] // 60
            if b < 4:
                loop[b] += 1
        assert total == len(kept) and counts.tolist() == loop.tolist()
