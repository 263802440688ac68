"""GPU tests of the alert path (cc_watch_*, WatchList, ObjectFinder.check_alerts): scores bit-equal to the f32 index's single-query
scan, pair independence, strictness at the tie, the sequential rule against the numpy model, edges, and the finder end to end."""
from dataclasses import replace

import numpy as np
import pytest

import watch_cases as wc

pytestmark = pytest.mark.gpu

BATCHES = (1, 3, 4, 5, 63, 64, 65, 255)
TABLES = (1, 7, 8, 9, 31, 32, 33, 64, 65, 300)


def _watch(dim=768):
    from clearcam_amd.objects import WatchList
    return WatchList(dim)


@pytest.mark.parametrize("dim", (256, 512, 768))
def test_scores_are_the_index_scan_scores_bit_for_bit(dim):
    """WatchList.scores(E) == the scores of an f32 EmbeddingIndex holding E, queried with the descriptions ONE AT A TIME (the scan
    path), for every batch size and table size; and within 2e-6 of the float64 product, the project's bar for the scan on unit rows."""
    from clearcam_amd.objects import EmbeddingIndex
    rng = np.random.default_rng(100 + dim)
    E, D = wc.unit_rows(rng, max(BATCHES), dim), wc.unit_rows(rng, max(TABLES), dim)
    exact = E.astype(np.float64) @ D.astype(np.float64).T
    w = _watch(dim)
    worst = 0.0
    for B in BATCHES:
        ix = EmbeddingIndex(dim, 256, storage="f32")
        ix.add(E[:B])
        ref = np.empty((B, len(D)), np.float32)
        for a in range(len(D)):
            ref[:, a] = ix.scores(D[a])[0]
            assert ix.last_scores_path() == 0                                # single queries take the scan path
        ix.close()
        for A in TABLES:
            w.set(D[:A], np.zeros(A, np.float32), np.zeros(A, np.int32))
            got = w.scores(E[:B])
            assert got.shape == (B, A) and np.array_equal(got, ref[:, :A]), (dim, B, A)
            worst = max(worst, float(np.abs(got - exact[:B, :A]).max()))
    print(f"dim {dim}: max |score - float64 product| = {worst:.3g}")
    assert worst <= 2e-6
    w.close()


def test_a_score_depends_on_its_pair_alone():
    import torch
    rng = np.random.default_rng(11)
    E, D = wc.unit_rows(rng, 130, 768), wc.unit_rows(rng, 70, 768)
    w = _watch()
    zeros = lambda n: (np.zeros(n, np.float32), np.zeros(n, np.int32))
    w.set(D, *zeros(70))
    full = w.scores(E)
    assert np.array_equal(w.scores(E[37:102]), full[37:102])                 # a sub-batch
    assert np.array_equal(w.scores(E[5]), full[5:6])                         # one crop, (dim,) input
    assert np.array_equal(w.scores(torch.as_tensor(E).cuda()), full)         # the batch in device memory
    perm = rng.permutation(70)
    w.set(D[perm], *zeros(70))
    assert np.array_equal(w.scores(E), full[:, perm])                        # a permuted alert table
    w.set(D[9:12], *zeros(3))
    assert np.array_equal(w.scores(E), full[:, 9:12])                        # a smaller table
    cols = [0, 3, 64, 255, 256, 767]
    onehot = np.zeros((len(cols), 768), np.float32)
    onehot[np.arange(len(cols)), cols] = 1.0
    w.set(onehot, *zeros(len(cols)))
    assert np.array_equal(w.scores(E), E[:, cols])                           # a one-hot description returns the column bit for bit
    with pytest.raises(ValueError):
        w.scores(np.zeros((2, 512), np.float32))                             # the width is checked
    with pytest.raises(ValueError):
        w.set(np.zeros((2, 512), np.float32), np.zeros(2), np.zeros(2))
    w.close()


def test_strictly_greater_at_the_tie_nan_and_other_cameras():
    rng = np.random.default_rng(12)
    E, D = wc.unit_rows(rng, 9, 768), wc.unit_rows(rng, 3, 768)
    w = _watch()
    grp = np.array([1, 0, 0], np.int32)                                       # alert 0 belongs to another camera
    crops = np.zeros(9, np.int32)
    w.set(D, np.zeros(3, np.float32), grp)
    S = w.scores(E)
    a = 2
    b = int(np.argmax(S[:, a]))                                               # no other crop scores above it
    s = S[b, a]
    thr = np.array([-1.0, 2.0, s], np.float32)                                # alert 0: threshold -1, every score passes it
    w.set(D, thr, grp)
    alert, score = w.match(E, crops)
    assert (alert == -1).all() and (score == 0).all()                         # score == threshold does not fire; another camera's alert never does
    thr[a] = np.nextafter(s, np.float32(-np.inf))
    w.set(D, thr, grp)
    alert, score = w.match(E, crops)
    want = np.full(9, -1, np.int32); want[b] = a
    assert np.array_equal(alert, want) and score[b] == s and (np.delete(score, b) == 0).all()
    # a crop row holding a NaN fires nothing and leaves its neighbours alone
    thr = np.array([-1.0, -1.0, -1.0], np.float32)                            # alerts 1 and 2 fire for the first two clean crops of camera 0
    w.set(D, thr, grp)
    En = E.copy(); En[0, 5] = np.nan; En[3, 700] = np.nan
    Sn = w.scores(En)
    assert np.isnan(Sn[[0, 3]]).all() and np.array_equal(np.delete(Sn, [0, 3], 0), np.delete(S, [0, 3], 0))
    alert, score = w.match(En, crops)
    assert alert.tolist() == [-1, 1, 2, -1, -1, -1, -1, -1, -1] and score[1] == S[1, 1] and score[2] == S[2, 2] and score[0] == 0
    ref = wc.resolve(Sn, thr, grp, crops, None)
    assert np.array_equal(alert, ref[0]) and np.array_equal(score, ref[1])
    w.close()


@pytest.mark.parametrize("seed", wc.SEEDS)
@pytest.mark.parametrize("shape", wc.WORLDS)
def test_match_is_the_reference_rule(shape, seed):
    """On the host test's worlds, with S taken from WatchList.scores and the thresholds recomputed from it: match == the numpy model
    exactly, alert and score, with `armed` given, with armed=None and with the outputs left on the device."""
    world = wc.world(*shape, seed)
    w = _watch()
    A = len(world.D)
    w.set(world.D, np.zeros(A, np.float32), world.alert_group)
    S = w.scores(world.E)
    assert np.abs(S - wc.product64(world.E, world.D)).max() <= 2e-6
    thr = wc.median_thresholds(S, world.alert_group, world.crop_group)
    w.set(world.D, thr, world.alert_group)
    for armed in (world.armed, None):
        want_alert, want_score = wc.resolve(S, thr, world.alert_group, world.crop_group, armed)
        alert, score = w.match(world.E, world.crop_group, armed)
        assert alert.dtype == np.int32 and score.dtype == np.float32
        assert np.array_equal(alert, want_alert) and np.array_equal(score, want_score)
        d_alert, d_score = w.match(world.E, world.crop_group, armed, device_out=True)
        assert d_alert.is_cuda and d_score.is_cuda
        assert np.array_equal(d_alert.cpu().numpy(), want_alert) and np.array_equal(d_score.cpu().numpy(), want_score)
        if armed is not None:                                                 # the host test's conditions, on the device's answer
            fired, later = wc.check_not_vacuous(S, thr, world, armed, alert)
            print(f"world {shape} seed {seed}: {fired} of {int(armed.sum())} armed alerts fired, {later} crops received a later alert")
    import torch
    alert, score = w.match(torch.as_tensor(world.E).cuda(), world.crop_group, world.armed)      # the batch resident on the device
    want_alert, want_score = wc.resolve(S, thr, world.alert_group, world.crop_group, world.armed)
    assert np.array_equal(alert, want_alert) and np.array_equal(score, want_score)
    w.close()


def test_edges_empty_table_full_table_words_and_a_single_hit():
    from clearcam_amd._lib import CCError
    from clearcam_amd.objects import WatchList
    rng = np.random.default_rng(13)
    E = wc.unit_rows(rng, 40, 768)
    w = _watch()
    assert len(w) == 0
    alert, score = w.match(E[:5], np.zeros(5, np.int32))                      # an empty table: nothing fires, nothing is launched
    assert alert.tolist() == [-1] * 5 and score.tolist() == [0.0] * 5
    d_alert, d_score = w.match(E[:5], np.zeros(5, np.int32), device_out=True)
    assert d_alert.cpu().tolist() == [-1] * 5 and d_score.cpu().tolist() == [0.0] * 5
    assert w.scores(E[:5]).shape == (5, 0)
    alert, score = w.match(E[:0], np.zeros(0, np.int32))                      # an empty batch
    assert alert.shape == (0,) and score.shape == (0,)

    D = wc.unit_rows(rng, 33, 768)                                            # set again: 33 alerts, two words
    zero_grp = np.zeros(33, np.int32)
    w.set(D, np.full(33, -1.0, np.float32), zero_grp)
    assert len(w) == 33
    alert, score = w.match(E, np.zeros(40, np.int32))                         # every pair hits: crop b takes alert b, the rest nothing
    S = w.scores(E)
    assert alert.tolist() == list(range(33)) + [-1] * 7
    assert np.array_equal(score[:33], S[np.arange(33), np.arange(33)]) and (score[33:] == 0).all()
    w.set(D[:0], np.zeros(0, np.float32), np.zeros(0, np.int32))              # A == 0 clears it
    assert len(w) == 0 and w.match(E[:2], np.zeros(2, np.int32))[0].tolist() == [-1, -1]

    # table indices on both sides of words 31/32 and 63/64: only those alerts are armed
    D = wc.unit_rows(rng, 70, 768)
    w.set(D, np.full(70, -1.0, np.float32), np.zeros(70, np.int32))
    armed = np.zeros(70, np.uint8); armed[[31, 32, 63, 64]] = 1
    alert, score = w.match(E[:6], np.zeros(6, np.int32), armed)
    S = w.scores(E[:6])
    assert alert.tolist() == [31, 32, 63, 64, -1, -1]
    assert np.array_equal(score[:4], S[np.arange(4), [31, 32, 63, 64]])

    # one alert is the only hit of every crop: the first crop gets it, the rest nothing
    thr = np.full(70, 2.0, np.float32); thr[40] = -1.0
    w.set(D, thr, np.zeros(70, np.int32))
    alert, score = w.match(E, np.zeros(40, np.int32))
    assert alert.tolist() == [40] + [-1] * 39 and score[0] == w.scores(E[:1])[0, 40] and (score[1:] == 0).all()

    # the largest table, two crops; the last alert is the only one above its threshold for the second crop's camera
    A = WatchList.MAX_ALERTS
    D = wc.unit_rows(rng, A, 768)
    grp = np.zeros(A, np.int32); grp[A - 1] = 1
    thr = np.full(A, 2.0, np.float32); thr[[1500, A - 1]] = -1.0
    w.set(D, thr, grp)
    assert len(w) == A
    alert, score = w.match(E[:2], np.array([0, 1], np.int32))
    S = w.scores(E[:2])
    assert S.shape == (2, A) and np.abs(S - wc.product64(E[:2], D)).max() <= 2e-6
    assert alert.tolist() == [1500, A - 1] and score[0] == S[0, 1500] and score[1] == S[1, A - 1]
    ref = wc.resolve(S, thr, grp, [0, 1], None)
    assert np.array_equal(alert, ref[0]) and np.array_equal(score, ref[1])

    with pytest.raises(CCError, match="at most 2048"):
        w.set(np.zeros((A + 1, 768), np.float32), np.zeros(A + 1, np.float32), np.zeros(A + 1, np.int32))
    assert len(w) == A                                                        # a refused table leaves the old one
    with pytest.raises(CCError, match="2\\^24"):
        w.set(D[:2], np.zeros(2, np.float32), np.array([0, 1 << 24], np.int32))
    with pytest.raises(CCError, match="dim % 256"):
        WatchList(320)
    with pytest.raises(ValueError):
        w.match(E[:3], np.zeros(2, np.int32))
    w.close()


def test_dim_512_and_a_wide_row():
    """The other widths: 512 (the face embedder's) against the model, and 4096, where a pass holds four descriptions."""
    rng = np.random.default_rng(14)
    for dim, B, A in ((512, 37, 45), (4096, 18, 13)):
        E, D = wc.unit_rows(rng, B, dim), wc.unit_rows(rng, A, dim)
        grp, crops = rng.integers(0, 3, A).astype(np.int32), rng.integers(0, 3, B).astype(np.int32)
        w = _watch(dim)
        w.set(D, np.zeros(A, np.float32), grp)
        S = w.scores(E)
        assert np.abs(S - wc.product64(E, D)).max() <= 2e-6
        thr = wc.median_thresholds(S, grp, crops)
        w.set(D, thr, grp)
        alert, score = w.match(E, crops)
        ref = wc.resolve(S, thr, grp, crops, None)
        assert np.array_equal(alert, ref[0]) and np.array_equal(score, ref[1]) and (alert >= 0).sum() >= 3
        w.close()


def test_object_finder_check_alerts_end_to_end(tmp_path):
    """ObjectFinder with seeded synthetic CLIP weights, two cameras with three alerts each: check_alerts on a batch of crop embeddings
    == AlertBook's rules walked literally over `desc_emb @ emb.T`; and every fired crop is found by searching the attached f32 store
    for the alert's description just above its threshold, with the score the alert fired with."""
    import torch
    from conftest import vocab_tokenizer
    from clearcam_amd.arch import CLIP_TINY
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.weights import synthetic_clip_state_dict
    arch = replace(CLIP_TINY, embed=768, t_vocab=49408)
    f = ObjectFinder(base_path=str(tmp_path / "cameras"))
    f.init_clip(state_dict=synthetic_clip_state_dict(arch, 4321), arch=arch, dtype="f32", tokenizer=vocab_tokenizer())
    rng = np.random.default_rng(15)
    B = 24
    crops = []
    for _ in range(B):                                                         # two flat colours side by side plus noise: crops that differ
        h, wd = int(rng.integers(30, 90)), int(rng.integers(30, 90))
        c = np.empty((h, wd, 3), np.float64)
        cut = int(rng.integers(5, wd - 5))
        c[:, :cut], c[:, cut:] = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
        crops.append(np.clip(c + rng.normal(0, 20, c.shape), 0, 255).astype(np.uint8))
    x = f.preprocess_crops(crops, arch.image_size)
    emb_dev = torch.empty(B, 768, device=x.device)
    f.model.precompute_embedding_device(x, emb_dev)
    torch.cuda.synchronize()
    emb = emb_dev.cpu().numpy()
    cams = ["gate" if i % 3 else "yard" for i in range(B)]
    paths = [str(tmp_path / "cameras" / cams[i] / "objects" / "2026-01-01" / f"{1000 + i}.0_{i + 1}_0.jpg") for i in range(B)]
    texts = {"gate": ["ferrari f40", "a person walking a dog", "text here"], "yard": ["A RED Car, parked!", "3 men 42 dogs 2024", "emoji 🚗 car"]}
    for cam, descs in texts.items():
        f.set_alerts(cam, {f"{cam}-{i}": {"desc": d} for i, d in enumerate(descs)})
    flat = f.alerts.flat()
    assert len(flat) == 6 and all(a.desc_emb is not None and a.desc_emb.shape == (768,) and a.threshold == 0.28 for _, _, a in flat)
    for (_, _, a), d in zip(flat, texts["gate"] + texts["yard"]):
        assert np.array_equal(a.desc_emb, f.model._encode_text(d, realize=True))     # the batch encode == the reference's lazy single encode
    # thresholds from the literal products: for each alert the middle of the widest gap in the middle third of its camera's scores, so
    # that about half of the crops pass and no score lies within rounding of a threshold
    for cam, k, a in flat:
        col = np.sort([float(a.desc_emb @ emb[i].T) for i in range(B) if cams[i] == cam])
        lo = len(col) // 3
        j = lo + int(np.argmax(np.diff(col[lo:len(col) - lo])))
        assert col[j + 1] - col[j] > 1e-5
        a.threshold = float((col[j] + col[j + 1]) / 2)
    f.alerts._changed()                                                        # thresholds changed: the table is uploaded again
    f.alerts.cams["yard"]["yard-1"].active = False

    def literal(now):
        out = []
        for i in range(B):
            for k, v in f.alerts.cams[cams[i]].items():
                if now - v.last_det < 60 or not v.is_active():
                    continue
                if v.desc is None:
                    continue
                similarity = float(v.desc_emb @ emb[i].T)
                if similarity > v.threshold:
                    out.append((i, k, similarity))
                    v.last_det = now
                    break
        return out

    want = literal(5000.0)
    for _, _, a in flat:
        a.last_det = 0.0
    got = f.check_alerts(paths, emb_dev, now=5000.0)                           # the embeddings never left the device
    assert [(p, k) for p, _, k, _, _ in got] == [(paths[i], k) for i, k, _ in want]
    assert len(got) >= 3 and {g[1] for g in got} == {"gate", "yard"} and "yard-1" not in {g[2] for g in got}
    assert all(g[1] == cams[paths.index(g[0])] and g[3] == f.alerts.cams[g[1]][g[2]].desc for g in got)
    assert np.allclose([g[4] for g in got], [s for _, _, s in want], atol=2e-6, rtol=0)
    assert f.check_alerts(paths, emb, now=5030.0) == []                        # everything that can fire is cooling down
    again = f.check_alerts(paths, emb, now=5060.0)                             # 60 s later, host embeddings: the same answer
    assert [(g[0], g[2], g[4]) for g in again] == [(g[0], g[2], g[4]) for g in got]

    assert f.attach_store() == 0
    for p, e in zip(paths, emb):
        f.add_embedding(p, e)
    for p, cam, k, desc, s in got:
        a = f.alerts.cams[cam][k]
        res, total = f.search_page(text_embedding=a.desc_emb, cam_name=cam, min_score=np.nextafter(np.float32(a.threshold), np.float32(np.inf)), count=B)
        assert (p, s) in res and total == len(res) and all(r[1] > a.threshold for r in res)   # found, with exactly the score it fired with
    f.remove_alerts("gate")
    assert [(g[0], g[2]) for g in f.check_alerts(paths, emb, now=9000.0)] == [(g[0], g[2]) for g in got if g[1] == "yard"]
    f.turn_off_clip()
