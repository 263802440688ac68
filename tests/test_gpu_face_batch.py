"""The batched face path (ObjectFinder.locate_faces / faces_from_rows / faces_from_crops / embed_faces, BlazeFace.detect_batch,
ADAFACE.embed_batch_device -> csrc/crop.hip face_letterbox_kernel + face_align_kernel, csrc/blaze.hip's batched plan) against the
per-crop path's own oracle: oracle/cv_warp_oracle.py for the pixels and the geometry, oracle/blazeface_oracle.py for the detector.

Thirteen seeded crops: eight yield a face, two have no detection (raw top scores 0.53 and 0.68), two have faces 30.7 and 14.7 px
wide (the 50 px rule), one has its cut above the image.  Every live case has its top score at least 1e-2 away from 0.85 and
1.4e-4 above the runner-up, 14 x the f32 score bar of 1e-5: the first surviving row is the same row on the GPU."""
import numpy as np
import pytest

from clearcam_amd.weights import synthetic_adaface_state_dict, synthetic_blazeface_state_dict
from oracle import cv_warp_oracle as cvo
from oracle.blazeface_oracle import BlazeFaceOracle

pytestmark = pytest.mark.gpu

SHAPES = [(720, 960), (1280, 900), (500, 500), (640, 640), (1280, 1280), (1280, 960), (300, 200), (96, 128), (64, 64), (2, 2),
          (400, 1300), (1081, 607), (900, 1280)]
PATTERN = [c == "F" for c in "FFFFNFFNNNNFF"]


@pytest.fixture(scope="module")
def crops():
    rng = np.random.default_rng(20)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]


@pytest.fixture(scope="module")
def finder():
    from clearcam_amd.objects import ObjectFinder
    f = ObjectFinder()
    f.init_face(blazeface_kwargs=dict(state_dict=synthetic_blazeface_state_dict(555), dtype="f32"),
                adaface_kwargs=dict(state_dict=synthetic_adaface_state_dict(777), dtype="f32"))
    yield f
    f.turn_off_face()


@pytest.fixture(scope="module")
def oracle():
    return BlazeFaceOracle(synthetic_blazeface_state_dict(555))


@pytest.fixture(scope="module")
def oracle_firsts(crops, oracle):
    """Per crop: (the oracle's first surviving row on the oracle-letterboxed image or None, img_to_face is not None)."""
    out = []
    for c in crops:
        seen = []

        def det(x):
            seen.append(np.asarray(oracle(x)))
            return seen[-1]
        face = cvo.img_to_face(c, det)
        alive = seen[0][seen[0][:, 0] != 0]
        out.append((alive[0] if len(alive) else None, face is not None))
    return out


@pytest.fixture(scope="module")
def located(finder, crops):
    return finder.locate_faces(crops)


@pytest.fixture(scope="module")
def host_faces(finder, crops):
    return finder.faces_from_crops(crops)


def _alive(d):
    return d[d[:, 16] != 0]


@pytest.mark.parametrize("n,shape", [(3, (640, 640)), (2, (360, 480))])
def test_detect_batch_matches_oracle_per_image(finder, oracle, n, shape):
    imgs = np.random.default_rng(n * 1000 + shape[0]).integers(0, 256, (n, *shape, 3), dtype=np.uint8)
    got_all = finder.blazeface.detect_batch(imgs)
    assert got_all.shape == (n, 896, 17) and got_all.dtype == np.float32
    scale = min(256 / shape[1], 256 / shape[0])
    for img, got in zip(imgs, got_all):                               # the bars of test_blazeface_f32_matches_oracle
        ref = oracle(img)
        ra, ga = _alive(ref), _alive(got)
        assert len(ra) > 10 and len(ga) == len(ra)
        box, score = np.abs(ra[:, :16] - ga[:, :16]).max(), np.abs(ra[:, 16] - ga[:, 16]).max()
        print(f"detect_batch {shape} box err {box:.3g} (bar {2e-3 / scale:.3g}), score err {score:.3g} (bar {1e-5 * 256 / scale:.3g})")
        assert box <= 2e-3 / scale
        assert score <= 1e-5 * 256 / scale
        assert np.allclose(ref[ref[:, 16] == 0], got[got[:, 16] == 0], atol=1e-6)
        assert np.array_equal(ref[:, 16] != 0, got[:, 16] != 0)
    with pytest.raises(ValueError):
        finder.blazeface.detect_batch(imgs[0])


def test_locate_matches_oracle_first_rows(located, oracle_firsts):
    rows, found = located
    assert rows.shape == (13, 17) and rows.dtype == np.float32 and found.dtype == np.bool_
    assert [face for _, face in oracle_firsts] == PATTERN          # the oracle's own pattern is the one the cases were chosen for
    assert found.tolist() == PATTERN
    for i, (first, face) in enumerate(oracle_firsts):
        if face:
            box, score = np.abs(rows[i, :16] - first[:16]).max(), abs(rows[i, 16] - first[16])
            print(f"crop {i}: box err {box:.3g} px (bar {2e-3 / 0.4:.3g}), score err {score:.3g} (bar {1e-5 * 256 / 0.4:.3g})")
            assert box <= 2e-3 / 0.4                                # the f32 bar at BlazeFace's 640 -> 256 scale
            assert score <= 1e-5 * 256 / 0.4


def _expected(crop, row, ok):
    det = np.asarray(row)[None] if ok else np.zeros((1, 17))
    return cvo.img_to_face(crop, lambda x: det)


def _same(got, want):
    return (got is None and want is None) or (got is not None and want is not None and got.shape == (112, 112, 3)
                                              and got.dtype == np.uint8 and np.array_equal(got, want))


def test_faces_are_bit_equal_to_the_per_crop_arithmetic(finder, crops, located, host_faces):
    rows, found = located
    assert len(host_faces) == 13
    compared = 0
    for i, c in enumerate(crops):
        want = _expected(c, rows[i], found[i])
        assert _same(host_faces[i], want), i
        compared += want is not None
    assert compared >= 8
    # 35 crops: one chunk of 32 and a tail of 3 padded to 4; every copy equals its original
    tiled = finder.faces_from_crops([crops[i % 13] for i in range(35)])
    assert len(tiled) == 35
    for j, got in enumerate(tiled):
        assert _same(got, host_faces[j % 13]), j


def _row(crop_hw, box, eye_a, eye_b):
    """A BlazeFace row in 640-letterbox coordinates from a box (x1, y1, x2, y2) and two eyes in crop pixels."""
    h, w = crop_hw
    scale = 640 / max(h, w)
    top, left = (640 - int(h * scale)) // 2, (640 - int(w * scale)) // 2
    r = np.zeros(17, np.float64)
    r[0], r[1], r[2], r[3] = box[1] * scale + top, box[0] * scale + left, box[3] * scale + top, box[2] * scale + left
    r[4], r[5], r[6], r[7] = eye_a[0] * scale + left, eye_a[1] * scale + top, eye_b[0] * scale + left, eye_b[1] * scale + top
    r[16] = 0.9
    return r.astype(np.float32)


def test_alignment_kernel_on_chosen_geometry(finder):
    rng = np.random.default_rng(21)
    A, B = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8), rng.integers(0, 256, (200, 150, 3), dtype=np.uint8)
    a, b = A.shape[:2], B.shape[:2]
    cases = [(A, _row(a, (200, 150, 320, 280), (230, 200), (290, 200))),          # eyes level
             (A, _row(a, (200, 150, 320, 280), (260, 180), (260, 240))),          # 90 degrees
             (A, _row(a, (200, 150, 320, 280), (290, 240), (250, 200))),          # -135 degrees
             (A, _row(a, (200, 150, 320, 280), (290, 200), (230, 200))),          # 180 degrees
             (A, _row(a, (-40, -30, 120, 110), (20, 30), (70, 30))),              # the face box leaves the crop at the left and the top
             (A, _row(a, (270, -90, 330, -30), (280, -58.5), (320, -58.5))),      # cut = the crop's first pixel row alone
             (A, _row(a, (560, 400, 700, 560), (600, 450), (660, 470))),          # ... at the right and the bottom
             (B, _row(b, (30, 40, 110, 130), (55, 80), (95, 80))),                # upscaled crop, level
             (B, _row(b, (30, 40, 110, 130), (95, 110), (55, 70))),               # -135 degrees
             (B, _row(b, (50, 60, 90, 110), (60, 80), (80, 80))),                 # 40 px wide: None
             (A, _row(a, (200, -400, 320, -300), (230, -350), (290, -350)))]      # cut above the image: None
    tilts = []
    for crop, row in cases[:4]:
        g = finder._face_geometry(row, *crop.shape[:2])
        tilts.append(round(float(np.degrees(np.arctan2(-g.rot[1, 0], g.rot[0, 0])))))
    assert tilts == [0, 90, -135, 180]
    g = finder._face_geometry(cases[5][1], 480, 640)
    assert g.ch == 1 and g.cy1 == 0
    crops = [c for c, _ in cases] + [A]
    rows = np.stack([r for _, r in cases] + [cases[0][1]])
    found = np.array([True] * len(cases) + [False])                   # the last: a row the caller marks as not found
    got = finder.faces_from_rows(crops, rows, found)
    want = [_expected(c, r, ok) for c, r, ok in zip(crops, rows, found)]
    assert [w is None for w in want] == [False] * 9 + [True] * 3
    for i in range(len(crops)):
        assert _same(got[i], want[i]), i
    dev, pos = finder.faces_from_rows(crops, rows, found, device_out=True)
    assert dev.is_cuda and tuple(dev.shape) == (9, 112, 112, 3) and pos.tolist() == list(range(9))
    assert np.array_equal(dev.cpu().numpy(), np.stack(want[:9]))


def test_embeddings_of_a_batch(finder, crops, host_faces):
    emb, valid = finder.embed_faces(crops)
    assert emb.shape == (13, 512) and emb.dtype == np.float32
    assert valid.tolist() == PATTERN
    assert not emb[~valid].any()
    ref = finder.adaface.embed_batch(np.stack([f for f in host_faces if f is not None]))
    err = np.abs(emb[valid] - ref).max()
    print(f"embed_faces against embed_batch of the host faces: max err {err:.3g} (bar 1e-6)")
    assert err < 1e-6                                                  # the f32 bar of tests/test_gpu_face.py
    assert np.abs(np.linalg.norm(emb[valid], axis=1) - 1).max() < 1e-5


def test_errors(finder):
    with pytest.raises(ValueError, match="crop 1"):
        finder.faces_from_crops([np.zeros((8, 8, 3), np.uint8), np.zeros((1, 700, 3), np.uint8)])
    with pytest.raises(ValueError):
        finder.faces_from_crops([])
    with pytest.raises(ValueError):
        finder.embed_faces([])
    with pytest.raises(ValueError):
        finder.faces_from_rows([np.zeros((8, 8, 3), np.uint8)], np.zeros((2, 17), np.float32), np.zeros(2, bool))


def test_c_abi_takes_host_pixels_too(finder, crops, located, host_faces):
    """cc_face_locate / cc_face_align with pixels_on_device = 0 (the library uploads the packed crops itself) against the
    device-buffer calls the Python path makes."""
    import ctypes as C
    import torch
    from clearcam_amd import _lib
    from clearcam_amd.objects import pack_crops
    pick = [6, 7, 2]                                                  # (300,200) face, (96,128) no face, (500,500) face
    sub = [crops[i] for i in pick]
    packed, off, hs, ws = pack_crops(sub)
    B = 4                                                             # a plan the batched tests have built: pad with the first crop
    off, hs, ws = (np.concatenate([a, a[:1]]) for a in (off, hs, ws))
    first, idx = np.empty((B, 17), np.float32), np.empty(B, np.int32)
    _lib.check(_lib.lib().cc_face_locate(finder.blazeface._h, _lib.ptr(packed), packed.size, _lib.ptr(off), _lib.ptr(hs), _lib.ptr(ws), B, 0,
                                         _lib.ptr(first), _lib.ptr(idx), None))
    rows, _ = located
    assert np.array_equal(first[:3], rows[pick]) and np.array_equal(first[3], first[0])
    assert (idx >= 0).tolist() == rows[pick + [pick[0]]].any(axis=1).tolist() and idx[0] >= 0 and idx[2] >= 0
    keep = [k for k, i in enumerate(pick) if host_faces[i] is not None]
    rec = (_lib.FaceAlignRec * len(keep))()
    for r, k in zip(rec, keep):
        g = finder._face_geometry(first[k], int(hs[k]), int(ws[k]))
        r.offset, r.h, r.w = int(off[k]), int(hs[k]), int(ws[k])
        r.cx1, r.cy1, r.cw, r.ch, r.out_w, r.out_h = g.cx1, g.cy1, g.cw, g.ch, g.out_w, g.out_h
        r.rot[:] = g.rot.reshape(-1).tolist()
        r.place[:] = g.place.astype(np.float64).reshape(-1).tolist()
    out = torch.empty((len(keep), 112, 112, 3), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().cc_face_align(_lib.ptr(packed), packed.size, 0, C.byref(rec), len(keep), _lib.ptr(out), 0, None))
    assert np.array_equal(out.cpu().numpy(), np.stack([host_faces[pick[k]] for k in keep]))
    rec[0].cw = int(ws[keep[0]]) + 1                                  # a cut that leaves its crop is refused, not read
    with pytest.raises(_lib.CCError, match="cut lies outside"):
        _lib.check(_lib.lib().cc_face_align(_lib.ptr(packed), packed.size, 0, C.byref(rec), len(keep), _lib.ptr(out), 0, None))


def test_index_faces_stores_and_finds_them(finder, crops, tmp_path):
    from clearcam_amd.objects import ObjectFinder
    from clearcam_amd.store import EmbeddingStore
    pick = [2, 8, 6]                                                  # face, no face, face
    base = str(tmp_path / "cameras")
    paths = [f"{base}/front/objects/2026-01-02/{100 + i}_{i}_0.jpg" for i in pick]
    f = ObjectFinder(base)
    f.blazeface, f.adaface, f.face = finder.blazeface, finder.adaface, True          # the module's models
    valid = f.index_faces(paths, [crops[i] for i in pick])
    assert valid.tolist() == [PATTERN[i] for i in pick] == [True, False, True]
    emb, _ = finder.embed_faces([crops[i] for i in pick])
    st = EmbeddingStore(f"{base}/front/faces/2026-01-02", 512)
    assert st.paths() == [paths[0], paths[2]] and np.array_equal(st.rows(), emb[[0, 2]])
    assert list(f.face_embeddings) == [paths[0], paths[2]]
    hits = f.search(text_embedding=emb[2], top_k=2, is_face=True)
    assert hits[0][0] == paths[2] and abs(hits[0][1] - 1) < 1e-5
