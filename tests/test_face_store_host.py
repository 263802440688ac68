"""Host side of the batched face path (no GPU): `ObjectFinder.add_face_embeddings` stores 512-d rows under <cam>/faces/<day>/ as
clearcam.py:1233-1241 does, `_load_all_embeddings(face=True)` reads them back, and `_face_geometry` keeps the 50 px rule."""
import os

import numpy as np
import pytest

from clearcam_amd.objects import FaceGeometry, ObjectFinder
from clearcam_amd.store import EmbeddingStore


def _unit_rows(n, dim, seed):
    e = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return e / np.linalg.norm(e, axis=1, keepdims=True)


def test_add_face_embeddings_writes_the_faces_folder_and_reloads(tmp_path):
    base = str(tmp_path / "cameras")
    paths = [f"{base}/front/objects/2026-01-02/100_1_0.jpg", f"{base}/front/objects/2026-01-02/101_2_0.jpg",
             f"{base}/yard/objects/2026-01-03/102_3_0.jpg"]
    emb = _unit_rows(3, 512, 5)
    f = ObjectFinder(base)
    before = f._version["face"]
    f.add_face_embeddings(paths, emb)
    assert f._version["face"] > before and list(f.face_embeddings) == paths
    assert all(f.face_embeddings[p].shape == (1, 512) for p in paths)
    for cam, day, rows in (("front", "2026-01-02", [0, 1]), ("yard", "2026-01-03", [2])):
        folder = os.path.join(base, cam, "faces", day)
        st = EmbeddingStore(folder, 512)
        assert st.paths() == [paths[i] for i in rows] and np.array_equal(st.rows(), emb[rows])
        assert not os.path.exists(os.path.join(base, cam, "objects", day, "embeddings.f32"))   # nothing lands beside the crops
    f.add_face_embeddings(paths[2:], emb[2])                                # a single (512,) row appends
    assert len(EmbeddingStore(os.path.join(base, "yard", "faces", "2026-01-03"), 512)) == 2
    assert not f.image_embeddings                                           # the crop dict is untouched

    fresh = ObjectFinder(base)
    fresh._load_all_embeddings(face=True)
    assert sorted(fresh.face_embeddings) == sorted(paths)
    for i, p in enumerate(paths):
        assert np.array_equal(fresh.face_embeddings[p], emb[i:i + 1])


def test_add_face_embeddings_rejects_other_widths(tmp_path):
    base = str(tmp_path / "cameras")
    f = ObjectFinder(base)
    p = [f"{base}/front/objects/2026-01-02/100_1_0.jpg"]
    with pytest.raises(ValueError, match="512"):
        f.add_face_embeddings(p, _unit_rows(1, 768, 1))
    with pytest.raises(ValueError):
        f.add_face_embeddings(p, _unit_rows(2, 512, 1))                     # two rows for one path
    assert not f.face_embeddings and not os.path.exists(base)


def _row(x1, x2):
    r = np.zeros(17, np.float32)
    r[:4] = [200, x1, 300, x2]                   # ymin, xmin, ymax, xmax in a 640 x 640 crop: letterbox scale 1, no padding
    r[4:8] = [x1 + 15, 240, x2 - 15, 240]
    return r


def test_face_geometry_keeps_the_50_px_rule():
    assert ObjectFinder._face_geometry(_row(100, 149.9), 640, 640) is None
    g = ObjectFinder._face_geometry(_row(100, 150.1), 640, 640)
    assert isinstance(g, FaceGeometry)
    assert (g.cx1, g.cy1, g.cw, g.ch) == (25, 140, 200, 200)               # twice the larger side (100) around the eyes' midpoint
    assert g.rot.dtype == np.float64 and g.place.dtype == np.float32 and (g.out_w, g.out_h) == (200, 200)
    # in a (320, 640) crop the same letterbox row is a face of the same width, 160 rows further up: the cut is clipped at the top
    g2 = ObjectFinder._face_geometry(_row(100, 150.1), 320, 640)
    assert (g2.cx1, g2.cy1, g2.cw, g2.ch) == (25, 0, 200, 180)
