"""ObjectFinder.forget / sync_store on an attached store: after crops leave the device matrix, every search answers exactly as a
second ObjectFinder freshly attached to a tree that never held them (same vectors -> the same f32 scores, compared with ==).

The trees are written from one specification ((camera, day) -> crops), each under its own root, so the stored paths are compared
relative to the root."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAMS, DAYS, PER = ("back", "front", "yard"), ("2026-01-01", "2026-01-02"), 40
FILTERS = ((None, None), ("back", None), ("front", None), (None, DAYS[0]), (None, DAYS[1]), ("back", DAYS[0]), ("yard", DAYS[1]))


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def spec():
    rng = np.random.default_rng(41)
    q = unit(rng.standard_normal(768))
    out, t = {}, 1000
    for cam in CAMS:
        for day in DAYS:
            crops = []
            for i in range(PER):
                t += 1
                name = f"{t}.0_{int(rng.integers(0, 12))}_2.jpg" if i % 9 else f"snap{t}.jpg"      # track ids shared across folders
                crops.append((name, unit(rng.standard_normal(768) + (2.0 if i % 7 == 3 else 0.0) * q)))
            out[(cam, day)] = crops
    out[("back", DAYS[0])].append(("notes.txt", unit(rng.standard_normal(768))))                   # a row the search never returns
    return out, q


def write_tree(root, folders):
    from clearcam_amd.store import EmbeddingStore
    for (cam, day), crops in folders.items():
        d = os.path.join(root, cam, "objects", day)
        EmbeddingStore(d, 768).append([f"{d}/{name}" for name, _ in crops], np.stack([v for _, v in crops]), durable=False)
    return root


def attached(root):
    from clearcam_amd.objects import ObjectFinder
    f = ObjectFinder(root)
    f.attach_store(capacity=64)
    return f


def answers(f, q):
    """Every filter x two depths -> [(path relative to the root, score)]"""
    out = {}
    for cam, day in FILTERS:
        for k in (10, 300):
            got = f.search(top_k=k, cam_name=cam, timestamp=day, text_embedding=q)
            out[(cam, day, k)] = [(os.path.relpath(p, f.base_path), s) for p, s in got]
    return out


def without(folders, *keys):
    return {k: v for k, v in folders.items() if k not in keys}


def test_forget_add_and_sync_equal_a_fresh_attach(tmp_path):
    folders, q = spec()
    a = attached(write_tree(str(tmp_path / "a" / "cameras"), folders))
    a._load_all_embeddings()
    assert len(a._dev["store"][0]) == len(a.image_embeddings) == 6 * PER + 1
    full = answers(a, q)
    assert full == answers(attached(write_tree(str(tmp_path / "full" / "cameras"), folders)), q)
    assert len(full[(None, None, 300)]) > 12 and full[("back", DAYS[0], 10)]

    # forget one (camera, day) folder: 40 crops and the row that is no crop
    gone = ("back", DAYS[0])
    before = set(a.image_embeddings)
    assert a.forget("back", DAYS[0]) == PER + 1
    b = attached(write_tree(str(tmp_path / "b" / "cameras"), without(folders, gone)))
    got = answers(a, q)
    assert got == answers(b, q) and got != full and got[("back", DAYS[0], 10)] == []
    lost = before - set(a.image_embeddings)
    assert len(lost) == PER + 1 and all(f"/cameras/back/objects/{DAYS[0]}/" in k for k in lost)
    assert len(a._dev["store"][0]) == len(a._dev["store"][1].paths) == 5 * PER
    assert a.forget("back", DAYS[0]) == 0                                       # nothing left to forget
    assert os.path.isdir(os.path.join(a.base_path, "back", "objects", DAYS[0]))  # nothing is deleted on disk

    # a new crop into the forgotten folder: its directory group is reused
    new = ("5000.0_3_2.jpg", unit(np.random.default_rng(42).standard_normal(768) + 3.0 * q))
    d = os.path.join(a.base_path, "back", "objects", DAYS[0])
    a.add_embedding(f"{d}/{new[0]}", new[1][None])
    folders_c = dict(without(folders, gone)); folders_c[gone] = [new]
    c = attached(write_tree(str(tmp_path / "c" / "cameras"), folders_c))
    got = answers(a, q)
    assert got == answers(c, q) and got[("back", DAYS[0], 10)][0][0].endswith(new[0])

    # the NVR deletes a day folder: sync_store drops its rows, once
    stale = ("front", DAYS[1])
    shutil.rmtree(os.path.join(a.base_path, "front", "objects", DAYS[1]))
    assert a.sync_store() == PER
    e = attached(write_tree(str(tmp_path / "e" / "cameras"), without(folders_c, stale)))
    assert answers(a, q) == answers(e, q)
    assert not any(f"/cameras/front/objects/{DAYS[1]}/" in k for k in a.image_embeddings)
    assert a.sync_store() == 0

    # a whole camera, then a whole day
    assert a.forget(cam_name="yard") == 2 * PER
    g = attached(write_tree(str(tmp_path / "g" / "cameras"), without(folders_c, stale, ("yard", DAYS[0]), ("yard", DAYS[1]))))
    assert answers(a, q) == answers(g, q)
    assert a.forget(timestamp=DAYS[1]) == PER                                   # back's second day is all that is left of it
    assert len(a._dev["store"][0]) == PER + 1 and a.forget(timestamp="1999-01-01") == 0


def test_forget_needs_an_argument_and_sync_store_needs_a_store(tmp_path):
    from clearcam_amd.objects import ObjectFinder
    folders, q = spec()
    a = attached(write_tree(str(tmp_path / "cameras"), folders))
    with pytest.raises(ValueError):
        a.forget()
    assert len(a._dev["store"][0]) == 6 * PER + 1
    assert ObjectFinder(str(tmp_path / "cameras")).sync_store() == 0            # nothing attached: a no-op
