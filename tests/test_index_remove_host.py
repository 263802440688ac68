"""_RowTable.remove(mask): the host-side description of the rows after a removal equals a table rebuilt from the surviving paths.

What is compared is everything ObjectFinder.search reads: paths, track ids, the directory string of every row, the (camera, day)
filters mapped to directory strings, and the per-directory `truthy` / `bad` marks.  Group ids and track slots of the old table are
stable (the device matrix keeps storing them), so they are compared with the table BEFORE the removal, not with the rebuilt one."""
import numpy as np
import pytest

from clearcam_amd.objects import _RowTable

CAMS, DAYS = ("front", "back", "yard"), ("2026-01-01", "2026-01-02")


def world():
    rng = np.random.default_rng(5)
    paths = []
    for i in range(600):
        cam, day = CAMS[rng.integers(3)], DAYS[rng.integers(2)]
        d = f"data/cameras/{cam}/objects/{day}"
        kind = rng.integers(10)
        if kind == 0:
            paths.append(f"{d}/snap{i}.jpg")                       # no track id
        elif kind == 1:
            paths.append(f"{d}/{1000 + i}.0_0_2.jpg")              # id 0: an id, but falsy
        elif kind == 2:
            paths.append(f"{d}/note{i}.txt")                       # group 0
        else:
            paths.append(f"{d}/{1000 + i}.0_{int(rng.integers(1, 40))}_2.jpg")
    paths.append("data/cameras/lone/objects/2026-01-01/1.0_0_2.jpg")
    paths.append("data/cameras/lone/objects/2026-01-01/2.0_77_2.jpg")     # the only truthy id of its folder
    paths.append("data/cameras/lone/objects/2026-01-01/snap.jpg")
    paths.append("data/cameras/odd/objects/2026-01-02/3.0_5_2.jpg")
    paths.append("data/cameras/odd/objects/2026-01-02/not_a_stamp.jpg")   # the only name of its folder event_img_info cannot parse
    paths.append("data\\cameras\\win\\objects\\2026-01-02\\4.0_9_2.jpg")
    return paths


def build(paths):
    t = _RowTable()
    t.extend(list(paths))
    return t


def by_dir(t, values):
    return {t.dirs[g]: values[g] for g in set(t.group) if g}


def assert_same(t, want):
    assert t.paths == want.paths and t.oid == want.oid
    assert [t.dirs[g] for g in t.group] == [want.dirs[g] for g in want.group]
    assert by_dir(t, t.truthy) == by_dir(want, want.truthy)
    assert by_dir(t, t.bad) == by_dir(want, want.bad)
    for cam in (None,) + CAMS + ("lone", "odd", "win", "nobody"):
        for day in (None,) + DAYS + ("1999-01-01",):
            a, b = t.allowed(cam, day), want.allowed(cam, day)
            live = lambda tab, al: {tab.dirs[g] for g in set(tab.group) if g and al[g]}
            assert live(t, a) == live(want, b), (cam, day)
    assert len(t.group) == len(t.oid) == len(t.slot) == len(t.paths)
    assert t.slots().tolist() == [-1 if o is None else t.slot_of[o] for o in t.oid]


def masks(paths):
    rng = np.random.default_rng(6)
    n = len(paths)
    m = {"nothing": np.zeros(n, bool), "everything": np.ones(n, bool), "random half": rng.random(n) < 0.5,
         "one folder": np.array(["/cameras/back/objects/2026-01-02/" in p for p in paths]),
         "the only truthy id": np.array([p.endswith("2.0_77_2.jpg") for p in paths]),
         "the only unparsable name": np.array([p.endswith("not_a_stamp.jpg") for p in paths]),
         "first and last": np.isin(np.arange(n), (0, n - 1))}
    m["uint8"] = m["random half"].astype(np.uint8) * 7
    return m


@pytest.mark.parametrize("name", list(masks(world())))
def test_remove_equals_a_table_rebuilt_from_the_survivors(name):
    paths = world()
    mask = masks(paths)[name]
    t, before = build(paths), build(paths)
    assert t.remove(mask) == int(np.count_nonzero(mask))
    assert_same(t, build([p for p, m in zip(paths, mask) if not m]))
    # group ids of the surviving directories and the slots of the track ids are what the device stores: unchanged
    assert t.dirs == before.dirs and t.dir_id == before.dir_id and t.slot_of == before.slot_of
    keep = np.flatnonzero(np.asarray(mask) == 0)
    assert t.group == [before.group[r] for r in keep] and t.slot == [before.slot[r] for r in keep]


def test_marks_follow_the_rows_that_carried_them():
    paths = world()
    t = build(paths)
    lone, odd = t.dir_id["data/cameras/lone/objects/2026-01-01/"], t.dir_id["data/cameras/odd/objects/2026-01-02/"]
    assert t.truthy[lone] and not t.bad[lone] and t.truthy[odd] and t.bad[odd]
    t.remove(masks(paths)["the only truthy id"])
    assert not t.truthy[lone] and t.truthy[odd] and t.bad[odd]
    t.remove([p.endswith("not_a_stamp.jpg") for p in t.paths])
    assert not t.bad[odd] and t.truthy[odd]


def test_a_later_crop_reuses_the_group_and_the_slot():
    paths = world()
    t = build(paths)
    d = "data/cameras/back/objects/2026-01-02/"
    g, slot77 = t.dir_id[d], t.slot_of[77]
    t.remove([d in p or p.endswith("2.0_77_2.jpg") for p in paths])
    assert g not in t.group and not t.truthy[g] and not t.bad[g]
    groups = t.extend([d + "9999.0_77_2.jpg"])
    assert groups.tolist() == [g] and t.group[-1] == g and t.truthy[g] and t.slot[-1] == slot77
    assert len(t.dirs) == len(build(paths).dirs)


def test_a_mask_of_the_wrong_length_is_refused():
    t = build(world())
    n = len(t.paths)
    with pytest.raises(ValueError):
        t.remove(np.zeros(n - 1, bool))
    assert len(t.paths) == n


def test_forget_without_an_attached_store_drops_the_dict_entries():
    from clearcam_amd.objects import ObjectFinder
    f = ObjectFinder("nowhere")
    paths = [p for p in world() if "\\" not in p]
    f.image_embeddings = {p: np.zeros((1, 768), np.float32) for p in paths}
    with pytest.raises(ValueError):
        f.forget()
    n = sum("/cameras/back/" in p and "/objects/2026-01-02/" in p for p in paths)
    assert n > 0 and f.forget("back", "2026-01-02") == n and len(f.image_embeddings) == len(paths) - n
    n_day = sum("/objects/2026-01-01/" in p for p in f.image_embeddings)
    assert f.forget(timestamp="2026-01-01") == n_day and not any("/objects/2026-01-01/" in p for p in f.image_embeddings)
    n_cam = sum("/cameras/front/" in p for p in f.image_embeddings)
    assert f.forget(cam_name="front") == n_cam and f.forget(cam_name="front") == 0
    assert f.sync_store() == 0
