"""The rows of one device matrix as the host knows them: crop names, folders, track slots, ts and class.  numpy and `os` only: no CLIP, no GPU."""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _lib


def event_img_info(image: str) -> dict:
    """``clearcam.py:1193``: '<ts>_<track id>_<class id>' crop file stem."""
    p = image.split("_")
    return {"ts": int(float(p[0])), "object_id": int(p[1]), "class_id": int(p[2])}


def pick_track_rows(row: int, members) -> np.ndarray:
    """The query rows of `ObjectFinder.similar(..., whole_track=True)`: `members` are the rows of the clicked crop's track (`row`
    among them).  Up to _lib.LIKE_MAX_ROWS rows: all of them.  More: the clicked row plus 63 of the m - 1 others, those at
    positions np.linspace(0, m - 2, 63).round() of the others in row order, so the pick spans the whole track, is the same on every
    call and never drops the clicked crop.  Ascending, distinct."""
    m = np.unique(np.asarray(members, np.int64))
    if int(row) not in m:
        raise ValueError("the clicked row is not among the track's rows")
    if m.size <= _lib.LIKE_MAX_ROWS:
        return m
    others = m[m != int(row)]
    at = np.linspace(0, others.size - 1, _lib.LIKE_MAX_ROWS - 1).round().astype(np.int64)
    return np.sort(np.r_[others[at], np.int64(row)])


class _RowTable:
    """Host-side description of the rows of one device matrix, built ONCE when rows are added, so that a search costs
    O(groups + candidates) Python instead of the reference's O(N) loop (models/objects.py:365-376).

    The reference filters a crop by two substring tests on its '/'-normalised path — f"/cameras/{cam}/" and
    f"/objects/{day}/" or "/objects/video/" (:368-371).  Both patterns end in '/', so they can only match inside the
    directory part of the path: rows are grouped by directory string and the tests run once per group.  Group 0 holds the
    rows the reference never returns (file name not *.jpg, :374)."""

    def __init__(self):
        self.paths: List[str] = []
        self.dirs: List[str] = [""]            # group id -> directory part (group 0: never allowed)
        self.dir_id: Dict[str, int] = {}
        self.truthy: List[bool] = [False]      # group has a crop whose track id is truthy (the `any(item[2] ...)` of :378)
        self.bad: List[bool] = [False]         # group has a *.jpg name event_img_info cannot parse (the reference raises on it)
        self.group: List[int] = []
        self.oid: List[Optional[int]] = []     # track id per row exactly as event_img_info returns it (any sign), None = no '_' in the name
        self.slot_of: Dict[int, int] = {}      # track id -> dense slot, in order of first appearance (id 0 and negative ids are ids)
        self.slot: List[int] = []              # slot per row, -1 where oid is None: what the device reduces by (EmbeddingIndex.search_tracks)
        self.ts: List[int] = []                # seconds into the day's recording per row (event_img_info's `ts`), _lib.ROW_NO_TS = none
        self.cls: List[int] = []               # detector class per row (event_img_info's `class_id`) in [0, 255], -1 = none
        self.row: Dict[str, int] = {}          # path -> row; a path stored twice names its last row (the reference's dict keeps the last value of a key)

    def row_of(self, path: str) -> int:
        """The row that holds `path` (a stored key, exactly as it was given); KeyError when there is none."""
        return self.row[path]

    @staticmethod
    def name_attrs(path: str) -> Tuple[int, int]:
        """(ts, class) of a crop as the device stores them: `event_img_info` of the '<ts>_<track>_<class>.jpg' name, i.e.
        int(float(first part)) and int(third part).  "None" (_lib.ROW_NO_TS / -1) when the name is no *.jpg, has no '_', does
        not parse, or the value does not fit (ts: an int32 other than ROW_NO_TS itself; class: [0, 255])."""
        fn = os.path.basename(path)
        if not fn.lower().endswith(".jpg") or "_" not in fn:
            return _lib.ROW_NO_TS, -1
        try:
            info = event_img_info(fn.split(".jpg")[0])
        except Exception:                      # noqa: BLE001  a name the reference raises on carries no attributes
            return _lib.ROW_NO_TS, -1
        ts, c = info["ts"], info["class_id"]
        return (ts if _lib.ROW_NO_TS < ts < (1 << 31) else _lib.ROW_NO_TS), (c if 0 <= c <= 255 else -1)

    def describe(self, path: str) -> Tuple[int, int]:
        norm = path.replace("\\", "/")
        fn = os.path.basename(path)
        if not fn.lower().endswith(".jpg"):
            return 0, None
        d = norm[:norm.rfind("/") + 1]
        g = self.dir_id.get(d)
        if g is None:
            g = self.dir_id[d] = len(self.dirs)
            self.dirs.append(d); self.truthy.append(False); self.bad.append(False)
        oid = None
        if "_" in fn:
            try:
                oid = event_img_info(fn.split(".jpg")[0])["object_id"]
            except Exception:                  # noqa: BLE001  names the reference raises on take the exact slow path at search time
                self.bad[g] = True
                oid = None
        if oid:                                # the reference's `any(item[2] ...)`: id 0 and None are falsy
            self.truthy[g] = True
        return g, oid

    def extend(self, paths) -> np.ndarray:
        groups = np.empty(len(paths), np.int32)
        base = len(self.paths)
        for i, p in enumerate(paths):
            g, oid = self.describe(p)
            groups[i] = g
            self.row[p] = base + i
            self.group.append(g); self.oid.append(oid)
            self.slot.append(-1 if oid is None else self.slot_of.setdefault(oid, len(self.slot_of)))
            ts, c = self.name_attrs(p)
            self.ts.append(ts); self.cls.append(c)
        self.paths.extend(paths)
        return groups

    def slots(self, start: int = 0) -> np.ndarray:
        return np.asarray(self.slot[start:], np.int32)

    def attrs(self, start: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(ts, class) of the rows from `start` on, as EmbeddingIndex.add takes them."""
        return np.asarray(self.ts[start:], np.int32), np.asarray(self.cls[start:], np.int32)

    def passing(self, where) -> np.ndarray:
        """Bool per row: the row passes the row filter (an `EmbeddingIndex.row_filter`, None: every row), as the device decides."""
        ok = np.ones(len(self.paths), bool)
        if where is None:
            return ok
        ts, c = self.attrs()
        if where.use_ts:
            ok &= (ts != _lib.ROW_NO_TS) & (ts >= where.ts_min) & (ts <= where.ts_max)
        if where.use_cls:
            bits = np.array([(int(where.cls_mask[i >> 6]) >> (i & 63)) & 1 for i in range(256)], bool)
            ok &= (c >= 0) & bits[np.clip(c, 0, 255)]
        return ok

    @staticmethod
    def dir_of(path: str) -> str:
        """The directory part `describe` groups by: '/'-normalised, with its trailing '/'."""
        norm = path.replace("\\", "/")
        return norm[:norm.rfind("/") + 1]

    def remove(self, mask) -> int:
        """Forget the rows with a non-zero entry in `mask` (one per row), in step with EmbeddingIndex.remove on the device: the
        survivors keep their order.  Directory group ids and track slots are stable (`dirs` / `dir_id` / `slot_of` keep their
        entries, the device keeps its ids), so a later crop of the same folder or track reuses them; `truthy` / `bad` are
        recomputed for the groups that lost rows.  Returns the number of rows forgotten."""
        drop = np.asarray(mask).reshape(-1) != 0
        if drop.size != len(self.paths):
            raise ValueError(f"expected one entry per row ({len(self.paths)}), got {drop.size}")
        gone = np.flatnonzero(drop)
        if gone.size == 0:
            return 0
        lost = {self.group[r] for r in gone.tolist()} - {0}
        keep = np.flatnonzero(~drop).tolist()
        self.paths = [self.paths[r] for r in keep]
        self.group = [self.group[r] for r in keep]
        self.oid = [self.oid[r] for r in keep]
        self.slot = [self.slot[r] for r in keep]
        self.ts = [self.ts[r] for r in keep]
        self.cls = [self.cls[r] for r in keep]
        self.row = {p: r for r, p in enumerate(self.paths)}
        for g in lost:
            self.truthy[g] = self.bad[g] = False
        for r, g in enumerate(self.group):
            if g in lost:
                oid = self.oid[r]
                if oid:
                    self.truthy[g] = True
                elif oid is None and "_" in os.path.basename(self.paths[r]):   # a name `describe` could not parse
                    self.bad[g] = True
        return int(gone.size)

    def allowed(self, cam_name, timestamp) -> np.ndarray:
        al = np.zeros(len(self.dirs), np.uint8)
        for g in range(1, len(self.dirs)):
            d = self.dirs[g]
            if cam_name and f"/cameras/{cam_name}/" not in d:
                continue
            if timestamp and f"/objects/{timestamp}/" not in d and "/objects/video/" not in d:
                continue
            al[g] = 1
        return al
