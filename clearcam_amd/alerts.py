"""Text-described alerts at ingest (``clearcam.py:1289-1307``) for a batch of crop embeddings.

The reference walks the camera's alerts for every crop on the host.  Here the descriptions stand on the device
(``WatchList``, cc_watch_*) and one ``match`` call answers a whole batch with one (alert, score) pair per crop;
``AlertBook`` keeps what the reference keeps on its alert objects (description, threshold, ``last_det``, active) and
turns the pairs into notifications.  ``AlertBook`` is plain Python: any matcher with ``WatchList.match``'s signature works.
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from . import _lib
from .helpers import as_numpy

DEFAULT_THRESHOLD = 0.28            # the reference's default for a described alert
COOLDOWN_S = 60.0                   # clearcam.py:1293 skips an alert while `now - last_det < 60`


class WatchList:
    """The standing table of alert descriptions on the device (cc_watch_*; include/clearcam_hip.h has the contract).

    Every (crop, alert) score is summed in the order of the embedding index's scan: it equals, bit for bit, the score an f32
    ``EmbeddingIndex`` holding the crop gives a single query with the description.  Not thread-safe."""

    MAX_ALERTS = 2048               # CC_WATCH_MAX_ALERTS

    def __init__(self, dim: int = 768, device: int = 0):
        self.dim, self.device = dim, device
        self._h = C.c_void_p()
        _lib.check(_lib.lib().cc_watch_create(C.byref(self._h), dim, device))

    def __len__(self) -> int:
        n = C.c_int()
        _lib.check(_lib.lib().cc_watch_size(self._h, C.byref(n)))
        return n.value

    def set(self, desc, thresholds, groups) -> None:
        """Replace the table: desc (A,dim) float32, one threshold and one camera number in [0, 2^24) per alert; the index in
        the table is the priority.  A == 0 clears it."""
        d = np.asarray(as_numpy(desc), dtype=np.float32)
        if d.size == 0:
            d = d.reshape(0, self.dim)
        if d.ndim != 2 or d.shape[1] != self.dim:
            raise ValueError(f"expected (A,{self.dim}) descriptions, got {d.shape}")
        d = np.ascontiguousarray(d)
        t = np.ascontiguousarray(np.asarray(thresholds, np.float32).reshape(-1))
        g = np.ascontiguousarray(np.asarray(groups, np.int32).reshape(-1))
        if t.shape[0] != d.shape[0] or g.shape[0] != d.shape[0]:
            raise ValueError("thresholds and groups: one entry per alert")
        _lib.check(_lib.lib().cc_watch_set(self._h, _lib.ptr(d), _lib.ptr(t), _lib.ptr(g), d.shape[0]))

    def _batch(self, emb):
        """-> (rows, on_device): (B,dim) float32, a host array or a contiguous CUDA tensor.  Any other width is refused."""
        if bool(getattr(emb, "is_cuda", False)):
            a = emb.contiguous().float()
            if a.shape[-1] != self.dim:
                raise ValueError(f"expected {self.dim}-d rows, got {tuple(a.shape)}")
            return a.reshape(-1, self.dim), True
        a = np.asarray(as_numpy(emb), dtype=np.float32)
        if a.ndim == 0 or a.shape[-1] != self.dim:
            raise ValueError(f"expected {self.dim}-d rows, got {a.shape}")
        return np.ascontiguousarray(a.reshape(-1, self.dim)), False

    def _streams(self):
        """(current torch stream, the stream to run on).  torch's default stream has the handle 0, which the library reads as
        "no stream given": a side stream fenced by the current one on both sides stands in for it (as EmbeddingIndex does)."""
        import torch
        dev = torch.device("cuda", self.device)
        cur = run = torch.cuda.current_stream(dev)
        if cur.cuda_stream == 0:
            if getattr(self, "_side_stream", None) is None:
                self._side_stream = torch.cuda.Stream(dev)
            run = self._side_stream
            run.wait_stream(cur)
        return cur, run

    def scores(self, emb) -> np.ndarray:
        """(B,A) float32: what the reference prints as `sim =` for every crop and alert."""
        a, on_dev = self._batch(emb)
        out = np.empty((a.shape[0], len(self)), np.float32)
        if out.size:
            cur, run = self._streams() if on_dev else (None, None)
            _lib.check(_lib.lib().cc_watch_scores(self._h, _lib.ptr(a), a.shape[0], int(on_dev), _lib.ptr(out), 0,
                                                  C.c_void_p(run.cuda_stream) if on_dev else None))
        return out

    def match(self, emb, crop_groups, armed=None, device_out: bool = False):
        """The reference's walk for the batch in order -> (alert (B,) int32, score (B,) float32): the table index of the alert
        each crop fires (-1: none) and its score (0: none).  crop_groups: one camera number per crop; armed: one byte per alert
        (None: all armed).  A fired alert is spent for the crops behind it.  device_out: CUDA torch tensors on the current
        torch stream, nothing waits."""
        a, on_dev = self._batch(emb)
        B = a.shape[0]
        cg = np.ascontiguousarray(np.asarray(crop_groups, np.int32).reshape(-1))
        if cg.shape[0] != B:
            raise ValueError(f"crop_groups: one camera number per crop ({B}), got {cg.shape[0]}")
        ar = None
        if armed is not None:
            ar = np.ascontiguousarray(np.asarray(armed).reshape(-1) != 0, dtype=np.uint8)
            if ar.shape[0] != len(self):
                raise ValueError(f"armed: one byte per alert ({len(self)}), got {ar.shape[0]}")
        L = _lib.lib()
        if device_out:
            import torch
            dev = torch.device("cuda", self.device)
            alert = torch.empty((B,), dtype=torch.int32, device=dev)
            score = torch.empty((B,), dtype=torch.float32, device=dev)
        else:
            alert, score = np.empty(B, np.int32), np.empty(B, np.float32)
        if B == 0:
            return alert, score
        use_torch = on_dev or device_out
        cur, run = self._streams() if use_torch else (None, None)
        # nothing waits for the stream with device outputs: the host inputs are staged by the library before it returns
        _lib.check(L.cc_watch_match(self._h, _lib.ptr(a), B, int(on_dev), _lib.ptr(cg), _lib.ptr(ar) if ar is not None else None,
                                    _lib.ptr(alert), _lib.ptr(score), int(device_out), C.c_void_p(run.cuda_stream) if use_torch else None))
        if use_torch and run is not cur:
            cur.wait_stream(run)
        return alert, score

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().cc_watch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_of(path: str) -> Optional[str]:
    """The camera of a crop path as clearcam.py:1290 takes it: the component after `cameras`.  None when there is none (the
    reference raises there; such a crop fires nothing here)."""
    parts = str(path).replace("\\", "/").split("/")
    try:
        i = parts.index("cameras")
    except ValueError:
        return None
    return parts[i + 1] if i + 1 < len(parts) and parts[i + 1] else None


class Alert:
    """What the reference keeps on an alert object and the ingest walk reads: desc, desc_emb, threshold, last_det, is_active."""

    __slots__ = ("desc", "desc_emb", "threshold", "last_det", "active")

    def __init__(self, desc=None, desc_emb=None, threshold: float = DEFAULT_THRESHOLD, last_det: float = 0.0, active=True):
        self.desc = desc
        self.desc_emb = None if desc_emb is None else np.asarray(as_numpy(desc_emb), np.float32).reshape(-1)
        self.threshold, self.last_det, self.active = float(threshold), float(last_det), active

    def is_active(self) -> bool:
        return bool(self.active() if callable(self.active) else self.active)


class AlertBook:
    """Host state of the alerts of every camera, and the flattened table a matcher works on.

    Cameras get dense group numbers in the order they are first seen; the table lists the cameras in that order and each
    camera's alerts in its mapping's order, so the index in the table is the reference's walk order within a camera.
    `version` changes with every change of the table (not with `last_det`): the device copy is uploaded once per change."""

    def __init__(self, dim: int = 768, cooldown: float = COOLDOWN_S):
        self.dim, self.cooldown = dim, float(cooldown)
        self.cams: Dict[str, Dict[object, Alert]] = {}
        self.group: Dict[str, int] = {}
        self.version = 0
        self._flat: Optional[List[Tuple[str, object, Alert]]] = None

    def set_camera(self, cam_name: str, alerts) -> None:
        """Replace one camera's alerts: an ordered mapping id -> Alert, or id -> {"desc", "threshold", "desc_emb", "active",
        "last_det"} (all optional but a described alert needs "desc")."""
        book: Dict[object, Alert] = {}
        for k, v in alerts.items():
            book[k] = v if isinstance(v, Alert) else Alert(**{f: v[f] for f in Alert.__slots__ if f in v})
            e = book[k].desc_emb
            if e is not None and e.size != self.dim:
                raise ValueError(f"alert {k!r}: desc_emb has {e.size} dimensions, expected {self.dim}")
        self.cams[cam_name] = book
        self.group.setdefault(cam_name, len(self.group))
        self._changed()

    def remove_camera(self, cam_name: str) -> None:
        if self.cams.pop(cam_name, None) is not None:      # the group number stays reserved: crops of the camera match nothing
            self._changed()

    def _changed(self) -> None:
        self._flat = None
        self.version += 1

    def flat(self) -> List[Tuple[str, object, Alert]]:
        """[(cam_name, alert id, Alert)] in table order."""
        if self._flat is None:
            self._flat = [(cam, k, a) for cam, book in self.cams.items() for k, a in book.items()]
        return self._flat

    def __len__(self) -> int:
        return len(self.flat())

    def missing(self) -> List[Tuple[str, object, Alert]]:
        """Described alerts whose description is not encoded yet (the reference encodes lazily, :1295-1297)."""
        return [x for x in self.flat() if x[2].desc is not None and x[2].desc_emb is None]

    def table(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(desc (A,dim) f32, threshold (A,) f32, group (A,) int32) for `WatchList.set`.  An alert without an embedding is a zero
        row; `armed` never arms it."""
        rows = self.flat()
        desc = np.zeros((len(rows), self.dim), np.float32)
        for i, (_, _, a) in enumerate(rows):
            if a.desc_emb is not None:
                desc[i] = a.desc_emb
        thr = np.asarray([a.threshold for _, _, a in rows], np.float32)
        grp = np.asarray([self.group[cam] for cam, _, _ in rows], np.int32)
        return desc, thr, grp

    def armed(self, now: float) -> np.ndarray:
        """One byte per alert of the table: the alerts the reference's walk would not skip at `now` (:1293-1294): cooldown over
        (`now - last_det < cooldown` skips, so exactly `cooldown` seconds re-arm), active, and described (with its embedding)."""
        return np.asarray([now - a.last_det >= self.cooldown and a.is_active() and a.desc is not None and a.desc_emb is not None
                           for _, _, a in self.flat()], np.uint8)

    def crop_groups(self, paths) -> np.ndarray:
        """The camera number of each crop path; -1 (no alert has it) for a camera without alerts or a path without one."""
        return np.asarray([self.group.get(camera_of(p), -1) if p is not None else -1 for p in paths], np.int32)

    def apply(self, alert_rows, scores, paths, now: float) -> list:
        """Take a matcher's answer: every fired alert gets `last_det = now`; -> [(path, cam_name, alert id, desc, score)] in
        crop order, one entry per crop that fired."""
        rows, out = self.flat(), []
        for b, (a, s) in enumerate(zip(np.asarray(alert_rows).reshape(-1).tolist(), np.asarray(scores).reshape(-1).tolist())):
            if a < 0:
                continue
            cam, k, al = rows[a]
            al.last_det = now
            out.append((paths[b], cam, k, al.desc, float(s)))
        return out

    def check(self, match: Callable, embs, paths, now: Optional[float] = None) -> list:
        """`armed`, one `match(embs, crop_groups, armed)` call, `apply`."""
        now = time.time() if now is None else now
        if len(paths) == 0 or len(self) == 0:
            return []
        alert_rows, scores = match(embs, self.crop_groups(paths), self.armed(now))
        return self.apply(alert_rows, scores, paths, now)
