"""The resident embedding index: ``EmbeddingIndex`` (a device matrix of crop embeddings and every question asked of it, cc_index_*) and
``row_filter`` (the time window / class filter those questions share).  ``clearcam_amd.objects`` re-exports both: ``ObjectFinder``
is built on them.

There is no CPU path: without the HIP library / a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .helpers import as_numpy


_I64P = C.POINTER(C.c_int64)


def row_filter(ts_range=None, classes=None) -> Optional["_lib.RowFilter"]:
    """The row filter of `rank` / `rank_device` / `timeline` (cc_row_filter), or None when neither argument is given.
    ts_range: (first, last) seconds, inclusive at both ends, either may be None for "open"; classes: the class ids that
    pass, each in [0, 255].  A row without the attribute never passes a filter on it.  An empty window (first > last, or
    outside int32) and an empty class set are errors: they could only answer nothing."""
    if ts_range is None and classes is None:
        return None
    f = _lib.RowFilter()
    if ts_range is not None:
        lo, hi = ts_range
        lo, hi = (-(1 << 31) if lo is None else int(lo)), ((1 << 31) - 1 if hi is None else int(hi))
        if lo > hi or lo >= 1 << 31 or hi < -(1 << 31):
            raise ValueError(f"ts_range ({lo}, {hi}) is empty")
        f.use_ts, f.ts_min, f.ts_max = 1, max(lo, -(1 << 31)), min(hi, (1 << 31) - 1)
    if classes is not None:
        ids = sorted({int(c) for c in np.asarray(classes).reshape(-1).tolist()})
        if not ids:
            raise ValueError("classes is empty")
        if ids[0] < 0 or ids[-1] > 255:
            raise ValueError("classes: ids in [0, 255]")
        f.use_cls = 1
        for c in ids:
            f.cls_mask[c >> 6] |= 1 << (c & 63)
    return f


class EmbeddingIndex:
    """Device-resident (N,dim) matrix with scan + top-k (cc_index_*).  storage "f32" (exact f32 scores), "bf16" (half the
    bytes per scan, scores within ~1e-3 for unit vectors; dim % 256 == 0 and at most 40960) or "i8" (int8 codes with one f32 scale per 32 elements: dim * 9 / 8
    bytes a row, scores within ~1e-3 as well; include/clearcam_hip.h has the rule).  `capacity` is the initial allocation; the
    matrix grows.

    Batches on "i8" rows: fewer than 18 queries are scored by scan passes, bit-identical to single queries; from 18 on (dim <= 4096)
    one MFMA launch scores the whole batch, the same exact products summed in another order (last-bit differences, the same error
    bound).  Either way a (query, row) score depends on that pair alone, equal rows tie exactly and ties break by row id.
    `last_scores_path()` tells which kernel ran."""

    STORAGE = {"f32": 0, "bf16": 2, "i8": 8}           # name -> the `storage` argument of cc_index_create_ex

    def __init__(self, dim: int = 768, capacity: int = 1 << 20, device: int = 0, storage: str = "f32"):
        self.dim, self.device, self.storage = dim, device, storage
        self._h = C.c_void_p()
        _lib.check(_lib.lib().cc_index_create_ex(C.byref(self._h), dim, max(int(capacity), 1), device, self.STORAGE[storage]))

    @property
    def capacity(self) -> int:
        c = C.c_int64()
        _lib.check(_lib.lib().cc_index_info(self._h, C.byref(c), None, None))
        return c.value

    def __len__(self) -> int:
        n = C.c_int64()
        _lib.check(_lib.lib().cc_index_size(self._h, C.byref(n)))
        return n.value

    row_filter = staticmethod(row_filter)

    # -- the marshalling every question shares ----------------------------------------------------------------------------------------
    def _allowed(self, allowed):
        """The (allowed pointer, n_groups) pair of a call.  A device caller waits for nothing, so the filter bytes stay referenced
        until the next call replaces them."""
        al = self._allowed_in_flight = None if allowed is None else np.ascontiguousarray(allowed, dtype=np.uint8)
        return (None, 0) if al is None else (_lib.ptr(al), int(al.size))

    @staticmethod
    def _where(where):
        return None if where is None else C.byref(where)

    @staticmethod
    def _page(Q: int, start: int, count: int):
        """The shape of one page of answers, or a (1, 1) stand-in when the library will name the error."""
        return (Q, count) if count >= 1 and start >= 0 and Q >= 1 else (1, 1)

    @staticmethod
    def _timeline_args(Q: int, t0, bin_seconds, n_bins):
        """((t0, bin_seconds, n_bins) as checked ints, the (Q, n_bins) uint32 counts a timeline call fills)."""
        t0, bin_seconds, n_bins = int(t0), int(bin_seconds), int(n_bins)
        if not -(1 << 31) <= t0 < 1 << 31 or not -(1 << 31) <= bin_seconds < 1 << 31 or not -(1 << 31) <= n_bins < 1 << 31:
            raise ValueError("t0, bin_seconds and n_bins must fit in int32")
        return (t0, bin_seconds, n_bins), np.zeros((Q, min(max(n_bins, 1), 4096)), np.uint32)   # outside [1, 4096]: the library names the error

    def _dev(self):
        """(the torch device of the index, numpy dtype -> torch dtype of an output), made once: a device call costs microseconds"""
        if getattr(self, "_torch_dev", None) is None:
            import torch
            self._torch_dev = torch.device("cuda", self.device), {np.int32: torch.int32, np.float32: torch.float32,
                                                                  np.uint32: torch.int32}        # uint32 counts travel in an int32 tensor
        return self._torch_dev

    def _outputs(self, device: bool, *specs):
        """One uninitialised output per (shape, numpy dtype) spec, None for a spec that is None: numpy arrays, or (device) CUDA
        tensors of the same shapes and dtypes."""
        if not device:
            return [None if s is None else np.empty(s[0], s[1]) for s in specs]
        from torch import empty
        dev, dtype = self._dev()
        return [None if s is None else empty(s[0], dtype=dtype[s[1]], device=dev) for s in specs]

    def _queries(self, q, device: bool):
        """(Q, dim) float32 queries where the call reads them: a contiguous numpy array, or (device) a CUDA tensor.  on_device=1 tells
        the library that BOTH the queries and the outputs are device pointers: a host query is uploaded here first, on the caller's
        stream (a host pointer handed to a device-to-device copy only works by accident of ROCm's pointer inference, and the
        temporary could be freed while the copy is pending)."""
        if not device:
            return np.ascontiguousarray(as_numpy(q), dtype=np.float32).reshape(-1, self.dim)
        import torch
        if not bool(getattr(q, "is_cuda", False)):
            q = torch.as_tensor(np.ascontiguousarray(as_numpy(q), dtype=np.float32)).to(self._dev()[0])
        return q.contiguous().float().reshape(-1, self.dim)

    def _run_stream(self, dev):
        """(current torch stream, the stream to hand to the library).  torch's default stream has the handle 0, which the library
        reads as "no stream given" (it then runs on the index's own stream, which nothing orders against torch): the work runs on a
        side stream fenced by the current one instead; `_call` fences the other side (`cur.wait_stream(run)`) behind the call."""
        import torch
        cur = run = torch.cuda.current_stream(dev)
        if cur.cuda_stream == 0:
            if getattr(self, "_side_stream", None) is None:
                self._side_stream = torch.cuda.Stream(dev)
            run = self._side_stream
            run.wait_stream(cur)
        return cur, run

    def _call(self, device: bool, fn, *made) -> None:
        """Run fn(on_device, stream), a library call already checked by fn.  A host call: (0, None), the library waits for its own
        stream.  A device call: on the stream `_run_stream` picks, fenced behind by the current torch stream; `made` are the tensors
        made for this call that it reads (a cast, a copy, an upload), which must outlive the launches that read them."""
        if not device:
            fn(0, None)
            return
        cur, run = self._run_stream(self._dev()[0])
        fn(1, C.c_void_p(run.cuda_stream))
        if run is not cur:
            cur.wait_stream(run)
            for t in made:
                if t is not None:
                    t.record_stream(run)

    @staticmethod
    def _row_numbers(rows) -> np.ndarray:
        a = np.asarray(rows)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError("row numbers must be integers")
        return np.ascontiguousarray(a.reshape(-1), dtype=np.int64)

    @staticmethod
    def _rows_ptr(ids: np.ndarray):
        """The int64* of `_row_numbers`' array (the pointer keeps the array alive)."""
        try:
            return _I64P(C.c_int64.from_buffer(ids))                # a third of the cost of ids.ctypes.data_as, in calls of a few microseconds
        except (TypeError, ValueError):                             # no rows, or a read-only array
            return ids.ctypes.data_as(_I64P)

    def add(self, emb, groups=None, tracks=None, ts=None, classes=None) -> None:
        """Append rows: (n,dim) / (n,1,dim) / (dim,) float32, host array or CUDA torch tensor.  Rows of any other width are
        rejected (a 512-d face row must never land in the 768-d crop matrix).  groups: one int per row (search filter unit).
        tracks: one slot per row, a dense number per distinct track id or -1 for a crop without one (`search_tracks`).
        ts: one int32 per row, the seconds into the day's recording, _lib.ROW_NO_TS for a row without; classes: one detector
        class in [0, 255] per row, -1 for a row without.  Not given: no row has the attribute (it then passes no filter on it)."""
        on_dev = bool(getattr(emb, "is_cuda", False))
        if on_dev:
            a = emb.contiguous().float()
            if a.shape[-1] != self.dim:
                raise ValueError(f"expected {self.dim}-d rows, got {tuple(a.shape)}")
            a = a.reshape(-1, self.dim)
        else:
            a = np.asarray(as_numpy(emb), dtype=np.float32)
            if a.ndim == 0 or a.shape[-1] != self.dim:
                raise ValueError(f"expected {self.dim}-d rows, got {a.shape}")
            a = np.ascontiguousarray(a.reshape(-1, self.dim))
        g = None
        if groups is not None:
            g = np.ascontiguousarray(np.asarray(groups, np.int32).reshape(-1))
            if g.shape[0] != a.shape[0] or (g.size and (g.min() < 0 or g.max() >= 1 << 24)):
                raise ValueError("groups: one id in [0, 2^24) per row")
        t = None
        if tracks is not None:
            t = np.ascontiguousarray(np.asarray(tracks, np.int32).reshape(-1))
            if t.shape[0] != a.shape[0] or (t.size and (t.min() < -1 or t.max() >= 1 << 24)):
                raise ValueError("tracks: one slot in [0, 2^24) or -1 per row")
        s = c = None
        if ts is not None:
            s64 = np.asarray(ts, np.int64).reshape(-1)
            if s64.shape[0] != a.shape[0] or (s64.size and (s64.min() < -(1 << 31) or s64.max() >= 1 << 31)):
                raise ValueError("ts: one int32 per row")
            s = np.ascontiguousarray(s64.astype(np.int32))
        if classes is not None:
            c = np.ascontiguousarray(np.asarray(classes, np.int32).reshape(-1))
            if c.shape[0] != a.shape[0] or (c.size and (c.min() < -1 or c.max() > 255)):
                raise ValueError("classes: one id in [0, 255] or -1 per row")
        _lib.check(_lib.lib().cc_index_add_described(self._h, _lib.ptr(a), a.shape[0], int(on_dev), _lib.ptr(g) if g is not None else None,
                                                     _lib.ptr(t) if t is not None else None, _lib.ptr(s) if s is not None else None,
                                                     _lib.ptr(c) if c is not None else None))

    def row_info(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ts (N,) int32, class (N,) int32) of every row as the device holds them (cc_index_row_info)."""
        n = len(self)
        ts, c = np.empty(n, np.int32), np.empty(n, np.int32)
        _lib.check(_lib.lib().cc_index_row_info(self._h, 0, n, _lib.ptr(ts), _lib.ptr(c)))
        return ts, c

    def remove(self, rows) -> int:
        """Take rows out; the survivors keep their order and are renumbered densely (new id = survivors before the row), so
        every search answers as an index built from the survivors would.  rows: a bool / uint8 mask with one entry per row
        (non-zero removes), or an array of row numbers.  Compaction in place on the device (cc_index_remove_rows): capacity
        and track slots stay.  Returns the number of rows removed."""
        a = np.asarray(rows)
        if a.dtype == np.bool_ or a.dtype == np.uint8:
            mask = np.ascontiguousarray(a.reshape(-1), dtype=np.uint8)
        else:
            ids = a.reshape(-1).astype(np.int64)
            n = len(self)
            if ids.size and (ids.min() < 0 or ids.max() >= n):
                raise IndexError(f"row numbers must be in [0, {n})")
            mask = np.zeros(n, np.uint8)
            mask[ids] = 1
        removed = C.c_int64()
        _lib.check(_lib.lib().cc_index_remove_rows(self._h, _lib.ptr(mask), int(mask.size), C.byref(removed)))
        return removed.value

    def remove_groups(self, drop) -> int:
        """`remove` for every row whose group id g has drop[g] != 0 (uint8, one byte per group; groups past the end of `drop`
        stay).  The keep flags are computed on the device from the stored group ids: no per-row work on the host."""
        d = np.ascontiguousarray(np.asarray(drop).reshape(-1), dtype=np.uint8)
        if d.size == 0:
            return 0
        removed = C.c_int64()
        _lib.check(_lib.lib().cc_index_remove_groups(self._h, _lib.ptr(d), int(d.size), C.byref(removed)))
        return removed.value

    def scores(self, q) -> np.ndarray:
        qa = np.ascontiguousarray(as_numpy(q), dtype=np.float32).reshape(-1, self.dim)
        out = np.empty((qa.shape[0], len(self)), np.float32)
        if len(self):
            _lib.check(_lib.lib().cc_index_scores(self._h, _lib.ptr(qa), qa.shape[0], _lib.ptr(out), 0, None))
        return out

    def last_scores_path(self) -> int:
        """Which kernel produced the scores of the last scoring call (scores / search* / rank) on this index: 0 scan passes,
        1 the f32 / bf16 MFMA GEMM, 2 the int8 MFMA kernel (cc_index_last_path)."""
        p = C.c_int()
        _lib.check(_lib.lib().cc_index_last_path(self._h, C.byref(p)))
        return p.value

    def _search(self, call: str, q, k: int, allowed, device: bool):
        qa = self._queries(q, device)
        idx, sc = self._outputs(device, ((qa.shape[0], k), np.int32), ((qa.shape[0], k), np.float32))
        self._call(device, lambda on_device, stream: _lib.check(getattr(_lib.lib(), call)(
            self._h, _lib.ptr(qa), qa.shape[0], k, *self._allowed(allowed), _lib.ptr(idx), _lib.ptr(sc), on_device, stream)), qa)
        return idx, sc

    def search(self, q, k: int, allowed=None) -> Tuple[np.ndarray, np.ndarray]:
        """(Q,dim) queries -> (idx (Q,k) int32, score (Q,k) f32), descending, ties by lower row id; -1/-inf past N.
        allowed: optional uint8 array, one entry per group id — only rows of groups with a non-zero entry compete."""
        return self._search("cc_index_search_groups", q, k, allowed, False)

    def search_device(self, q, k: int):
        """`search` with the result left on the GPU: (idx int32, score f32) CUDA torch tensors on the current torch stream,
        for callers that keep going on the device (clearcam_amd.dist.ShardedIndex: all-gather + merge)."""
        return self._search("cc_index_search_groups", q, k, None, True)

    def search_tracks(self, q, k: int, allowed=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search` with tracks as the answers (models/objects.py:378-390 on the device): among the allowed rows every track
        slot counts once, with its best row (equal scores: the lower row), and rows of slot -1 count as themselves.  Descending
        by score; equal scores: tracks by their first allowed row, then the slot-less rows by row id.  Fewer than k answers
        leave -1/-inf at the end.  One call, exact for any data: no candidate list to widen."""
        return self._search("cc_index_search_tracks", q, k, allowed, False)

    def search_tracks_device(self, q, k: int, allowed=None):
        """`search_tracks` with the result left on the GPU, like `search_device` (allowed stays a host array)."""
        return self._search("cc_index_search_tracks", q, k, allowed, True)

    @staticmethod
    def cut_f32(min_score) -> np.float32:
        """The smallest float32 that is >= the caller's cut (a Python float; None: -inf, no cut).  Scores are float32 and the
        reference tests `score < cut` in double, so `score >= cut_f32(cut)` in f32 keeps exactly what `not score < cut` keeps."""
        if min_score is None:
            return np.float32(-np.inf)
        t = float(min_score)
        with np.errstate(over="ignore"):
            c = np.float32(t)
        if float(c) < t:                                   # rounded down: one step up
            c = np.nextafter(c, np.float32(np.inf))
        return c

    def _rank(self, q, start, count, allowed, min_score, tracks, ts_range, classes, device: bool, with_total: bool):
        where = self.row_filter(ts_range, classes)
        qa = self._queries(q, device)
        start, count = int(start), int(count)
        shape = self._page(qa.shape[0], start, count)
        idx, sc = self._outputs(device, (shape, np.int32), (shape, np.float32))
        total = np.zeros(qa.shape[0], np.int64) if with_total else None
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_rank_where(
            self._h, _lib.ptr(qa), qa.shape[0], start, count, float(self.cut_f32(min_score)), 1 if tracks else 0, *self._allowed(allowed),
            self._where(where), _lib.ptr(idx), _lib.ptr(sc), _lib.ptr(total), on_device, stream)), qa)
        return idx, sc, total

    def rank(self, q, start: int, count: int, allowed=None, min_score=None, tracks: bool = True, ts_range=None,
             classes=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Answers start .. start+count-1 of the WHOLE descending order -> (idx (Q,count) int32, score (Q,count) f32, total (Q,)
        int64), at any depth and of any length, in one call (cc_index_rank_where).  tracks=True: the answers and their order are those of
        `search_tracks`; False: every allowed row answers for itself, ordered as `search` orders them.  Only answers with
        score >= min_score exist (`cut_f32` of the value given): ranks are counted among them and `total` is their number, so a
        cut inside a run of equal scores keeps the whole run.  -1/-inf past the last answer.
        ts_range / classes (`row_filter`): only rows that pass compete, and the call answers as an index built from those rows
        alone would - a track is reduced among its passing rows and placed by its first passing one."""
        return self._rank(q, start, count, allowed, min_score, tracks, ts_range, classes, False, True)

    def rank_device(self, q, start: int, count: int, allowed=None, min_score=None, tracks: bool = True, with_total: bool = True,
                    ts_range=None, classes=None):
        """`rank` with idx / score left on the GPU like `search_tracks_device`.  `total` still comes back as a host array, which
        costs one wait for the stream; with_total=False returns None in its place and waits for nothing."""
        return self._rank(q, start, count, allowed, min_score, tracks, ts_range, classes, True, with_total)

    def timeline(self, q, t0: int, bin_seconds: int, n_bins: int, allowed=None, min_score=None, tracks: bool = True, ts_range=None,
                 classes=None) -> Tuple[np.ndarray, np.ndarray]:
        """How the answers of `rank` (same arguments) spread over time -> (counts (Q, n_bins) int64, total (Q,) int64), in one call
        (cc_index_timeline).  An answer falls into bin floor((ts - t0) / bin_seconds), ts being that of the row `rank` names for it
        (a track: its best passing crop); an answer without ts or outside the n_bins bins is counted in `total` only, which
        equals `rank`'s total.  bin_seconds >= 1, 1 <= n_bins <= 4096, t0 an int32."""
        where = self.row_filter(ts_range, classes)
        qa = self._queries(q, False)
        bins, counts = self._timeline_args(qa.shape[0], t0, bin_seconds, n_bins)
        total = np.zeros(qa.shape[0], np.int64)
        _lib.check(_lib.lib().cc_index_timeline(self._h, _lib.ptr(qa), qa.shape[0], float(self.cut_f32(min_score)), 1 if tracks else 0,
                                                *self._allowed(allowed), self._where(where), *bins, _lib.ptr(counts), _lib.ptr(total), 0, None))
        return counts.astype(np.int64), total

    # -- query by stored rows: the queries are rows of this matrix (cc_index_fetch_rows / cc_index_rank_like) ------------------------
    LIKE_EXCLUDE = {None: 0, "rows": _lib.LIKE_EXCLUDE_ROWS, "track": _lib.LIKE_EXCLUDE_TRACK}

    def fetch(self, rows, device_out: bool = False):
        """What the index holds for `rows` (numbers in any order, repeats allowed, at least one), decoded -> (n, dim) float32:
        f32 rows as they were added, bf16 rows as the bf16 values, i8 rows as code * scale.  One gather on the device
        (cc_index_fetch_rows).  device_out: a CUDA torch tensor on the current torch stream, nothing waited for.  A number outside
        the index is an error."""
        ids = self._row_numbers(rows)
        out, = self._outputs(device_out, ((ids.size, self.dim), np.float32))
        self._call(device_out, lambda on_device, stream: _lib.check(_lib.lib().cc_index_fetch_rows(
            self._h, self._rows_ptr(ids), int(ids.size), _lib.ptr(out), on_device, stream)))
        return out

    def _rank_like(self, rows, start, count, allowed, min_score, tracks, exclude, ts_range, classes, device: bool, with_total: bool):
        where = self.row_filter(ts_range, classes)
        start, count = int(start), int(count)
        shape = self._page(1, start, count)
        idx, sc = self._outputs(device, (shape, np.int32), (shape, np.float32))
        total = np.zeros(1, np.int64) if with_total else None
        if exclude not in self.LIKE_EXCLUDE:
            raise ValueError('exclude: None, "rows" or "track"')
        ids = self._row_numbers(rows)
        flags = (_lib.RANK_TRACKS if tracks else 0) | self.LIKE_EXCLUDE[exclude]
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_rank_like(
            self._h, self._rows_ptr(ids), int(ids.size), start, count, float(self.cut_f32(min_score)), flags, *self._allowed(allowed),
            self._where(where), _lib.ptr(idx), _lib.ptr(sc), _lib.ptr(total), on_device, stream)))
        return idx, sc, total

    def rank_like(self, rows, start: int, count: int, allowed=None, min_score=None, tracks: bool = True, exclude=None, ts_range=None,
                  classes=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`rank` for ONE query made of 1 .. 64 stored rows ("more like this crop", or like any crop of this track) -> (idx
        (1, count) int32, score (1, count) f32, total (1,) int64).  A row's score is its best score against any of `rows`
        (scored as `scores(fetch(rows))` scores them, by the same kernel route), and that vector is ranked exactly as `rank`
        ranks a query's: same answers per track, tie rules, cut, filters and padding.  exclude="rows": the query rows do not
        compete; "track": no row of their directory group and track slot does (they must share one group and one slot >= 0).
        A copy of an excluded crop elsewhere still answers, with the same score.  No embedding leaves or enters the GPU
        (cc_index_rank_like)."""
        return self._rank_like(rows, start, count, allowed, min_score, tracks, exclude, ts_range, classes, False, True)

    def rank_like_device(self, rows, start: int, count: int, allowed=None, min_score=None, tracks: bool = True, exclude=None,
                         with_total: bool = True, ts_range=None, classes=None):
        """`rank_like` with idx / score left on the GPU, as `rank_device` leaves them; with_total=False waits for nothing."""
        return self._rank_like(rows, start, count, allowed, min_score, tracks, exclude, ts_range, classes, True, with_total)


    # -- compound search: weighted, all-of and negative terms in one ranking (cc_index_rank_terms / cc_index_timeline_terms) -----------
    TERM_ROLE = {"rank": _lib.TERM_RANK, "require": _lib.TERM_REQUIRE, "reject": _lib.TERM_REJECT}
    COMBINE = {"max": _lib.COMBINE_MAX, "min": _lib.COMBINE_MIN, "sum": _lib.COMBINE_SUM}

    def _terms(self, q, rows, roles, weights, cuts, combine, exclude, tracks):
        """The query side of a compound call, checked -> (vectors (n_vec, dim) f32 or None, row numbers int64, (T,) _lib.Term array,
        the combine rule, the flags).  Terms 0 .. n_vec-1 are the vectors, the stored rows follow; roles / weights / cuts have one
        entry per term in that order (roles None: every term ranks; weights None: 1.0; a cut None: 0, read only for "require" /
        "reject", where it is `cut_f32` of the value given)."""
        if exclude not in self.LIKE_EXCLUDE:
            raise ValueError('exclude: None, "rows" or "track"')
        if combine not in self.COMBINE:
            raise ValueError('combine: "max", "min" or "sum"')
        qa = None
        if q is not None:
            if bool(getattr(q, "is_cuda", False)):
                qa = q.contiguous().float().reshape(-1, self.dim)
            else:
                qa = np.ascontiguousarray(as_numpy(q), dtype=np.float32).reshape(-1, self.dim)
        ids = self._row_numbers([] if rows is None else rows)
        n_vec = 0 if qa is None else int(qa.shape[0])
        T = n_vec + int(ids.size)
        roles = ["rank"] * T if roles is None else list(roles)
        weights = [1.0] * T if weights is None else list(weights)
        cuts = [None] * T if cuts is None else list(cuts)
        if not (len(roles) == len(weights) == len(cuts) == T):
            raise ValueError(f"roles, weights and cuts need one entry per term ({T})")
        terms = (_lib.Term * max(T, 1))()
        for t, (role, wt, cut) in enumerate(zip(roles, weights, cuts)):
            if role not in self.TERM_ROLE:
                raise ValueError('role: "rank", "require" or "reject"')
            terms[t].role, terms[t].weight = self.TERM_ROLE[role], float(wt)
            terms[t].cut = 0.0 if cut is None else float(self.cut_f32(cut))
        return qa, ids, terms, self.COMBINE[combine], (_lib.RANK_TRACKS if tracks else 0) | self.LIKE_EXCLUDE[exclude]

    def _term_vectors(self, qa, device: bool):
        """The vectors of `_terms` where the call reads them: with the outputs, on the host or on the device."""
        if qa is None:
            return None
        if not device:
            return qa if isinstance(qa, np.ndarray) else qa.cpu().numpy()
        if not isinstance(qa, np.ndarray):
            return qa
        import torch
        return torch.as_tensor(qa).to(self._dev()[0])            # on_device: the vectors are a device pointer too

    def _terms_head(self, qa, ids, terms, combine):
        """The arguments h .. combine of cc_index_rank_terms / cc_index_timeline_terms"""
        return (self._h, _lib.ptr(qa), 0 if qa is None else int(qa.shape[0]), self._rows_ptr(ids) if ids.size else None, int(ids.size), terms, combine)

    def _rank_terms(self, q, rows, roles, weights, cuts, combine, start, count, allowed, min_score, tracks, exclude, ts_range, classes, which,
                    device: bool, with_total: bool):
        qa, ids, terms, comb, flags = self._terms(q, rows, roles, weights, cuts, combine, exclude, tracks)
        where = self.row_filter(ts_range, classes)
        qa = self._term_vectors(qa, device)
        start, count = int(start), int(count)
        shape = self._page(1, start, count)
        idx, sc, wh = self._outputs(device, (shape, np.int32), (shape, np.float32), (shape, np.int32) if which else None)
        total = np.zeros(1, np.int64) if with_total else None
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_rank_terms(
            *self._terms_head(qa, ids, terms, comb), start, count, float(self.cut_f32(min_score)), flags, *self._allowed(allowed), self._where(where),
            _lib.ptr(idx), _lib.ptr(sc), _lib.ptr(wh), _lib.ptr(total), on_device, stream)), qa)
        return (idx, sc, total, wh) if which else (idx, sc, total)

    def rank_terms(self, q=None, rows=None, roles=None, weights=None, cuts=None, combine: str = "max", start: int = 0, count: int = 100,
                   allowed=None, min_score=None, tracks: bool = True, exclude=None, ts_range=None, classes=None, which: bool = False):
        """`rank` for ONE compound question of up to 64 terms -> (idx (1, count) int32, score (1, count) f32, total (1,) int64[, which
        (1, count) int32]).  The terms are the vectors `q` ((n_vec, dim), e.g. text embeddings) followed by the stored rows `rows`,
        scored in one batch as `scores(np.vstack([q, fetch(rows)]))` scores them.  roles[t]: "rank" - the term contributes to the
        ranking value through `combine` ("max" / "min" of the rank terms' scores, or "sum": the float32 sum of weights[t] * score in
        term order, negative weights allowed); "require" - a row competes only if the term scores it >= cuts[t]; "reject" - a row
        scored >= cuts[t] does not compete ("white van, but not this one").  The value vector is ranked exactly as `rank` ranks a
        query's among the rows left: same answers per track (reduced among the surviving rows, placed by the first of them), tie
        rules, cut, filters and padding.  exclude="rows" / "track": as in `rank_like`, for the stored rows that are rank terms.  A
        copy of a rejected crop elsewhere is rejected with it; a copy of an excluded one still answers.  which=True: per answer
        the term that made its value (max / min: the lowest-numbered one attaining it; sum: the one with the largest product),
        -1 past the last answer (cc_index_rank_terms)."""
        return self._rank_terms(q, rows, roles, weights, cuts, combine, start, count, allowed, min_score, tracks, exclude, ts_range, classes, which,
                                False, True)

    def rank_terms_device(self, q=None, rows=None, roles=None, weights=None, cuts=None, combine: str = "max", start: int = 0, count: int = 100,
                          allowed=None, min_score=None, tracks: bool = True, exclude=None, with_total: bool = True, ts_range=None, classes=None,
                          which: bool = False):
        """`rank_terms` with idx / score (and which) left on the GPU, as `rank_like_device` leaves them, on the current torch stream
        (`distinct_device` can run behind it); with_total=False returns None for the total and waits for nothing."""
        return self._rank_terms(q, rows, roles, weights, cuts, combine, start, count, allowed, min_score, tracks, exclude, ts_range, classes, which,
                                True, with_total)

    def timeline_terms(self, t0: int, bin_seconds: int, n_bins: int, q=None, rows=None, roles=None, weights=None, cuts=None, combine: str = "max",
                       allowed=None, min_score=None, tracks: bool = True, exclude=None, ts_range=None, classes=None) -> Tuple[np.ndarray, np.ndarray]:
        """How the answers of `rank_terms` (same terms and arguments) spread over time -> (counts (1, n_bins) int64, total (1,) int64),
        binned as `timeline` bins them; `total` equals `rank_terms`' total (cc_index_timeline_terms)."""
        qa, ids, terms, comb, flags = self._terms(q, rows, roles, weights, cuts, combine, exclude, tracks)
        qa = self._term_vectors(qa, False)
        where = self.row_filter(ts_range, classes)
        bins, counts = self._timeline_args(1, t0, bin_seconds, n_bins)
        total = np.zeros(1, np.int64)
        _lib.check(_lib.lib().cc_index_timeline_terms(*self._terms_head(qa, ids, terms, comb), float(self.cut_f32(min_score)), flags,
                                                      *self._allowed(allowed), self._where(where), *bins, _lib.ptr(counts), _lib.ptr(total), 0, None))
        return counts.astype(np.int64), total


    # -- together: rows with a partner nearby in time (cc_index_rank_near / cc_index_timeline_near) ----------------------------------------
    def _near_side(self, x, device: bool):
        """One side of a together call -> (vector or None, row number or -1): an int is a stored row, anything else a (dim,) vector
        (a numpy array for a host call, a CUDA tensor for a device call)."""
        if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
            return None, int(x)
        if device:
            import torch
            dev = self._dev()[0]
            if not bool(getattr(x, "is_cuda", False)):
                x = torch.as_tensor(np.ascontiguousarray(as_numpy(x), dtype=np.float32)).to(dev)
            v = x.contiguous().float().reshape(-1)
        else:
            v = np.ascontiguousarray(as_numpy(x), dtype=np.float32).reshape(-1)
        if int(v.shape[0]) != self.dim:
            raise ValueError(f"a side of a together call is one vector of {self.dim} floats or one stored row")
        return v, -1

    def _near_question(self, a, b, within, partners, cut_b, value, min_score, tracks, device: bool):
        """The question of a together call, checked -> the arguments h .. flags of cc_index_rank_near without start / count, and the
        vectors to keep alive"""
        if value not in _lib.NEAR_VALUE:
            raise ValueError('value: "a" or "min"')
        within, partners = int(within), int(partners)
        if not -(1 << 31) <= within < 1 << 31 or not -(1 << 31) <= partners < 1 << 31:
            raise ValueError("within and partners must fit in int32")
        (va, ra), (vb, rb) = self._near_side(a, device), self._near_side(b, device)
        head = (self._h, _lib.ptr(va), ra, _lib.ptr(vb), rb, within, partners, float(self.cut_f32(cut_b)), _lib.NEAR_VALUE[value])
        return head, (float(self.cut_f32(min_score)), _lib.RANK_TRACKS if tracks else 0), (va, vb)

    def _near_filters(self, allowed, where_a, where_b):
        return (*self._allowed(allowed), self._where(where_a), self._where(where_b))

    def _rank_near(self, a, b, within, start, count, partners, cut_b, value, allowed, min_score, tracks, ts_range, classes, b_ts_range, b_classes,
                   device: bool, with_total: bool):
        head, tail, keep = self._near_question(a, b, within, partners, cut_b, value, min_score, tracks, device)
        wa, wb = self.row_filter(ts_range, classes), self.row_filter(b_ts_range, b_classes)
        start, count = int(start), int(count)
        shape = self._page(1, start, count)
        idx, sc, pr, ps = self._outputs(device, (shape, np.int32), (shape, np.float32), (shape, np.int32), (shape, np.float32))
        total, n_partners = (np.zeros(1, np.int64), np.zeros(1, np.int64)) if with_total else (None, None)
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_rank_near(
            *head, start, count, *tail, *self._near_filters(allowed, wa, wb), _lib.ptr(idx), _lib.ptr(sc), _lib.ptr(pr), _lib.ptr(ps), _lib.ptr(total),
            _lib.ptr(n_partners), on_device, stream)), *keep)
        return idx, sc, total, pr, ps, (int(n_partners[0]) if with_total else None)

    def rank_near(self, a, b, within, start: int = 0, count: int = 100, partners: int = _lib.NEAR_DEFAULT_PARTNERS, cut_b=None, value: str = "min",
                  allowed=None, min_score=None, tracks: bool = True, ts_range=None, classes=None, b_ts_range=None, b_classes=None):
        """`rank` for the rows of question `a` that have a partner - an answer of question `b` - within `within` seconds in the same
        group -> (idx (1, count) int32, score (1, count) f32, total (1,) int64, partner (1, count) int32, partner_score (1, count) f32,
        n_partners int).  `a` / `b`: a (dim,) vector or an int, a stored row.  The partner list is the first `partners` (at most 16384)
        answers of an ungrouped `rank` of `b` with the cut `cut_b` and the filter b_ts_range / b_classes, among rows that have a ts;
        n_partners is its length without the cap.  A row's partner is the first entry of that list - the best-scoring one - that is
        another row of the same group, at most `within` seconds away (64-bit difference) and not a crop of the row's own track; a row
        without one does not compete.  value "a": the ranking value is `a`'s score; "min": the smaller of that and the partner's
        score for `b`.  Everything else - answers per track, tie rules, `min_score` (on the value), ts_range / classes (for `a`),
        `allowed` (for both), padding - is `rank`'s.  partner / partner_score: per answer the partner's row and its score for `b`, -1 /
        -inf past the last answer (cc_index_rank_near)."""
        return self._rank_near(a, b, within, start, count, partners, cut_b, value, allowed, min_score, tracks, ts_range, classes, b_ts_range,
                               b_classes, False, True)

    def rank_near_device(self, a, b, within, start: int = 0, count: int = 100, partners: int = _lib.NEAR_DEFAULT_PARTNERS, cut_b=None, value: str = "min",
                         allowed=None, min_score=None, tracks: bool = True, with_total: bool = True, ts_range=None, classes=None, b_ts_range=None,
                         b_classes=None):
        """`rank_near` with idx / score / partner / partner_score left on the GPU, as `rank_device` leaves them, on the current torch
        stream; with_total=False returns None for total and n_partners and waits for nothing."""
        return self._rank_near(a, b, within, start, count, partners, cut_b, value, allowed, min_score, tracks, ts_range, classes, b_ts_range,
                               b_classes, True, with_total)

    def timeline_near(self, a, b, within, t0: int, bin_seconds: int, n_bins: int, partners: int = _lib.NEAR_DEFAULT_PARTNERS, cut_b=None,
                      value: str = "min", allowed=None, min_score=None, tracks: bool = True, ts_range=None, classes=None, b_ts_range=None,
                      b_classes=None):
        """How the answers of `rank_near` (same question) spread over time -> (counts (1, n_bins) int64, total (1,) int64, n_partners
        int), binned as `timeline` bins them; total and n_partners equal `rank_near`'s (cc_index_timeline_near)."""
        head, tail, _keep = self._near_question(a, b, within, partners, cut_b, value, min_score, tracks, False)
        wa, wb = self.row_filter(ts_range, classes), self.row_filter(b_ts_range, b_classes)
        bins, counts = self._timeline_args(1, t0, bin_seconds, n_bins)
        total, n_partners = np.zeros(1, np.int64), np.zeros(1, np.int64)
        _lib.check(_lib.lib().cc_index_timeline_near(*head, *tail, *self._near_filters(allowed, wa, wb), *bins, _lib.ptr(counts),
                                                     _lib.ptr(total), _lib.ptr(n_partners), 0, None))
        return counts.astype(np.int64), total, int(n_partners[0])


    # -- distinct answers: near-duplicate answers of a ranked list folded into the first of them (cc_index_gram / cc_index_distinct) ----
    def gram(self, rows, device_out: bool = False):
        """Pairwise similarities of stored rows -> (n, n) float32, out[i][j] = <fetch(rows)[i], fetch(rows)[j]> in f32, 1 <= n <= 1024
        (cc_index_gram).  A pair's value depends on its two stored rows alone and the matrix equals its transpose bit for bit.
        device_out: a CUDA torch tensor on the current torch stream, nothing waited for."""
        ids = self._row_numbers(rows)
        n = int(ids.size)
        side = n if 1 <= n <= _lib.DISTINCT_MAX_DEPTH else 1                       # the library names the error
        out, = self._outputs(device_out, ((side, side), np.float32))
        self._call(device_out, lambda on_device, stream: _lib.check(_lib.lib().cc_index_gram(
            self._h, self._rows_ptr(ids), n, _lib.ptr(out), on_device, stream)))
        return out

    def _distinct(self, idx, score, same_at, start, count, device: bool, with_total: bool):
        if device:
            import torch
            dev = self._dev()[0]
            ia = idx.to(device=dev, dtype=torch.int32).contiguous()
            cast = lambda s: s.to(device=dev, dtype=torch.float32).contiguous()      # noqa: E731
        else:
            ia = np.ascontiguousarray(np.asarray(idx), dtype=np.int32)
            cast = lambda s: np.ascontiguousarray(as_numpy(s), dtype=np.float32)    # noqa: E731
        ia = ia.reshape(1, -1) if ia.ndim < 2 else ia.reshape(ia.shape[0], -1)
        Q, depth = int(ia.shape[0]), int(ia.shape[1])
        count = depth if count is None else int(count)
        sa = None if score is None else cast(score).reshape(Q, depth)
        shape = self._page(Q, 0, count)
        oi, os_, od = self._outputs(device, (shape, np.int32), (shape, np.float32) if sa is not None else None, (shape, np.int32))
        total = np.zeros(max(Q, 1), np.int64) if with_total else None
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_distinct(
            self._h, _lib.ptr(ia), _lib.ptr(sa), Q, depth, float(same_at), int(start), count, _lib.ptr(oi), _lib.ptr(os_), _lib.ptr(od),
            _lib.ptr(total), on_device, stream)), ia, sa)
        return oi, os_, od, total

    def distinct(self, idx, score=None, same_at: float = 0.9, start: int = 0, count=None):
        """Thin ranked lists of row numbers -> (idx (Q, count) int32, score (Q, count) f32 or None, dups (Q, count) int32, total (Q,)
        int64).  idx (Q, depth) or (depth,), depth <= 1024, Q <= 64, in ranked order (e.g. `rank(q, 0, depth)[0]`); entries < 0 or
        >= len(self) are absent.  Walking a list in order, an entry is kept unless `gram` of it and an entry KEPT before it is
        >= same_at (float32); a dropped entry is counted in `dups` of the first kept entry that matches it.  The kept entries are
        the answers: start .. start+count-1 of them come back (count: depth by default), -1 / -inf / 0 past the last, and `total`
        is their number.  `score` is passed through (cc_index_distinct)."""
        return self._distinct(idx, score, same_at, start, count, False, True)

    def distinct_device(self, idx, score=None, same_at: float = 0.9, start: int = 0, count=None, with_total: bool = True):
        """`distinct` for CUDA tensors, e.g. the idx / score of `rank_device` or `rank_like_device`: the answers stay on the GPU, on
        the current torch stream.  `total` comes back as a host array, which costs one wait for the stream; with_total=False
        returns None in its place and waits for nothing."""
        return self._distinct(idx, score, same_at, start, count, True, with_total)


    # -- day digest: every distinct object among the competing rows once, with count and times (cc_index_digest) -----------------------
    DIGEST_BY = {"count": _lib.DIGEST_BY_COUNT, "first": _lib.DIGEST_BY_FIRST}

    def _digest(self, same_at, start, count, allowed, ts_range, classes, max_leaders, by, owners, device: bool, with_total: bool):
        where = self.row_filter(ts_range, classes)
        count = int(max_leaders) if count is None else int(count)
        k = count if count >= 1 else 1                                             # the library names the error
        n = len(self)
        *out, owner = self._outputs(device, *[((k,), np.int32)] * 4, ((max(n, 1),), np.int32) if owners else None)
        totals = np.zeros(3, np.int64) if with_total else None
        if by not in self.DIGEST_BY:
            raise ValueError('by: "count" or "first"')
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_digest(
            self._h, float(same_at), int(max_leaders), self.DIGEST_BY[by], *self._allowed(allowed), self._where(where), int(start), count,
            *(_lib.ptr(o) for o in out), _lib.ptr(owner), _lib.ptr(totals), on_device, stream)))
        return (*out, totals, owner[:n]) if owners else (*out, totals)

    def digest(self, same_at: float = 0.9, start: int = 0, count=None, allowed=None, ts_range=None, classes=None, max_leaders: int = 1024,
               by: str = "count", owners: bool = False):
        """What is in the index, every distinct object once -> (rows (count,) int32, counts (count,) int32, ts_first (count,) int32,
        ts_last (count,) int32, totals (3,) int64[, owner (len(self),) int32]).  No query: the rows that compete are `rank`'s with
        tracks=False (allowed, ts_range, classes), walked in row order, which is ingest order.  A row joins the first-created leader
        whose `gram` with it is >= same_at (float32), else it becomes a leader while fewer than max_leaders (<= 1024) exist, else
        it is left over.  Per leader: its row (the first sighting), its members (itself included) and the min / max ts among them
        (_lib.ROW_NO_TS: none has one).  by="count": most members first, equal counts by row; "first": in order of appearance.
        Entries start .. start+count-1 come back (count: max_leaders by default), -1 / 0 / ROW_NO_TS past the last.  totals: leaders,
        competing rows, left-over rows; the counts of all leaders sum to totals[1] - totals[2].  owners=True: per index row its
        leader's row, -1 where the row did not compete, -2 where it was left over (cc_index_digest)."""
        return self._digest(same_at, start, count, allowed, ts_range, classes, max_leaders, by, owners, False, True)

    def digest_device(self, same_at: float = 0.9, start: int = 0, count=None, allowed=None, ts_range=None, classes=None, max_leaders: int = 1024,
                      by: str = "count", owners: bool = False, with_total: bool = True):
        """`digest` with rows / counts / ts_first / ts_last (and owner) left on the GPU as CUDA torch tensors on the current torch
        stream.  `totals` comes back as a host array, which costs one wait for the stream; with_total=False returns None in its
        place and nothing but tensors comes back (inside, the call reads back one number, the count of competing rows)."""
        return self._digest(same_at, start, count, allowed, ts_range, classes, max_leaders, by, owners, True, with_total)


    # -- seen before: up to 1024 stored rows against all competing rows, reduced per object (cc_index_sightings) --------------------------
    def _sightings(self, rows, same_at, allowed, ts_range, classes, skip_self, group_counts, with_total, device: bool):
        where = self.row_filter(ts_range, classes)
        n, g = int(np.asarray(rows).size), int(group_counts)
        n, g = (n if 1 <= n <= _lib.SIGHT_MAX_OBJECTS else 1), (g if 0 <= g <= _lib.SIGHT_MAX_GROUPS else 1)   # outside: the library names the error
        out = self._outputs(device, ((n,), np.int32), ((n,), np.int32), ((n,), np.float32), ((n, g), np.uint32) if group_counts else None)
        total = np.zeros(1, np.int64) if with_total else None
        ids = self._row_numbers(rows)
        self._call(device, lambda on_device, stream: _lib.check(_lib.lib().cc_index_sightings(
            self._h, self._rows_ptr(ids), int(ids.size), float(same_at), _lib.SIGHT_SKIP_SELF if skip_self else 0, *self._allowed(allowed),
            self._where(where), *(_lib.ptr(o) for o in out), int(group_counts), _lib.ptr(total), on_device, stream)))
        return (*out, None if total is None else int(total[0]))

    def sightings(self, rows, same_at: float = 0.9, allowed=None, ts_range=None, classes=None, skip_self: bool = False, group_counts: int = 0,
                  with_total: bool = True):
        """Stored rows (the objects, 1 .. 1024 of them, repeats allowed) against ALL competing rows -> (count (n,) int32, best_row (n,)
        int32, best_score (n,) f32, group_counts (n, group_counts) uint32 or None, total).  The rows that compete are `rank`'s with
        tracks=False (allowed, ts_range, classes); an object need not compete itself.  The value of a pair is `gram` of the two rows
        (that very float).  count: the pairs >= same_at (float32); best: the pair with the largest value, equal values by the lower
        row, -1 / -inf without a pair, whatever same_at; group_counts[i][g]: the matches of object i in group g (matches in groups
        >= group_counts are in count only).  skip_self: the pair of an object with its own row number does not exist.  total: the
        number of competing rows (cc_index_sightings)."""
        return self._sightings(rows, same_at, allowed, ts_range, classes, skip_self, group_counts, with_total, False)

    def sightings_device(self, rows, same_at: float = 0.9, allowed=None, ts_range=None, classes=None, skip_self: bool = False,
                         group_counts: int = 0, with_total: bool = True):
        """`sightings` with the four outputs left on the GPU as CUDA torch tensors on the current torch stream (rows stay a host
        list; the uint32 group counts come in an int32 tensor).  with_total=False returns None for the total and waits for nothing:
        inside, nothing is read back."""
        return self._sightings(rows, same_at, allowed, ts_range, classes, skip_self, group_counts, with_total, True)


    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().cc_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
