"""Host-side mirror of ``detection/yolov9.py``: same class name, constructor and call surface,
compute in libclearcam_hip (HIP/MFMA) through the C ABI in include/clearcam_hip.h.

    model = YOLOv9("c", 640, state_dict=sd)          # reference: YOLOv9(size, res) + download
    preds = jit_infer(model, Tensor(frame), cache).numpy()     # (300,6) float32, clearcam.py:583

There is no CPU path: without the HIP library / a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .arch import YOLO_ARCH
from .helpers import Tensor, as_numpy
from .weights import load_safetensors

# "f16s": f16 activations with every conv weight carried as two f16 planes (W = W_hi + W_lo, ~22 significant bits, f32 accumulation):
# the 16-bit mode whose WEIGHTS are exact to f32 for any checkpoint.  "f16h" keeps the second plane only where it is needed - the 1x1
# convs of the backbone (blocks 0-9) and the stem conv; every other conv carries one f16 plane with controlled rounding (which balances a
# 3x3 filter's taps and has nothing to balance in a 1x1) - and stays as close to the f32 oracle on three independently calibrated
# un-rounded checkpoints at 1.4x the frame rate.  Plain f16 / bf16 round every weight
# to 11 / 8 bits: speed modes.  "f32" is the exact-arithmetic parity mode.
DTYPES = {"f32": 0, "float32": 0, "f16": 1, "float16": 1, "half": 1, "bf16": 2, "bfloat16": 2, "f16s": 3, "f16_split": 3, "f16h": 4, "f16c": 5}
MAX_DET = 300


# -- ragged batches: frames of different sizes that letterbox to one network shape ------------------------------------------------------
def letterbox_geometry(h: int, w: int, res: int) -> Tuple[int, int, int, int]:
    """(new_h, new_w, pad_y, pad_x) of an h x w frame letterboxed to `res` (yolov9.py:390-403), from the library's host-only helper: the
    very values the ragged entry points group by."""
    v = [C.c_int() for _ in range(4)]
    _lib.check(_lib.lib().cc_letterbox_geometry(int(h), int(w), int(res), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def network_shape(h: int, w: int, res: int) -> Tuple[int, int]:
    """(Hn, Wn): what the network sees of an h x w frame at `res`.  Frames with the same network shape can share a ragged batch."""
    nh, nw, py, px = letterbox_geometry(h, w, res)
    return nh + 2 * py, nw + 2 * px


class RaggedGroup:
    """The frames of a detect_frames call that run as ONE ragged batch: same network shape, same element type, same residency.
    index: their positions in the caller's list; offsets / heights / widths: the three host tables of cc_yolo_detect_ragged for the
    frames packed back to back in that order; nbytes: size of the packed buffer."""

    def __init__(self, shape, f32, on_device):
        self.shape, self.f32, self.on_device = shape, f32, on_device
        self.index: List[int] = []
        self.heights: List[int] = []
        self.widths: List[int] = []

    def finish(self):
        es = 4 if self.f32 else 1
        sizes = np.asarray(self.heights, np.int64) * np.asarray(self.widths, np.int64) * 3 * es
        self.offsets = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64))
        self.nbytes = int(sizes.sum())
        self.heights = np.ascontiguousarray(self.heights, np.int32)
        self.widths = np.ascontiguousarray(self.widths, np.int32)
        return self

    def tables(self):
        i32p = C.POINTER(C.c_int32)
        return (self.offsets.ctypes.data_as(C.POINTER(C.c_int64)), self.heights.ctypes.data_as(i32p), self.widths.ctypes.data_as(i32p))


def _frame_kind(i: int, f):
    """(h, w, is_f32, on_device) of frame i, ValueError naming i otherwise."""
    on_dev = bool(getattr(f, "is_cuda", False))
    shape = tuple(getattr(f, "shape", ()))
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"frame {i}: must be (H,W,3), got shape {shape}")
    dt = str(f.dtype).replace("torch.", "")
    if dt not in ("uint8", "float32"):
        raise ValueError(f"frame {i}: must be uint8 or float32, got {dt}")
    return int(shape[0]), int(shape[1]), dt == "float32", on_dev


def group_frames(frames: Sequence, res: int) -> List[RaggedGroup]:
    """The host part of detect_frames, a pure function of the frames' shapes and dtypes: one RaggedGroup per (network shape, element
    type, residency) in order of first appearance, frames inside a group in input order.  ValueError (with the frame's index) for a
    frame that is not (H,W,3) uint8 / float32 or whose letterbox is not a multiple of 32."""
    groups: Dict[tuple, RaggedGroup] = {}
    for i, f in enumerate(frames):
        h, w, f32, on_dev = _frame_kind(i, f)
        hn, wn = network_shape(h, w, res)
        if hn <= 0 or wn <= 0 or hn % 32 or wn % 32:
            raise ValueError(f"frame {i}: {h}x{w} letterboxes to {hn}x{wn} at res {res}, not a multiple of 32 (the reference graph cannot run this shape either)")
        g = groups.setdefault((hn, wn, f32, on_dev), RaggedGroup((hn, wn), f32, on_dev))
        g.index.append(i); g.heights.append(h); g.widths.append(w)
    return [g.finish() for g in groups.values()]


def pack_group(frames: Sequence, g: RaggedGroup, buf: np.ndarray) -> np.ndarray:
    """Host frames of group g, back to back, into the uint8 buffer `buf` (>= g.nbytes; e.g. a view of pinned memory): one copy per frame."""
    for i, off in zip(g.index, g.offsets):
        a = np.ascontiguousarray(as_numpy(frames[i]))
        n = a.nbytes
        buf[off:off + n] = a.reshape(-1).view(np.uint8)
    return buf


def scatter_rows(groups: Sequence[RaggedGroup], outs: Sequence[np.ndarray], n: int) -> np.ndarray:
    """Per-group (B_g,300,6) rows back into input order: (n,300,6)."""
    out = np.empty((n, MAX_DET, 6), np.float32)
    for g, o in zip(groups, outs):
        out[g.index] = o
    return out


class RaggedTicket:
    """submit_frames' handle: the library tickets of its groups plus everything that has to stay alive until wait()."""

    def __init__(self, n, groups, tickets, bufs, outs):
        self.n, self.groups, self.tickets, self.bufs, self.outs = n, groups, tickets, bufs, outs


class YOLOv9:
    def __init__(self, size: str = "t", res: int = 1280, state_dict: Optional[Dict[str, np.ndarray]] = None,
                 weights: Optional[str] = None, dtype: str = "f16h", device: int = 0, calibration_frames=None):
        """dtype: "f16h" (default) - f16 activations, split f16 weights in the backbone's 1x1 convs and the stem, one controlled-rounded
        f16 plane elsewhere: detections within the reference tolerance on un-rounded float32 checkpoints; "f16s" - split weights in every
        conv (weights exact to f32 whatever the checkpoint; 0.7x the rate); "f32" - the exact-arithmetic parity mode (5x slower); "f16" / "bf16" - speed modes whose 11 / 8-bit weight
        rounding (controlled rounding: filter sums preserved) moves boxes by up to a pixel / several pixels on the conditioned synthetic checkpoint.  f16
        storage saturates at 65504: a checkpoint whose activations exceed that needs "bf16" or "f32".
        "f16c" (round 5) - one f16 plane per conv (two in the stem conv) at plain f16's rate, the 1x1 convs' weights rounded by a
        calibration-aware recursion on `calibration_frames` ((B,H,W,3) BGR uint8 / float32 array: a few frames of the camera; default: four
        frames of seeded white noise) - "f16h"'s tolerance on inputs like the calibration frames."""
        if size not in YOLO_ARCH and size != "e":
            raise ValueError(f"unsupported size {size!r}: t, s, m, c, e")
        self.size, self.res, self.dtype, self.device = size, res, dtype, device
        if state_dict is None:
            # reference: safe_load(fetch(".../yolov9-{size}.safetensors")) (yolov9.py:372); no network here
            path = weights or os.path.join(os.environ.get("CLEARCAM_WEIGHTS_DIR", "weights"), f"yolov9-{size}.safetensors")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path} not found: pass state_dict= or weights= (the reference downloads "
                                        f"yolov9-{size}.safetensors from HuggingFace; there is no network here)")
            state_dict = load_safetensors(path)
        L = _lib.lib()
        self._h = C.c_void_p()
        _lib.check(L.cc_yolo_create(C.byref(self._h), size.encode(), res, DTYPES[dtype], device))
        for name, arr in state_dict.items():
            if name.endswith(("anchors", "strides")):      # Tensor attributes the reference recomputes per call
                continue
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shp = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            _lib.check(L.cc_yolo_load(self._h, name.encode(), _lib.ptr(a), shp, a.ndim))
        if calibration_frames is not None:
            if dtype != "f16c":
                raise ValueError('calibration_frames are for dtype "f16c"')
            f = np.ascontiguousarray(as_numpy(calibration_frames))
            if f.ndim != 4 or f.shape[3] != 3 or f.dtype not in (np.uint8, np.float32):
                raise ValueError(f"calibration_frames must be (B,H,W,3) uint8 or float32, got {f.shape} {f.dtype}")
            _lib.check(L.cc_yolo_calibrate(self._h, _lib.ptr(f), f.shape[0], f.shape[1], f.shape[2], int(f.dtype == np.float32)))
        _lib.check(L.cc_yolo_finalize(self._h))

    def calibration_info(self):
        """dtype "f16c": (packed 1x1 convs rounded by the calibration-aware recursion, convs left to the plain controlled rounding)."""
        a, b = C.c_int(), C.c_int()
        _lib.check(_lib.lib().cc_yolo_calibration_info(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- reference surface ------------------------------------------------------------------------
    def __call__(self, frame) -> Tensor:
        """``YOLOv9.__call__(frame)``: (H,W,3) BGR uint8/float32 -> Tensor (300,6)."""
        f = as_numpy(frame)
        if f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"frame must be (H,W,3), got {f.shape}")
        return Tensor(self.detect_batch(f[None])[0])

    # -- batched extension (one camera per row) ---------------------------------------------------
    def detect_batch(self, frames) -> np.ndarray:
        """(B,H,W,3) BGR uint8/float32 host array or CUDA torch tensor -> (B,300,6) float32 ndarray."""
        L = _lib.lib()
        on_dev = bool(getattr(frames, "is_cuda", False))
        if on_dev:
            import torch
            f = frames.contiguous()
            is_f32 = f.dtype == torch.float32
            if not is_f32 and f.dtype != torch.uint8:
                raise TypeError("device frames must be uint8 or float32")
            B, H, W, ch = f.shape
            torch.cuda.current_stream(f.device).synchronize()
        else:
            f = as_numpy(frames)
            if f.dtype != np.uint8:
                f = f.astype(np.float32, copy=False)
            f = np.ascontiguousarray(f)
            is_f32 = f.dtype == np.float32
            B, H, W, ch = f.shape
        if ch != 3:
            raise ValueError("frames must be (B,H,W,3)")
        out = np.empty((B, MAX_DET, 6), np.float32)
        _lib.check(L.cc_yolo_detect(self._h, _lib.ptr(f), B, H, W, int(is_f32), int(on_dev), _lib.ptr(out), 0, None))
        return out

    def detect_batch_device(self, frames, out):
        """Device-resident variant for benchmarks: frames/out are CUDA torch tensors; no host copies, no sync."""
        import torch
        B, H, W, _ = frames.shape
        s = torch.cuda.current_stream(frames.device).cuda_stream
        _lib.check(_lib.lib().cc_yolo_detect(self._h, _lib.ptr(frames), B, H, W, int(frames.dtype == torch.float32), 1,
                                             _lib.ptr(out), 1, C.c_void_p(s)))
        return out

    # -- ragged batches: cameras of different resolutions in one batch -----------------------------
    def network_shape(self, h: int, w: int) -> Tuple[int, int]:
        """(Hn, Wn) the network sees of an h x w frame at this model's res (needs nothing of the model but `res`)."""
        return network_shape(h, w, self.res)

    def _pinned(self, nbytes: int):
        """A pinned uint8 torch tensor of at least nbytes from the model's free list (sizes rounded up to a power of two)."""
        import torch
        size = 1 << max(12, int(nbytes - 1).bit_length())
        pool = self.__dict__.setdefault("_pin_pool", {})
        free = pool.setdefault(size, [])
        return free.pop() if free else torch.empty(size, dtype=torch.uint8).pin_memory()

    def _unpin(self, t) -> None:
        self._pin_pool[t.numel()].append(t)

    def _pack(self, frames, g: RaggedGroup):
        """Group g's packed pixels: (tensor to keep alive, pinned?) - device frames are concatenated on the device, host frames are
        packed ONCE into pinned memory."""
        if g.on_device:
            import torch
            return torch.cat([frames[i].contiguous().view(torch.uint8).reshape(-1) for i in g.index]), False
        buf = self._pinned(g.nbytes)
        pack_group(frames, g, buf.numpy())
        return buf, True

    def detect_frames(self, frames: Sequence) -> np.ndarray:
        """A sequence of (H_i,W_i,3) BGR uint8 / float32 frames of ANY sizes (numpy arrays or torch tensors, host or device) ->
        (N,300,6) float32 rows in input order.  Frames are grouped by network shape (and element type / residency); each group runs
        as one ragged batch of that shape's plan (cc_yolo_detect_ragged).  Row i is bit-identical to `self(frames[i])`."""
        L = _lib.lib()
        groups = group_frames(frames, self.res)
        outs = []
        for g in groups:
            pixels, pinned = self._pack(frames, g)
            s = None
            if g.on_device:
                import torch
                s = C.c_void_p(torch.cuda.current_stream(pixels.device).cuda_stream)
            o = np.empty((len(g.index), MAX_DET, 6), np.float32)
            try:
                _lib.check(L.cc_yolo_detect_ragged(self._h, _lib.ptr(pixels), *g.tables(), len(g.index), int(g.f32), int(g.on_device), _lib.ptr(o), 0, s))
            finally:
                if pinned:
                    self._unpin(pixels)
            outs.append(o)
        return scatter_rows(groups, outs, len(frames))

    def detect_ragged_device(self, pixels, offsets: np.ndarray, heights: np.ndarray, widths: np.ndarray, out):
        """Device-resident ragged batch for pipelines: `pixels` a uint8 CUDA tensor holding frame b (heights[b] x widths[b] x 3 uint8) at
        byte offsets[b]; the tables are int64 / int32 / int32 numpy arrays; out a (B,300,6) float32 CUDA tensor.  All frames must share
        one network shape.  Ordered on the current torch stream; no host copies, no sync."""
        import torch
        i32p = C.POINTER(C.c_int32)
        s = torch.cuda.current_stream(pixels.device).cuda_stream
        _lib.check(_lib.lib().cc_yolo_detect_ragged(self._h, _lib.ptr(pixels), offsets.ctypes.data_as(C.POINTER(C.c_int64)), heights.ctypes.data_as(i32p),
                                                    widths.ctypes.data_as(i32p), len(offsets), 0, 1, _lib.ptr(out), 1, C.c_void_p(s)))
        return out

    def submit_frames(self, frames: Sequence) -> RaggedTicket:
        """The ragged counterpart of submit(): queue the frames of detect_frames on the next detector slot(s) - one submission per
        group - and return at once; wait(ticket, host=True) returns the (N,300,6) rows, bit-identical to detect_frames(frames).
        Host frames are packed into pinned memory here, so the caller's arrays may be reused immediately; device frames are
        concatenated on the current torch stream."""
        import torch
        L = _lib.lib()
        groups = group_frames(frames, self.res)
        tickets, bufs, outs = [], [], []
        for g in groups:
            pixels, pinned = self._pack(frames, g)
            B = len(g.index)
            ob = self._pinned(B * MAX_DET * 6 * 4)
            s = C.c_void_p(torch.cuda.current_stream(pixels.device).cuda_stream) if g.on_device else None
            t = C.c_longlong()
            _lib.check(L.cc_yolo_submit_ragged(self._h, _lib.ptr(pixels), *g.tables(), B, int(g.f32), int(g.on_device), _lib.ptr(ob), 0, s, C.byref(t)))
            tickets.append(t.value); bufs.append((pixels, pinned)); outs.append(ob)
        return RaggedTicket(len(frames), groups, tickets, bufs, outs)

    def _wait_frames(self, ticket: RaggedTicket) -> np.ndarray:
        import torch
        L = _lib.lib()
        for t in ticket.tickets:
            _lib.check(L.cc_yolo_wait(self._h, t, None))
        outs = [o[:len(g.index) * MAX_DET * 6 * 4].view(torch.float32).numpy().reshape(len(g.index), MAX_DET, 6) for g, o in zip(ticket.groups, ticket.outs)]
        rows = scatter_rows(ticket.groups, outs, ticket.n)          # copies: the pinned buffers go back to the free list
        for (pixels, pinned), ob in zip(ticket.bufs, ticket.outs):
            if pinned:
                self._unpin(pixels)
            self._unpin(ob)
        ticket.bufs, ticket.outs = [], []
        return rows

    # -- batches in flight (throughput mode: one GPU serving many cameras) --------------------------
    def set_in_flight(self, n: int) -> None:
        """n slots (own stream, arena and graph each): consecutive submit() calls overlap - the last layers of one batch run beside
        the first layers of the next.  Results are bit-identical to detect_batch_device; n = 1 is the default."""
        _lib.check(_lib.lib().cc_yolo_set_in_flight(self._h, n))
        self.in_flight = n

    def submit(self, frames, out) -> int:
        """Queue one batch on the next slot: `frames` (B,H,W,3) uint8 / float32 and `out` (B,300,6) float32 are torch tensors, each
        either on the device or in PINNED host memory (then the slot's stream also carries the upload / download, which overlap the
        other slots' kernels); numpy arrays are taken as pageable host memory (correct, but the runtime stages such copies and the
        call may block).  Device frames are taken as ready on the current torch stream, which does NOT wait for the result -
        wait(ticket) does.  `frames` and `out` must stay alive (and `out` unshared with other submissions in flight) until then."""
        B, H, W, _ = frames.shape
        t = C.c_longlong()
        if isinstance(frames, np.ndarray) or isinstance(out, np.ndarray):
            if not (isinstance(frames, np.ndarray) and isinstance(out, np.ndarray)):
                raise TypeError("frames and out must both be torch tensors or both numpy arrays")
            if not frames.flags.c_contiguous or not out.flags.c_contiguous or out.dtype != np.float32 or frames.dtype not in (np.uint8, np.float32):
                raise ValueError("frames: C-contiguous uint8 / float32, out: C-contiguous float32")
            _lib.check(_lib.lib().cc_yolo_submit(self._h, _lib.ptr(frames), B, H, W, int(frames.dtype == np.float32), 0, _lib.ptr(out), 0, None, C.byref(t)))
            return t.value
        import torch
        if not frames.is_contiguous() or not out.is_contiguous():
            raise ValueError("frames and out must be contiguous")
        if (not frames.is_cuda and not frames.is_pinned()) or (not out.is_cuda and not out.is_pinned()):
            raise ValueError("host tensors handed to submit() must be pinned")
        s = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream if frames.is_cuda else 0
        _lib.check(_lib.lib().cc_yolo_submit(self._h, _lib.ptr(frames), B, H, W, int(frames.dtype == torch.float32), int(frames.is_cuda),
                                             _lib.ptr(out), int(out.is_cuda), C.c_void_p(s), C.byref(t)))
        return t.value

    def wait(self, ticket, host: bool = False):
        """Make the current torch stream (host=True: the calling thread) wait for a submission's result.  A submit_frames ticket is
        always waited for on the host and its (N,300,6) rows are returned."""
        if isinstance(ticket, RaggedTicket):
            return self._wait_frames(ticket)
        import torch
        s = None if host else C.c_void_p(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        _lib.check(_lib.lib().cc_yolo_wait(self._h, ticket, s))

    # -- parity taps --------------------------------------------------------------------------------
    def get_tensor(self, name: str, frames=None) -> np.ndarray:
        """A named intermediate of the last detect call as float32 (include/clearcam_hip.h lists the names); frames = (b0, nb): only
        frames [b0, b0 + nb) are copied (CCError if the range leaves [0, B))."""
        L = _lib.lib()
        shp, nd = (C.c_int64 * 4)(), C.c_int()
        if frames is None:
            get = lambda out: L.cc_yolo_get_tensor(self._h, name.encode(), out, shp, C.byref(nd))                          # noqa: E731
        else:
            b0, nb = (int(v) for v in frames)
            get = lambda out: L.cc_yolo_get_tensor_frames(self._h, name.encode(), b0, nb, out, shp, C.byref(nd))           # noqa: E731
        _lib.check(get(None))
        out = np.empty(tuple(shp[i] for i in range(nd.value)), np.float32)
        _lib.check(get(_lib.ptr(out)))
        return out

    def nonfinite(self) -> int:
        """Anchors whose logits were not finite since the last query (f16 activations past 65504): non-zero means this checkpoint needs
        dtype "bf16" or "f32".  Host-output calls (detect_batch, __call__) raise by themselves; device-output / submit() calls do not."""
        n = C.c_int()
        _lib.check(_lib.lib().cc_yolo_nonfinite(self._h, C.byref(n)))
        return n.value

    def last_gpu_ms(self) -> float:
        ms = C.c_float()
        _lib.check(_lib.lib().cc_yolo_last_gpu_ms(self._h, C.byref(ms)))
        return ms.value

    def profile(self, iters: int = 3) -> dict:
        """Per-kernel-family GPU time of the last plan (hipEvents around every launch, eager replay)."""
        ms, macs, n = (C.c_float * 5)(), C.c_double(), C.c_int()
        _lib.check(_lib.lib().cc_yolo_profile(self._h, iters, ms, C.byref(macs), C.byref(n)))
        return {"conv_ms": ms[0], "pool_ms": ms[1], "decode_ms": ms[2], "nms_ms": ms[3], "stem_ms": ms[4],
                "alg_macs_per_step": macs.value, "conv_launches": n.value}

    def profile_graph(self, which: int, iters: int = 10) -> float:
        """ms per replay of a subset of the last plan's launches captured into a hipGraph of its own (one event pair around `iters`
        replays): which = 0 the conv / GEMM launches, 1 every other launch, 2 the whole step."""
        ms = C.c_float()
        _lib.check(_lib.lib().cc_yolo_profile_graph(self._h, iters, which, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().cc_yolo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
