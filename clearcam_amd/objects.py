"""Host-side mirror of ``models/objects.py``: ``OpenCLIP`` (image + text towers) and ``ObjectFinder``
(embedding store + search), same names / signatures / return conventions, compute in libclearcam_hip.

    finder = ObjectFinder(); finder.init_clip(state_dict=sd)
    emb = jit_infer(finder.model.precompute_embedding, Tensor(img).unsqueeze(0), finder.jit_cache).numpy()   # clearcam.py:1285
    q   = finder.model._encode_text("white van").numpy()                                                     # clearcam.py:667
    hits = finder.search(query="white van", top_k=10)                                                         # clearcam.py:669

There is no CPU path: without the HIP library / a GPU every call raises.
"""
from __future__ import annotations

import ctypes as C
import os
import pickle
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from .alerts import AlertBook, WatchList  # noqa: F401  (re-exported: the alert surface belongs to this module's ObjectFinder)
from .arch import CLIP_L14, ClipArch
from .helpers import Tensor, as_numpy
from .index import EmbeddingIndex, row_filter  # noqa: F401  (re-exported: this module's ObjectFinder is built on them)
from .row_table import _RowTable, event_img_info, pick_track_rows  # noqa: F401  (re-exported: callers and tools import them from here)
from .weights import load_safetensors
from .yolov9 import DTYPES


class OpenCLIP:
    """``models/objects.py:21-186``.  ``state_dict`` replaces the HuggingFace download (:91)."""

    def __init__(self, base_path: str = "data/cameras", state_dict: Optional[Dict[str, np.ndarray]] = None,
                 weights: Optional[str] = None, arch: ClipArch = CLIP_L14, dtype: str = "bf16", device: int = 0,
                 tokenizer=None):
        self.base_path, self.arch, self.dtype, self.device = base_path, arch, dtype, device
        self._tokenizer = tokenizer
        if state_dict is None:
            path = weights or os.path.join(os.environ.get("CLEARCAM_WEIGHTS_DIR", "weights"),
                                           "CLIP-ViT-L-14-laion2B-s32B-b82K.safetensors")
            if not os.path.exists(path):
                raise FileNotFoundError(f"{path} not found: pass state_dict= or weights= (the reference downloads the "
                                        "checkpoint from HuggingFace; there is no network here)")
            state_dict = load_safetensors(path)
        L = _lib.lib()
        cfg = _lib.ClipConfig(*[getattr(arch, f) for f, _ in _lib.ClipConfig._fields_])
        self._h = C.c_void_p()
        _lib.check(L.cc_clip_create(C.byref(self._h), C.byref(cfg), DTYPES[dtype], device))
        for name, arr in state_dict.items():
            if name == "attn_mask":            # a Tensor attribute in the reference (:76); recomputed in-kernel
                continue
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shp = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            _lib.check(L.cc_clip_load(self._h, name.encode(), _lib.ptr(a), shp, a.ndim))
        _lib.check(L.cc_clip_finalize(self._h))

    @property
    def tokenizer(self):
        if self._tokenizer is None:
            from .clip_tokenizer import SimpleTokenizer
            self._tokenizer = SimpleTokenizer()
        return self._tokenizer

    # -- reference surfaces ---------------------------------------------------------------------------
    def precompute_embedding(self, x) -> Tensor:
        """:94-133 — (B,3,224,224) float32 -> Tensor (B,768), unit norm."""
        a = np.ascontiguousarray(as_numpy(x), dtype=np.float32)
        s = self.arch.image_size
        if a.ndim != 4 or a.shape[1:] != (3, s, s):
            raise ValueError(f"expected (B,3,{s},{s}), got {a.shape}")
        out = np.empty((a.shape[0], self.arch.embed), np.float32)
        _lib.check(_lib.lib().cc_clip_encode_image(self._h, _lib.ptr(a), a.shape[0], 0, _lib.ptr(out), 0, None))
        return Tensor(out)

    def precompute_embedding_device(self, x, out):
        """Device-resident variant (CUDA torch tensors in and out, no host copies) for benchmarks."""
        import torch
        s = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(_lib.lib().cc_clip_encode_image(self._h, _lib.ptr(x), x.shape[0], 1, _lib.ptr(out), 1, C.c_void_p(s)))
        return out

    # -- batches in flight (many small batches: the reference encodes one crop per call, :356-363) -----------------------------------
    def set_in_flight(self, n: int) -> None:
        """n slots (own stream, buffers and graph each) for submit_image(); results are bit-identical to precompute_embedding."""
        _lib.check(_lib.lib().cc_clip_set_in_flight(self._h, n))

    def submit_image(self, x, out) -> int:
        """Queue one (B,3,224,224) float32 batch -> `out` (B,768) float32 on the next slot; CUDA or PINNED-host torch tensors.
        Device input is taken as ready on the current torch stream, which does not wait for the result - wait(ticket) does."""
        import torch
        if not x.is_contiguous() or not out.is_contiguous() or x.dtype != torch.float32 or out.dtype != torch.float32:
            raise ValueError("x and out must be contiguous float32 tensors")
        if (not x.is_cuda and not x.is_pinned()) or (not out.is_cuda and not out.is_pinned()):
            raise ValueError("host tensors handed to submit_image() must be pinned")
        t = C.c_longlong()
        s = torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else 0
        _lib.check(_lib.lib().cc_clip_submit_image(self._h, _lib.ptr(x), x.shape[0], int(x.is_cuda), _lib.ptr(out), int(out.is_cuda),
                                                   C.c_void_p(s), C.byref(t)))
        return t.value

    def wait(self, ticket: int, host: bool = False) -> None:
        """Make the current torch stream (host=True: the calling thread) wait for a submission's embeddings."""
        import torch
        s = None if host else C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(_lib.lib().cc_clip_wait(self._h, ticket, s))

    def encode_tokens(self, tokens) -> np.ndarray:
        """Batch form of ``encode_text`` (:145-186): (B,77) int -> (B,768) float32."""
        t = np.ascontiguousarray(as_numpy(tokens), dtype=np.int32)
        if t.ndim != 2 or t.shape[1] != self.arch.t_ctx:
            raise ValueError(f"expected (B,{self.arch.t_ctx}) tokens, got {t.shape}")
        out = np.empty((t.shape[0], self.arch.embed), np.float32)
        _lib.check(_lib.lib().cc_clip_encode_text(self._h, _lib.ptr(t), t.shape[0], _lib.ptr(out), 0, None))
        return out

    def _encode_text(self, query: str, realize: bool = False):
        """:135-143 — str -> Tensor (768,) (ndarray if realize)."""
        emb = self.encode_tokens(self.tokenizer.tokens_for_model(query))[0]
        return emb if realize else Tensor(emb)

    def last_gpu_ms(self) -> float:
        ms = C.c_float()
        _lib.check(_lib.lib().cc_clip_last_gpu_ms(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().cc_clip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Term(NamedTuple):
    """One term of `ObjectFinder.compound`: exactly one of text (a query string, encoded by the CLIP text tower), path (a stored
    crop, by its key or the endpoint's form, as `similar` takes it) or embedding (a vector of the index's width).  role "rank": the
    term contributes to the ranking value (weight: its factor under combine="sum"); "require": only crops it scores >= cut compete;
    "reject": crops it scores >= cut do not."""
    text: Optional[str] = None
    path: Optional[str] = None
    embedding: object = None
    role: str = "rank"
    weight: float = 1.0
    cut: Optional[float] = None


def pack_crops(crops, tail: int = 0):
    """List of (H,W,3) uint8 arrays -> (packed bytes, offsets int64, heights int32, widths int32): the packed-buffer convention of
    cc_crop_preprocess / cc_face_locate / cc_face_align.  `tail` zero bytes are appended behind the last crop."""
    crops = [np.ascontiguousarray(c, dtype=np.uint8) for c in crops]
    for c in crops:
        if c.ndim != 3 or c.shape[2] != 3 or c.size == 0:
            raise ValueError(f"crop must be a non-empty (H,W,3) uint8 array, got {c.shape}")
    if len(crops) == 0:
        raise ValueError("no crops")
    sizes = np.array([c.size for c in crops], np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
    packed = np.concatenate([c.reshape(-1) for c in crops] + ([np.zeros(tail, np.uint8)] if tail else []))
    hs = np.array([c.shape[0] for c in crops], np.int32)
    ws = np.array([c.shape[1] for c in crops], np.int32)
    return packed, offsets, hs, ws


def preprocess_crops(crops, size: int = 224, device: int = 0):
    """cc_crop_preprocess over a list of (H,W,3) uint8 arrays (host) -> torch device tensor (B,3,size,size) f32."""
    import torch
    packed, offsets, hs, ws = pack_crops(crops)
    B = len(hs)
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device=torch.device("cuda", device))
    _lib.check(_lib.lib().cc_crop_preprocess(_lib.ptr(packed), _lib.ptr(offsets), _lib.ptr(hs), _lib.ptr(ws), B, 0, size, _lib.ptr(out), device,
                                   torch.cuda.current_stream(device).cuda_stream))
    return out


class FaceGeometry(NamedTuple):
    """What `ObjectFinder._face_geometry` hands to the two warps: the cut rectangle inside the crop, the forward matrix that levels
    it into an out_w x out_h image (float64), and the forward matrix that places the eyes in the 112 x 112 face (float32)."""
    cx1: int
    cy1: int
    cw: int
    ch: int
    rot: np.ndarray
    out_w: int
    out_h: int
    place: np.ndarray


class _PackedCrops(NamedTuple):
    buf: object                # CUDA uint8 tensor: the packed crops + three zero bytes
    nbytes: int
    offsets: np.ndarray
    hs: np.ndarray
    ws: np.ndarray


# -- what ObjectFinder's questions share: argument checks (each names the question it speaks for), the scope, rows and scores to answers --
def _row_kw(ts_range, classes):
    """-> (row filter or None, the keyword arguments that carry it to the index: none without a filter)"""
    where = row_filter(ts_range, classes)
    return where, ({} if where is None else {"ts_range": ts_range, "classes": classes})


def _page_args(name: str, start, count) -> Tuple[int, int]:
    start, count = int(start), int(count)
    if start < 0 or count < 1:
        raise ValueError(f"{name} needs start >= 0 and count >= 1")
    return start, count


def _bin_args(name: str, t0, bin_seconds, n_bins) -> Tuple[int, int, int]:
    t0, bin_seconds, n_bins = int(t0), int(bin_seconds), int(n_bins)
    if bin_seconds < 1 or not 1 <= n_bins <= 4096:
        raise ValueError(f"{name} needs bin_seconds >= 1 and 1 <= n_bins <= 4096")
    return t0, bin_seconds, n_bins


def _cut_arg(cut, name: str = "min_score"):
    if cut is not None and cut != cut:
        raise ValueError(f"{name} is NaN")
    return cut


def _choice_arg(name: str, value, choices) -> None:
    """`value` is one of `choices` (None, or names), which the message lists in their order"""
    if value not in choices:
        said = [str(c) if c is None else f'"{c}"' for c in choices]
        raise ValueError(f"{name}: {', '.join(said[:-1])} or {said[-1]}")


class _Scope(NamedTuple):
    """What a question resolves once, before its one index call."""
    index: object
    table: _RowTable
    allowed: np.ndarray        # per directory group: the folder is one of (cam_name, timestamp)
    grouped: bool              # a live folder holds a truthy track id: answers are grouped per track (models/objects.py:378)
    bad: bool                  # a live folder holds a *.jpg name the reference raises on
    where: object              # the row filter, None: every row
    kw: dict                   # what carries the row filter to the index


def _competing(s: _Scope, ok=None) -> List[int]:
    """The rows of the live folders that pass the row filter (`ok`: a bool per row that stands in for it)"""
    ok = s.table.passing(s.where) if ok is None else ok
    return [r for r in range(len(s.table.paths)) if s.allowed[s.table.group[r]] and ok[r]]


def _raise_as_reference(table: _RowTable, rows) -> None:
    """Let the names among `rows` that the reference itself would raise on raise the same way"""
    for r in rows:
        fn = os.path.basename(table.paths[r])
        if "_" in fn:
            event_img_info(fn.split(".jpg")[0])


def _answers(table: _RowTable, rows, scores, *columns) -> list:
    """One query's rows (a list, -1 where the page ran out) and scores, as the index returns them -> [(path, score, *columns)]"""
    paths = table.paths
    if not columns:                                # the common page, kept to the plain comprehension: a hundred answers per call
        return [(paths[r], float(v)) for r, v in zip(rows, scores) if r >= 0]
    return [(paths[r], float(v), *rest) for r, v, *rest in zip(rows, scores, *columns) if r >= 0]


def _above(full, min_score) -> list:
    """A host-ranked list of (path, score) cut as the device cuts it"""
    return [r for r in full if min_score is None or not r[1] < min_score]


def _ts_or_none(t) -> Optional[int]:
    return None if t == _lib.ROW_NO_TS else int(t)


class ObjectFinder:
    """``models/objects.py:188-422``.  The face pipeline per crop as in the reference (`img_to_face`, `preprocess_face`) and
    for batches of crops (`faces_from_crops`, `embed_faces`, `index_faces`: two device passes, the same pixels)."""

    def __init__(self, base_path: str = "data/cameras"):
        self.base_path = base_path
        self.image_embeddings: Dict[str, np.ndarray] = {}
        self.face_embeddings: Dict[str, np.ndarray] = {}
        self.clip = False
        self.jit_cache: dict = {}
        self.model: Optional[OpenCLIP] = None
        # one device matrix + row table per source: "store" (attach_store), "image" / "face" (the reference's dicts).
        # They never share state: a face search cannot replace the attached crop matrix, and 512-d rows cannot enter it.
        self._dev: Dict[str, Tuple[EmbeddingIndex, _RowTable]] = {}
        self._dev_sig: Dict[str, tuple] = {}
        self._version = {"image": 0, "face": 0}
        self._stores: Dict[str, object] = {}
        self.index_storage = "f32"             # "bf16" halves the scan bytes, "i8" takes 9/8 byte per element (scores within ~1e-3 either way)
        self.alerts = AlertBook(768)           # text-described alerts per camera (set_alerts / check_alerts)
        self._watch: Optional[WatchList] = None
        self._watch_version = -1               # the AlertBook.version the device table was uploaded for

    def init_clip(self, **clip_kwargs):
        """:199-206 (warm-up included: the first call per shape builds and captures the hipGraph)."""
        if self.clip:
            return
        self.clip = True
        self.model = OpenCLIP(**clip_kwargs)
        s = self.model.arch.image_size
        for _ in range(2):
            self.model.precompute_embedding(np.random.rand(1, 3, s, s).astype(np.float32))

    def turn_off_clip(self):
        self.clip = False
        if self.model is not None:
            self.model.close()
        self.model = None

    # -- face models (:213-222): BlazeFace detector + AdaFace embedder on the same engine ------------------------
    def init_face(self, blazeface_kwargs: Optional[dict] = None, adaface_kwargs: Optional[dict] = None):
        """:213-217.  `self.blazeface(Tensor(img)).numpy()` -> (896,17) and `self.adaface(Tensor(face112)).numpy()` -> (1,512)
        are the reference's two face call surfaces (objects.py:254, clearcam.py:674,1236); `img_to_face` joins them."""
        if getattr(self, "face", False):
            return
        from .adaface import ADAFACE
        from .blazeface import BlazeFace
        self.blazeface = BlazeFace(**(blazeface_kwargs or {}))
        self.adaface = ADAFACE(**(adaface_kwargs or {}))
        self.face = True

    def turn_off_face(self):
        """:219-222"""
        for name in ("blazeface", "adaface"):
            m = getattr(self, name, None)
            if m is not None:
                m.close()
            setattr(self, name, None)
        self.face = False

    # -- face crop alignment (:243-354) ------------------------------------------------------------------------
    EYE_LEFT, EYE_RIGHT, FACE_SIZE = (38.0, 51.0), (73.0, 51.0), 112      # where the eyes land in the aligned face

    def img_to_face(self, orig):
        """RGB crop -> aligned 112x112 face (channel-swapped like the reference's final cvtColor) or None.  Steps as in the
        reference: letterbox to 640 and run BlazeFace; first surviving detection; reject faces narrower than 50 px; cut a
        square of twice the face size around the eyes' midpoint; rotate it so the eyes are level; scale and shift so they
        land on EYE_LEFT / EYE_RIGHT.  The pixel operations are clearcam_amd.cvops (GPU, OpenCV-compatible)."""
        from . import cvops
        full = np.ascontiguousarray(orig)
        h, w = full.shape[:2]
        scale = 640 / max(h, w)
        dev = self.blazeface.device                               # pixel ops on the GPU that runs the face models
        small = cvops.resize_linear(full, (int(w * scale), int(h * scale)), dev)
        gap_w, gap_h = 640 - small.shape[1], 640 - small.shape[0]
        top, left = gap_h // 2, gap_w // 2
        boxed = cvops.copy_make_border(small, top, gap_h - top, left, gap_w - left)
        found = self.blazeface(Tensor(boxed)).numpy()
        found = found[found[:, 0] != 0]
        if found.shape[0] == 0:
            return None
        g = self._face_geometry(found[0], h, w)
        if g is None:
            return None
        cut = full[g.cy1:g.cy1 + g.ch, g.cx1:g.cx1 + g.cw]
        level = cvops.warp_affine(cut, g.rot, (g.out_w, g.out_h), dev)
        face = cvops.warp_affine(level, g.place, (self.FACE_SIZE, self.FACE_SIZE), dev)
        return np.ascontiguousarray(face[:, :, ::-1])

    @classmethod
    def _face_geometry(cls, first, h: int, w: int) -> Optional[FaceGeometry]:
        """The arithmetic of `img_to_face` between the detector and the two warps, in float64 on the host, shared by the per-crop
        and the batched path so that both cut, rotate and place the same pixels.  first: the first surviving BlazeFace row
        (17 values in the coordinates of the 640 letterbox of an h x w crop).  None: face narrower than 50 px, or an empty cut."""
        scale = 640 / max(h, w)
        gap_w, gap_h = 640 - int(w * scale), 640 - int(h * scale)
        top, left = gap_h // 2, gap_w // 2
        offset = np.array([left, top])
        y1, x1, y2, x2 = ((float(first[0]) - top) / scale, (float(first[1]) - left) / scale,
                          (float(first[2]) - top) / scale, (float(first[3]) - left) / scale)
        eye_a = (np.array([first[4], first[5]]) - offset) / scale
        eye_b = (np.array([first[6], first[7]]) - offset) / scale
        if (x2 - x1) < 50:
            return None
        goal_a, goal_b = np.array(cls.EYE_LEFT), np.array(cls.EYE_RIGHT)
        mid = (eye_a + eye_b) / 2
        tilt = np.degrees(np.arctan2(eye_b[1] - eye_a[1], eye_b[0] - eye_a[0]))
        side = max(x2 - x1, y2 - y1) * 2.0
        H, W = h, w
        cx1, cy1 = max(0, int(mid[0] - side / 2)), max(0, int(mid[1] - side / 2))
        cx2, cy2 = min(W, int(mid[0] + side / 2)), min(H, int(mid[1] + side / 2))
        if cx2 <= cx1 or cy2 <= cy1:
            return None
        ch, cw = cy2 - cy1, cx2 - cx1
        corner = np.array([cx1, cy1])
        from .cvops import rotation_matrix_2d
        rot = rotation_matrix_2d((cw / 2, ch / 2), float(tilt), 1.0)
        c, s_ = abs(rot[0, 0]), abs(rot[0, 1])
        out_w, out_h = int(ch * s_ + cw * c), int(ch * c + cw * s_)
        rot[0, 2] += out_w / 2 - cw / 2
        rot[1, 2] += out_h / 2 - ch / 2
        a_rot = rot[:, :2] @ (eye_a - corner) + rot[:, 2]
        b_rot = rot[:, :2] @ (eye_b - corner) + rot[:, 2]
        zoom = np.linalg.norm(goal_b - goal_a) / np.linalg.norm(b_rot - a_rot)
        place = np.array([[zoom, 0, goal_a[0] - a_rot[0] * zoom], [0, zoom, goal_a[1] - a_rot[1] * zoom]], np.float32)
        return FaceGeometry(cx1, cy1, cw, ch, rot, out_w, out_h, place)

    # -- the same for a batch of crops: two device passes, one small download between them ---------------------------------
    FACE_CHUNK = 32                # crops per BlazeFace pass; tails are padded to a power of two: six plans at the most

    def _upload_crops(self, crops) -> "_PackedCrops":
        """Pack the crops as `preprocess_crops` does and upload them once; both passes read that buffer.  Three zero bytes behind the
        last crop are the blank 1 x 1 image that pads a tail chunk."""
        import torch
        packed, offsets, hs, ws = pack_crops(crops, tail=3)
        for i, (h, w) in enumerate(zip(hs.tolist(), ws.tolist())):
            scale = 640 / max(h, w)
            if int(h * scale) == 0 or int(w * scale) == 0:
                raise ValueError(f"crop {i} ({h} x {w}): a side of its 640 letterbox would be 0")
        dev = torch.device("cuda", self.blazeface.device)
        buf = torch.as_tensor(packed).to(dev)
        torch.cuda.current_stream(dev).synchronize()          # the library's own streams read the buffer: it has to be there
        return _PackedCrops(buf, int(packed.size), offsets, hs, ws)

    def _locate(self, pk: "_PackedCrops"):
        """-> (rows (B,17), found (B,), geometry per crop or None)"""
        B = len(pk.hs)
        rows, idx = np.zeros((B, 17), np.float32), np.full(B, -1, np.int32)
        L = _lib.lib()
        for lo in range(0, B, self.FACE_CHUNK):
            n = min(self.FACE_CHUNK, B - lo)
            nb = 1 << (n - 1).bit_length()                     # next power of two
            off = np.full(nb, pk.nbytes - 3, np.int64); off[:n] = pk.offsets[lo:lo + n]
            hs = np.ones(nb, np.int32); hs[:n] = pk.hs[lo:lo + n]
            ws = np.ones(nb, np.int32); ws[:n] = pk.ws[lo:lo + n]
            first, fidx = np.empty((nb, 17), np.float32), np.empty(nb, np.int32)
            _lib.check(L.cc_face_locate(self.blazeface._h, _lib.ptr(pk.buf), pk.nbytes, _lib.ptr(off), _lib.ptr(hs), _lib.ptr(ws), nb, 1,
                                        _lib.ptr(first), _lib.ptr(fidx), None))
            rows[lo:lo + n], idx[lo:lo + n] = first[:n], fidx[:n]
        geos = self._geometries(pk, rows, idx >= 0)
        return rows, np.array([g is not None for g in geos], bool), geos

    def _geometries(self, pk: "_PackedCrops", rows, found) -> List[Optional[FaceGeometry]]:
        rows, found = np.asarray(rows), np.asarray(found, bool)
        B = len(pk.hs)
        if rows.shape != (B, 17) or found.shape != (B,):
            raise ValueError(f"expected rows ({B},17) and found ({B},), got {rows.shape} and {found.shape}")
        geos: List[Optional[FaceGeometry]] = [None] * B
        for i in np.flatnonzero(found).tolist():
            g = geos[i] = self._face_geometry(rows[i], int(pk.hs[i]), int(pk.ws[i]))
            if g is not None and (g.out_w <= 0 or g.out_h <= 0):
                raise ValueError(f"crop {i}: empty destination size")         # what cvops.warp_affine says in img_to_face
        return geos

    def _align(self, pk: "_PackedCrops", geos, device_out: bool):
        import torch
        B = len(pk.hs)
        pos = [i for i in range(B) if geos[i] is not None]
        geo = [geos[i] for i in pos]
        dev = pk.buf.device
        faces = torch.empty((len(pos), self.FACE_SIZE, self.FACE_SIZE, 3), dtype=torch.uint8, device=dev)
        if pos:
            rec = (_lib.FaceAlignRec * len(pos))()
            for r, i, g in zip(rec, pos, geo):
                r.offset, r.h, r.w = int(pk.offsets[i]), int(pk.hs[i]), int(pk.ws[i])
                r.cx1, r.cy1, r.cw, r.ch, r.out_w, r.out_h = g.cx1, g.cy1, g.cw, g.ch, g.out_w, g.out_h
                r.rot[:] = np.asarray(g.rot, np.float64).reshape(-1).tolist()
                r.place[:] = np.asarray(g.place, np.float64).reshape(-1).tolist()
            _lib.check(_lib.lib().cc_face_align(_lib.ptr(pk.buf), pk.nbytes, 1, C.byref(rec), len(pos), _lib.ptr(faces), dev.index,
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if device_out:
            return faces, np.asarray(pos, np.int64)
        out: List[Optional[np.ndarray]] = [None] * B
        host = faces.cpu().numpy()
        for k, i in enumerate(pos):
            out[i] = host[k]
        return out

    def locate_faces(self, crops) -> Tuple[np.ndarray, np.ndarray]:
        """First pass of the batched `img_to_face`: every crop letterboxed to 640 on the GPU (ragged, one launch), BlazeFace over
        the batch, and per crop the first surviving detection -> (rows (B,17) float32, found (B,) bool).  rows[i] is the row
        `img_to_face` names `first` for crop i (zeros when nothing was detected); found[i] says that crop i yields a face: a
        detection that also passes `_face_geometry` (at least 50 px wide, a cut inside the crop)."""
        return self._locate(self._upload_crops(crops))[:2]

    def faces_from_rows(self, crops, rows, found, device_out: bool = False):
        """Second pass: `_face_geometry` per found row on the host, then cut, level and place every face in one launch (the
        levelled image is never written).  Returns a list with one (112,112,3) uint8 array or None per crop - bit for bit what
        `img_to_face` returns for that row - or, with device_out=True, a CUDA uint8 tensor (n,112,112,3) and the positions of
        its rows among the crops."""
        pk = self._upload_crops(crops)
        return self._align(pk, self._geometries(pk, rows, found), device_out)

    def faces_from_crops(self, crops, device_out: bool = False):
        """`img_to_face` for a batch: `locate_faces` then `faces_from_rows` over ONE upload of the packed crops."""
        pk = self._upload_crops(crops)
        return self._align(pk, self._locate(pk)[2], device_out)

    def embed_faces(self, crops) -> Tuple[np.ndarray, np.ndarray]:
        """Crops -> (emb (B,512) float32, valid (B,) bool): aligned faces stay on the GPU and go straight into AdaFace.  Rows of
        crops without a face are zero.  AdaFace runs on at most FACE_CHUNK faces at a time, in power-of-two pieces (a plan per
        batch size: six at the most)."""
        import torch
        faces, pos = self.faces_from_crops(crops, device_out=True)
        emb, valid = np.zeros((len(crops), 512), np.float32), np.zeros(len(crops), bool)
        n, lo, parts = int(faces.shape[0]), 0, []
        while lo < n:
            step = min(self.FACE_CHUNK, 1 << ((n - lo).bit_length() - 1))
            parts.append(self.adaface.embed_batch_device(faces[lo:lo + step]))
            lo += step
        if parts:
            emb[pos] = torch.cat(parts).cpu().numpy()
            valid[pos] = True
        return emb, valid

    def add_face_embeddings(self, paths, embs) -> None:
        """The face twin of `add_embedding`, what clearcam.py:1233-1241 does per crop: 512-d rows keyed by the crop paths, appended
        to the store of <cam>/faces/<day>/ (the crop's <cam>/objects/<day>/ folder with `objects` replaced), entered in
        `face_embeddings`, face version bumped (the next face search rebuilds its device matrix)."""
        from .store import EmbeddingStore
        paths = [str(p) for p in paths]
        e = np.asarray(as_numpy(embs), np.float32)
        if e.ndim == 0 or e.shape[-1] != 512:
            raise ValueError(f"expected 512-d face embeddings, got {e.shape}")
        e = e.reshape(-1, 512)
        if e.shape[0] != len(paths):
            raise ValueError(f"{len(paths)} paths for {e.shape[0]} rows")
        by_folder: Dict[str, List[int]] = {}
        for i, p in enumerate(paths):
            day = os.path.dirname(p)
            by_folder.setdefault(os.path.join(os.path.dirname(os.path.dirname(day)), "faces", os.path.basename(day)), []).append(i)
        for folder, rows in by_folder.items():
            st = self._stores.get(folder)
            if st is None:
                st = self._stores[folder] = EmbeddingStore(folder, 512)
            st.append([paths[i] for i in rows], e[rows])
        for i, p in enumerate(paths):
            self.face_embeddings[p] = e[i:i + 1].copy()
        if paths:
            self._version["face"] += 1

    def index_faces(self, paths, crops) -> np.ndarray:
        """Re-index person crops for face search: `embed_faces`, then `add_face_embeddings` for the crops that show a face.
        Returns valid (B,) bool."""
        paths = list(paths)
        if len(paths) != len(crops):
            raise ValueError(f"{len(paths)} paths for {len(crops)} crops")
        emb, valid = self.embed_faces(crops)
        keep = np.flatnonzero(valid).tolist()
        if keep:
            self.add_face_embeddings([paths[i] for i in keep], emb[keep])
        return valid

    def preprocess_face(self, img):
        """:232-241 for an already decoded RGB array: a 112x112x3 image is taken as is, anything else is aligned."""
        img = np.asarray(img)
        return img if img.shape == (112, 112, 3) else self.img_to_face(img)

    def preprocess(self, img):
        """:237-242 — cv2.resize(img,(224,224),INTER_CUBIC) -> f32/255 -> (x-0.5)/0.5 -> CHW, on the GPU
        (cc_crop_preprocess: OpenCV's 8-bit fixed-point cubic).  Returns (3,224,224) float32 like the reference."""
        return self.preprocess_crops([img]).cpu().numpy()[0]

    def preprocess_crops(self, crops, size: int = 224, device: Optional[int] = None):
        """Batch form of :237-242: list of (H,W,3) uint8 crops of any size -> device tensor (B,3,size,size) float32,
        the input `OpenCLIP.precompute_embedding_device` takes.  One H2D copy of the packed crops, one kernel."""
        return preprocess_crops(crops, size, self.model.device if (device is None and self.model) else (device or 0))

    # -- store ------------------------------------------------------------------------------------
    def _load_all_embeddings(self, face: bool = False):
        """:392-422 — merge every per-day embeddings.pkl under base_path, drop stale keys.  Folders written by
        `add_embedding` (append-only store files, clearcam_amd/store.py) are read as well, so the rows this class itself
        stored are not mistaken for stale keys."""
        from .store import EmbeddingStore
        valid, target = set(), (self.face_embeddings if face else self.image_embeddings)
        key = "face" if face else "image"
        files = []
        if os.path.isdir(self.base_path):
            for cam in os.listdir(self.base_path):
                objects = os.path.join(self.base_path, cam, "faces" if face else "objects")
                if not os.path.isdir(objects):
                    continue
                for day in os.listdir(objects):
                    for name in ("embeddings.pkl", "embeddings.idx", "embeddings.f32"):
                        f = os.path.join(objects, day, name)
                        if os.path.exists(f):
                            st_ = os.stat(f)
                            files.append((f, st_.st_mtime_ns, st_.st_size))
        sig = (tuple(sorted(files)), len(target))
        if getattr(self, "_files_sig", {}).get(key) == sig:
            return                                           # nothing on disk changed since the last reload: keep dict and device matrix
        for folder in sorted({os.path.dirname(f) for f, _, _ in files}):
            f = os.path.join(folder, "embeddings.pkl")
            if os.path.exists(f):
                with open(f, "rb") as fh:
                    emb = pickle.load(fh).get("embeddings", {})
                valid.update(emb.keys())
                target.update(emb)
            if os.path.exists(os.path.join(folder, "embeddings.idx")):
                st = EmbeddingStore(folder, 512 if face else 768)
                rows = st.rows()
                for i, p in enumerate(st.paths()):
                    valid.add(p)
                    target[p] = np.array(rows[i:i + 1])
        for k in set(target) - valid:
            del target[k]
        self._version[key] += 1
        if not hasattr(self, "_files_sig"):
            self._files_sig = {}
        self._files_sig[key] = (sig[0], len(target))

    # -- append-only store (clearcam_amd/store.py) instead of one pickle per folder ---------------------------
    def _new_index(self, dim: int, rows: int) -> EmbeddingIndex:
        return EmbeddingIndex(dim, max(2 * rows, 1024), device=self.model.device if self.model else 0, storage=self.index_storage)

    @staticmethod
    def _add_rows(index: EmbeddingIndex, table: "_RowTable", rows, paths) -> None:
        """Rows into the device matrix with their directory group and, where the index reduces per track, their track slot;
        where it keeps them, also the ts and the class of their names (the attached store and the dict-built indexes alike)."""
        groups = table.extend(paths)
        first = len(table.paths) - len(paths)
        if hasattr(index, "row_info"):             # the index keeps ts / class per row (row filters, timeline)
            ts, classes = table.attrs(first)
            index.add(rows, groups, table.slots(first), ts=ts, classes=classes)
        elif hasattr(index, "search_tracks"):
            index.add(rows, groups, table.slots(first))
        else:
            index.add(rows, groups)

    def _replace(self, key: str, index: EmbeddingIndex, table: "_RowTable"):
        old = self._dev.pop(key, None)
        if old is not None:
            old[0].close()
        self._dev[key] = (index, table)

    def attach_store(self, capacity: Optional[int] = None) -> int:
        """Load every stored crop under base_path (store files and/or the reference's pickles) straight into the device
        matrix: no per-crop dict entries, one H2D copy.  Subsequent `search` calls scan it; `add_embedding` appends (the
        matrix grows as needed).  Returns the number of rows."""
        from .store import load_all
        paths, rows = load_all(self.base_path, 768)
        index = EmbeddingIndex(768, max(capacity or 0, 2 * len(paths), 1024), device=self.model.device if self.model else 0,
                               storage=self.index_storage)
        table = _RowTable()
        if len(paths):
            self._add_rows(index, table, rows, list(paths))
        self._replace("store", index, table)
        self._attached = True
        return len(paths)

    def add_embedding(self, path: str, emb) -> None:
        """What clearcam.py:1282-1287 does per crop (load pickle, insert, rewrite pickle) as one appended row: on disk in
        the crop's day folder, in the dict the reference exposes, and in the attached device matrix."""
        from .store import EmbeddingStore
        e = np.asarray(as_numpy(emb), np.float32).reshape(1, -1)
        if e.shape[1] != 768:
            raise ValueError(f"expected a 768-d crop embedding, got {e.shape[1]}")
        folder = os.path.dirname(path)
        st = self._stores.get(folder)
        if st is None:
            st = self._stores[folder] = EmbeddingStore(folder, 768)
        st.append([path], e)
        self.image_embeddings[path] = e
        self._version["image"] += 1
        if getattr(self, "_attached", False):
            index, table = self._dev["store"]
            self._add_rows(index, table, e, [path])

    # -- text-described alerts at ingest (clearcam.py:1289-1307) ------------------------------------------------
    def set_alerts(self, cam_name: str, alerts) -> None:
        """Replace one camera's alerts: an ordered mapping id -> {"desc": str, "threshold": 0.28, "desc_emb": optional,
        "active": optional bool or callable, "last_det": optional}.  The mapping's order is the priority (the reference walks
        `alerts.items()`).  Descriptions without an embedding are encoded in ONE text batch (the reference encodes them one by
        one on first use, :1295-1297) and the embeddings are kept on the alert."""
        self.alerts.set_camera(cam_name, alerts)
        todo = self.alerts.missing()
        if todo:
            if self.model is None:
                raise RuntimeError("set_alerts needs init_clip() to encode descriptions given without desc_emb")
            tokens = np.concatenate([self.model.tokenizer.tokens_for_model(a.desc) for _, _, a in todo])
            for (_, _, a), e in zip(todo, self.model.encode_tokens(tokens)):
                a.desc_emb = np.array(e, np.float32)
            self.alerts._changed()

    def remove_alerts(self, cam_name: str) -> None:
        self.alerts.remove_camera(cam_name)

    def _watch_list(self) -> WatchList:
        """The device table of the alert book, uploaded when the book changed (once per change, not per crop)."""
        if self._watch is None:
            self._watch = WatchList(768, device=self.model.device if self.model else 0)
        if self._watch_version != self.alerts.version:
            self._watch.set(*self.alerts.table())
            self._watch_version = self.alerts.version
        return self._watch

    def check_alerts(self, paths, embs, now: Optional[float] = None) -> list:
        """The alert walk of clearcam.py:1289-1307 for a batch of crops in arrival order: `embs` (B,768), a host array or a
        CUDA torch tensor (what `precompute_embedding_device` left on the GPU), `paths` their crop paths (the camera is the
        component after `cameras`).  -> [(path, cam_name, alert id, desc, score)] for the crops that fired, in crop order;
        every fired alert gets `last_det = now` and is spent for the crops behind it.  One `WatchList.match` call: only the
        B (alert, score) pairs leave the GPU.  Notifying and exporting the clip stay the caller's."""
        paths = list(paths)
        if not paths or len(self.alerts) == 0:
            return []
        return self.alerts.check(self._watch_list().match, embs, paths, now)

    # -- retention: the NVR deletes day folders (clearcam.py:1347-1381, :574-578); the matrix has to forget their crops ------------
    def _forget_dirs(self, gone) -> int:
        """Drop every crop whose directory string satisfies `gone` from image_embeddings and from the attached matrix.
        Returns the crops dropped: rows of the attached matrix, or dict entries when no store is attached."""
        stale = [k for k in self.image_embeddings if gone(_RowTable.dir_of(k))]
        for k in stale:
            del self.image_embeddings[k]
        if stale:
            self._version["image"] += 1
        if not getattr(self, "_attached", False):
            return len(stale)
        index, table = self._dev["store"]
        drop = np.zeros(len(table.dirs), np.uint8)
        for g in range(1, len(table.dirs)):
            drop[g] = gone(table.dirs[g])
        group = np.asarray(table.group, np.int64)
        mask = drop[group] != 0 if group.size else np.zeros(0, bool)
        loose = [r for r in np.flatnonzero(group == 0).tolist() if gone(_RowTable.dir_of(table.paths[r]))]   # names that are no *.jpg
        if loose:                                     # group 0 mixes folders: these rows go by number
            mask[loose] = True
            n = index.remove(mask)
        elif drop.any():
            n = index.remove_groups(drop)             # flags from the group ids on the device: one call, no per-row upload
        else:
            return 0
        table.remove(mask)
        assert n == int(mask.sum()) and len(index) == len(table.paths)
        return n

    def forget(self, cam_name=None, timestamp=None) -> int:
        """Drop every crop whose directory contains `/cameras/<cam_name>/` and / or `/objects/<timestamp>/` (both given: both
        must match) from `image_embeddings` and, when a store is attached, from the device matrix, which is compacted in
        place.  Nothing is deleted on disk: that is the NVR's job (clearcam.py:1347-1381, :574-578).  Returns the number of
        crops dropped."""
        if not cam_name and not timestamp:
            raise ValueError("forget() needs cam_name and / or timestamp")

        def gone(d: str) -> bool:
            return (not cam_name or f"/cameras/{cam_name}/" in d) and (not timestamp or f"/objects/{timestamp}/" in d)
        return self._forget_dirs(gone)

    def sync_store(self) -> int:
        """The reference's stale-key rule (models/objects.py:414-415) for the attached matrix: drop the crops whose day folder
        no longer exists on disk, which is what `_cleanup_oldest_files` leaves behind.  Returns the rows dropped; 0 when no
        store is attached."""
        if not getattr(self, "_attached", False):
            return 0
        exists: Dict[str, bool] = {}

        def gone(d: str) -> bool:
            if d not in exists:
                exists[d] = os.path.isdir(d) if d else True
            return not exists[d]
        return self._forget_dirs(gone)

    def _device_index(self, embeddings: Dict[str, np.ndarray], key: str = "image") -> Tuple[EmbeddingIndex, "_RowTable"]:
        """(Re)build the HBM-resident matrix of one of the reference's dicts when it changed (the reference reloads before
        every search; `_load_all_embeddings` / `add_embedding` bump the version when they change anything)."""
        sig = (id(embeddings), len(embeddings), self._version[key])
        if key not in self._dev or self._dev_sig.get(key) != sig:
            paths = [p for p, e in embeddings.items() if e is not None]
            dim = int(np.asarray(embeddings[paths[0]]).size) if paths else (512 if key == "face" else 768)
            index, table = self._new_index(dim, len(paths)), _RowTable()
            if paths:
                self._add_rows(index, table, np.stack([np.asarray(embeddings[p], np.float32).reshape(-1) for p in paths]), paths)
            self._replace(key, index, table)
            self._dev_sig[key] = sig
        return self._dev[key]

    # -- search (:356-390) ------------------------------------------------------------------------------
    @staticmethod
    def _rank(table: "_RowTable", rows, scores, grouped: bool):
        """The tail of the reference's search (:378-390) over candidate rows given in ascending row order (= the dict's
        iteration order): best crop per track id, id-less crops appended, stable sort by score."""
        if grouped:
            best, loose = {}, []
            for r, sc in zip(rows, scores):
                oid = table.oid[r]
                if oid is not None:
                    if oid not in best or sc > best[oid][1]:
                        best[oid] = (table.paths[r], sc)
                else:
                    loose.append((table.paths[r], sc))
            results = list(best.values()) + loose
        else:
            results = [(table.paths[r], sc) for r, sc in zip(rows, scores)]
        results.sort(key=lambda x: x[1], reverse=True)
        return results

    def _is_attached(self, is_face) -> bool:
        return getattr(self, "_attached", False) and not is_face and len(self._dev["store"][1].paths) > 0

    def _has_rows(self, is_face) -> bool:
        return bool(self.face_embeddings if is_face else self.image_embeddings) or self._is_attached(is_face)

    def _index_and_table(self, is_face):
        """The device matrix a search runs on and its row table: the attached store, or the one built from the reference's dict."""
        if self._is_attached(is_face):
            return self._dev["store"]
        return self._device_index(self.face_embeddings if is_face else self.image_embeddings, "face" if is_face else "image")

    # -- the one path of the questions, in this order: argument checks that need no state (ValueError); nothing stored (the reference's
    # -- line, the empty answer); an index that cannot answer (RuntimeError); stored paths (KeyError) and vector widths (ValueError); no
    # -- live folder (the empty answer); folders with names that do not parse (fall back or raise, per question); the one index call.
    def _store(self, is_face, needs=(), cannot=None):
        """First step of a question's scope -> (index, table), or None when nothing is stored.  `needs`: the index methods the
        question cannot do without."""
        if not self._has_rows(is_face):
            print("No embeddings available.")
            return None
        index, table = self._index_and_table(is_face)
        for m in needs:
            if not hasattr(index, m):
                raise RuntimeError(cannot)
        return index, table

    @staticmethod
    def _scope(index, table: "_RowTable", cam_name, timestamp, where, kw, no_host_ranking=None) -> Optional[_Scope]:
        """Second step: the folders -> the scope, or None when no folder is live.  no_host_ranking: the name of a question that grows
        none, for which a live folder with names the reference raises on is an error."""
        allowed = table.allowed(cam_name, timestamp)
        live = np.flatnonzero(allowed)
        if live.size == 0:
            return None
        bad = [g for g in live if table.bad[g]]
        if bad and no_host_ranking:
            raise ValueError(f"{no_host_ranking} cannot rank the folder {table.dirs[bad[0]]}: it holds crop names that do not parse")
        return _Scope(index, table, allowed, any(table.truthy[g] for g in live), bool(bad), where, kw)

    def _vector(self, what: str, src, is_text: bool, index, is_face) -> np.ndarray:
        """A query text (encoded by the CLIP text tower), an embedding or an ndarray -> a flat float32 vector of the index's width
        (what=None: of whatever width, as a `Term`'s text always was)"""
        v = np.asarray(as_numpy(self.model._encode_text(src).numpy() if is_text else src), np.float32).reshape(-1)
        if what is not None and v.size != index.dim:
            raise ValueError(f"{what} has {v.size} dimensions, the {'face' if is_face else 'crop'} index {index.dim}")
        return v

    def _search_setup(self, query, cam_name, timestamp, text_embedding, is_face, ts_range, classes):
        """What `search`, `search_page` and `timeline` share: -> (q, scope) or None when there is nothing to search."""
        where, kw = _row_kw(ts_range, classes)
        store = self._store(is_face)
        if store is None:
            return None
        q = self._vector("query", query if text_embedding is None else text_embedding, text_embedding is None, store[0], is_face)
        s = self._scope(*store, cam_name, timestamp, where, kw)
        return None if s is None else (q, s)

    @staticmethod
    def _host_page(s: _Scope, full, min_score, distinct, depth, start, count):
        """The tail of a question ranked on the host, `full` its (path, score) list: cut, then sliced - or with `distinct` the page of
        its first `depth` answers thinned by their rows in the index."""
        kept = _above(full, min_score)
        if distinct is None:
            return kept[start:start + count], len(kept)
        if not hasattr(s.index, "distinct"):
            raise RuntimeError("this index cannot thin its answers")
        head = kept[:depth]
        if not head:
            return [], 0
        rows = np.array([s.table.row_of(p) for p, _ in head], np.int32)
        oi, os_, od, total = s.index.distinct(rows, np.array([v for _, v in head], np.float32), distinct, start, min(count, len(head)))
        return _answers(s.table, oi[0].tolist(), os_[0], od[0].tolist()), int(total[0])

    @staticmethod
    def _ranked_page(s: _Scope, method: str, ask, distinct, depth, start, count):
        """One page of a ranking by the index -> (results, total, what the index returned).  ask(fn, start, count, **more) makes the
        question's call of fn: the index's `method`, or with `distinct` its _device twin over the first `depth` answers, which are
        thinned where they are: only the page of the kept ones leaves the GPU."""
        rows = len(s.table.paths)
        if distinct is None:
            out = ask(getattr(s.index, method), start, min(count, rows))
            return _answers(s.table, out[0][0].tolist(), out[1][0]), int(out[2][0]), out
        out = ask(getattr(s.index, method + "_device"), 0, min(depth, rows), with_total=False)
        oi, os_, od, total = s.index.distinct_device(out[0], out[1], distinct, start, min(count, int(out[0].shape[-1])))
        return _answers(s.table, oi[0].cpu().tolist(), os_[0].cpu().numpy(), od[0].cpu().tolist()), int(total[0]), out

    def search_page(self, query=None, start=0, count=100, cam_name=None, timestamp=None, text_embedding=None, is_face=False, min_score=None,
                    ts_range=None, classes=None, distinct=None, distinct_depth=1024):
        """One page of the results, what the search endpoint computes (clearcam.py:1108-1118 + `send_results`, :686-705) by asking
        for top_k = start + count, cutting at the first score below 0.21 and slicing: -> (results, total) with
        results == [r for r in search(..., top_k=everything) if not r[1] < min_score][start:start+count] and total the length of
        that filtered list.  One `EmbeddingIndex.rank` call at any depth; only `count` (path, score) pairs leave the GPU.
        ts_range=(first, last) seconds into the day, inclusive, and classes=[ids] narrow the search to the crops whose name
        '<ts>_<track>_<class>.jpg' carries a ts inside the window / one of the classes (`EmbeddingIndex.row_filter`): the result is
        what `search` gives over those crops alone.  Whether answers are grouped per track is decided as without a row filter,
        from the track ids of ALL crops in the allowed folders, not only of the passing ones.
        distinct=<float>: near-duplicate answers are folded (`EmbeddingIndex.distinct`): the first min(distinct_depth, rows)
        answers of the ranking above are walked in order on the device and an answer whose stored embedding has a dot product
        >= distinct with one KEPT before it is dropped - one object under many track ids, days or cameras answers once.  The page
        is cut from the kept answers: -> ([(path, score, dups)], total), dups the answers folded into that one ("+12 similar") and
        total the kept answers among those first distinct_depth.  None: exactly the call without it."""
        start, count = _page_args("search_page", start, count)
        _cut_arg(min_score)
        distinct, distinct_depth = self._distinct_args(distinct, distinct_depth)
        setup = self._search_setup(query, cam_name, timestamp, text_embedding, is_face, ts_range, classes)
        if setup is None:
            return [], 0
        q, s = setup
        if s.bad or not hasattr(s.index, "rank"):
            # names the reference raises on (it raises here too), or an index that cannot rank: the whole list, cut on the host
            return self._host_page(s, self._search(q, s, len(s.table.paths)), min_score, distinct, distinct_depth, start, count)
        return self._ranked_page(s, "rank", lambda fn, at, n, **more: fn(q, at, n, s.allowed, min_score, tracks=s.grouped, **more, **s.kw),
                                 distinct, distinct_depth, start, count)[:2]

    @staticmethod
    def _distinct_args(distinct, distinct_depth):
        """The two arguments of a distinct page, checked before any GPU work -> (None or float, int)."""
        if distinct is None:
            return None, distinct_depth
        distinct = _cut_arg(float(distinct), "distinct")
        distinct_depth = int(distinct_depth)
        if not 1 <= distinct_depth <= _lib.DISTINCT_MAX_DEPTH:
            raise ValueError(f"distinct_depth must be in [1, {_lib.DISTINCT_MAX_DEPTH}]")
        return distinct, distinct_depth

    def _stored_row(self, table: "_RowTable", path: str) -> int:
        """The row of a stored crop named by its key, or by the endpoint's '/<cam>/objects/<day>/<file>' under base_path."""
        names = [path]
        if path.startswith("/"):
            names += [os.path.join(self.base_path, path.lstrip("/")), self.base_path.rstrip("/\\") + path]
        for name in names:
            if name in table.row:
                return table.row_of(name)
        raise KeyError(path)

    def similar(self, path, start=0, count=100, cam_name=None, timestamp=None, is_face=False, min_score=None, ts_range=None, classes=None,
                whole_track=False, exclude=None, distinct=None, distinct_depth=1024):
        """"More like this stored crop": what the search endpoint answers for `similar_img` (clearcam.py:1112-1114 -> `run_clip`,
        :671-675) -> (results, total) as `search_page` returns them.  The reference reads the jpg back, preprocesses and embeds it
        again; here the embedding is the row the index already holds, gathered on the device (`EmbeddingIndex.rank_like`): no file
        is read and no model runs.  `path`: the crop's stored key, or the endpoint's '/<cam>/objects/<day>/<file>' (joined to
        base_path); an unknown one raises KeyError.  Folders, cut, row filter and grouping per track are `search_page`'s.
        whole_track=True: the query is every crop of the clicked crop's track (same folder and track id; at most 64 of them,
        `pick_track_rows`), and a crop scores by its best match among them - a track seen from several sides finds what one crop
        of it would miss.  A crop without a track id stands alone.  exclude="rows": the query crops are not answers; "track":
        no crop of the clicked track is ("rows" for a crop without a track id).  distinct / distinct_depth: as in `search_page`,
        the answers then are (path, score, dups)."""
        where, kw = _row_kw(ts_range, classes)
        start, count = _page_args("similar", start, count)
        _cut_arg(min_score)
        distinct, distinct_depth = self._distinct_args(distinct, distinct_depth)
        _choice_arg("exclude", exclude, (None, "rows", "track"))
        store = self._store(is_face)
        if store is None:
            return [], 0
        index, table = store
        row = self._stored_row(table, path)
        if not hasattr(index, "rank_like"):                 # behind the lookup, where it always stood: an unknown path is a KeyError on any index
            raise RuntimeError("this index cannot be queried by its stored rows")
        group, slot = table.group[row], table.slot[row]

        def of_track():
            return (np.asarray(table.group) == group) & (np.asarray(table.slot) == slot)
        rows = np.array([row], np.int64)
        if slot < 0:
            exclude = "rows" if exclude == "track" else exclude
        elif whole_track:
            rows = pick_track_rows(row, np.flatnonzero(of_track()))
        s = self._scope(index, table, cam_name, timestamp, where, kw)
        if s is None:
            return [], 0
        if s.bad:
            # names the reference raises on: `search` with the clicked row's embedding raises the same way.  Where a row filter hides
            # those names from it, the answer is ranked on the host from the index's own scores.
            q = index.fetch(rows)
            full = self._search(self._vector("query", q[list(rows).index(row)], False, index, is_face), s, len(table.paths))
            if len(rows) > 1 or exclude:
                v = index.scores(q).max(axis=0)
                ok = table.passing(where)
                if exclude == "track":
                    ok &= ~of_track()
                elif exclude == "rows":
                    ok[rows] = False
                cand = _competing(s, ok)
                full = self._rank(table, cand, [float(v[r]) for r in cand], s.grouped)
            return self._host_page(s, full, min_score, distinct, distinct_depth, start, count)
        return self._ranked_page(s, "rank_like", lambda fn, at, n, **more: fn(rows, at, n, s.allowed, min_score, tracks=s.grouped, exclude=exclude,
                                                                             **more, **kw), distinct, distinct_depth, start, count)[:2]

    def _compound_setup(self, terms, combine, cam_name, timestamp, is_face, min_score, exclude, ts_range=None, classes=None):
        """What `compound` and `compound_timeline` share, everything checked before any GPU work -> (scope, the keyword arguments of
        `EmbeddingIndex.rank_terms` that say what is asked, row filter included, order) or None when there is nothing to search.  The index takes the
        vectors before the stored rows: order[t] is the position in `terms` of the index's term t."""
        where, kw = _row_kw(ts_range, classes)
        terms = [t if isinstance(t, Term) else Term(*t) for t in terms]
        if not 1 <= len(terms) <= _lib.TERMS_MAX:
            raise ValueError(f"compound needs 1 .. {_lib.TERMS_MAX} terms")
        for t in terms:
            if sum(x is not None for x in (t.text, t.path, t.embedding)) != 1:
                raise ValueError("a Term needs exactly one of text, path and embedding")
            if t.role not in EmbeddingIndex.TERM_ROLE:
                raise ValueError('a Term\'s role: "rank", "require" or "reject"')
            if t.role != "rank" and (t.cut is None or t.cut != t.cut):
                raise ValueError("a require / reject Term needs a cut")
        if not any(t.role == "rank" for t in terms):
            raise ValueError("compound needs at least one rank Term")
        _choice_arg("combine", combine, EmbeddingIndex.COMBINE)
        _choice_arg("exclude", exclude, (None, "rows", "track"))
        _cut_arg(min_score)
        store = self._store(is_face, ("rank_terms",), "this index cannot rank compound questions")
        if store is None:
            return None
        index, table = store
        vec_at = [i for i, t in enumerate(terms) if t.path is None]
        row_at = [i for i, t in enumerate(terms) if t.path is not None]
        rows = np.array([self._stored_row(table, terms[i].path) for i in row_at], np.int64)
        given = {i: self._vector("a Term's embedding", terms[i].embedding, False, index, is_face) for i in vec_at if terms[i].embedding is not None}
        s = self._scope(index, table, cam_name, timestamp, where, kw, no_host_ranking="compound search")
        if s is None:
            return None
        vecs = [given[i] if i in given else self._vector(None, terms[i].text, True, index, is_face) for i in vec_at]
        order = vec_at + row_at
        ranked = [int(r) for r, i in zip(rows, row_at) if terms[i].role == "rank"]
        if exclude == "track" and ranked and all(table.slot[r] < 0 for r in ranked):
            exclude = "rows"                        # crops without a track id stand alone, as in `similar`
        ask = dict(q=np.stack(vecs) if vecs else None, rows=rows if rows.size else None, roles=[terms[i].role for i in order],
                   weights=[terms[i].weight for i in order], cuts=[terms[i].cut for i in order], combine=combine, allowed=s.allowed,
                   min_score=min_score, tracks=s.grouped, exclude=exclude, **kw)
        return s, ask, order

    def compound(self, terms, start=0, count=100, combine="max", cam_name=None, timestamp=None, is_face=False, min_score=None, ts_range=None,
                 classes=None, exclude=None, explain=False, distinct=None, distinct_depth=1024):
        """One ranking for a question made of several terms -> (results, total) as `search_page` returns them.  `terms`: 1 .. 64
        `Term`s - texts, stored crops and embeddings, each with a role: "rank" terms make a crop's score (combine="max" / "min" of
        their scores, or "sum" of weight * score, where a negative weight means "less of this"), a "require" term must score the
        crop >= its cut ("person, AND it looks like this clicked crop"), a "reject" term must not ("white van, but not this one":
        the clicked van and every crop that looks like it leave the results).  Folders, cut, row filter and grouping per track are
        `search_page`'s; exclude="rows" / "track" is `similar`'s, for the stored crops that are rank terms; distinct /
        distinct_depth as in `search_page`.  explain=True appends to each result the position in `terms` of the term that made its
        score (max / min: the first one attaining it; sum: the one with the largest product).  An unknown path raises KeyError;
        a folder with crop names the reference raises on raises ValueError.  One `EmbeddingIndex.rank_terms` call: only `count`
        answers leave the GPU, no score matrix."""
        start, count = _page_args("compound", start, count)
        distinct, distinct_depth = self._distinct_args(distinct, distinct_depth)
        setup = self._compound_setup(terms, combine, cam_name, timestamp, is_face, min_score, exclude, ts_range, classes)
        if setup is None:
            return [], 0
        s, ask, order = setup
        res, total, out = self._ranked_page(s, "rank_terms", lambda fn, at, n, **more: fn(start=at, count=n, which=explain, **more, **ask),
                                            distinct, distinct_depth, start, count)
        if explain and distinct is None:
            res = [r + (order[w],) for r, w in zip(res, out[3][0].tolist())]
        elif explain:                               # a row answers once: the term of a kept answer is that of its row in the list walked
            term_of = dict(zip(out[0][0].cpu().tolist(), out[3][0].cpu().tolist()))
            res = [r + (order[term_of[s.table.row_of(r[0])]],) for r in res]
        return res, total

    def compound_timeline(self, terms, t0=0, bin_seconds=3600, n_bins=24, combine="max", cam_name=None, timestamp=None, is_face=False,
                          min_score=None, ts_range=None, classes=None, exclude=None):
        """How the results of `compound` (same terms and arguments) spread over the day -> (counts (n_bins,) int64, total), binned as
        `timeline` bins them; `total` is `compound`'s.  One `EmbeddingIndex.timeline_terms` call."""
        t0, bin_seconds, n_bins = _bin_args("compound_timeline", t0, bin_seconds, n_bins)
        setup = self._compound_setup(terms, combine, cam_name, timestamp, is_face, min_score, exclude, ts_range, classes)
        if setup is None:
            return np.zeros(n_bins, np.int64), 0
        s, ask, _ = setup
        c, total = s.index.timeline_terms(t0, bin_seconds, n_bins, **ask)
        return c[0], int(total[0])

    @staticmethod
    def _together_source(x):
        """What a side of `together` is given as -> "text", "path" or "embedding": a str that names a crop file ('*.jpg', a stored
        key or the endpoint's form) is a path, any other str a query text, everything else an embedding.  A `Term` names its one
        source itself."""
        if isinstance(x, Term):
            if sum(v is not None for v in (x.text, x.path, x.embedding)) != 1:
                raise ValueError("a side of together needs exactly one of text, path and embedding")
            return "text" if x.text is not None else "path" if x.path is not None else "embedding"
        if isinstance(x, str):
            return "path" if x.lower().endswith(".jpg") else "text"
        if x is None:
            raise ValueError("a side of together needs exactly one of text, path and embedding")
        return "embedding"

    def _together_setup(self, a, b, within, cam_name, timestamp, is_face, min_score, min_partner, value, partners, ts_range=None, classes=None,
                        with_classes=None):
        """What `together` and `together_timeline` share, everything checked before any GPU work -> (scope, the keyword arguments of
        `EmbeddingIndex.rank_near` that say what is asked, row filters included) or None when there is nothing to search."""
        where, kw = _row_kw(ts_range, classes)
        if row_filter(None, with_classes) is not None:
            kw["b_classes"] = with_classes
        kinds = [self._together_source(a), self._together_source(b)]
        _choice_arg("value", value, _lib.NEAR_VALUE)
        within, partners = int(within), int(partners)
        if not 0 <= within < 1 << 31:
            raise ValueError("within: seconds in [0, 2^31)")
        if not 1 <= partners <= _lib.NEAR_MAX_PARTNERS:
            raise ValueError(f"partners must be in [1, {_lib.NEAR_MAX_PARTNERS}]")
        for cut in (min_score, min_partner):
            _cut_arg(cut, "min_score / min_partner")
        store = self._store(is_face, ("rank_near",), "this index cannot join two questions")
        if store is None:
            return None
        index, table = store
        sides = []
        for x, kind in zip((a, b), kinds):
            src = getattr(x, kind) if isinstance(x, Term) else x
            sides.append(self._stored_row(table, src) if kind == "path" else self._vector("a side of together", src, kind == "text", index, is_face))
        s = self._scope(index, table, cam_name, timestamp, where, kw, no_host_ranking="together")
        if s is None:
            return None
        return s, dict(a=sides[0], b=sides[1], within=within, partners=partners, cut_b=min_partner, value=value, allowed=s.allowed, min_score=min_score,
                       tracks=s.grouped, **kw)

    def together(self, a, b, within=30, start=0, count=100, cam_name=None, timestamp=None, is_face=False, min_score=0.21, min_partner=0.21, value="min",
                 ts_range=None, classes=None, with_classes=None, partners=_lib.NEAR_DEFAULT_PARTNERS):
        """Two objects at once: the crops that answer `a` while something that answers `b` is seen within `within` seconds in the
        same folder ("a person while a white van is at the gate") -> ([(path, score, partner_path, partner_score, dt_seconds)],
        {"total", "partners", "partners_left"}).  `a` / `b`: a query string, a stored crop's path (its key or the endpoint's form; a
        string ending in .jpg) or an embedding - or a `Term` naming exactly one of text / path / embedding - resolved as `compound`
        resolves its terms; an unknown path raises KeyError.  The partners are the best `partners` crops for `b` scoring >=
        min_partner (with_classes: only crops of those classes) that have a time; a crop's partner is the best of them near it that is
        neither the crop nor a crop of its own track, dt_seconds the partner's time minus the crop's.  value="min": a result scores
        the smaller of its own score for `a` and its partner's for `b`; "a": its own alone.  Folders, min_score, ts_range / classes
        (for `a`) and grouping per track are `search_page`'s.  "partners": the crops that qualified as partners, "partners_left":
        those beyond the cap, which took no part.  One `EmbeddingIndex.rank_near` call: only the page leaves the GPU."""
        start, count = _page_args("together", start, count)
        setup = self._together_setup(a, b, within, cam_name, timestamp, is_face, min_score, min_partner, value, partners, ts_range, classes, with_classes)
        if setup is None:
            return [], {"total": 0, "partners": 0, "partners_left": 0}
        s, ask = setup
        table = s.table
        idx, sc, total, pr, ps, n_partners = s.index.rank_near(start=start, count=min(count, len(table.paths)), **ask)
        res = [(table.paths[r], float(v), table.paths[p], float(w), int(table.ts[p]) - int(table.ts[r]))
               for r, v, p, w in zip(idx[0].tolist(), sc[0], pr[0].tolist(), ps[0]) if r >= 0]
        return res, {"total": int(total[0]), "partners": min(n_partners, ask["partners"]), "partners_left": max(n_partners - ask["partners"], 0)}

    def together_timeline(self, a, b, within=30, t0=0, bin_seconds=3600, n_bins=24, cam_name=None, timestamp=None, is_face=False, min_score=0.21,
                          min_partner=0.21, value="min", ts_range=None, classes=None, with_classes=None, partners=_lib.NEAR_DEFAULT_PARTNERS):
        """How the results of `together` (same question) spread over the day -> (counts (n_bins,) int64, total), binned as `timeline`
        bins them; `total` is `together`'s.  One `EmbeddingIndex.timeline_near` call."""
        t0, bin_seconds, n_bins = _bin_args("together_timeline", t0, bin_seconds, n_bins)
        setup = self._together_setup(a, b, within, cam_name, timestamp, is_face, min_score, min_partner, value, partners, ts_range, classes, with_classes)
        if setup is None:
            return np.zeros(n_bins, np.int64), 0
        s, ask = setup
        c, total, _ = s.index.timeline_near(t0=t0, bin_seconds=bin_seconds, n_bins=n_bins, **ask)
        return c[0], int(total[0])

    def search(self, query=None, top_k=10, cam_name=None, timestamp=None, text_embedding=None, is_face=False, ts_range=None, classes=None):
        """:356-390.  ts_range / classes: the row filter of `search_page`; with one given the device ranks (`EmbeddingIndex.rank`),
        and grouping per track is decided as without it, from the track ids of all crops in the allowed folders."""
        setup = self._search_setup(query, cam_name, timestamp, text_embedding, is_face, ts_range, classes)
        return [] if setup is None or top_k <= 0 else self._search(*setup, top_k)

    def _search(self, q, s: _Scope, top_k):
        """`search` inside a scope; with top_k = every row, the whole list for the questions that fall back to ranking on the host"""
        index, table, allowed, grouped, exact_loop, where, kw = s.index, s.table, s.allowed, s.grouped, s.bad, s.where, s.kw
        if where is None and grouped and not exact_loop and top_k <= 1024 and hasattr(index, "search_tracks"):
            # the device reduces per track id and selects (one call, exact whatever the data: thousands of crops of one track, ties)
            idx, sc = index.search_tracks(q, int(top_k), allowed)
            return _answers(table, idx[0].tolist(), sc[0])
        if not exact_loop and hasattr(index, "rank"):
            # top_k > 1024, or no truthy track id among the allowed crops (the reference does not group then): the device ranks the
            # whole order and hands back its head.  At most one answer per row: "everything" (top_k = 10**9) allocates no more.
            idx, sc, _ = index.rank(q, 0, min(int(top_k), len(table.paths)), allowed, None, tracks=grouped, **kw)
            return _answers(table, idx[0].tolist(), sc[0])
        # An index without `rank` (no track ids among the allowed rows, top_k > 1024 or no search_tracks either):
        # GPU: filtered top-K' (one HBM pass + radix select); host: the reference's best-per-track-id tail on K' rows.
        # The answer is exact once the top_k-th result scores strictly above the weakest candidate (no unseen row can
        # enter or change it) or every allowed row has been seen; otherwise K' grows, and past 1024 the full score vector
        # is ranked (many crops of few tracks above everything else: rare).
        kk = min(1024, max(128, 16 * int(top_k)))
        while not exact_loop and where is None:             # a row filter the index cannot apply: the full score vector below
            idx, sc = index.search(q, kk, allowed)
            keep = idx[0] >= 0
            rows, scs = idx[0][keep], sc[0][keep]
            order = np.argsort(rows, kind="stable")
            results = self._rank(table, rows[order].tolist(), [float(v) for v in scs[order]], grouped)
            if rows.size < kk:                              # every allowed row was a candidate: this IS the reference's loop
                return results[:top_k]
            if len(results) >= top_k and results[top_k - 1][1] > float(scs.min()):
                # Bit-equal scores among the answers (duplicate crops): the reference orders them by the first appearance of their
                # track id over ALL rows (dict order + stable sort), which a candidate list cannot know - rank the whole vector then.
                head = [sc_ for _, sc_ in results[:top_k + 1]]
                if len(set(head)) == len(head):
                    return results[:top_k]
                break
            if kk == 1024:
                break
            kk = min(1024, kk * 4)
        scores = index.scores(q)[0]                         # the whole score vector, ranked like the reference does it
        rows = _competing(s)
        if exact_loop:                                      # names the reference itself would raise on: let it raise the same way
            _raise_as_reference(table, rows)
        return self._rank(table, rows, [float(scores[r]) for r in rows], grouped)[:top_k]

    def timeline(self, query=None, t0=0, bin_seconds=3600, n_bins=24, cam_name=None, timestamp=None, text_embedding=None, is_face=False,
                 min_score=0.21, ts_range=None, classes=None):
        """How the hits of a query spread over the day -> (counts (n_bins,) int64, total): the results `search_page` would page
        through (same folders, cut and row filter; grouped per track as `search_page` decides it), counted by the ts of each
        result's crop into bin (ts - t0) // bin_seconds.  A result whose name carries no ts, or whose bin lies outside
        [0, n_bins), is counted in `total` only; `total` is `search_page`'s.  One `EmbeddingIndex.timeline` call: n_bins counters
        leave the GPU, no scores."""
        t0, bin_seconds, n_bins = _bin_args("timeline", t0, bin_seconds, n_bins)
        _cut_arg(min_score)
        counts = np.zeros(n_bins, np.int64)
        setup = self._search_setup(query, cam_name, timestamp, text_embedding, is_face, ts_range, classes)
        if setup is None:
            return counts, 0
        q, s = setup
        if s.bad or not hasattr(s.index, "timeline"):
            kept = _above(self._search(q, s, len(s.table.paths)), min_score)
            for path, _ in kept:
                ts = _RowTable.name_attrs(path)[0]
                if ts != _lib.ROW_NO_TS and 0 <= (ts - t0) // bin_seconds < n_bins:
                    counts[(ts - t0) // bin_seconds] += 1
            return counts, len(kept)
        c, total = s.index.timeline(q, t0, bin_seconds, n_bins, s.allowed, min_score, tracks=s.grouped, **s.kw)
        return c[0], int(total[0])

    def _digest_setup(self, name, needs, orders, cam_name, timestamp, is_face, same_at, start, count, ts_range, classes, by):
        """What `digest` and `seen_before` share -> (scope or None when there is nothing to walk, same_at, start, count).  Names the
        reference raises on raise the same way, as `search` lets them, where they are among the crops that compete."""
        where, kw = _row_kw(ts_range, classes)
        start, count = _page_args(name, start, count)
        same_at = _cut_arg(float(same_at), "same_at")
        _choice_arg("by", by, orders)
        store = self._store(is_face, needs, "this index cannot summarise its rows")
        s = None if store is None else self._scope(*store, cam_name, timestamp, where, kw)
        if s is not None and s.bad:
            _raise_as_reference(s.table, _competing(s))
        return s, same_at, start, count

    def digest(self, cam_name=None, timestamp=None, is_face=False, same_at=0.9, start=0, count=100, ts_range=None, classes=None, by="count"):
        """"What was on this camera today?": every distinct object among the stored crops of the allowed folders once ->
        ([(path, count, ts_first, ts_last)], {"objects", "crops", "left_over"}).  The reference shows a day's `objects/` folder crop
        by crop, up to 20 crops per track plus one every 10 s for as long as it lives: a parked car owns a tenth of the day.  Here
        the crops are walked in stored order on the device (`EmbeddingIndex.digest`): a crop joins the first object whose first
        crop is at least same_at similar to it, and an entry is that first crop's path, how many crops joined it and the first /
        last ts among their names (None: no name carries one).  by="count": the most seen first; "first": in order of appearance.
        Folders and row filter are `search_page`'s; no query, no model.  "objects" is the number of entries there are (at most
        1024 in one call), "crops" the crops that competed, "left_over" those that matched none of 1024 objects.  A *.jpg name the
        reference cannot parse raises ValueError where `search` would raise on it: among the crops that compete."""
        s, same_at, start, count = self._digest_setup("digest", ("digest",), EmbeddingIndex.DIGEST_BY, cam_name, timestamp, is_face, same_at, start, count,
                                                      ts_range, classes, by)
        if s is None:
            return [], {"objects": 0, "crops": 0, "left_over": 0}
        rows, counts, t0, t1, totals = s.index.digest(same_at, start, min(count, _lib.DIGEST_MAX_LEADERS), s.allowed, by=by, **s.kw)
        out = [(s.table.paths[r], int(c), _ts_or_none(a), _ts_or_none(b))
               for r, c, a, b in zip(rows.tolist(), counts.tolist(), t0.tolist(), t1.tolist()) if r >= 0]
        return out, {"objects": int(totals[0]), "crops": int(totals[1]), "left_over": int(totals[2])}

    SEEN_BY = ("new", "count", "first")

    @staticmethod
    def _dir_cam_day(d: str):
        """(camera, day) of a directory group '.../cameras/<cam>/objects/<day>/'; None where the part is missing."""
        def part(key):
            i = d.find(key)
            if i < 0:
                return None
            j = d.find("/", i + len(key))
            return d[i + len(key):j] if j >= 0 else None
        return part("/cameras/"), part("/objects/")

    def seen_before(self, cam_name=None, timestamp=None, is_face=False, same_at=0.9, start=0, count=100, ts_range=None, classes=None,
                    history_cam=None, by="new"):
        """"Which of today's objects have we seen before, and which are new?" -> ([(path, count_today, ts_first, ts_last, seen_before,
        days, cams, last_day, best_path, best_score)], {"objects", "new", "crops", "left_over", "history_crops"}).  The objects are
        `digest`'s of (cam_name, timestamp) in order of first appearance, up to 1024 (same folders, row filter, validation and
        behaviour on unparsable names).  The history is every folder `history_cam` allows (None: all cameras) that the digest did not
        take, filtered by `classes` (ts_range is seconds into today and does not apply).  One `EmbeddingIndex.sightings` call scores
        all objects against the whole history on the device: seen_before = the history crops at least same_at similar to the
        object's first crop, days = the distinct <day> folders among them, cams = their cameras (sorted), last_day = the largest such
        day string or None, best_path / best_score = the closest history crop whether it matches or not (None / None without
        history).  by="new": objects never seen before first, then most crops today, then order of appearance; "count" / "first":
        `digest`'s orders.  Entries start .. start+count-1 come back.  "new" counts the objects with seen_before == 0,
        "history_crops" the history crops that competed."""
        s, same_at, start, count = self._digest_setup("seen_before", ("digest", "sightings"), self.SEEN_BY, cam_name, timestamp, is_face, same_at, start,
                                                      count, ts_range, classes, by)
        if s is None:
            return [], {"objects": 0, "new": 0, "crops": 0, "left_over": 0, "history_crops": 0}
        index, table, allowed = s.index, s.table, s.allowed
        rows, counts, t0, t1, totals = index.digest(same_at, 0, _lib.DIGEST_MAX_LEADERS, allowed, by="first", **s.kw)
        lead = [r for r in rows.tolist() if r >= 0]
        n = len(lead)
        history = (np.asarray(table.allowed(history_cam, None)) != 0) & (np.asarray(allowed) == 0)
        seen = np.zeros(n, np.int64)
        best_row, best_score = np.full(n, -1, np.int64), np.full(n, -np.inf, np.float32)
        groups = np.zeros((n, len(table.dirs)), np.int64)
        history_crops = 0
        if n and history.any():
            seen, best_row, best_score, groups, history_crops = index.sightings(lead, same_at, history.astype(np.uint8), classes=classes,
                                                                                group_counts=len(table.dirs))
        where_of = [self._dir_cam_day(d) for d in table.dirs]
        entries = []
        for i, r in enumerate(lead):
            hit = [where_of[g] for g in np.flatnonzero(np.asarray(groups[i])).tolist()]
            days = {d for _, d in hit if d is not None}
            b = int(best_row[i])
            entries.append((table.paths[r], int(counts[i]), _ts_or_none(t0[i]), _ts_or_none(t1[i]),
                            int(seen[i]), len(days), sorted({c for c, _ in hit if c is not None}), max(days) if days else None,
                            table.paths[b] if b >= 0 else None, float(best_score[i]) if b >= 0 else None))
        order = list(range(n))                                                # by="first": the digest's own order
        if by == "count":
            order.sort(key=lambda i: (-entries[i][1], lead[i]))
        elif by == "new":
            order.sort(key=lambda i: (entries[i][4] != 0, -entries[i][1], lead[i]))
        info = {"objects": int(totals[0]), "new": sum(1 for e in entries if e[4] == 0), "crops": int(totals[1]), "left_over": int(totals[2]),
                "history_crops": int(history_crops)}
        return [entries[i] for i in order[start:start + count]], info
