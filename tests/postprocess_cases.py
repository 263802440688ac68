"""References and crafted inputs of tests/test_gpu_postprocess.py, checked on the CPU by tests/test_postprocess_host.py (helper module;
not a conftest).  Everything here is NumPy / PyTorch-CPU.

Continuous stages (DDetect decode and the two 1x1 convs in front of it): plain float64 restatements.  The same code evaluated in float32
(`dtype=np.float32`) is the round-off floor a kernel's error is judged against.
Discrete stages (top-k, NMS, scale_boxes; BlazeFace's sort, overlap rule and back-map): the oracle's own float32 code, fed rows whose
arithmetic is EXACT in float32 - small integer coordinates for the detector, dyadic rationals for BlazeFace - so that a correct kernel
matches it bit for bit and every case can state which branch of the kernel it reaches.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from oracle import yolov9_oracle as yo
from oracle.blazeface_oracle import BlazeFaceOracle

STRIDES = (8.0, 16.0, 32.0)
CONF = 0.25
MAX_DET = 300


def split_value(w: torch.Tensor) -> torch.Tensor:
    """The value the two f16 planes of the "f16s" mode hold for a weight tensor (yolo.hip pack_convs): w 2^e = hi + lo with 2^e
    putting the largest magnitude in [2^14, 2^15)."""
    e = 14 - int(np.floor(np.log2(float(w.abs().max()))))
    ws = w * (2.0 ** e)
    hi = ws.to(torch.float16).float()
    lo = (ws - hi).to(torch.float16).float()
    return (hi + lo) * (2.0 ** -e)


# ---------------------------------------------------------------------------------------------------------------------------------
# DDetect decode (detection/yolov9.py:209-220, 263-282, 440-448) in NumPy
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Decoded:
    box: np.ndarray        # (B,A,4) x1,y1,x2,y2
    score: np.ndarray      # (B,A) best class score, NOT thresholded
    cls: np.ndarray        # (B,A) first index of the maximum
    gap: np.ndarray        # (B,A) best score minus second best


def decode_np(raws: Sequence[np.ndarray], dfl_w: np.ndarray, dtype=np.float64) -> Decoded:
    """raws: per level (B,H,W,144) logits [4 sides x 16 bins | 80 classes].  DFL softmax-expectation, dist2bbox, * stride, sigmoid, class
    max with first-index ties, all in `dtype`."""
    w = dfl_w.astype(dtype)
    boxes, scores, clss, gaps = [], [], [], []
    for raw, stride in zip(raws, STRIDES):
        r = raw.astype(dtype)
        B, H, W, _ = r.shape
        bins = r[..., :64].reshape(B, H * W, 4, 16)
        e = np.exp(bins - bins.max(-1, keepdims=True))
        d = ((e / e.sum(-1, keepdims=True)) * w).sum(-1)                      # (B,HW,4) left, top, right, bottom
        a = np.arange(H * W)
        ax, ay = ((a % W) + 0.5).astype(dtype), ((a // W) + 0.5).astype(dtype)
        lx, ly, rx, ry = ax - d[..., 0], ay - d[..., 1], ax + d[..., 2], ay + d[..., 3]
        cx, cy, bw, bh = (lx + rx) / 2 * dtype(stride), (ly + ry) / 2 * dtype(stride), (rx - lx) * dtype(stride), (ry - ly) * dtype(stride)
        boxes.append(np.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), -1))
        sg = 1 / (1 + np.exp(-r[..., 64:].reshape(B, H * W, 80)))
        top = np.sort(sg, -1)
        scores.append(top[..., -1]); gaps.append(top[..., -1] - top[..., -2]); clss.append(sg.argmax(-1))
    return Decoded(np.concatenate(boxes, 1), np.concatenate(scores, 1), np.concatenate(clss, 1), np.concatenate(gaps, 1))


def rows_of(d: Decoded, conf: float = CONF) -> np.ndarray:
    """(B,A,6) rows as decode_kernel writes them."""
    s = np.where(d.score >= conf, d.score, 0.0)
    return np.concatenate((d.box, s[..., None], d.cls[..., None].astype(d.box.dtype)), -1)


def level_offsets(levels) -> List[int]:
    off, out = 0, []
    for h, w in levels:
        out.append(off); off += h * w
    return out + [off]


# ---------------------------------------------------------------------------------------------------------------------------------
# decode_kernel case
# ---------------------------------------------------------------------------------------------------------------------------------
DECODE_LEVELS = ((12, 20), (6, 10), (3, 5))      # 315 anchors x 3 images = 945 threads: the fourth 256-thread block is ragged; W != H tells a % W from a / W
DECODE_B = 3
TIE_CLASSES = ((7, 42), (0, 79), (3, 4))          # pairs in different float4 groups of the class scan: the lower index must win


@dataclass
class DecodeCase:
    raws: List[np.ndarray]
    dfl_w: np.ndarray
    planted: Dict[str, Tuple[int, int]] = field(default_factory=dict)     # edge name -> (image, anchor)


def decode_case(seed: int = 0) -> DecodeCase:
    """Box logits ~ N(0,3), class logits ~ N(-3.6,1) (about half the anchors clear 0.25), DFL weights uniform in [0,15].  Planted at each
    level's first and last cell, in rotating images: a side with 16 equal bins, a side saturated on one bin (+80 against -80) and the
    reverse, and anchors whose two best classes carry the identical logit."""
    rng = np.random.default_rng(seed)
    raws = []
    for h, w in DECODE_LEVELS:
        r = np.empty((DECODE_B, h, w, 144), np.float32)
        r[..., :64] = rng.normal(0, 3, (DECODE_B, h, w, 64))
        r[..., 64:] = rng.normal(-3.6, 1, (DECODE_B, h, w, 80))
        raws.append(r)
    case = DecodeCase(raws, rng.uniform(0, 15, 16).astype(np.float32))
    off = level_offsets(DECODE_LEVELS)

    def cell(l, last):
        h, w = DECODE_LEVELS[l]
        return raws[l].reshape(DECODE_B, h * w, 144), (h * w - 1 if last else 0)

    def plant(name, l, last, b, fn):
        flat, a = cell(l, last)
        fn(flat[b, a])
        flat[b, a, 64 + 11] = 2.0                                             # the anchor clears the threshold: its score is compared
        case.planted[name] = (b, off[l] + a)

    def uniform(v): v[16:32] = 1.5
    def one_hot(v): v[32:48] = -80.0; v[32 + 11] = 80.0
    def one_cold(v): v[0:16] = 80.0; v[5] = -80.0

    def tie(pair):
        def f(v): v[64 + pair[0]] = 3.0; v[64 + pair[1]] = 3.0
        return f
    plant("uniform_side", 0, False, 0, uniform)
    plant("saturated_side", 0, True, 1, one_hot)
    plant("inverse_saturated_side", 1, False, 2, one_cold)
    plant("tie_7_42", 1, True, 0, tie(TIE_CLASSES[0]))
    plant("tie_0_79", 2, False, 1, tie(TIE_CLASSES[1]))
    plant("tie_3_4", 2, True, 2, tie(TIE_CLASSES[2]))
    plant("saturated_side_l2", 2, True, 0, one_hot)
    plant("uniform_side_l1", 1, False, 1, uniform)
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# head_tail_kernel case: the two 1x1 convs in front of the decode
# ---------------------------------------------------------------------------------------------------------------------------------
TAIL_LEVELS_MAIN = ((20, 12), (10, 6), (5, 3))   # B = 3: M = 720 / 180 / 45 - second block of level 0 ends in a ragged 64-pixel tile (720 = 512 + 3 * 64 + 16),
TAIL_B_MAIN = 3                                  # level 2 in a ragged 16-pixel fragment (45 = 2 * 16 + 13); blk1 = 2, blk2 = 3
TAIL_LEVELS_SMALL = ((8, 8), (4, 4), (2, 2))
TAIL_B_SMALL = 1
TIE_PAIR = (5, 58)                               # class 5: fragment 0, lane group 1; class 58: fragment 3, lane group 2
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f16s": torch.float16}


@dataclass
class TailCase:
    levels: Tuple[Tuple[int, int], ...]
    B: int
    ch: int
    bx: List[np.ndarray]       # per level (B,H,W,64) float32, values the storage type holds
    cl: List[np.ndarray]       # per level (B,H,W,ch)
    w2: List[np.ndarray]       # (64,16,1,1) float32 as handed to the entry (not rounded)
    b2: List[np.ndarray]
    w3: List[np.ndarray]       # (80,ch,1,1)
    b3: List[np.ndarray]
    dfl_w: np.ndarray


# (ch, small) -> seed whose float64 reference has at most 1 % of the anchors with a top-two gap inside (0, 1e-4), no score within 1e-5 of
# the threshold and the tied pair on top somewhere (searched upwards from 0; tests/test_postprocess_host.py holds them to it)
TAIL_SEEDS = {(128, False): 0, (128, True): 1, (256, False): 3, (256, True): 4}


def tail_case(dtype: str, ch: int, small: bool = False, seed: int = None) -> TailCase:
    """Activations ~ N(0,1) rounded to the storage type, weights scaled so that the logits have a standard deviation of about 2.  Class
    rows TIE_PAIR are identical (weights and bias), their bias raised by 2.5 so that they are the maximum on a share of the pixels."""
    levels, B = (TAIL_LEVELS_SMALL, TAIL_B_SMALL) if small else (TAIL_LEVELS_MAIN, TAIL_B_MAIN)
    seed = TAIL_SEEDS[(ch, small)] if seed is None else seed
    rng = np.random.default_rng(seed + ch + (1000 if small else 0))
    t = TORCH_DT[dtype]
    q = lambda a: torch.from_numpy(a.astype(np.float32)).to(t).float().numpy()       # noqa: E731
    c = TailCase(levels, B, ch, [], [], [], [], [], [], rng.uniform(0, 15, 16).astype(np.float32))
    for h, w in levels:
        c.bx.append(q(rng.normal(0, 1, (B, h, w, 64))))
        c.cl.append(q(rng.normal(0, 1, (B, h, w, ch))))
        c.w2.append((rng.normal(0, 1, (64, 16, 1, 1)) * 2 / 4).astype(np.float32))
        c.b2.append(rng.normal(0, 0.5, 64).astype(np.float32))
        w3 = (rng.normal(0, 1, (80, ch, 1, 1)) * 2 / ch ** 0.5).astype(np.float32)
        b3 = rng.normal(0, 0.5, 80).astype(np.float32)
        b3[TIE_PAIR[0]] = 2.5
        w3[TIE_PAIR[1]] = w3[TIE_PAIR[0]]; b3[TIE_PAIR[1]] = b3[TIE_PAIR[0]]
        c.w3.append(w3); c.b3.append(b3)
    return c


def kernel_weights(dtype: str, w: np.ndarray) -> np.ndarray:
    """The value the kernel multiplies by for OIHW float32 weights `w`: the controlled rounding of the plain 16-bit modes
    (cc_round_weights: host code of the library), the sum of the two planes for "f16s"."""
    if dtype == "f16s":
        return split_value(torch.from_numpy(w)).numpy()
    from clearcam_amd import _lib
    out = np.empty_like(w)
    co, ci, k = w.shape[0], w.shape[1], w.shape[2]
    _lib.check(_lib.lib().cc_round_weights({"f16": 1, "bf16": 2}[dtype], _lib.ptr(np.ascontiguousarray(w)), co, ci, k, _lib.ptr(out)))
    return out


def tail_logits(c: TailCase, dtype: str, np_dtype=np.float64) -> List[np.ndarray]:
    """Per level (B,H,W,144): cv2[l][2] (four groups of 16 -> 16) and cv3[l][2] over the stored activations, in `np_dtype`."""
    out = []
    for l in range(3):
        w2 = kernel_weights(dtype, c.w2[l]).reshape(4, 16, 16).astype(np_dtype)          # (group, out, in)
        w3 = kernel_weights(dtype, c.w3[l]).reshape(80, c.ch).astype(np_dtype)
        bx = c.bx[l].astype(np_dtype).reshape(*c.bx[l].shape[:3], 4, 16)
        box = np.einsum("bhwgi,goi->bhwgo", bx, w2).reshape(*c.bx[l].shape[:3], 64) + c.b2[l].astype(np_dtype)
        cls = c.cl[l].astype(np_dtype) @ w3.T + c.b3[l].astype(np_dtype)
        out.append(np.concatenate((box, cls), -1).astype(np_dtype))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# topk_nms_kernel cases: rows with exact float32 arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
LB_HW = (384, 640)                                # network shape of the letterbox geometries
UNIFORM_SRC = (270, 480)                          # gain 4/3, pad_y 12, pad_x 0
RAGGED_SRCS = ((270, 480), (480, 270), (384, 640), (1080, 1920), (100, 333), (719, 1279), (200, 640))


def geometry(src_hw, lb_hw=LB_HW) -> np.ndarray:
    """(pad_x, pad_y, gain, src_w, src_h) as Builder::head_finish computes NmsP's: double arithmetic, then one cast to float."""
    gain = min(lb_hw[0] / src_hw[0], lb_hw[1] / src_hw[1])
    return np.array([(lb_hw[1] - src_hw[1] * gain) / 2, (lb_hw[0] - src_hw[0] * gain) / 2, gain, src_hw[1], src_hw[0]], np.float64).astype(np.float32)


def distinct_scores(n: int) -> np.ndarray:
    """n distinct float32 values in [0.25, 1]."""
    s = (0.25 + 0.75 * np.arange(1, n + 1) / n).astype(np.float32)
    assert len(np.unique(s)) == n and s.min() >= 0.25 and s.max() <= 1
    return s


def random_rows(rng, A: int) -> np.ndarray:
    """A rows with score 0: integer boxes (some past every edge of the letterboxed frame), random classes."""
    r = np.zeros((A, 6), np.float32)
    r[:, 0] = rng.integers(-40, 660, A); r[:, 1] = rng.integers(-40, 400, A)
    r[:, 2] = r[:, 0] + rng.integers(1, 60, A); r[:, 3] = r[:, 1] + rng.integers(1, 60, A)
    r[:, 5] = rng.integers(0, 80, A)
    return r


def grid_rows(A: int) -> np.ndarray:
    """A rows with score 0 and pairwise disjoint 10 x 10 boxes, class 1."""
    r = np.zeros((A, 6), np.float32)
    a = np.arange(A)
    r[:, 0] = 12 * (a % 50); r[:, 1] = 12 * (a // 50); r[:, 2] = r[:, 0] + 10; r[:, 3] = r[:, 1] + 10; r[:, 5] = 1
    return r


def selection_scenarios(A: int, nzs: Sequence[int], seed: int, extra: bool) -> List[Tuple[str, np.ndarray]]:
    rng = np.random.default_rng(seed)
    out = []
    for nz in nzs:                                                            # nz positive rows at random anchors, distinct scores
        r = random_rows(rng, A)
        r[rng.permutation(A)[:nz], 4] = rng.permutation(distinct_scores(max(nz, 1)))[:nz]
        out.append((f"nz{nz}", r))
    r = random_rows(rng, A); r[:, 4] = 0.5
    out.append(("all_equal", r))                                              # the selection resolves in the anchor bytes: anchors 0..299
    if not extra:
        return out
    r = random_rows(rng, A)                                                   # 700 positives of seven values: the 300th place is inside a run
    r[rng.permutation(A)[:700], 4] = rng.permutation(np.repeat(np.float32([0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]), (130, 120, 110, 100, 90, 80, 70)))
    out.append(("seven_values", r))
    r = random_rows(rng, A)                                                   # 600 positives that differ in the lowest mantissa byte only
    r[rng.permutation(A)[:600], 4] = (np.uint32(0x3F000000) + rng.integers(0, 256, 600).astype(np.uint32)).view(np.float32)
    out.append(("low_byte", r))
    r = random_rows(rng, A); r[:200, 4] = rng.permutation(distinct_scores(200))
    out.append(("head200", r))                                                # zero fill = anchors 200..299
    r = random_rows(rng, A); r[A - 40:, 4] = rng.permutation(distinct_scores(40))
    out.append(("tail40", r))
    return out


def nms_scenarios(A: int) -> List[Tuple[str, np.ndarray]]:
    out = []
    r = np.zeros((A, 6), np.float32)                                          # every other row: score 0, zero box, class 0

    def put(a, box, score, cls):
        r[a] = (*box, score, cls)
    # chain: IoU(0,1) = 80/120, IoU(1,2) = 70/130, IoU(0,2) = 50/150: row 1 is suppressed and still suppresses row 2
    put(10, (0, 0, 10, 10), 0.99, 3); put(700, (2, 0, 12, 10), 0.98, 3); put(20, (5, 0, 15, 10), 0.97, 3)
    # IoU = 9/20 = float32(0.45), not above it: kept
    put(30, (0, 50, 14, 51), 0.96, 3); put(31, (5, 50, 20, 51), 0.95, 3)
    # IoU = 1/2: dropped
    put(40, (0, 100, 15, 101), 0.94, 3); put(41, (5, 100, 20, 101), 0.93, 3)
    # the same overlap, different classes: kept
    put(50, (0, 150, 15, 151), 0.92, 3); put(51, (5, 150, 20, 151), 0.91, 4)
    # identical zero-area boxes: 0/0 compares false, kept
    put(60, (33, 200, 33, 200), 0.90, 3); put(61, (33, 200, 33, 200), 0.89, 3)
    # past every edge of the source frame
    put(70, (-30, 250, 5, 260), 0.88, 5); put(71, (630, 250, 700, 260), 0.87, 6); put(72, (100, -20, 110, 5), 0.86, 7); put(73, (100, 370, 110, 420), 0.85, 8)
    out.append(("pairs", r.copy()))
    r = np.zeros((A, 6), np.float32)
    r[500:800] = (7, 9, 40, 50, 0, 2); r[500:800, 4] = distinct_scores(300)[::-1]
    out.append(("identical300", r.copy()))                                    # only the best row survives
    for i in (297, 298, 296):                                                 # suppressor i (thread i % 3 of row 299's trio), victim 299
        r = grid_rows(A)
        r[:300, 4] = distinct_scores(300)[::-1]                               # sorted row k = anchor k
        r[299, :4] = r[i, :4]
        out.append((f"trio{i % 3}", r))
    return out


def nms_launches() -> Dict[str, Tuple[List[str], np.ndarray]]:
    """name -> (scenario names, rows (B,A,6)): one launch each."""
    big = selection_scenarios(2100, (0, 1, 299, 300, 301, 511, 512, 513, 2100), 1, True) + nms_scenarios(2100)
    a189 = selection_scenarios(189, (0, 1, 100, 189), 2, False)
    a525 = selection_scenarios(525, (0, 299, 300, 301, 512, 525), 3, False)
    return {k: ([n for n, _ in v], np.stack([r for _, r in v])) for k, v in (("a2100", big), ("a189", a189), ("a525", a525))}


def nms_expected(rows: np.ndarray, src_hws: Sequence[Tuple[int, int]]) -> np.ndarray:
    """postprocess_rows + scale_boxes of the oracle, image b with source size src_hws[b] (one entry: every image)."""
    kept = yo.YOLOv9Oracle.postprocess_rows(torch.from_numpy(rows))
    hws = list(src_hws) * (len(rows) if len(src_hws) == 1 else 1)
    return np.stack([yo.YOLOv9Oracle.scale_boxes(LB_HW, kept[b], hws[b]).numpy() for b in range(len(rows))])


# ---------------------------------------------------------------------------------------------------------------------------------
# blaze_post_kernel cases
# ---------------------------------------------------------------------------------------------------------------------------------
BLAZE_SCALE = min(256 / 640, 256 / 480)          # a 480 x 640 source: scale 0.4; the crafted launches choose their own pads
BLAZE_THR, BLAZE_IOU = 0.85, 0.3


@dataclass
class BlazeLaunch:
    names: List[str]
    raw: np.ndarray            # (N,896,16) regressor outputs in anchor order
    score: np.ndarray          # (N,896) score logits
    pad_top: int
    pad_left: int
    scale: float = BLAZE_SCALE


def blaze_split(raw: np.ndarray, score: np.ndarray):
    """(N,896,16), (N,896) -> r8 (N,16,16,32), r16 (N,8,8,96), c8 (N,16,16,2), c16 (N,8,8,6) as the heads write them."""
    n = len(raw)
    return (np.ascontiguousarray(raw[:, :512].reshape(n, 16, 16, 32)), np.ascontiguousarray(raw[:, 512:].reshape(n, 8, 8, 96)),
            np.ascontiguousarray(score[:, :512].reshape(n, 16, 16, 2)), np.ascontiguousarray(score[:, 512:].reshape(n, 8, 8, 6)))


def blaze_put(raw: np.ndarray, a: int, anchors: np.ndarray, ymin, xmin, ymax, xmax):
    """Anchor a's raw box so that it decodes to the given corners in 1/256 units of the network frame (integers: exact)."""
    ax, ay = float(anchors[a, 0]) * 256, float(anchors[a, 1]) * 256
    raw[a, 0] = (xmin + xmax) / 2 - ax; raw[a, 1] = (ymin + ymax) / 2 - ay
    raw[a, 2] = xmax - xmin; raw[a, 3] = ymax - ymin


# (image name -> {label: anchor}) of the crafted overlap scenarios, for the tests to look rows up by
BLAZE_MARKS: Dict[str, Dict[str, int]] = {}
BLAZE_PAD_TOP, BLAZE_PAD_LEFT = 16, 8


def _int_raws(rng) -> np.ndarray:
    r = rng.integers(-60, 61, (896, 16)).astype(np.float32)
    r[:, 2:4] = rng.integers(8, 81, (896, 2))
    return r


def blaze_launches(anchors: np.ndarray, seed: int = 0) -> Dict[str, BlazeLaunch]:
    """Crafted images: integer raws over the real anchors, so every decoded coordinate is a dyadic rational and the overlap quotients
    are correctly rounded on both sides.  Score logits 20 and above are exactly 1 in float32 on both sides; the other alive rows carry
    logits 0.5 apart.  One random image (raws ~ N(0,40), logits ~ N(0,2): about a fifth of the anchors alive)."""
    rng = np.random.default_rng(seed)
    low = lambda: np.full(896, -5.0, np.float32)                                       # noqa: E731  sigmoid(-5) < 0.85
    imgs = []
    imgs.append(("none_alive_padded", _int_raws(rng), low()))
    imgs.append(("all_score_one", _int_raws(rng), np.full(896, 1000.0, np.float32)))
    # the overlap rule; groups far apart; ranks by descending logit
    raw, sc, marks, k = _int_raws(rng), low(), {}, [0]

    def put(label, a, box):
        blaze_put(raw, a, anchors, *box)
        sc[a] = 8.0 - 0.5 * k[0]; k[0] += 1
        marks[label] = a
    put("eq_a", 300, (20, 20, 30, 30)); put("eq_b", 17, (20, 24, 30, 40))              # 60 / 200 = 3/10: kept
    put("gt_a", 600, (60, 20, 70, 60)); put("gt_b", 18, (60, 29, 70, 120))             # 310 / 1000: dropped
    put("ch_a", 5, (100, 20, 110, 30)); put("ch_b", 890, (100, 22, 110, 32)); put("ch_c", 6, (100, 27, 110, 37))   # 80/120, 50/150; a-c 30/170
    imgs.append(("overlap_rule", raw, sc)); BLAZE_MARKS["overlap_rule"] = marks
    # the best row's ymin maps to exactly 0 after the back-map: passed over by the first-row pick
    raw, sc, marks = _int_raws(rng), low(), {}
    blaze_put(raw, 400, anchors, BLAZE_PAD_TOP, 40, BLAZE_PAD_TOP + 30, 70); sc[400] = 8.0; marks["best"] = 400
    blaze_put(raw, 50, anchors, 120, 40, 150, 70); sc[50] = 7.0; marks["next"] = 50
    imgs.append(("ymin_zero", raw, sc)); BLAZE_MARKS["ymin_zero"] = marks
    for i in range(2):
        r = rng.normal(0, 40, (896, 16)).astype(np.float32)
        r[:, 2:4] += 64                                                                 # sizes around a quarter of the frame: the boxes overlap
        imgs.append((f"random{i}", r, rng.normal(0, 2, 896).astype(np.float32)))
    padded = BlazeLaunch([n for n, _, _ in imgs], np.stack([r for _, r, _ in imgs]), np.stack([s for _, _, s in imgs]), BLAZE_PAD_TOP, BLAZE_PAD_LEFT)
    plain = BlazeLaunch(["none_alive"], _int_raws(rng)[None], low()[None], 0, 0)
    return {"plain": plain, "padded": padded}


def blaze_expected(anchors: np.ndarray, L: BlazeLaunch):
    """The oracle's decode, postprocess and back-map per image -> rows (N,896,17), first (N,17), first_idx (N): the first row whose ymin
    is not 0, as `found[found[:, 0] != 0][0]` picks it, zeros and -1 when there is none."""
    o = BlazeFaceOracle({"anchors": anchors})
    rows, first, idx = [], [], []
    for raw, sc in zip(L.raw, L.score):
        d = o.back_map(o.postprocess(o.decode(torch.from_numpy(raw), torch.from_numpy(sc))), L.scale, L.pad_top, L.pad_left).numpy()
        nz = np.flatnonzero(d[:, 0] != 0)
        rows.append(d); idx.append(int(nz[0]) if len(nz) else -1)
        first.append(d[nz[0]] if len(nz) else np.zeros(17, np.float32))
    return np.stack(rows), np.stack(first), np.array(idx, np.int32)


def blaze_margins(anchors: np.ndarray, raw: np.ndarray, score: np.ndarray) -> Tuple[float, float]:
    """Float64: distance of the nearest sigmoid to 0.85, and of the nearest IoU between two rows over the threshold to 0.3."""
    r, a = raw.astype(np.float64), anchors.astype(np.float64)
    xc, yc, w, h = r[:, 0] / 256 * a[:, 2] + a[:, 0], r[:, 1] / 256 * a[:, 3] + a[:, 1], r[:, 2] / 256 * a[:, 2], r[:, 3] / 256 * a[:, 3]
    s = 1 / (1 + np.exp(-np.clip(score.astype(np.float64), -100, 100)))
    m = s >= BLAZE_THR
    y1, x1, y2, x2 = (yc - h / 2)[m], (xc - w / 2)[m], (yc + h / 2)[m], (xc + w / 2)[m]
    iw = np.clip(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), 0, None)
    ih = np.clip(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), 0, None)
    area = (x2 - x1) * (y2 - y1)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = iw * ih / (area[:, None] + area[None] - iw * ih)
    iou = iou[np.triu_indices(len(area), 1)]
    return float(np.abs(s - BLAZE_THR).min()), float(np.nanmin(np.abs(iou - BLAZE_IOU))) if len(iou) else 1.0
