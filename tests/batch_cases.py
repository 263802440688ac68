"""Batches of production size built from four distinct inputs per model, and the check that holds such a batch to the CPU oracle
(helper module; not a conftest).  Shared by tests/test_batch_cases_host.py (no device: the pattern, the planted faults, the separation of
the inputs) and tests/test_gpu_plan_batches.py (the AdaFace, BlazeFace and CLIP L/14 plans at the batch sizes where the selector picks
new kernels, tests/plan_route_table.py).

The oracle is evaluated on the K = 4 distinct inputs only; pattern(B) says which input stands at which of the B positions.  check_rows
then asks two things of the B output rows: (a) every row meets the model's own parity bar against the oracle row of its input, and
(b) all copies of one input are bit-equal.  The neighbours of a copy differ from copy to copy (pattern: neighbours always differ, no
short period), so a row that is swapped, shifted or contaminated by a neighbour breaks (b) even in the 16-bit modes, whose cosine bars
are too loose to tell two inputs apart.

THE BARS are the project's own, restated here with their source line; there are no new numbers:
    CLIP L/14   f32        max |got - ref| <= 2e-5 and cos >= 1 - 1e-6                   tests/test_gpu_reference_run.py:62
    CLIP L/14   f16, bf16  cos >= 1 - 1e-4                                               tests/test_gpu_clip.py:59
    AdaFace     f32        max |got - ref| < 2e-5 (and cos >= 1 - 2e-5)                  tests/test_gpu_face.py:18,31
    AdaFace     f16        cos >= 1 - 2e-3                                               tests/test_gpu_face.py:18
    AdaFace     bf16       cos >= 1 - 2e-2                                               tests/test_gpu_face.py:18
    BlazeFace   f32        the conditions of test_blazeface_f32_matches_oracle           tests/test_gpu_blazeface.py:32-38
    BlazeFace   f16, bf16  the conditions of test_blazeface_16bit_modes                  tests/test_gpu_blazeface.py:47-50
A bar is a callable (got_row, want_row) -> (ok, error / bar, text); error / bar is what the GPU module prints as its record.
"""
from __future__ import annotations

from typing import Callable, Dict, Sequence, Tuple

import numpy as np

K = 4
KINDS = ("noise", "gradient", "blocks", "quarter")
MAX_PERIOD = 16

# The batch sizes tests/test_gpu_plan_batches.py runs (tests/plan_route_table.py: the batches at which new routes appear; 255 is bench.py's).
BATCHES = {"adaface": (12, 40, 256), "blazeface": (32,), "clip_image": (8, 64, 255), "clip_text": (8, 64)}
SMALL = {"adaface": 3, "blazeface": 3, "clip_image": 2, "clip_text": 2}      # the batch of each model's existing oracle test
ALL_B = tuple(sorted({b for v in BATCHES.values() for b in v}))

# One seed per structure and model, chosen so that the separation conditions of tests/test_batch_cases_host.py hold on the oracle's outputs.
# BlazeFace's seeded checkpoint keeps no row on a mid-grey or slowly varying frame (its scores follow the local brightness level), so its
# gradient runs through about sixteen periods; the seeds are those whose every anchor score stays 4e-3 or more (400 x the f32 score bar) away from the 0.85 test.
CLIP_SEEDS = (11, 12, 13, 14)
FACE_SEEDS = (21, 22, 23, 24)
BLAZE_SEEDS = (31, 34, 37, 35)
BLAZE_CYCLES = 16.0


# ---- which input stands where ------------------------------------------------------------------------------------------------------------
def pattern(B: int, k: int = K) -> np.ndarray:
    """(B,) int: the input at each position.  Deterministic from B; neighbours differ, and the last differs from the first too (a row
    that wraps round meets another input).  B < k: the first B inputs."""
    if B <= k:
        return np.arange(B)
    rng = np.random.default_rng(B)
    p = np.zeros(B, np.int64)
    for i in range(1, B):
        p[i] = (p[i - 1] + 1 + rng.integers(0, k - 1)) % k
    while p[B - 1] == p[B - 2] or p[B - 1] == p[0]:
        p[B - 1] = (p[B - 1] + 1) % k
    return p


def pattern_faults(p: np.ndarray, k: int = K) -> list:
    """What is wrong with a pattern (empty: nothing).  A period q is only looked for up to half the length: a longer one never repeats."""
    B, bad = len(p), []
    if B > 1 and (p[1:] == p[:-1]).any():
        bad.append("two neighbours are the same input")
    if set(p.tolist()) != set(range(min(B, k))):
        bad.append("an input does not occur")
    for q in range(1, min(MAX_PERIOD, B // 2) + 1):
        if B > k and (p[q:] == p[:-q]).all():
            bad.append(f"periodic with period {q}")
    return bad


def expand(want_rows: np.ndarray, p: np.ndarray) -> np.ndarray:
    """The batch a faultless device would return: the oracle's rows placed by the pattern."""
    return np.ascontiguousarray(np.asarray(want_rows)[p])


# ---- four inputs of different structure ----------------------------------------------------------------------------------------------------
def structured(kind: str, seed: int, h: int, w: int, cycles: float = 1.0) -> np.ndarray:
    """(h, w, 3) float64 in [0, 1): uniform noise; a smooth gradient (per channel one sine of about `cycles` periods across the image, in a seeded direction);
    blocks of flat colour with hard edges (a seeded grid of 6 to 14 cells a side); noise scaled to a quarter of the range."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.random((h, w, 3))
    if kind == "quarter":
        return 0.25 * rng.random((h, w, 3))
    if kind == "gradient":
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
        out = np.empty((h, w, 3))
        for c in range(3):
            a, f, ph = rng.uniform(0, 2 * np.pi), cycles * rng.uniform(0.75, 1.5), rng.uniform(0, 2 * np.pi)
            out[..., c] = 0.5 + 0.5 * np.sin(2 * np.pi * f * (np.cos(a) * xx + np.sin(a) * yy) + ph)
        return np.clip(out, 0, 1 - 1e-9)
    assert kind == "blocks", kind
    n = int(rng.integers(6, 15))
    ys, xs = np.sort(rng.choice(np.arange(1, h), n - 1, replace=False)), np.sort(rng.choice(np.arange(1, w), n - 1, replace=False))
    u = rng.random((n, n, 3))
    colour = np.where(rng.random((n, n, 3)) < 0.5, 0.12 * u, 1 - 0.12 * u)      # saturated: every channel of a block near black or near white
    return colour[np.searchsorted(ys, np.arange(h), side="right")][:, np.searchsorted(xs, np.arange(w), side="right")]


def _u8(v: np.ndarray) -> np.ndarray:
    return np.minimum(np.floor(v * 256), 255).astype(np.uint8)


def clip_images(size: int, seeds: Sequence[int] = CLIP_SEEDS) -> np.ndarray:
    """(4, 3, size, size) float32 in [-1, 1): the value range of tests/test_gpu_clip.py's inputs."""
    return np.stack([(structured(kd, s, size, size) * 2 - 1).astype(np.float32).transpose(2, 0, 1) for kd, s in zip(KINDS, seeds)])


def face_crops(seeds: Sequence[int] = FACE_SEEDS) -> np.ndarray:
    """(4, 112, 112, 3) uint8 aligned-face inputs of AdaFace."""
    return np.stack([_u8(structured(kd, s, 112, 112)) for kd, s in zip(KINDS, seeds)])


def blaze_images(seeds: Sequence[int] = BLAZE_SEEDS) -> np.ndarray:
    """(4, 640, 640, 3) uint8 frames of BlazeFace."""
    return np.stack([_u8(structured(kd, s, 640, 640, BLAZE_CYCLES)) for kd, s in zip(KINDS, seeds)])


def text_tokens(arch) -> np.ndarray:
    """(4, ctx) int32: the four prompts of test_gpu_clip._toks (3 tokens, 39 tokens, empty, full length): the EOT position differs from row to row."""
    from test_gpu_clip import _toks
    return _toks(arch)


def separation(want_rows: np.ndarray) -> float:
    """The smallest max |a - b| over the pairs of oracle rows: what must exceed the bar many times for a swapped row to fail it."""
    w = np.asarray(want_rows, np.float64).reshape(len(want_rows), -1)
    return min(float(np.abs(w[i] - w[j]).max()) for i in range(len(w)) for j in range(i + 1, len(w)))


# ---- the bars ------------------------------------------------------------------------------------------------------------------------------
Bar = Callable[[np.ndarray, np.ndarray], Tuple[bool, float, str]]


def _cos(got, want) -> float:
    return float((np.asarray(got, np.float64) * np.asarray(want, np.float64)).sum())


def cos_bar(tol: float) -> Bar:
    def bar(got, want):
        if not np.isfinite(got).all():
            return False, float("inf"), "not finite"
        miss = 1 - _cos(got, want)
        return miss <= tol, miss / tol, f"1 - cos = {miss:.3g} (bar {tol:g})"
    return bar


def abs_cos_bar(abs_tol: float, cos_tol: float, strict: bool) -> Bar:
    def bar(got, want):
        if not np.isfinite(got).all():
            return False, float("inf"), "not finite"
        err, miss = float(np.abs(np.asarray(got, np.float64) - want).max()), 1 - _cos(got, want)
        ok = (err < abs_tol if strict else err <= abs_tol) and miss <= cos_tol
        return ok, max(err / abs_tol, miss / cos_tol), f"max |got - ref| = {err:.3g} (bar {abs_tol:g}), 1 - cos = {miss:.3g} (bar {cos_tol:g})"
    return bar


def _alive(d):
    return d[d[:, 16] != 0]


def blaze_f32_bar(shape=(640, 640)) -> Bar:
    scale = min(256 / shape[1], 256 / shape[0])

    def bar(got, ref):
        if got.shape != (896, 17) or not np.array_equal(ref[:, 16] != 0, got[:, 16] != 0):
            return False, float("inf"), f"other rows survive: {int((got[:, 16] != 0).sum())} against the oracle's {int((ref[:, 16] != 0).sum())}"
        ra, ga = _alive(ref), _alive(got)
        if not (len(ra) > 10 and len(ga) == len(ra)):
            return False, float("inf"), f"{len(ra)} surviving rows in the oracle, {len(ga)} on the device"
        box, score = float(np.abs(ra[:, :16] - ga[:, :16]).max()), float(np.abs(ra[:, 16] - ga[:, 16]).max())
        zeros = bool(np.allclose(ref[ref[:, 16] == 0], got[got[:, 16] == 0], atol=1e-6))
        ok = box <= 2e-3 / scale and score <= 1e-5 * 256 / scale and zeros
        return ok, max(box / (2e-3 / scale), score / (1e-5 * 256 / scale)), (f"box err {box:.3g} (bar {2e-3 / scale:.3g}), score err {score:.3g} "
                                                                             f"(bar {1e-5 * 256 / scale:.3g}), suppressed rows zero: {zeros}")
    return bar


def blaze_16bit_bar(dtype: str) -> Bar:
    px = 8 if dtype == "f16" else 30

    def bar(got, ref):
        r, g = _alive(ref), _alive(got)
        if not np.isfinite(got).all():
            return False, float("inf"), "not finite"
        room = max(3, len(r) // 4)
        hit = sum(1 for row in r if len(g) and np.abs(g[:, :4] - row[:4]).max(1).min() < px)
        ok = abs(len(g) - len(r)) <= room and hit >= 0.6 * len(r)
        ratio = max(abs(len(g) - len(r)) / room, (len(r) - hit) / (0.4 * len(r)) if len(r) else 0.0)
        return ok, ratio, f"{len(g)} rows against the oracle's {len(r)} (room {room}), {hit} of them within {px} px (at least {0.6 * len(r):.1f})"
    return bar


BARS: Dict[Tuple[str, str], Bar] = {
    ("clip", "f32"): abs_cos_bar(2e-5, 1e-6, strict=False), ("clip", "f16"): cos_bar(1e-4), ("clip", "bf16"): cos_bar(1e-4),
    ("adaface", "f32"): abs_cos_bar(2e-5, 2e-5, strict=True), ("adaface", "f16"): cos_bar(2e-3), ("adaface", "bf16"): cos_bar(2e-2),
    ("blazeface", "f32"): blaze_f32_bar(), ("blazeface", "f16"): blaze_16bit_bar("f16"), ("blazeface", "bf16"): blaze_16bit_bar("bf16"),
}
F32_ABS_BAR = {"clip": 2e-5, "adaface": 2e-5}


# ---- the check -----------------------------------------------------------------------------------------------------------------------------
def check_rows(got: np.ndarray, want_rows: np.ndarray, p: np.ndarray, bar: Bar) -> float:
    """Hold a batch to the oracle rows of its inputs; returns the worst error / bar.  Raises AssertionError naming the first offending
    position and its input: (a) got[i] misses `bar` against want_rows[p[i]], or (b) two copies of one input are not bit-equal."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    assert len(got) == len(p), f"{len(got)} rows for a batch of {len(p)}"
    worst = 0.0
    for i in range(len(p)):
        ok, ratio, text = bar(got[i], np.asarray(want_rows[p[i]]))
        assert ok, f"position {i} (input {int(p[i])}) misses the bar: {text}"
        worst = max(worst, ratio)
    bits = got.reshape(len(p), -1).view(np.uint32)
    first = {}
    for i in range(len(p)):
        f = first.setdefault(int(p[i]), i)
        if f != i and not np.array_equal(bits[i], bits[f]):
            n = int((bits[i] != bits[f]).sum())
            raise AssertionError(f"position {i} is not bit-equal to position {f}, both copies of input {int(p[i])}: {n} of {bits.shape[1]} words differ, "
                                 f"max |difference| {float(np.nanmax(np.abs(got[i].astype(np.float64) - got[f]))):.3g}")
    return worst
