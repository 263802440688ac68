"""Case tables, input makers and float64 references of tests/test_gpu_glue_kernels.py, held on the CPU by tests/test_glue_cases_host.py
(helper module; not a conftest).  NumPy / PyTorch-CPU only.

The kernels are the ones BETWEEN the convs - launch_pool's ten kernels and fuse_kernel (clearcam_amd/csrc/conv_direct.hip), affine_kernel
and face_pre_kernel (face.hip) - and the conv loaders that read two sources or an upsampled / averaged one (conv_mfma_kernel<SIMPLE =
false>, conv_direct_kernel, the eight-wave kernel's `two` loader, conv_adown.hip).  A case is ONE launch through a cc_dev_* entry and
names the kernel it must reach.

Two kinds of input:
  grid    multiples of 2^-4 in [-8, 8): exact in bf16, f16 and f32.  Every f32 sum of at most 6 of them (|sum| <= 48 = 768 / 16: ten
          bits) and the x 0.25 of a 2x2 average are exact, so a kernel rounds ONCE, to the storage type, and must return
          round_storage(y64) bit for bit (tests/test_glue_cases_host.py evaluates every grid case in numpy float32 in the kernel's
          summation order and finds the float64 value: the licence for that demand).
  normal  N(0,1) rounded to the storage type.
Buffers are wider than the view wherever a case has a view, and every channel outside a view is NaN: in inputs so that a read outside
the slice poisons the result, in outputs so that a stray store shows.  Seeds come from the case name through zlib.crc32.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

import numpy as np
import torch

import restart_check as rc

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f16s": torch.float16}
DTI = {"f32": 0, "f16": 1, "bf16": 2, "f16s": 3}
ALL3 = ("f32", "f16", "bf16")
U24 = 2.0 ** -24

# PoolKernel (clearcam_amd/csrc/kernels.h)
(POOL_SCALAR, POOL_VEC_MAX1, POOL_VEC_MAX2, POOL_VEC_MAX3, POOL_VEC_MAX5, POOL_VEC_AVG2, POOL_AVG2_ROWS4, POOL_AVG2_ROWS8, POOL_AVGMAX,
 POOL_AVGMAX_ROWS2) = range(10)
POOL_NAMES = ["scalar", "vec_max1", "vec_max2", "vec_max3", "vec_max5", "vec_avg2", "avg2_rows4", "avg2_rows8", "avgmax", "avgmax_rows2"]
# ConvKernel / phase schedules (conv_select.h), the averaging kernel's own code (clearcam_hip.h CC_DEV_CONV_ADOWN), ConvVariant values
DIRECT, GENERIC, BIG, PHASE = 0, 1, 2, 3
SCHED0, ONE_TILE, BUFFER, PERSIST = range(4)
ADOWN = 100
V_AUTO, V_DIRECT, V_GENERIC, V_PHASE, V_PIX32_4 = 0, 1, 2, 7, 97


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


def storage(a: np.ndarray, dt: str) -> np.ndarray:
    """float64 values -> the nearest value of the storage type (ties to even), as float64."""
    if dt == "f32":
        return a.astype(np.float32).astype(np.float64)
    return rc.round_storage(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)), "f16" if dt == "f16s" else dt).numpy()


def make_input(name: str, shape, dt: str, kind: str) -> np.ndarray:
    """float64 values the storage type holds exactly.  kind: "grid" | "grid_neg" (multiples of 2^-4 in [-8, 0)) | "normal"."""
    g = np.random.default_rng(seed_of(f"{name}|{dt}|{kind}"))
    if kind == "grid":
        return g.integers(-128, 128, shape).astype(np.float64) / 16.0
    if kind == "grid_neg":
        return g.integers(-128, 0, shape).astype(np.float64) / 16.0
    assert kind == "normal", kind
    return storage(g.standard_normal(shape), dt)


def in_nan_buffer(x: np.ndarray, cstride: int, coff: int) -> np.ndarray:
    """(.., C) -> (.., cstride) with x in channels [coff, coff + C) and NaN everywhere else."""
    buf = np.full(x.shape[:-1] + (cstride,), np.nan)
    buf[..., coff:coff + x.shape[-1]] = x
    return buf


# =====================================================================================================================================
# pools
# =====================================================================================================================================
@dataclass(frozen=True)
class PoolCase:
    name: str
    mode: int                           # 0 avg, 1 max (-inf padding), 2 avg 2x2 s1 then max k s p
    k: int
    stride: int
    pad: int
    H: int
    W: int
    expect: int                         # the PoolKernel the launch must report
    C: int = 16
    B: int = 2
    in_cstride: int = 0                 # 0: C (dense)
    in_coff: int = 0
    out_cstride: int = 0
    out_coff: int = 0
    pool_rows: Optional[int] = None     # cc_dev_set("pool_rows") around the launch
    dtypes: Tuple[str, ...] = ALL3
    negative: bool = False              # the grid input is all negative: zero padding instead of -inf would win
    refused: bool = False

    @property
    def ics(self) -> int:
        return self.in_cstride or self.C

    @property
    def ocs(self) -> int:
        return self.out_cstride or self.C

    @property
    def out_hw(self) -> Tuple[int, int]:
        if self.mode == 0:
            return (self.H - self.k) // self.stride + 1, (self.W - self.k) // self.stride + 1
        h, w = (self.H - 1, self.W - 1) if self.mode == 2 else (self.H, self.W)
        return (h + 2 * self.pad - self.k) // self.stride + 1, (w + 2 * self.pad - self.k) // self.stride + 1

    @property
    def grid_kind(self) -> str:
        return "grid_neg" if self.negative else "grid"


def _pool_cases() -> List[PoolCase]:
    cs: List[PoolCase] = []
    # ---- ADown / AConv: avg 2x2 s1.  Ho = 66 = 8 * 8 + 2: the last row group of the eight-row kernel is partial (and of the four-row one)
    a = PoolCase("avg2_67x21", 0, 2, 1, 0, 67, 21, POOL_AVG2_ROWS8, in_cstride=32, in_coff=8, out_cstride=24, out_coff=8)
    cs += [a, replace(a, name=a.name + "-rows4", pool_rows=4, expect=POOL_AVG2_ROWS4),
           replace(a, name=a.name + "-rows1", pool_rows=1, expect=POOL_VEC_AVG2),
           replace(a, name="avg2_9x13", H=9, W=13, expect=POOL_VEC_AVG2)]          # Ho < 64: the one-row kernel by rule
    # ---- ADown's second branch: avg 2x2 s1 then max 3x3 s2 p1.  Ho = 33: the two-row kernel ends on a single row
    m = PoolCase("avgmax_66x23", 2, 3, 2, 1, 66, 23, POOL_AVGMAX_ROWS2, in_cstride=32, in_coff=16, out_cstride=24, out_coff=8)
    cs += [m, replace(m, name=m.name + "-rows1", pool_rows=1, expect=POOL_AVGMAX),
           replace(m, name="avgmax_10x9", H=10, W=9, expect=POOL_AVGMAX),                  # the last window's row ph = H - 1 lies outside the averaged map: skipped
           replace(m, name="avgmax_9x10", H=9, W=10, expect=POOL_AVGMAX)]                  # ... and here that row does not exist, the column does
    # ---- SPPELAN: max 5x5 s1 p2; on 3x3 every window is clipped on both sides
    s = PoolCase("max5_7x6", 1, 5, 1, 2, 7, 6, POOL_VEC_MAX5, in_cstride=32, in_coff=8, out_cstride=32, out_coff=16)
    cs += [s, replace(s, name="max5_3x3", H=3, W=3), replace(s, name="max5_3x3-neg", H=3, W=3, negative=True)]
    k3 = PoolCase("max3_7x10", 1, 3, 2, 1, 7, 10, POOL_VEC_MAX3, in_cstride=24, in_coff=8)
    cs += [k3, replace(k3, name=k3.name + "-neg", negative=True)]
    # ---- BlazeFace's max_pool2d(2, 2): dense, and into a channel slice of a wider map (odd size: the last row / column is dropped)
    k2 = PoolCase("max2_8x8", 1, 2, 2, 0, 8, 8, POOL_VEC_MAX2)
    cs += [k2, replace(k2, name="max2_9x9_slice", H=9, W=9, C=24, out_cstride=48, out_coff=24), replace(k2, name="max2_9x9-neg", H=9, W=9, negative=True)]
    # ---- AdaFace's MaxPool2d(1, 2): a strided copy
    k1 = PoolCase("max1_7x7", 1, 1, 2, 0, 7, 7, POOL_VEC_MAX1, in_cstride=24, in_coff=8)
    cs += [k1, replace(k1, name=k1.name + "-neg", negative=True)]
    # ---- scalar fallback: channel counts that are not whole 16-byte chunks (YOLOv9-m's widths), coff 4; k = 4 has no vector instantiation
    for dt, C, ics in (("f16", 12, 20), ("f32", 6, 12)):
        sc = PoolCase(f"scalar_c{C}_avg2", 0, 2, 1, 0, 7, 9, POOL_SCALAR, C=C, in_cstride=ics, in_coff=4, out_cstride=ics, out_coff=4, dtypes=(dt,))
        cs += [sc, replace(sc, name=f"scalar_c{C}_max3", mode=1, k=3, stride=2, pad=1), replace(sc, name=f"scalar_c{C}_max3-neg", mode=1, k=3, stride=2, pad=1, negative=True),
               replace(sc, name=f"scalar_c{C}_max4", mode=1, k=4, stride=2, pad=1)]
    cs.append(PoolCase("scalar_c16_max4-neg", 1, 4, 2, 1, 7, 9, POOL_SCALAR, negative=True))   # aligned channels still fall back where no vector kernel has the window
    # ---- refused: the avg-max kernels need whole 16-byte channel chunks
    cs.append(PoolCase("avgmax_c12-refused", 2, 3, 2, 1, 10, 9, -1, C=12, in_cstride=20, in_coff=4, out_cstride=20, out_coff=4, dtypes=("f16",), refused=True))
    return cs


POOL_CASES: List[PoolCase] = _pool_cases()
assert len({c.name for c in POOL_CASES}) == len(POOL_CASES)


def _taps(x: np.ndarray, k: int, stride: int, pad: int, Ho: int, Wo: int, fill: float) -> List[np.ndarray]:
    """The k*k window taps of every output position, row-major (the kernels' order), each (B, Ho, Wo, C); padding = fill."""
    B, H, W, C = x.shape
    Hp, Wp = max(H + 2 * pad, (Ho - 1) * stride + k), max(W + 2 * pad, (Wo - 1) * stride + k)
    xp = np.full((B, Hp, Wp, C), fill)
    xp[:, pad:pad + H, pad:pad + W] = x
    return [xp[:, r:r + (Ho - 1) * stride + 1:stride, s:s + (Wo - 1) * stride + 1:stride] for r in range(k) for s in range(k)]


def avg2_ref(x: np.ndarray) -> np.ndarray:
    """avg_pool2d(2, 1, 0) of (B, H, W, C) in float64, taps summed in the kernels' order."""
    t = _taps(x, 2, 1, 0, x.shape[1] - 1, x.shape[2] - 1, 0.0)
    return (((t[0] + t[1]) + t[2]) + t[3]) * 0.25


def pool_ref(c: PoolCase, x: np.ndarray, dt: Optional[str] = None) -> np.ndarray:
    """float64 result of the case on x (B, H, W, C), NOT rounded.  Mode 2 with dt given follows the model's order - average, ROUND to the
    storage type, max; without dt the average is not rounded (rounding is monotone: round_storage of this equals that, held on the host)."""
    Ho, Wo = c.out_hw
    if c.mode == 0:
        t = _taps(x, c.k, c.stride, 0, Ho, Wo, 0.0)
        acc = np.zeros_like(t[0])
        for v in t:
            acc = acc + v
        return acc * (1.0 / (c.k * c.k))
    if c.mode == 2:
        x = avg2_ref(x)
        if dt is not None:
            x = storage(x, dt)
    return np.maximum.reduce(_taps(x, c.k, c.stride, c.pad, Ho, Wo, -np.inf))


def pool_abs_taps(c: PoolCase, x: np.ndarray) -> np.ndarray:
    """sum |taps| per output element: the magnitude an f32 evaluation's rounding errors scale with (mode 2: the largest over the window)."""
    Ho, Wo = c.out_hw
    if c.mode == 0:
        return np.add.reduce(_taps(np.abs(x), c.k, c.stride, 0, Ho, Wo, 0.0))
    if c.mode == 2:
        a = np.add.reduce(_taps(np.abs(x), 2, 1, 0, x.shape[1] - 1, x.shape[2] - 1, 0.0))
        return np.maximum.reduce(_taps(a, c.k, c.stride, c.pad, Ho, Wo, 0.0))
    return np.zeros((x.shape[0], Ho, Wo, x.shape[3]))


def pool_f32_emulation(c: PoolCase, x: np.ndarray) -> np.ndarray:
    """The case in numpy float32 in the kernels' summation order (((0 + t0) + t1) + ...) x 1/k^2, max in f32; float32 result."""
    Ho, Wo = c.out_hw
    x = x.astype(np.float32)

    def avg(taps, k):
        acc = np.zeros_like(taps[0])
        for v in taps:
            acc = (acc + v).astype(np.float32)
        return (acc * np.float32(1.0 / (k * k))).astype(np.float32)

    if c.mode == 0:
        return avg(_taps(x, c.k, c.stride, 0, Ho, Wo, np.float32(0)), c.k)
    if c.mode == 2:
        x = avg(_taps(x, 2, 1, 0, x.shape[1] - 1, x.shape[2] - 1, np.float32(0)), 2)
    return np.maximum.reduce([t.astype(np.float32) for t in _taps(x, c.k, c.stride, c.pad, Ho, Wo, -np.inf)])


@functools.lru_cache(maxsize=None)
def pool_problem(c: PoolCase, dt: str, kind: str):
    """(x, y64, sum |taps|) of a case; shared and never modified."""
    x = make_input(c.name, (c.B, c.H, c.W, c.C), dt, kind)
    return x, pool_ref(c, x), pool_abs_taps(c, x)


# =====================================================================================================================================
# CBFuse
# =====================================================================================================================================
@dataclass(frozen=True)
class FuseCase:
    name: str
    shifts: Tuple[int, ...]
    views: Tuple[Tuple[int, int], ...]  # (cstride, coff) per input
    out_view: Tuple[int, int] = (16, 0)
    B: int = 2
    Ho: int = 8
    Wo: int = 12
    C: int = 16
    dtypes: Tuple[str, ...] = ALL3
    refused: bool = False

    @property
    def n(self) -> int:
        return len(self.shifts)

    def in_hw(self, i: int) -> Tuple[int, int]:
        s = self.shifts[i]
        return ((self.Ho - 1) >> s) + 1, ((self.Wo - 1) >> s) + 1


FUSE_CASES: List[FuseCase] = [
    FuseCase("fuse3", (2, 1, 0), ((32, 8), (24, 8), (48, 32))),
    FuseCase("fuse1", (0,), ((16, 0),)),
    FuseCase("fuse6_out_slice", (2, 2, 1, 1, 0, 0), ((16, 0), (32, 16), (24, 8), (16, 0), (32, 8), (40, 24)), out_view=(32, 8)),
    # 4 channels are half a 16-byte chunk of a 16-bit type, 2 half a chunk of f32
    FuseCase("fuse3_coff4-refused", (2, 1, 0), ((32, 8), (24, 4), (48, 32)), dtypes=("f16", "bf16"), refused=True),
    FuseCase("fuse3_coff2-refused", (2, 1, 0), ((32, 8), (24, 2), (48, 32)), dtypes=("f32",), refused=True),
]


def fuse_ref(c: FuseCase, xs: List[np.ndarray]) -> np.ndarray:
    """sum over the inputs of x_i[ho >> shift_i, wo >> shift_i] in float64, in input order."""
    ho, wo = np.arange(c.Ho), np.arange(c.Wo)
    acc = np.zeros((c.B, c.Ho, c.Wo, c.C))
    for x, s in zip(xs, c.shifts):
        acc = acc + x[:, (ho >> s)[:, None], (wo >> s)[None, :]]
    return acc


def fuse_f32_emulation(c: FuseCase, xs: List[np.ndarray]) -> np.ndarray:
    ho, wo = np.arange(c.Ho), np.arange(c.Wo)
    acc = np.zeros((c.B, c.Ho, c.Wo, c.C), np.float32)
    for x, s in zip(xs, c.shifts):
        acc = (acc + x.astype(np.float32)[:, (ho >> s)[:, None], (wo >> s)[None, :]]).astype(np.float32)
    return acc


@functools.lru_cache(maxsize=None)
def fuse_problem(c: FuseCase, dt: str, kind: str):
    xs = [make_input(f"{c.name}|{i}", (c.B,) + c.in_hw(i) + (c.C,), dt, kind) for i in range(c.n)]
    return xs, fuse_ref(c, xs), fuse_ref(c, [np.abs(x) for x in xs])


# =====================================================================================================================================
# affine (AdaFace's BatchNorm in front of a padded conv) and face preprocessing
# =====================================================================================================================================
AFFINE_SHAPES = ((35, 64), (3, 512))                    # (B * H * W, C)
CANCEL = 2.0 ** -6


@functools.lru_cache(maxsize=None)
def affine_problem(rows: int, C: int, dt: str):
    """x (rows, C) in the storage type, float32 scale / shift of both signs, y64 = x s + t and A = |x s| + |t| in float64.
    Where x s and t cancel below CANCEL * A the sign of x is flipped: the kernel's two f32 roundings move the result by at most 2^-23 A,
    which then stays under half a quantum of either 16-bit type at y64 (>= 2^-9 |y64| >= 2^-15 A), so that the value it rounds to the
    storage type is one of the two that bracket y64 - the licence for the 16-bit bar (held on the host)."""
    g = np.random.default_rng(seed_of(f"affine|{rows}|{C}|{dt}"))
    x = storage(g.standard_normal((rows, C)), dt)
    scale = (g.uniform(0.25, 2.0, C) * np.where(np.arange(C) % 3 == 0, -1.0, 1.0)).astype(np.float32)
    shift = (g.uniform(0.05, 1.5, C) * np.where(np.arange(C) % 2 == 0, -1.0, 1.0)).astype(np.float32)
    s64, t64 = scale.astype(np.float64), shift.astype(np.float64)
    A = np.abs(x * s64) + np.abs(t64)
    x = np.where(np.abs(x * s64 + t64) < CANCEL * A, -x, x)
    return x, scale, shift, x * s64 + t64, A


FACE_RES = 112


@functools.lru_cache(maxsize=None)
def face_frames(f32: bool, B: int = 2) -> np.ndarray:
    """(B, 112, 112, 3) frames: uint8 with all 256 values in every channel of every frame, or float32 in [0, 255] off the integers."""
    g = np.random.default_rng(seed_of(f"face_pre|{int(f32)}"))
    n = FACE_RES * FACE_RES
    if f32:
        return g.uniform(0.0, 255.0, (B, FACE_RES, FACE_RES, 3)).astype(np.float32)
    out = np.empty((B, n, 3), np.uint8)
    for b in range(B):
        for ch in range(3):
            out[b, :, ch] = g.permutation(np.arange(n) % 256)
    return out.reshape(B, FACE_RES, FACE_RES, 3)


def face_pre_ref(frames: np.ndarray, cpad: int) -> np.ndarray:
    """((x[..., ::-1] / 255) - 0.5) / 0.5 in numpy float32 (IEEE division, as the kernel's __fdiv_rn), channels 3 .. cpad zero; float32."""
    v = frames[..., ::-1].astype(np.float32)
    v = ((v / np.float32(255.0)).astype(np.float32) - np.float32(0.5)).astype(np.float32) / np.float32(0.5)
    out = np.zeros(frames.shape[:3] + (cpad,), np.float32)
    out[..., :3] = v
    return out


# =====================================================================================================================================
# convs over two sources / an upsampled source / the 2x2 average
# =====================================================================================================================================
@dataclass(frozen=True)
class SrcView:
    H: int
    W: int
    C: int
    shift: int = 0
    cstride: int = 0                    # 0: C (dense)
    coff: int = 0

    @property
    def cs(self) -> int:
        return self.cstride or self.C


@dataclass(frozen=True)
class ConvCase:
    name: str
    s0: SrcView
    s1: Optional[SrcView]
    H: int                              # the conv's logical input
    W: int
    Cout: int
    k: int
    expect: Tuple[int, int, int, int, int, int]      # kernel, sched, bm, bn, simple, two - what cc_dev_conv_src reports
    stride: int = 1
    act: int = 1
    variant: int = 0
    phase_flags: Optional[int] = None
    ex_variant: Optional[int] = None    # variant of the cc_conv2d_ex launch over the materialised input that must give the same bits (None: no such launch)
    dtypes: Tuple[str, ...] = ("f16", "bf16")
    B: int = 2
    refused: bool = False

    @property
    def Cin(self) -> int:
        return self.s0.C + (self.s1.C if self.s1 else 0)

    @property
    def out_hw(self) -> Tuple[int, int]:
        p = self.k // 2
        return (self.H + 2 * p - self.k) // self.stride + 1, (self.W + 2 * p - self.k) // self.stride + 1

    @property
    def problem_id(self):
        return (self.s0, self.s1, self.H, self.W, self.Cout, self.k, self.stride, self.act, self.B)


def _conv_cases() -> List[ConvCase]:
    cs: List[ConvCase] = []
    G32 = (GENERIC, 0, 32, 32, 0, 0)                      # what the selector takes for a few tiles of 16-bit data: 32 x 32 tiles, four stages
    DIR = (DIRECT, 0, 128, 128, 0, 0)

    def both_acts(c: ConvCase) -> List[ConvCase]:
        return [c, replace(c, name=c.name + "-act0", act=0)]

    # ---- 1x1 over Concat(Upsample(a), b): the first conv of the neck's ELAN blocks.  M = 280: ragged against 128- and 256-pixel tiles
    for nm, s0, s1 in (("cat_up_1x1", SrcView(5, 7, 64, shift=1), SrcView(10, 14, 64)), ("cat_swap", SrcView(10, 14, 64), SrcView(5, 7, 64, shift=1))):
        base = ConvCase(nm, s0, s1, 10, 14, 64, 1, G32, ex_variant=V_PIX32_4)
        cs += both_acts(replace(base, name=nm + "-auto_c64"))
        for tag, pf, sched in (("sched0", 0, SCHED0), ("one_tile", 32, ONE_TILE), ("persist", 512, PERSIST)):
            cs += both_acts(replace(base, name=f"{nm}-phase_{tag}", Cout=256, variant=V_PHASE, phase_flags=pf, expect=(PHASE, sched, 256, 256, 0, 1), ex_variant=V_PHASE,
                                         dtypes=("f16", "bf16", "f16s")))
        cs += both_acts(replace(base, name=nm + "-direct", variant=V_DIRECT, expect=DIR, ex_variant=None, dtypes=("f16", "bf16", "f32")))
        cs += both_acts(replace(base, name=nm + "-generic", variant=V_GENERIC, expect=(GENERIC, 0, 128, 64, 0, 0), ex_variant=V_GENERIC, dtypes=("f16", "bf16", "f32", "f16s")))
        cs.append(replace(base, name=nm + "-direct_split", variant=V_DIRECT, expect=DIR, ex_variant=None, dtypes=("f16s",)))
    # ---- channel-slice sources, Cin = 32 + 40: the source boundary falls inside a 64-wide K step (and inside a tap's channels for 3x3)
    v0, v1 = SrcView(9, 11, 32, cstride=64, coff=16), SrcView(9, 11, 40, cstride=56, coff=8)
    for k in (1, 3):
        base = ConvCase(f"cat_views_{k}x{k}", v0, v1, 9, 11, 64, k, G32, ex_variant=V_PIX32_4)
        gen = (GENERIC, 0, 128, 64, 0, 0)
        cs += [replace(base, name=base.name + "-auto"), replace(base, name=base.name + "-auto-act0", act=0),
               replace(base, name=base.name + "-generic", variant=V_GENERIC, expect=gen, ex_variant=V_GENERIC, dtypes=("f16", "bf16", "f32")),
               replace(base, name=base.name + "-direct", variant=V_DIRECT, expect=DIR, ex_variant=None, dtypes=("f16", "bf16", "f32")),
               replace(base, name=base.name + "-split", variant=V_GENERIC, expect=gen, ex_variant=None, dtypes=("f16s",))]
    # ---- 3x3 over Concat(Upsample(a), b) on a 6 x 8 map: every window touches the zero padding
    u0, u1 = SrcView(3, 4, 32, shift=1), SrcView(6, 8, 16)
    for stride in (1, 2):
        base = ConvCase(f"cat_3x3_s{stride}", u0, u1, 6, 8, 32, 3, G32, stride=stride, ex_variant=V_PIX32_4)
        cs += [replace(base, name=base.name + "-auto"),
               replace(base, name=base.name + "-generic", variant=V_GENERIC, expect=(GENERIC, 0, 128, 32, 0, 0), ex_variant=V_GENERIC, dtypes=("f16", "bf16", "f32")),
               replace(base, name=base.name + "-generic-act0", act=0, variant=V_GENERIC, expect=(GENERIC, 0, 128, 32, 0, 0), ex_variant=V_GENERIC),
               replace(base, name=base.name + "-direct", variant=V_DIRECT, expect=DIR, ex_variant=None, dtypes=("f16", "bf16", "f32"))]
    # ---- one upsampled source: the non-simple loader without a second source
    base = ConvCase("up_only_3x3", u0, None, 6, 8, 32, 3, G32, ex_variant=V_PIX32_4)
    cs += [replace(base, name=base.name + "-auto"), replace(base, name=base.name + "-auto-act0", act=0),
           replace(base, name=base.name + "-generic", variant=V_GENERIC, expect=(GENERIC, 0, 128, 32, 0, 0), ex_variant=V_GENERIC, dtypes=("f16", "bf16", "f32")),
           replace(base, name=base.name + "-direct", variant=V_DIRECT, expect=DIR, ex_variant=None, dtypes=("f16", "bf16", "f32"))]
    # ---- ADown's first branch in one launch: 3x3 s2 over the 2x2 average of channels [64, 128) of a 9 x 11 map (the conv sees 8 x 10, gives 4 x 5)
    a0 = SrcView(9, 11, 64, shift=-1, cstride=128, coff=64)
    for cout in (64, 128):
        base = ConvCase(f"adown_c{cout}", a0, None, 8, 10, cout, 3, (ADOWN, 0, 128, cout, 0, 0), stride=2)
        cs += both_acts(base)
    r = ConvCase("adown-refused", a0, None, 8, 10, 64, 3, (-1,) * 6, stride=2, refused=True)
    cs += [replace(r, name="adown_f32-refused", dtypes=("f32",)), replace(r, name="adown_split-refused", dtypes=("f16s",)),
           replace(r, name="adown_cin32-refused", s0=SrcView(9, 11, 32, shift=-1, cstride=128, coff=64))]
    return cs


CONV_CASES: List[ConvCase] = _conv_cases()
assert len({c.name for c in CONV_CASES}) == len(CONV_CASES)


def materialise(c: ConvCase, xs: List[np.ndarray], dt: str) -> np.ndarray:
    """What the conv's loader sees: each source (B, H, W, C) nearest-upsampled by 2^shift (and cropped to the logical input) or, shift -1,
    its 2x2 stride-1 average rounded ONCE to the storage type; sources concatenated over channels -> (B, H, W, Cin) float64."""
    parts = []
    for s, x in zip([c.s0] + ([c.s1] if c.s1 else []), xs):
        if s.shift < 0:
            v = storage(avg2_ref(x), dt)
        else:
            v = np.repeat(np.repeat(x, 1 << s.shift, axis=1), 1 << s.shift, axis=2)[:, :c.H, :c.W]
        assert v.shape[1:3] == (c.H, c.W), (c.name, v.shape)
        parts.append(v)
    return np.concatenate(parts, axis=-1)


@functools.lru_cache(maxsize=16)
def conv_problem(pid, dt: str):
    """Sources (NHWC float64, storage values), weights / bias (float32), the materialised input (NCHW), y64 and A = sum |x||w| + |bias|;
    N(0,1) inputs and weights / sqrt(K) as tests/test_gpu_conv_epilogues._problem draws them.  dtype f16s keeps the float32 weights as
    they are and the reference multiplies by the value their two f16 planes hold (restart_check.split_values)."""
    s0, s1, H, W, Cout, k, stride, act, B = pid
    cin = s0.C + (s1.C if s1 else 0)
    g = torch.Generator().manual_seed(seed_of(repr(pid)) % (2 ** 31))
    t = TORCH_DT[dt]
    xs = [torch.randn(B, s.H, s.W, s.C, generator=g).to(t).double().numpy() for s in ([s0] + ([s1] if s1 else []))]
    w = torch.randn(Cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    if dt != "f16s":
        w = w.to(t).float()
    b = torch.randn(Cout, generator=g) * 0.1
    case = ConvCase("", s0, s1, H, W, Cout, k, (0,) * 6, stride=stride, act=act, B=B)
    x = torch.from_numpy(materialise(case, xs, dt)).permute(0, 3, 1, 2).contiguous()
    w_eff = rc.split_values([w])[0] if dt == "f16s" else w.double()
    y64 = rc.conv64_ex(x, w_eff, b, stride, 1, act)
    mag = rc.conv_abs64(x, w_eff, b, stride, 1)
    return xs, w, b, x, y64, mag
