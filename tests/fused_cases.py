"""Case tables, input makers and float64 references of tests/test_gpu_fused_kernels.py, held on the CPU by tests/test_fused_cases_host.py
(helper module; not a conftest).  NumPy / PyTorch-CPU only.

The kernels are the three that keep intermediates on chip: csp_fused_kernel (clearcam_amd/csrc/csp_fused.hip; weights resident in LDS or
streamed), csp_tile_kernel (csp_tile.hip) and stem_fused_kernel (detect.hip).  A case is ONE launch through cc_dev_csp / cc_dev_stem
(csrc/dev_fused.hip) and names the kernel variant it must reach.

Inputs as tests/glue_cases.py draws them: N(0,1) rounded to the storage type, seeds from the case name.  Weights are N(0,1) / sqrt(K)
float32 (the entries pack them as the detector does; the references multiply by restart_check.effective_weights of them).  Biases are
N(0, 0.5) - NOT small: SiLU(bias) where a halo pixel outside the image must be zero moves the border outputs by many ulps.  Buffers are
wider than the view wherever a case has a view, NaN in every channel outside it.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

import restart_check as rc
from oracle import yolov9_oracle as yo

TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
DTI = {"f16": 1, "bf16": 2}
# *choice of cc_dev_csp (clearcam_amd/csrc/kernels.h CspKernel, clearcam_hip.h CC_DEV_CSP_LAYERS) and its `variant` argument
RESIDENT, STREAMED, TILE, LAYERS = 0, 1, 2, 3
KERNEL_NAMES = ["fused-resident", "fused-streamed", "tile", "four launches"]
V_AUTO, V_FUSED, V_STREAM, V_TILE, V_LAYERS = range(5)


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode()) % (2 ** 31)


def storage(t: torch.Tensor, sdt: str) -> torch.Tensor:
    return rc.round_storage(t, sdt)


# =====================================================================================================================================
# RepNCSP
# =====================================================================================================================================
@dataclass(frozen=True)
class CspCase:
    B: int
    H: int
    W: int
    hid: int = 32
    dt: str = "f16"
    split: int = 0
    views: bool = False                 # x_cstride = 2 hid + 16, x_coff = 8; out_cstride = 2 hid + 8, out_coff = 8
    why: str = ""

    @property
    def name(self) -> str:
        return f"{self.B}x{self.H}x{self.W}-h{self.hid}-{self.dt}-s{self.split}" + ("-views" if self.views else "")

    @property
    def C2(self) -> int:
        return 2 * self.hid

    @property
    def x_view(self) -> Tuple[int, int]:
        return (self.C2 + 16, 8) if self.views else (self.C2, 0)

    @property
    def out_view(self) -> Tuple[int, int]:
        return (self.C2 + 8, 8) if self.views else (self.C2, 0)

    @property
    def variants(self) -> Tuple[Tuple[int, int], ...]:
        """(variant argument, the kernel it must report), the first one csp_fused_kernel as the launcher picks it by width."""
        if self.hid == 64 or self.split:
            v = [(V_FUSED, STREAMED)]
        else:
            v = [(V_FUSED, RESIDENT), (V_STREAM, STREAMED)]
        if self.hid == 32 and self.split != 1:
            v.append((V_TILE, TILE))
        return tuple(v)

    @property
    def stage_images(self) -> int:
        """Images whose stages are held to float64 (check (a)): all, or image 0 where the float64 convs would take more than a few seconds."""
        return self.B if self.B * self.H * self.W * self.hid * self.hid <= 3 * 80 * 160 * 32 * 32 else 1


# csp_fused tiles are 8 x 16, csp_tile tiles 16 x 32; every shape runs on every kernel its width / split has
_SHAPES = [
    (1, 3, 5, False, "the image is smaller than the halo"),
    (2, 8, 16, False, "one csp_fused tile per image, every halo pixel outside the image"),
    (2, 16, 32, False, "one csp_tile tile per image, every halo pixel outside the image"),
    (2, 9, 17, True, "a one-pixel ragged csp_fused tile on both axes; channel views"),
    (2, 17, 33, True, "a one-pixel ragged csp_tile tile on both axes; channel views"),
    (1, 7, 15, False, "one pixel short of a tile"),
    (1, 24, 48, False, "a centre csp_fused tile whose whole halo is inside the image"),
    (1, 48, 96, False, "a centre csp_tile tile whose whole halo is inside the image"),
]
_BIG_FUSED = (3, 80, 160, False, "300 csp_fused tiles on at most 256 persistent blocks, 100 per image: two tiles per block, the walk crosses images")
_BIG_TILE = (3, 160, 320, False, "300 csp_tile tiles on at most 256 persistent blocks, 100 per image")
_SMALL = [_SHAPES[0], _SHAPES[3], _SHAPES[4], _SHAPES[6]]


def _csp_cases() -> List[CspCase]:
    cs: List[CspCase] = []

    def add(shapes, **kw):
        cs.extend(CspCase(B, H, W, views=v, why=why, **kw) for B, H, W, v, why in shapes)

    add(_SHAPES + [_BIG_FUSED, _BIG_TILE], hid=32, dt="f16", split=0)
    add(_SMALL + [_BIG_FUSED], hid=32, dt="bf16", split=0)
    add(_SMALL + [_SHAPES[1]], hid=64, dt="f16", split=0)
    add(_SMALL, hid=64, dt="bf16", split=0)
    add(_SMALL, hid=32, dt="f16", split=1)
    add(_SMALL, hid=64, dt="f16", split=1)
    add(_SMALL + [_BIG_TILE], hid=32, dt="f16", split=2)
    add(_SMALL + [_BIG_FUSED], hid=64, dt="f16", split=2)
    return cs


CSP_CASES: List[CspCase] = _csp_cases()
assert len({c.name for c in CSP_CASES}) == len(CSP_CASES)
CONV_NAMES = ("cv1", "cv2", "rep", "bott", "cv3")


@functools.lru_cache(maxsize=None)
def csp_weights(hid: int, dt: str, split: int):
    """The five convs (float32 OIHW, bias) and the float64 values the launches multiply by.  Shared by every shape of a (hid, dt, split)."""
    g = torch.Generator().manual_seed(seed_of(f"csp|{hid}|{dt}|{split}"))
    C2 = 2 * hid
    shapes = {"cv1": (hid, C2, 1, 1), "cv2": (hid, C2, 1, 1), "rep": (hid, hid, 3, 3), "bott": (hid, hid, 3, 3), "cv3": (C2, C2, 1, 1)}
    w = {n: torch.randn(*s, generator=g) / (s[1] * s[2] * s[3]) ** 0.5 for n, s in shapes.items()}
    b = {n: torch.randn(s[0], generator=g) * 0.5 for n, s in shapes.items()}
    if split:
        # One crafted weight per conv puts the largest magnitudes of cv1 | cv2 (as drawn: [0.25, 0.5)), the two 3x3 convs and cv3 in four
        # different binades, so that the packs' four 2^-e output scales all differ: a kernel that applies one conv's scale to another's
        # accumulator is off by a power of two.  (As drawn, three of the four split cases had os12 == os3.)
        w["rep"][0, 0, 1, 1], w["bott"][0, 0, 1, 1], w["cv3"][0, 0, 0, 0] = 0.75, 3.0, 1.5
    s1, s3 = split != 0, split == 1
    e12 = rc.effective_weights([w["cv1"], w["cv2"]], dt, s1)               # packed together: one scale for both under split
    eff = {"cv12": torch.cat(e12, 0), "rep": rc.effective_weights([w["rep"]], dt, s3)[0], "bott": rc.effective_weights([w["bott"]], dt, s3)[0],
           "cv3": rc.effective_weights([w["cv3"]], dt, s1)[0]}
    return w, b, eff


@functools.lru_cache(maxsize=None)
def csp_input(c: CspCase) -> torch.Tensor:
    """(B, H, W, 2 hid) float64 storage values."""
    g = torch.Generator().manual_seed(seed_of(f"x|{c.B}x{c.H}x{c.W}|{c.hid}|{c.dt}"))
    return storage(torch.randn(c.B, c.H, c.W, c.C2, generator=g).double(), c.dt)


def nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).contiguous()


# The stages, NCHW float64 in, y64 (NOT rounded) out: each takes the storage values of the stage before it.
def stage_ab(c: CspCase, x: torch.Tensor) -> torch.Tensor:
    _, b, eff = csp_weights(c.hid, c.dt, c.split)
    return rc.conv64_ex(x, eff["cv12"], torch.cat([b["cv1"], b["cv2"]]), act=1)


def stage_t(c: CspCase, a: torch.Tensor) -> torch.Tensor:
    _, b, eff = csp_weights(c.hid, c.dt, c.split)
    return rc.conv64_ex(a, eff["rep"], b["rep"], act=1)                      # zero padding of a: k // 2 all round


def stage_u(c: CspCase, a: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    _, b, eff = csp_weights(c.hid, c.dt, c.split)
    return rc.conv64_ex(t, eff["bott"], b["bott"], act=1, res=a)             # a + SiLU(conv3x3 t): one rounding, of the sum


def stage_out(c: CspCase, ub: torch.Tensor) -> torch.Tensor:
    _, b, eff = csp_weights(c.hid, c.dt, c.split)
    return rc.conv64_ex(ub, eff["cv3"], b["cv3"], act=1)


def csp_reference(c: CspCase, x: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The whole block in float64 (NCHW), rounding to storage exactly where the kernel does; storage values of ab, t, ub, out."""
    r = lambda y: storage(y, c.dt)
    ab = r(stage_ab(c, x))
    a, b = ab[:, :c.hid], ab[:, c.hid:]
    t = r(stage_t(c, a))
    ub = torch.cat([r(stage_u(c, a, t)), b], 1)
    return {"ab": ab, "t": t, "ub": ub, "out": r(stage_out(c, ub))}


def expected_choice(c: CspCase, variant: int, dbg: int = 0, tile_mode: int = 1) -> int:
    """choose_csp (csp_fused.hip) restated: what cc_dev_csp_choice must answer."""
    if variant == V_LAYERS:
        return LAYERS
    stream = variant == V_STREAM
    mode = tile_mode if variant == V_AUTO else 2 if variant == V_TILE else 0
    tiles32 = c.B * ((c.H + 15) // 16) * ((c.W + 31) // 32)
    tile_ok = c.hid == 32 and c.split in (0, 2) and (c.dt == "f16" or c.split == 0)
    if mode != 0 and not stream and not dbg and (tiles32 >= 256 or mode == 2) and tile_ok:
        return TILE
    return RESIDENT if c.hid == 32 and not stream and c.split == 0 else STREAMED


# =====================================================================================================================================
# letterbox + first conv
# =====================================================================================================================================
SCRATCH_SMALL, SCRATCH_BIG = 128 * 72 * 2, 256 * 72 * 2          # stem_fused_kernel's source-byte stage (detect.hip)


@dataclass(frozen=True)
class StemCase:
    H: int
    W: int
    res: int
    f32: bool = False
    letterboxed: Tuple[int, int, int, int] = (0, 0, 0, 0)        # nh, nw, pad_y, pad_x the issue's table states
    need: Optional[int] = None          # stem_needs_big's figure in bytes, where the table states it
    big: bool = False
    staged: str = "all"                 # tiles that stage their source bytes in LDS: "all" | "some" | "none"
    B: int = 2
    why: str = ""

    @property
    def name(self) -> str:
        return f"{self.H}x{self.W}-res{self.res}" + ("-f32" if self.f32 else "-u8")


STEM_CASES: List[StemCase] = [
    StemCase(64, 64, 64, letterboxed=(64, 64, 0, 0), why="identity taps"),
    StemCase(23, 37, 64, letterboxed=(40, 64, 12, 0), why="upscale; row bytes = 3 mod 4; padding rows"),
    StemCase(37, 23, 64, letterboxed=(64, 40, 0, 12), why="upscale; padding columns"),
    StemCase(100, 128, 64, letterboxed=(50, 64, 7, 0), need=14144, why="2x downscale; small scratch, staged"),
    StemCase(187, 301, 96, letterboxed=(60, 96, 2, 0), need=34020, big=True, why="3.1x downscale; BIG scratch, staged; odd row alignment"),
    StemCase(135, 240, 64, letterboxed=(36, 64, 14, 0), need=48384, big=True, why="3.75x downscale; the bound exceeds BIG: each tile decides for itself"),
    StemCase(270, 480, 64, letterboxed=(36, 64, 14, 0), big=True, staged="none", why="7.5x downscale; no tile fits: direct loads"),
    StemCase(23, 37, 64, f32=True, letterboxed=(40, 64, 12, 0), staged="none", why="float32 frames are never staged"),
    StemCase(100, 128, 64, f32=True, letterboxed=(50, 64, 7, 0), staged="none", why="float32 frames, downscale"),
]
STEM_DTYPES = ("f16", "bf16", "f16s")                            # f16s: f16 storage, two weight planes (the low-plane MFMA)
STEM_COUTS = (16, 32, 64)
RAGGED_FRAMES = ((64, 64), (100, 128), (135, 240), (270, 480))   # all letterbox to 64 x 64 at res 64
RAGGED_RES = 64


def stem_need_bytes(H: int, W: int, nh: int, nw: int) -> int:
    """stem_needs_big's figure (detect.hip): bytes the source rectangle of a 33 x 33 patch can take in the stage."""
    nr, nc = (33 * H + nh - 1) // nh + 2, (33 * W + nw - 1) // nw + 2
    return nr * ((nc * 3 + 6) // 4) * 4


def stem_tile_staging(H: int, W: int, res: int, f32: bool, big: bool) -> List[bool]:
    """Per 16 x 16 output tile: does stem_fused_kernel stage the tile's source bytes in LDS?  Its own rule, restated from the oracle's tables."""
    nh, nw, pad_y, pad_x = yo.letterbox_geometry(H, W, res)
    Hn, Wn = nh + 2 * pad_y, nw + 2 * pad_x
    xlo, xhi, _ = yo.interp_axis_tables(W, nw)
    ylo, yhi, _ = yo.interp_axis_tables(H, nh)
    out = []
    for oy0 in range(0, Hn // 2, 16):
        for ox0 in range(0, Wn // 2, 16):
            Y0, X0 = 2 * oy0 - 1, 2 * ox0 - 1
            yy0, yy1 = max(Y0 - pad_y, 0), min(Y0 + 32 - pad_y, nh - 1)
            xx0, xx1 = max(X0 - pad_x, 0), min(X0 + 32 - pad_x, nw - 1)
            some = yy0 <= yy1 and xx0 <= xx1
            if not some:
                out.append(False)
                continue
            nrows, rowbytes = int(yhi[yy1]) - int(ylo[yy0]) + 1, (int(xhi[xx1]) - int(xlo[xx0]) + 1) * 3
            out.append(not f32 and nrows * ((rowbytes + 6) // 4) * 4 <= (SCRATCH_BIG if big else SCRATCH_SMALL))
    return out


def stem_frames(H: int, W: int, f32: bool, B: int) -> np.ndarray:
    """(B, H, W, 3) BGR frames: uint8 noise, or float32 in [0, 255] off the integers."""
    g = np.random.default_rng(seed_of(f"frames|{H}x{W}|{int(f32)}"))
    if f32:
        return g.uniform(0.0, 255.0, (B, H, W, 3)).astype(np.float32)
    return g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def stem_weights(cout: int, dt: str):
    """(w float32 (cout,3,3,3), bias, the float64 values the launch multiplies by)."""
    g = torch.Generator().manual_seed(seed_of(f"stem|{cout}|{dt}"))
    w = torch.randn(cout, 3, 3, 3, generator=g) / 27 ** 0.5
    b = torch.randn(cout, generator=g) * 0.5
    return w, b, rc.effective_weights([w], "f16" if dt == "f16s" else dt, dt == "f16s")[0]


def stem_network_input(frames: np.ndarray, res: int, sdt: str) -> torch.Tensor:
    """The oracle's letterbox (bit-exact to preprocess_kernel: tests/test_gpu_yolo.py test_letterbox_uint8_bit_exact), BGR -> RGB, / 255 in
    float32, rounded to the storage type: (B, 3, Hn, Wn) float64 storage values."""
    lb = np.stack([yo.letterbox(f, res) for f in frames])
    v = (lb[..., ::-1].astype(np.float32) / np.float32(255.0)).astype(np.float32)
    return nchw(storage(torch.from_numpy(np.ascontiguousarray(v)).double(), sdt))


def stem_reference(frames: np.ndarray, res: int, cout: int, dt: str) -> torch.Tensor:
    """y64 (B, cout, Hn / 2, Wn / 2), NOT rounded: conv 3x3 stride 2 pad 1 of the network input, bias, SiLU."""
    w, b, eff = stem_weights(cout, dt)
    return rc.conv64(stem_network_input(frames, res, "f16" if dt == "f16s" else dt), eff, b, stride=2)


def ragged_layout() -> Tuple[List[int], int]:
    """Byte offsets of RAGGED_FRAMES in one packed buffer, = 0, 1, 2, 3 (mod 4), and the buffer's size: it ends at the last frame's last byte."""
    offs, at = [], 0
    for i, (h, w) in enumerate(RAGGED_FRAMES):
        while at % 4 != i % 4:
            at += 1
        offs.append(at)
        at += h * w * 3
    return offs, at
