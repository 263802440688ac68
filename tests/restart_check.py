"""Float64 restart checker for one conv launch of the 16-bit detector (helper module of tests/test_gpu_plan_restart.py and
tests/test_restart_check.py; not a conftest).

A conv launch of the 16-bit modes multiplies storage-rounded activations by the weights the library packed, accumulates in f32, runs the
epilogue (fma(acc, oscale, bias), SiLU, the residual add where the op has one) in f32 and rounds ONCE to the storage type
(clearcam_amd/csrc/conv_tile.h ``direct_tile``).  Recomputed from the launch's own inputs with the same effective weights in float64, the
unrounded result ``y64`` is the exact value the launch approximates: a faithful kernel returns ``round(y64)`` everywhere except where f32
accumulation noise - a tiny fraction of an ulp - straddles a rounding midpoint, and there it returns the other neighbour of ``y64``.

``check`` holds a launch to four bars (defaults in BARS, set from the MI355X measurements in tests/test_gpu_plan_restart.py):
  1. every element is one of the two storage values that bracket ``y64`` (chained units: within ``ulps`` quanta of ``y64``);
  2. the share of elements that differ from ``round(y64)`` is at most R;
  3. that share is at most R_cell in every (frame, 16x16-pixel, 32-channel) cell (plus a 3-element allowance for ragged edge cells) -
     one wrong tile hides in the whole-tensor rate, not here;
  4. the 99th percentile of the differing elements' distance from the rounding midpoint between the two candidates is at most D ulps:
     accumulation noise only flips values that sit almost on a midpoint, while a wrong rounding mode, bias, K-slab or tap spreads the
     flips over the whole [0, 0.5] ulp range.
Distances are measured in units of the storage type's quantum (ulp) at y64, floored at f16's smallest normal 2^-14 (FLOOR) for both
types: near zero the f32 accumulation noise of a K-term sum (~1e-7..1e-6 absolute on these layers) exceeds the spacing of small values,
so there an element counts as faithful within FLOOR of y64 and its midpoint distance is taken in units of FLOOR.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

TORCH_T = {"f16": torch.float16, "bf16": torch.bfloat16}
_FMT = {"f16": (11, -14), "bf16": (8, -126)}        # (significand bits, exponent of the smallest normal)

# Default bars: R (whole tensor), R_cell (per cell), D (p99 midpoint distance, ulps) of a single launch from the GPU's own inputs, about
# 3x the worst of 280 such launches measured on the MI355X (0.105 %, 0.59 %, 0.0009 ulp; tests/test_gpu_plan_restart.py's docstring).
BARS = {"R": 3e-3, "R_cell": 2e-2, "D": 3e-3}
FLOOR = 2.0 ** -14


# -- storage rounding --------------------------------------------------------------------------------------------------------
def quantum(x: torch.Tensor, sdt: str) -> torch.Tensor:
    """Spacing of the storage type's values around float64 x (the ulp of x's binade; the subnormal spacing below the smallest normal)."""
    p, emin = _FMT[sdt]
    _, e = torch.frexp(x.abs().to(torch.float64))   # |x| = m 2^e, m in [0.5, 1): leading bit 2^(e-1)
    e = torch.clamp(e - 1, min=emin)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - (p - 1))


def round_storage(x: torch.Tensor, sdt: str) -> torch.Tensor:
    """float64 -> nearest storage value (ties to even), as float64; one rounding (torch's own f64 -> f16 goes through f32)."""
    x = x.to(torch.float64)
    q = quantum(x, sdt)
    return torch.round(x / q) * q                   # power-of-two scaling: exact; torch.round = half to even


def bracket(y64: torch.Tensor, sdt: str):
    """The two storage values lo <= y64 <= hi (equal when y64 is one)."""
    q = quantum(y64, sdt)
    return torch.floor(y64 / q) * q, torch.ceil(y64 / q) * q, q


# -- effective weights -------------------------------------------------------------------------------------------------------
def controlled(w: torch.Tensor, sdt: str) -> torch.Tensor:
    """cc_round_weights: the controlled rounding cc_yolo_finalize applies to a one-plane conv (held to LowPrecOracle.q_feedback on the
    host by tests/test_abi_and_host.py), float32 values."""
    from clearcam_amd import _lib
    wn = np.ascontiguousarray(w.detach().to(torch.float32).numpy())
    out = np.empty(wn.size, np.float32)
    co, ci, k = wn.shape[0], wn.shape[1], wn.shape[2]
    _lib.check(_lib.lib().cc_round_weights({"f16": 1, "bf16": 2}[sdt], _lib.ptr(wn), co, ci, k, _lib.ptr(out)))
    return torch.from_numpy(out.reshape(wn.shape))


def split_values(ws: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """The value two f16 planes hold for convs PACKED TOGETHER (yolo.hip pack_convs, split = 1): one power of two 2^e over all of them,
    putting the largest magnitude in [2^14, 2^15); hi = f16(w 2^e), lo = f16(w 2^e - hi) (the difference is exact in f32); the epilogue's
    oscale = 2^-e is exact.  Float64 results."""
    mx = max(float(w.abs().max()) for w in ws)
    e = 14 - (math.frexp(mx)[1] - 1) if mx > 0 and math.isfinite(mx) else 0
    out = []
    for w in ws:
        vs = w.to(torch.float32) * (2.0 ** e)
        hi = vs.to(torch.float16).to(torch.float32)
        lo = (vs - hi).to(torch.float16).to(torch.float32)
        out.append((hi.double() + lo.double()) * (2.0 ** -e))
    return out


def effective_weights(ws: Sequence[torch.Tensor], sdt: str, split: bool) -> List[torch.Tensor]:
    """The float64 values a launch multiplies by, for the tensors packed into it (e.g. [cv1, cv2] of a RepNCSP)."""
    if split:
        return split_values(ws)
    return [controlled(w, sdt).double() for w in ws]


def f16h_split(name: str, k: int, size: str = "c") -> bool:
    """Does dtype "f16h" carry this conv as two planes?  yolo.hip cc_yolo_create / Builder::pconv: every conv of block <= split_all_last
    (the stem conv: 0; "e": 1) and the 1x1 convs of block <= split_1x1_last (the backbone: 9; "e": 29)."""
    blk = int(name.split(".")[2])
    all_last, one_last = (1, 29) if size == "e" else (0, 9)
    return blk <= all_last or (k == 1 and blk <= one_last)


# -- the reference ------------------------------------------------------------------------------------------------------------
def conv64(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int = 1, groups: int = 1, act: bool = True,
           res: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Storage-rounded input (NCHW) times effective weights, accumulated in float64, then bias, SiLU and the residual in float64: y64,
    NOT rounded.  Products of two <= 22-bit significands are exact in float64 and the sums carry ~1e-16 relative error."""
    y = F.conv2d(x.to(torch.float64), w.to(torch.float64), None if b is None else b.to(torch.float64), stride=stride,
                 padding=w.shape[-1] // 2, groups=groups)
    if act:
        y = y * torch.sigmoid(y)
    if res is not None:
        y = y + res.to(torch.float64)
    return y


GELU_C0, GELU_C1 = 0.7978845608028654, 0.044715     # clearcam_amd/csrc/conv_tile.h activate<T, 2>: 0.5 x (1 + tanh(C0 (x + C1 x^3)))


def pads_for(H: int, W: int, k: int, stride: int, pad: int, Ho: int, Wo: int):
    """(top, bottom, left, right) zero padding that a ConvP with `pad` and an explicit Ho x Wo reads (conv_params, net_common.h): `pad`
    rows / columns before the input, whatever the last window needs behind it (negative: trailing rows no window reaches)."""
    return pad, (Ho - 1) * stride + k - pad - H, pad, (Wo - 1) * stride + k - pad - W


def _conv_padded(x, w, stride, groups, pad4):
    t, b, l, r = pad4
    return F.conv2d(F.pad(x, (l, r, t, b)), w, None, stride=stride, padding=0, groups=groups)


def conv64_ex(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int = 1, groups: int = 1, act: int = 0,
              slope: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, pad4=None) -> torch.Tensor:
    """conv64 with every epilogue of ConvP (common.h), in the kernels' order, all in float64 and NOT rounded: explicit zero padding per
    side (pad4 = (top, bottom, left, right); None = k // 2 all round), groups, bias, then act 1 SiLU / 2 tanh-GELU / 3 PReLU with
    slope[channel], then the residual (NCHW, same grid as the output), then act 4's ReLU."""
    k = w.shape[-1]
    pad4 = (k // 2,) * 4 if pad4 is None else pad4
    y = _conv_padded(x.to(torch.float64), w.to(torch.float64), stride, groups, pad4)
    if b is not None:
        y = y + b.to(torch.float64).view(1, -1, 1, 1)
    if act == 1:
        y = y * torch.sigmoid(y)
    elif act == 2:
        y = 0.5 * y * (1.0 + torch.tanh(GELU_C0 * (y + GELU_C1 * y * y * y)))
    elif act == 3:
        y = torch.where(y > 0, y, slope.to(torch.float64).view(1, -1, 1, 1) * y)
    if res is not None:
        y = y + res.to(torch.float64)
    if act == 4:
        y = torch.clamp(y, min=0.0)
    return y


def conv_abs64(x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], stride: int = 1, groups: int = 1,
               res: Optional[torch.Tensor] = None, pad4=None) -> torch.Tensor:
    """A = sum |x| |w| + |bias| + |res| per output element in float64: the magnitude an f32 evaluation's rounding errors scale with."""
    k = w.shape[-1]
    pad4 = (k // 2,) * 4 if pad4 is None else pad4
    a = _conv_padded(x.to(torch.float64).abs(), w.to(torch.float64).abs(), stride, groups, pad4)
    if b is not None:
        a = a + b.to(torch.float64).abs().view(1, -1, 1, 1)
    if res is not None:
        a = a + res.to(torch.float64).abs()
    return a


# -- the comparison -----------------------------------------------------------------------------------------------------------
def _cell_rates(flip: torch.Tensor):
    """(N, C, H, W) bool -> (flips, elements) per (frame, 32-channel, 16x16-pixel) cell."""
    N, Cc, H, W = flip.shape
    pc, ph, pw = (-Cc) % 32, (-H) % 16, (-W) % 16
    f = F.pad(flip.to(torch.float32), (0, pw, 0, ph, 0, pc))
    one = F.pad(torch.ones_like(flip, dtype=torch.float32), (0, pw, 0, ph, 0, pc))
    sh = (N, (Cc + pc) // 32, 32, (H + ph) // 16, 16, (W + pw) // 16, 16)
    return f.reshape(sh).sum((2, 4, 6)), one.reshape(sh).sum((2, 4, 6))


def check(gpu: torch.Tensor, y64: torch.Tensor, sdt: str, name: str = "", R: float = None, R_cell: float = None, D: float = None,
          ulps: Optional[float] = None, enforce: bool = True) -> Dict[str, float]:
    """Hold a launch's output `gpu` (NCHW, the storage values as float32 / float64) to its float64 reference `y64` (bars above; None =
    BARS).  ulps=None: bar 1 strict (one of the two bracketing values); a number: |gpu - y64| <= ulps quanta (chained units).
    Returns the statistics; with enforce=True a failed bar raises AssertionError naming `name`."""
    R = BARS["R"] if R is None else R
    R_cell = BARS["R_cell"] if R_cell is None else R_cell
    D = BARS["D"] if D is None else D
    assert gpu.shape == y64.shape, (name, tuple(gpu.shape), tuple(y64.shape))
    g = gpu.to(torch.float64)
    y = y64.to(torch.float64)
    lo, hi, q = bracket(y, sdt)
    r = round_storage(y, sdt)
    q = torch.clamp(q, min=FLOOR)
    finite = torch.isfinite(g)
    flip = (g != r) & finite
    dist_ulp = (g - y).abs() / q
    faithful = finite & ((g == lo) | (g == hi) | (dist_ulp < 1.0))
    mid = (lo + hi) * 0.5
    bd = ((y - mid).abs() / q)[flip]                # distance of y64 from the midpoint, in ulps, where the launch took the other side
    fc, nc = _cell_rates(flip)
    n = g.numel()
    st = {
        "n": n,
        "differ": float(flip.sum()) / n,
        "max_cell": float((fc / nc).max()),
        "cell_excess": float((fc - (R_cell * nc + 3)).max()),
        "p99_boundary": float(torch.quantile(bd.float(), 0.99)) if bd.numel() else 0.0,
        "not_faithful": int((~faithful).sum()),
        "max_ulp": float(dist_ulp[finite].max()) if bool(finite.any()) else float("inf"),
        "nonfinite": int((~finite).sum()),
    }
    if enforce:
        assert_bars(st, name, R, R_cell, D, ulps)
    return st


def assert_bars(st: Dict[str, float], name: str = "", R: float = None, R_cell: float = None, D: float = None,
                ulps: Optional[float] = None) -> None:
    """The assertions of `check` on statistics it returned (with the same R_cell: cell_excess is relative to it)."""
    R = BARS["R"] if R is None else R
    R_cell = BARS["R_cell"] if R_cell is None else R_cell
    D = BARS["D"] if D is None else D
    if ulps is None:
        assert st["not_faithful"] == 0, (name, "elements neither of the two storage values that bracket y64 (nor within FLOOR)", st)
    else:
        assert st["nonfinite"] == 0 and st["max_ulp"] <= ulps, (name, f"elements further than {ulps} ulps from y64", st)
    assert st["differ"] <= R, (name, f"share differing from round(y64) above {R}", st)
    assert st["cell_excess"] <= 0, (name, f"a 16x16x32 cell differs on more than {R_cell} of its elements", st)
    assert st["p99_boundary"] <= D, (name, f"flips away from the rounding midpoints (p99 above {D} ulp)", st)


def fmt(name: str, st: Dict[str, float]) -> str:
    return (f"{name:44s} n {st['n']:>10d}  differ {100 * st['differ']:.3f} %  max cell {100 * st['max_cell']:.2f} %  "
            f"p99 midpoint dist {st['p99_boundary']:.4f} ulp  max {st['max_ulp']:.3f} ulp")
