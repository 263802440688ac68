"""Every conv epilogue the CLIP, AdaFace and BlazeFace plans reach, ONE launch per case through cc_conv2d_ex_route, against float64.

The per-kernel tests of tests/test_gpu_yolo.py run "bias + SiLU or nothing, dense 16-bit output" only; the other plans share the
selector and the kernels but use tanh-GELU, PReLU with per-channel slopes, ReLU after a 16-bit residual, an f32 residual that is the f32
output itself, f32 output, channel-slice views, asymmetric padding through Ho / Wo and a stride-2 1x1.  Each kernel family has its own
copy of that logic (conv_tile.h stage_tile / direct_tile, conv_persist.hip epilogue16 / epilogue32, conv_wave.hip, conv_direct.hip,
conv_tile64.hip, conv_stream.hip).  The case table (tests/epilogue_cases.py) forces each family onto each epilogue it can run; the entry
reports the kernel that ran and a case that lands anywhere else fails.

Inputs and weights are representable in the storage type, so the float64 reference (restart_check.conv64_ex) is the exact value a launch
approximates.
  16-bit outputs: restart_check.check, bar 1 strict (every element one of the two storage values around y64), R / R_cell = rc.BARS,
                  D = 3x the worst measured here (BARS below).
  f32 outputs:    |got - y64| <= 2 (K + 8) 2^-24 A, A = sum |x||w| + |bias| + |res| in float64 per element: the bound of a K-term f32
                  sum in any order, doubled for the matrix unit's unspecified internal rounding; 2K for f32 storage (the products round
                  too), plus 16 * 2^-24 |y64| for expf / tanhf where f32 storage runs act 1 / 2.
Output buffers start as NaN (a kernel that stores nothing, or not everywhere, fails; a channel-slice case must leave the channels
outside its slice NaN); in-place cases (f32, and the detector's 16-bit one) start as the residual.

Measured on the MI355X: the comment above BARS and docs/measurement.md ("Conv epilogues against float64").
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import epilogue_cases as ec
import restart_check as rc
from clearcam_amd import _lib

pytestmark = pytest.mark.gpu
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DTI = {"f32": 0, "f16": 1, "bf16": 2}
U24 = 2.0 ** -24

# Bars.  rc.BARS (R 0.3 %, R_cell 2 %, D 0.003 ulp) were measured on SiLU launches of the detector.  Measured here against the float64
# reference on the MI355X over all 267 16-bit tests (docs/measurement.md, "Conv epilogues against float64"), worst case of each kind:
#   R       0.126 % of a tensor   (direct_1x1_28_32, act 2, f16)                            -> rc.BARS["R"] holds
#   R_cell  1.04 % of a cell      (big_3x3_odd, act 2, f16; K = 1728)                       -> rc.BARS["R_cell"] holds
#   D       0.0094 ulp            (big_3x3_odd with the 16-bit residual, f16, on every wide kernel; bf16: 0.0073, the persistent kernel's
#                                  stride-2 residual; tile64 0.0047, generic 32 x 32 0.0050, wave / weights-stationary 0.0036)
# D exceeds the detector's bar where the epilogue puts many outputs near zero (conv + N(0,1) residual, PReLU with small slopes): there
# the f32 accumulation noise of a K-term sum of O(1) magnitude (~2^-24) is a larger share of the output's quantum.  Bar 1 stays strict
# on every case (each element is one of the two storage values around y64; max 0.509 ulp).  D = 3 x 0.0094.  R and R_cell stay.
# The detector's epilogues added later (SiLU on every family, SiLU + a 16-bit residual that is the output buffer; 64 tests): R 0.118 %,
# R_cell 1.04 %, D 0.0051 ulp (big_3x3_odd-tile128-silu_inplace16, f16) - under the figures above.
# The plans' K loops at their own depth added later (epilogue_cases._DEEP_ROUTES, K up to 4608 where 1728 was the deepest measured; 62
# 16-bit tests; docs/measurement.md, "Plan conv routes at their own K depth"): bar 1 holds on every case (max 0.520 ulp), R 0.276 %
# (adaface-deep-g32_6-3x3s2_c256-act0_res16, f16), R_cell 0.49 %, D 0.0194 ulp (adaface-deep-g128x64_3-3x3_c256-act0_res16, bf16; f16
# worst 0.0106) - under the bars, which stay.  f32 outputs there: err / bound at most 0.0008 (K = 1024 with the in-place residual).
# f32 outputs: the largest err / bound was 0.0163 (the persistent kernel's M = 33 300, K = 64 GEMM with the in-place residual).
BARS = dict(R=rc.BARS["R"], R_cell=rc.BARS["R_cell"], D=2.8e-2)

PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in ec.CASES for dt in c.dtypes]


@functools.lru_cache(maxsize=12)
def _problem(ref_id, dtype, res_kind):
    """Inputs of a case (NCHW, representable in the storage type) and its float64 reference; shared by the cases that differ only in the
    kernel they force and never modified."""
    B, Cin, H, W, Cout, k, stride, groups, act, pad, (Ho, Wo), _ = ref_id
    g = torch.Generator().manual_seed(1000 + (Cin * 31 + Cout * 7 + k * 3 + H + act) % 997)
    t = TDT[dtype]
    x = torch.randn(B, Cin, H, W, generator=g).to(t).float()
    w = (torch.randn(Cout, Cin // groups, k, k, generator=g) / (Cin // groups * k * k) ** 0.5).to(t).float()
    b = torch.randn(Cout, generator=g) * 0.1
    slope = (torch.rand(Cout, generator=g) * 0.5 - 0.1) if act == 3 else None          # distinct per channel, both signs
    res = None
    if res_kind is not None:
        res = torch.randn(B, Cout, Ho, Wo, generator=g)
        if res_kind == "storage":
            res = res.to(t).float()
    pad4 = rc.pads_for(H, W, k, stride, pad, Ho, Wo)
    y64 = rc.conv64_ex(x, w, b, stride, groups, act, slope, res, pad4)
    mag = rc.conv_abs64(x, w, b, stride, groups, res, pad4)
    return x, w, b, slope, res, y64, mag


def run_case(c: ec.Case, dtype: str):
    """Launch the case; returns (rc, the eight ints of choice, NCHW result as float64, channels outside the output slice as a tensor or None)."""
    L = _lib.lib()
    t = TDT[dtype]
    Ho, Wo = c.out_hw
    res_kind = None if c.res is None else ("storage" if c.res in ("storage", "inplace16") else "f32")
    x, w, b, slope, res, y64, mag = _problem(c.ref_id, dtype, res_kind)
    xd = x.permute(0, 2, 3, 1).contiguous().to("cuda", t)
    out_f32 = c.out_f32 or dtype == "f32"
    out = torch.full((c.B, Ho, Wo, c.ocs), float("nan"), dtype=torch.float32 if out_f32 else t, device="cuda")
    resd, rcs = None, c.res_cstride or c.Cout
    if c.res == "inplace":
        assert out_f32 and c.ocs == c.Cout and rcs == c.Cout
        out.copy_(res.permute(0, 2, 3, 1))
        resd = out
    elif c.res == "inplace16":                         # the 16-bit residual IS the output buffer (the detector's RepNBottleneck)
        assert not out_f32 and c.ocs == c.Cout and rcs == c.Cout
        out.copy_(res.permute(0, 2, 3, 1))
        resd = out
    elif c.res is not None:
        resd = torch.full((c.B, Ho, Wo, rcs), float("nan"), dtype=torch.float32 if c.res == "f32" else t, device="cuda")
        resd[..., c.res_coff:c.res_coff + c.Cout] = res.permute(0, 2, 3, 1).to(resd.dtype)
    d = _lib.ConvDesc(DTI[dtype], c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.groups, c.act, c.pad, c.Ho, c.Wo,
                      int(c.out_f32), c.out_cstride, c.out_coff, int(c.res in ("f32", "inplace")), c.res_cstride, c.res_coff, c.variant)
    wn, bn = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    sn = None if slope is None else np.ascontiguousarray(slope.numpy())
    choice = (C.c_int * _lib.CONV_CHOICE_INTS)(*([-1] * _lib.CONV_CHOICE_INTS))      # kernel, sched, bm, bn, simple, two, cprw, ns
    torch.cuda.synchronize()
    try:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", c.phase_flags))
        # cc_conv2d_ex_route: cc_conv2d_ex's launch, reporting the K loop too (cc_conv2d_ex itself keeps its four-int choice)
        code = L.cc_conv2d_ex_route(C.byref(d), _lib.ptr(xd), _lib.ptr(wn), _lib.ptr(bn), _lib.ptr(sn), _lib.ptr(resd), _lib.ptr(out), choice, None)
    finally:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", -1))
    o = out.cpu()
    got = o[..., c.out_coff:c.out_coff + c.Cout].permute(0, 3, 1, 2).to(torch.float64)
    outside = torch.cat([o[..., :c.out_coff], o[..., c.out_coff + c.Cout:]], -1) if c.ocs != c.Cout else None
    return code, tuple(choice), got, outside, y64, mag


def f32_bound(c: ec.Case, dtype: str, y64, mag):
    K = c.k * c.k * c.Cin
    bound = 2.0 * ((2 * K if dtype == "f32" else K) + 8) * U24 * mag
    if dtype == "f32" and c.act in (1, 2):
        bound = bound + 16 * U24 * y64.abs()
    return bound


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_conv_epilogue_matches_float64(case, dtype):
    c = case
    code, choice, got, outside, y64, mag = run_case(c, dtype)
    assert code == 0, (c.name, _lib.lib().cc_last_error().decode(errors="replace"))
    assert choice[:4] == c.expect, (c.name, "the selector ran", choice, "not the kernel this case is about", c.expect)
    if c.ext is not None:                              # the deep-K cases name their K loop too: simple, two, cprw, ns
        assert choice == c.expect + c.ext, (c.name, "the selector ran", choice, "not the route this case is about", c.expect + c.ext)
    if outside is not None:
        assert bool(torch.isnan(outside).all()), (c.name, "channels outside the output slice were written")
    if c.out_f32 or dtype == "f32":
        assert bool(torch.isfinite(got).all()), (c.name, "elements not written or not finite", int((~torch.isfinite(got)).sum()))
        bound = f32_bound(c, dtype, y64, mag)
        ratio = float(((got - y64).abs() / bound).max())
        print(f"{c.name + '-' + dtype:52s} route {choice}  f32 err/bound {ratio:.4f}")
        assert ratio <= 1.0, (c.name, "f32 output beyond 2 (K + 8) 2^-24 A", ratio)
    else:
        st = rc.check(got, y64, dtype, enforce=False, **BARS)
        print(f"{rc.fmt(c.name + '-' + dtype, st)}  route {choice}")
        rc.assert_bars(st, c.name, ulps=None, **BARS)


def test_forced_kernel_refuses_an_epilogue_it_cannot_run():
    """The streaming 1x1 kernel has no PReLU and the 3x3 64 -> 64 tile kernel no GELU: forcing them is an error, not another kernel."""
    base = next(c for c in ec.CASES if c.name == "stream_256_256_ragged-gelu")
    t64 = next(c for c in ec.CASES if c.name == "tile64_ragged-res16")
    for c in (ec.replace(base, act=3), ec.replace(t64, act=2)):
        code, choice, got, _, _, _ = run_case(c, "f16")
        assert code != 0 and bool(torch.isnan(got).all()), (c.name, code, choice)
