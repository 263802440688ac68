"""Every conv route of the DETECTOR plans, ONE launch per case through cc_dev_conv_det, against float64 - and the proof that the cases
reach what the plans reach.

tests/test_gpu_conv_epilogues.py and tests/test_gpu_plan_routes.py do this for CLIP, AdaFace and BlazeFace; the detector differs in two
ways they do not cover.  Its default mode carries convs as TWO f16 weight planes, which changes the K loop of every kernel family, and
its RepNBottleneck adds a 16-bit residual that is the output buffer itself.  tests/test_gpu_plan_restart.py recomputes the shipped plan
in float64, but 640 x 640 at B = 64 has no ragged tile anywhere; mixed-resolution batches do.  The case table
(tests/detector_route_cases.py) puts each family on the smallest ragged shape.

(a) test_detector_route_case_matches_float64: the reference is restart_check.conv64_ex over storage-rounded inputs and the values the
    packed planes hold (restart_check.effective_weights).  16-bit outputs: restart_check.check, bar 1 strict, R / R_cell = rc.BARS, D per
    kind (below).  f32 outputs: test_gpu_conv_epilogues.f32_bound with K = Ktot, both planes counted.  Outputs start NaN with one spare
    image behind the batch and NaN channels around a slice; in-place cases start as the residual.
(b) test_every_detector_route_has_a_single_launch_case: YOLOv9-C at 640 with the route log on - one 1080 x 1920 frame, eight frames of
    four sizes through detect_frames, 64 frames of 640 x 640 - logs extended route keys (the eleven fields of epilogue_cases plus split,
    simple, two, cprw, ns); each must be reached by a case of epilogue_cases, glue_cases.CONV_CASES or detector_route_cases, or stand in
    detector_route_cases.MERGED with a covered key and a reason.  Launches that bypass launch_conv_chosen (the averaging ADown conv, the
    fused RepNCSP / stem / head-tail kernels, the pools) are not in the log; they have float64 tests of their own.

Measured on the MI355X: the comment above BARS and docs/measurement.md ("Detector conv routes against float64").
"""
import ctypes as C

import numpy as np
import pytest
import torch

import detector_route_cases as drc
import restart_check as rc
from clearcam_amd import _lib
from test_gpu_conv_epilogues import BARS as EPILOGUE_BARS, f32_bound

pytestmark = pytest.mark.gpu
NAN = float("nan")
NREC = _lib.ROUTE_REC_INTS

# D bars (p99 distance of the differing elements from the rounding midpoint, ulps): 3 x the worst measured on the MI355X against the
# float64 reference, per kind of case; R and R_cell are rc.BARS, bar 1 is strict.  The kernels are deterministic: the margin is for
# other seeds.  Measured over the 101 16-bit tests of this file (docs/measurement.md, "Detector conv routes against float64"), worst of
# each kind with the committed seeds, and in brackets with the seeds of an earlier draft of the table (same shapes, other inputs):
#   two planes                 p99 0.0040 ulp  (gen_3x3_64_80-act0, big256 / phase 3x3 192 -> 512)     [0.0055, the 3x3 192 -> 512 cases]
#                              differ 0.177 % (small9_3x3_256_40), cell 1.04 % (3x3 192 -> 512), max 0.504 ulp           -> rc.BARS hold
#   in-place 16-bit residual   p99 0.0086 ulp  (plan-g128x64_3-3x3-inplace16-2p; one plane: 0.0049 f16, 0.0000 bf16)      [0.0067, big128]
#                              differ 0.109 %, cell 1.04 % (big128_3x3_128_128-inplace16)                                -> rc.BARS hold
#   one plane, no residual     p99 0.0030 ulp  (plan-one_tile-3x3s2-1p, f16): the epilogue suite's D = 2.8e-2 stays
# In-place cases sit higher for the epilogue suite's reason: conv + N(0,1) residual puts many outputs near zero, where the f32
# accumulation noise of a K-term sum is a larger share of the output's quantum.  Each bar is 3 x the larger of the two figures.
D_TWO_PLANES = 1.65e-2                                 # 3 x 0.0055
D_INPLACE16 = 2.6e-2                                   # 3 x 0.0086


def bars_of(c: drc.DCase, dtype: str):
    d = D_INPLACE16 if c.res == "inplace16" else (D_TWO_PLANES if dtype == "f16s" else EPILOGUE_BARS["D"])
    return dict(R=rc.BARS["R"], R_cell=rc.BARS["R_cell"], D=d)


def run_case(c: drc.DCase, dtype: str):
    """Launch the case; (code, the eight ints of choice, NCHW result as float64, channels outside the output slice or None, the spare
    image, the problem)."""
    L = _lib.lib()
    t = rc.TORCH_T[drc.SDT[dtype]]
    prob = drc.problem(c.problem_id, dtype)
    x, w, b, res = prob[0], prob[1], prob[2], prob[3]
    Ho, Wo = c.out_hw
    xds = [s.permute(0, 2, 3, 1).contiguous().to("cuda", t) for s in prob[7]]
    guarded = torch.full((c.B + 1, Ho, Wo, c.ocs), NAN, dtype=torch.float32 if c.out_f32 else t, device="cuda")
    out = guarded[:c.B]
    resd = None
    if c.res == "inplace16":
        assert not c.out_f32
        out[..., c.out_coff:c.out_coff + c.Cout] = res.permute(0, 2, 3, 1).to(t)
        resd = out
    elif c.res == "storage":
        rcs = c.res_cstride or c.Cout
        resd = torch.full((c.B, Ho, Wo, rcs), NAN, dtype=t, device="cuda")
        resd[..., c.res_coff:c.res_coff + c.Cout] = res.permute(0, 2, 3, 1).to(t)
    else:
        assert c.res is None, c.res
    d = drc.desc_of(c, dtype)
    s0, s1 = drc.src_descs(c, xds[0].data_ptr(), xds[-1].data_ptr())
    wn, bn = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    choice = (C.c_int * 8)(*([-1] * 8))
    torch.cuda.synchronize()
    try:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", c.phase_flags))
        code = L.cc_dev_conv_det(C.byref(d), C.byref(s0), C.byref(s1) if s1 is not None else None, _lib.ptr(wn), _lib.ptr(bn), _lib.ptr(resd), _lib.ptr(out), choice, None)
    finally:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", -1))
    o = guarded.cpu()
    got = o[:c.B, ..., c.out_coff:c.out_coff + c.Cout].permute(0, 3, 1, 2).to(torch.float64)
    outside = torch.cat([o[:c.B, ..., :c.out_coff], o[:c.B, ..., c.out_coff + c.Cout:]], -1) if c.ocs != c.Cout else None
    return code, tuple(choice), got, outside, o[c.B], prob


PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in drc.CASES for dt in c.dtypes]


@pytest.mark.parametrize("case,dtype", PARAMS)
def test_detector_route_case_matches_float64(case, dtype):
    c = case
    code, choice, got, outside, spare, prob = run_case(c, dtype)
    y64, mag = prob[5], prob[6]
    assert code == 0, (c.name, _lib.lib().cc_last_error().decode(errors="replace"))
    assert choice == c.expect + c.ext, (c.name, "the selector ran", choice, "not the kernel this case is about", c.expect + c.ext)
    assert bool(torch.isnan(spare).all()), (c.name, "stores past the last output pixel")
    if outside is not None:
        assert bool(torch.isnan(outside).all()), (c.name, "channels outside the output slice were written")
    if c.out_f32:
        assert bool(torch.isfinite(got).all()), (c.name, "elements not written or not finite", int((~torch.isfinite(got)).sum()))
        kc = drc.replace(c, Cin=c.Cin // c.groups * c.planes)              # f32_bound counts K = k k Cin: the terms one output sums, both planes
        ratio = float(((got - y64).abs() / f32_bound(kc, drc.SDT[dtype], y64, mag)).max())
        print(f"{c.name + '-' + dtype:52s} route {choice}  f32 err/bound {ratio:.4f}")
        assert ratio <= 1.0, (c.name, "f32 output beyond 2 (K + 8) 2^-24 A", ratio)
    else:
        bars = bars_of(c, dtype)
        st = rc.check(got, y64, drc.SDT[dtype], enforce=False, **bars)
        print(f"{rc.fmt(c.name + '-' + dtype, st)}  route {choice}")
        rc.assert_bars(st, c.name, ulps=None, **bars)


# ---- (b) the plans' routes -----------------------------------------------------------------------------------------------------------------
def take_log():
    """Read and clear the route log: {extended route key: (B, H, W, Cin, Cout, Ho, Wo) of the first layer that logged it}."""
    cap = 1 << 12
    buf = (C.c_int * (cap * NREC))()
    out = {}
    n0, n1 = len(drc.ec.KEY_FIELDS), len(drc.ec.KEY_FIELDS) + 7
    while True:                                          # records that do not fit stay in the log for the next call
        n = C.c_int(0)
        _lib.check(_lib.lib().cc_route_log_take(buf, cap, C.byref(n)))
        got = min(n.value, cap)
        for r in np.frombuffer(buf, np.int32, got * NREC).reshape(got, NREC):
            out.setdefault(tuple(int(v) for v in r[:n0]) + tuple(int(v) for v in r[n1:]), tuple(int(v) for v in r[n0:n1]))
        if n.value <= cap:
            return out


MIXED_SIZES = ((360, 640), (480, 640), (720, 1280), (600, 800))     # network shapes 384 x 640 and 480 x 640 at res 640, four frames each


def detector_logs(dtype: str, sd):
    """{batch tag: log} of YOLOv9-C at res 640 over the three batches.  A plan is built at the first call with a shape and batch size: its
    launches run once eagerly and once under graph capture, and that is when they are logged (a graph replay calls no launcher)."""
    from clearcam_amd.yolov9 import YOLOv9
    L = _lib.lib()
    rng = np.random.default_rng(11)
    frame = lambda h, w: rng.integers(0, 256, (h, w, 3), dtype=np.uint8)       # noqa: E731
    m = YOLOv9("c", 640, state_dict=sd, dtype=dtype, device=0)
    logs = {}
    try:
        _lib.check(L.cc_dev_set(b"route_log", 1))
        take_log()
        m.detect_batch(frame(1080, 1920)[None])
        logs["B1_384x640"] = take_log()
        m.detect_frames([frame(h, w) for h, w in MIXED_SIZES * 2])
        logs["mixed8"] = take_log()
        m.detect_batch(rng.integers(0, 256, (64, 640, 640, 3), dtype=np.uint8))
        logs["B64_640x640"] = take_log()
    finally:
        _lib.check(L.cc_dev_set(b"route_log", 0))
        take_log()
        m.close()
    return logs


@pytest.fixture(scope="module")
def yolo_c_weights():
    from clearcam_amd.weights import synthetic_yolov9_state_dict
    return synthetic_yolov9_state_dict("c")             # routes do not depend on weight values


@pytest.mark.parametrize("dtype", ["f16h", "f16s", "bf16"])
def test_every_detector_route_has_a_single_launch_case(dtype, yolo_c_weights):
    covered = drc.covered_keys()
    for k, (to, why) in drc.MERGED.items():
        assert to in covered and why.strip() and drc.merge_is_legal(k, to), ("a merged key needs a covered key it may merge into and a reason", k)
    logs = detector_logs(dtype, yolo_c_weights)
    assert all(logs.values()), (dtype, "no conv launch was logged", {b: len(v) for b, v in logs.items()})
    missing, direct, merged = {}, set(), set()
    for tag, log in logs.items():
        for key, shape in log.items():
            if key in covered:
                direct.add(key)
            elif key in drc.MERGED:
                merged.add(key)
            else:
                missing.setdefault(key, (tag,) + shape)
    lines = [f"  {drc.describe(k)}   first in {v[0]}: B,H,W,Cin,Cout,Ho,Wo = {v[1:]}" for k, v in sorted(missing.items())]
    print(f"detector {dtype}: " + ", ".join(f"{tag}: {len(log)} keys" for tag, log in logs.items())
          + f"; {len(direct)} covered directly, {len(merged)} merged, {len(missing)} missing")
    assert not missing, f"detector {dtype}: {len(missing)} route keys no single-launch case reaches:\n" + "\n".join(lines)
    assert set(logs["B1_384x640"]) != set(logs["B64_640x640"]), (dtype, "the log is the same at B = 1 and at B = 64: it does not see the selector")
