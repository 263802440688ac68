"""The kernels between the convs and the two-source conv loaders, ONE launch per case through the cc_dev_* entries, against float64.

Cases, inputs and references: tests/glue_cases.py (held on the CPU by tests/test_glue_cases_host.py).
  pools, CBFuse  grid inputs: bit-equal to round_storage(y64) (the f32 cast for f32 storage), the reported PoolKernel is the case's,
                 channels outside the output view still NaN.  Normal inputs: one of the two storage values that bracket y64; f32 storage:
                 |got - y64| <= 3 * 2^-24 * sum |taps| for the averages and CBFuse, max pools exact.
  affine         16-bit: one of the two storage values that bracket y64; f32: |got - y64| <= 2^-23 (|x s| + |t|) (two f32 roundings).
  face pre       bit-equal to the numpy float32 evaluation rounded once to the storage type, channels 3 .. cpad exactly 0.
  convs          as test_gpu_conv_epilogues.test_conv_epilogue_matches_float64: restart_check.check with that file's BARS, its
                 f32_bound for f32 storage, the reported choice equal to the case's.  The generic and eight-wave cases also equal, bit for
                 bit, a single-source launch of the same kernel over the materialised input (upsample and concat done on the host).
  refused        a nonzero return, an error text, the output still all NaN.

Every output buffer carries one more image than the launch writes (NaN before and after): a store past the last row shows there.

Measured on the MI355X (docs/measurement.md, "Glue kernels and two-source loaders, one launch each"): no grid element differs; the f32
averages reach 0.18 of their bar, CBFuse 0.61, affine 0.68; the 16-bit convs R 0.195 %, R_cell 0.31 %, D 0.0070 ulp (D stays at the
epilogue suite's 2.8e-2), the f32 convs 0.0103 of their bound; every generic and eight-wave case is bit for bit the single-source launch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import glue_cases as gc
import restart_check as rc
from clearcam_amd import _lib
from test_gpu_conv_epilogues import BARS, f32_bound

pytestmark = pytest.mark.gpu
TDT = gc.TORCH_DT
NAN = float("nan")


def _dev(a: np.ndarray, dt: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(TDT[dt]).to("cuda")


def _err() -> str:
    return _lib.lib().cc_last_error().decode(errors="replace")


def _split_view(o: torch.Tensor, coff: int, C: int):
    """(values of the view as float64 numpy, the channels outside it)."""
    return o[..., coff:coff + C].double().numpy(), torch.cat([o[..., :coff], o[..., coff + C:]], -1)


def _assert_storage_result(name, got, y64, mag, dt, kind, exact):
    """grid: bit-equal to round_storage(y64).  normal: 16-bit one of the two bracketing values; f32 exact (max) or within 3 * 2^-24 * mag."""
    assert np.isfinite(got).all(), (name, "elements not written or not finite", int((~np.isfinite(got)).sum()))
    if kind != "normal" or (dt == "f32" and exact):
        want = gc.storage(y64, dt)
        bad = got != want
        print(f"{name:40s} {dt:5s} {kind:8s} differing {int(bad.sum())} of {got.size}")
        assert not bad.any(), (name, dt, kind, "not round_storage(y64)", int(bad.sum()), float(np.abs(got - want).max()))
    elif dt == "f32":
        ratio = float((np.abs(got - y64) / np.maximum(3 * gc.U24 * mag, 1e-300)).max())
        print(f"{name:40s} {dt:5s} {kind:8s} err / (3 * 2^-24 * sum |taps|) {ratio:.4f}")
        assert ratio <= 1.0, (name, "f32 result beyond 3 * 2^-24 * sum |taps|", ratio)
    else:
        lo, hi, _ = rc.bracket(torch.from_numpy(y64), dt)
        g = torch.from_numpy(got)
        ok = (g == lo) | (g == hi)
        off = float((g != rc.round_storage(torch.from_numpy(y64), dt)).double().mean())
        print(f"{name:40s} {dt:5s} {kind:8s} not the nearest {100 * off:.4f} %  outside the bracket {int((~ok).sum())}")
        assert bool(ok.all()), (name, dt, "elements that are neither storage value around y64", int((~ok).sum()))


# ---- pools -----------------------------------------------------------------------------------------------------------------------------
def run_pool(c: gc.PoolCase, dt: str, x: np.ndarray):
    L = _lib.lib()
    Ho, Wo = c.out_hw
    xd = _dev(gc.in_nan_buffer(x, c.ics, c.in_coff), dt)
    out = torch.full((c.B + 1, Ho, Wo, c.ocs), NAN, dtype=TDT[dt], device="cuda")      # one more image: the guard behind the output
    k = C.c_int(-1)
    torch.cuda.synchronize()
    try:
        if c.pool_rows is not None:
            _lib.check(L.cc_dev_set(b"pool_rows", c.pool_rows))
        code = L.cc_dev_pool(gc.DTI[dt], _lib.ptr(xd), c.ics, c.in_coff, _lib.ptr(out), c.ocs, c.out_coff, c.B, c.H, c.W, c.C, Ho, Wo, c.k,
                             c.stride, c.pad, c.mode, C.byref(k), None)
    finally:
        if c.pool_rows is not None:
            _lib.check(L.cc_dev_set(b"pool_rows", -1))
    return code, k.value, out.cpu()


POOL_PARAMS = [pytest.param(c, dt, kind, id=f"{c.name}-{dt}-{kind}") for c in gc.POOL_CASES if not c.refused for dt in c.dtypes
               for kind in ((c.grid_kind,) if c.negative else ("grid", "normal"))]


@pytest.mark.parametrize("case,dt,kind", POOL_PARAMS)
def test_pool_matches_float64(case, dt, kind):
    c = case
    x, y64, mag = gc.pool_problem(c, dt, kind)
    code, kernel, o = run_pool(c, dt, x)
    assert code == 0, (c.name, _err())
    assert kernel == c.expect, (c.name, "ran", gc.POOL_NAMES[kernel], "not the kernel this case is about", gc.POOL_NAMES[c.expect])
    got, outside = _split_view(o[:c.B], c.out_coff, c.C)
    assert bool(torch.isnan(outside).all()), (c.name, "channels outside the output view were written")
    assert bool(torch.isnan(o[c.B]).all()), (c.name, "stores past the last output row")
    _assert_storage_result(c.name, got, y64, mag, dt, kind, exact=c.mode == 1)


# ---- CBFuse ----------------------------------------------------------------------------------------------------------------------------
def run_fuse(c: gc.FuseCase, dt: str, xs):
    L = _lib.lib()
    bufs = [_dev(gc.in_nan_buffer(x, cs, co), dt) for x, (cs, co) in zip(xs, c.views)]
    out = torch.full((c.B + 1, c.Ho, c.Wo, c.out_view[0]), NAN, dtype=TDT[dt], device="cuda")
    ptrs = (C.c_void_p * c.n)(*[b.data_ptr() for b in bufs])
    arr = lambda v: (C.c_int * c.n)(*v)
    torch.cuda.synchronize()
    code = L.cc_dev_fuse(gc.DTI[dt], c.n, ptrs, arr([c.in_hw(i)[0] for i in range(c.n)]), arr([c.in_hw(i)[1] for i in range(c.n)]),
                         arr([v[0] for v in c.views]), arr([v[1] for v in c.views]), arr(c.shifts), _lib.ptr(out), c.out_view[0], c.out_view[1],
                         c.B, c.Ho, c.Wo, c.C, None)
    return code, out.cpu()


FUSE_PARAMS = [pytest.param(c, dt, kind, id=f"{c.name}-{dt}-{kind}") for c in gc.FUSE_CASES if not c.refused for dt in c.dtypes for kind in ("grid", "normal")]


@pytest.mark.parametrize("case,dt,kind", FUSE_PARAMS)
def test_fuse_matches_float64(case, dt, kind):
    c = case
    xs, y64, mag = gc.fuse_problem(c, dt, kind)
    code, o = run_fuse(c, dt, xs)
    assert code == 0, (c.name, _err())
    got, outside = _split_view(o[:c.B], c.out_view[1], c.C)
    assert bool(torch.isnan(outside).all()), (c.name, "channels outside the output view were written")
    assert bool(torch.isnan(o[c.B]).all()), (c.name, "stores past the last output row")
    _assert_storage_result(c.name, got, y64, mag, dt, kind, exact=False)


# ---- affine, face preprocessing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,ch", gc.AFFINE_SHAPES)
@pytest.mark.parametrize("dt", gc.ALL3)
def test_affine_matches_float64(rows, ch, dt):
    L = _lib.lib()
    x, scale, shift, y64, A = gc.affine_problem(rows, ch, dt)
    xd, sd, td = _dev(x, dt), torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda()
    out = torch.full((rows, ch), NAN, dtype=TDT[dt], device="cuda")
    torch.cuda.synchronize()
    assert L.cc_dev_affine(gc.DTI[dt], _lib.ptr(xd), _lib.ptr(out), _lib.ptr(sd), _lib.ptr(td), rows * ch, ch, None) == 0, _err()
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    if dt == "f32":
        ratio = float((np.abs(got - y64) / (2.0 ** -23 * A)).max())
        print(f"affine {rows}x{ch} f32  err / (2^-23 (|x s| + |t|)) {ratio:.4f}")
        assert ratio <= 1.0, ratio
    else:
        lo, hi, _ = rc.bracket(torch.from_numpy(y64), dt)
        g = torch.from_numpy(got)
        ok = (g == lo) | (g == hi)
        print(f"affine {rows}x{ch} {dt}  outside the bracket {int((~ok).sum())}  not the nearest {int((g != rc.round_storage(torch.from_numpy(y64), dt)).sum())}")
        assert bool(ok.all()), int((~ok).sum())
    inplace = xd.clone()                                   # the plan runs it in place
    assert L.cc_dev_affine(gc.DTI[dt], _lib.ptr(inplace), _lib.ptr(inplace), _lib.ptr(sd), _lib.ptr(td), rows * ch, ch, None) == 0, _err()
    assert torch.equal(inplace.cpu(), out.cpu())


@pytest.mark.parametrize("f32_frames", (False, True), ids=("u8", "f32frames"))
@pytest.mark.parametrize("dt", gc.ALL3)
def test_face_pre_is_bit_exact(dt, f32_frames):
    L = _lib.lib()
    frames, cpad = gc.face_frames(f32_frames), 8
    want = torch.from_numpy(gc.face_pre_ref(frames, cpad)).to(TDT[dt])
    fd = torch.from_numpy(frames).cuda()
    out = torch.full(tuple(want.shape), NAN, dtype=TDT[dt], device="cuda")
    torch.cuda.synchronize()
    assert L.cc_dev_face_pre(gc.DTI[dt], _lib.ptr(fd), int(f32_frames), _lib.ptr(out), frames.shape[0], cpad, None) == 0, _err()
    o = out.cpu()
    assert bool((o[..., 3:] == 0).all()), "padding channels are not zero"
    bad = o.double() != want.double()
    assert not bool(bad.any()), (dt, int(bad.sum()))


# ---- convs over two sources ------------------------------------------------------------------------------------------------------------
def run_conv(c: gc.ConvCase, dt: str):
    """Launch the case; returns (code, choice, NCHW result as float64, the device output, problem).  The output buffer holds one more image
    than the launch writes; it must stay NaN."""
    L = _lib.lib()
    prob = gc.conv_problem(c.problem_id, dt)
    xs, w, b = prob[0], prob[1], prob[2]
    views = [c.s0] + ([c.s1] if c.s1 else [])
    bufs = [_dev(gc.in_nan_buffer(x, s.cs, s.coff), dt) for s, x in zip(views, xs)]
    descs = [_lib.SrcDesc(buf.data_ptr(), s.H, s.W, s.cs, s.coff, s.C, s.shift) for s, buf in zip(views, bufs)]
    Ho, Wo = c.out_hw
    guarded = torch.full((c.B + 1, Ho, Wo, c.Cout), NAN, dtype=TDT[dt], device="cuda")
    out = guarded[:c.B]
    d = _lib.ConvDesc(gc.DTI[dt], c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, 1, c.act, -1, 0, 0, 0, 0, 0, 0, 0, 0, c.variant)
    wn, bn = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    choice = (C.c_int * 6)(*([-1] * 6))
    torch.cuda.synchronize()
    try:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", c.phase_flags))
        code = L.cc_dev_conv_src(C.byref(d), C.byref(descs[0]), C.byref(descs[1]) if c.s1 else None, _lib.ptr(wn), _lib.ptr(bn), _lib.ptr(out), choice, None)
    finally:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", -1))
    assert bool(torch.isnan(guarded[c.B]).all()), (c.name, "stores past the last output pixel")
    return code, tuple(choice), out.cpu().permute(0, 3, 1, 2).to(torch.float64), out, prob


def run_materialised(c: gc.ConvCase, dt: str, prob):
    """The same conv over the materialised input through a single-source entry, forced onto the same kernel; (choice or None, device output)."""
    L = _lib.lib()
    _, w, b, x, _, _ = prob
    xd = x.permute(0, 2, 3, 1).contiguous().to(TDT[dt]).to("cuda")
    Ho, Wo = c.out_hw
    out = torch.full((c.B, Ho, Wo, c.Cout), NAN, dtype=TDT[dt], device="cuda")
    wn, bn = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    torch.cuda.synchronize()
    try:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", c.phase_flags))
        if dt == "f16s":                                   # cc_conv2d_ex has no split weights; cc_conv2d_nhwc packs as the detector does
            _lib.check(L.cc_conv2d_nhwc(3, _lib.ptr(xd), c.B, c.H, c.W, c.Cin, _lib.ptr(wn), _lib.ptr(bn), c.Cout, c.k, c.stride, 1, c.act, _lib.ptr(out), c.ex_variant, None))
            return None, out
        d = _lib.ConvDesc(gc.DTI[dt], c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, 1, c.act, -1, 0, 0, 0, 0, 0, 0, 0, 0, c.ex_variant)
        choice = (C.c_int * 4)(-1, -1, -1, -1)
        _lib.check(L.cc_conv2d_ex(C.byref(d), _lib.ptr(xd), _lib.ptr(wn), _lib.ptr(bn), None, None, _lib.ptr(out), choice, None))
        return tuple(choice), out
    finally:
        if c.phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", -1))


CONV_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in gc.CONV_CASES if not c.refused for dt in c.dtypes]


@pytest.mark.parametrize("case,dt", CONV_PARAMS)
def test_two_source_conv_matches_float64(case, dt):
    c = case
    code, choice, got, out_dev, prob = run_conv(c, dt)
    y64, mag = prob[4], prob[5]
    assert code == 0, (c.name, _err())
    assert choice == c.expect, (c.name, "the selector ran", choice, "not the kernel this case is about", c.expect)
    if dt == "f32":
        assert bool(torch.isfinite(got).all()), (c.name, "elements not written or not finite", int((~torch.isfinite(got)).sum()))
        ratio = float(((got - y64).abs() / f32_bound(c, dt, y64, mag)).max())
        print(f"{c.name + '-' + dt:52s} route {choice}  f32 err/bound {ratio:.4f}")
        assert ratio <= 1.0, (c.name, "f32 output beyond 2 (2K + 8) 2^-24 A", ratio)
    else:
        sdt = "f16" if dt == "f16s" else dt
        st = rc.check(got, y64, sdt, enforce=False, **BARS)
        print(f"{rc.fmt(c.name + '-' + dt, st)}  route {choice}")
        rc.assert_bars(st, c.name, ulps=None, **BARS)
    if c.ex_variant is not None and (dt != "f16s" or c.k == 1):
        ex_choice, ex_out = run_materialised(c, dt, prob)
        if ex_choice is not None:
            assert ex_choice == c.expect[:4], (c.name, "the single-source launch ran", ex_choice, "not", c.expect[:4])
        same = torch.equal(out_dev.view(torch.int16 if dt != "f32" else torch.int32), ex_out.view(torch.int16 if dt != "f32" else torch.int32))
        assert same, (c.name, dt, "bits differ from the single-source launch over the materialised input",
                      int((out_dev.float() != ex_out.float()).sum()))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refused_cases_leave_the_output_untouched():
    L = _lib.lib()
    n = 0
    for c in gc.POOL_CASES:
        for dt in (c.dtypes if c.refused else ()):
            code, _, o = run_pool(c, dt, gc.pool_problem(c, dt, "grid")[0])
            assert code != 0 and _err() and bool(torch.isnan(o).all()), (c.name, code, _err())
            n += 1
    for c in gc.FUSE_CASES:
        for dt in (c.dtypes if c.refused else ()):
            code, o = run_fuse(c, dt, gc.fuse_problem(c, dt, "grid")[0])
            assert code != 0 and _err() and bool(torch.isnan(o).all()), (c.name, code, _err())
            n += 1
    for c in gc.CONV_CASES:
        for dt in (c.dtypes if c.refused else ()):
            code, choice, got, _, _ = run_conv(c, dt)
            assert code != 0 and _err() and bool(torch.isnan(got).all()), (c.name, code, choice, _err())
            n += 1
    assert n >= 6
    xd = torch.zeros(16, 12, dtype=torch.float16, device="cuda")             # 12 channels are no whole number of 16-byte chunks
    out = torch.full((16, 12), NAN, dtype=torch.float16, device="cuda")
    sd = torch.ones(12, device="cuda")
    assert L.cc_dev_affine(1, _lib.ptr(xd), _lib.ptr(out), _lib.ptr(sd), _lib.ptr(sd), 16 * 12, 12, None) != 0 and _err()
    assert bool(torch.isnan(out).all())
