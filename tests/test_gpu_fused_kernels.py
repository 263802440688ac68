"""The fused RepNCSP kernels and the fused letterbox + stem kernel, ONE launch per check through cc_dev_csp / cc_dev_stem
(clearcam_amd/csrc/dev_fused.hip), against float64.

Cases, inputs and references: tests/fused_cases.py (held on the CPU by tests/test_fused_cases_host.py).

RepNCSP (csp_fused_kernel with resident and with streamed weights, csp_tile_kernel), per case:
  (a) stage by stage against float64, each stage from the GPU's OWN previous stage (csp_fused_kernel's dbg dumps), so that a rounding flip
      upstream cannot excuse a later stage: [a | b] from x, t from the dumped a, [u | b] from the dumped a and t, out from the dumped
      [u | b].  restart_check.check, bar 1 strict; R / R_cell / D = restart_check.BARS, the residual stage u with the D of
      tests/test_gpu_conv_epilogues.py (its residual epilogues).  The dumps are whole images (every tile dumps its inner pixels), so t
      is compared on EVERY pixel against the 3x3 of the dumped a with zero padding - border pixels included: a halo pixel outside the
      image that holds SiLU(bias) instead of zero fails here, on the stage that is wrong.
  (b) bit for bit against the four conv launches the kernel replaces, on the same packed weights (cc_dev_csp variant 4: launch_conv four
      times, as Builder::csp_branch lays them out): every dump and the output.
  (c) kernel against kernel: every kernel the case's width / split has returns the same bits (dumps too, where it has them), and
      *choice names the kernel the case asked for.
  Outside the output view every element is still NaN (for the t dump: the view's upper hid channels too), and so is the guard image
  behind the output.
Letterbox + stem (stem_fused_kernel: Cout 16 / 32 / 64, small / BIG scratch, staged / direct source loads, uint8 / float32 frames,
uniform / ragged, split weights), per case: the output against the float64 reference with restart_check.BARS, bar 1 strict; NaN
outside the output view; a ragged batch equals each of its frames' uniform launch bit for bit.

Measured on the MI355X (docs/measurement.md, "Fused multi-conv kernels, one launch each"): no element of 261 checked tensors outside the
two storage values around y64 (furthest 0.503 ulp); RepNCSP stages R at most 0.208 % (one element of 480), R_cell 0.42 % (3.12 % = one
element of a 32-element edge cell, inside the 3-element allowance), D 0.0023 ulp on ab / t / out and 0.0031 ulp on the residual stage u;
the stem R 0.031 %, R_cell 0.07 %, D 0.0012 ulp; every dump and output bit for bit the four launches and the other kernels.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_cases as fc
import restart_check as rc
from clearcam_amd import _lib
from test_gpu_conv_epilogues import BARS as RES_BARS

pytestmark = pytest.mark.gpu
NAN = float("nan")
STAGE_BARS = {"ab": rc.BARS, "t": rc.BARS, "u": RES_BARS, "out": rc.BARS}


def _err() -> str:
    return _lib.lib().cc_last_error().decode(errors="replace")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


# ---- RepNCSP ---------------------------------------------------------------------------------------------------------------------------
class CspRun:
    """One case on the device: the input in its NaN-padded buffer, the five convs as host arrays."""

    def __init__(self, c: fc.CspCase):
        self.c = c
        w, b, _ = fc.csp_weights(c.hid, c.dt, c.split)
        self.w = [np.ascontiguousarray(w[n].numpy()) for n in fc.CONV_NAMES]
        self.b = [np.ascontiguousarray(b[n].numpy()) for n in fc.CONV_NAMES]
        self.wp = (C.c_void_p * 5)(*[a.ctypes.data for a in self.w])
        self.bp = (C.c_void_p * 5)(*[a.ctypes.data for a in self.b])
        xcs, xco = c.x_view
        buf = torch.full((c.B, c.H, c.W, xcs), NAN, dtype=torch.float64)
        buf[..., xco:xco + c.C2] = fc.csp_input(c)
        self.xd = buf.to(fc.TORCH_DT[c.dt]).cuda()

    def launch(self, variant: int, dbg: int, want: int) -> torch.Tensor:
        """-> the output view (B, H, W, 2 hid) on the host, storage type; checks the return code, the choice and everything outside the view."""
        c = self.c
        ocs, oco = c.out_view
        out = torch.full((c.B + 1, c.H, c.W, ocs), NAN, dtype=fc.TORCH_DT[c.dt], device="cuda")     # one more image: the guard behind the output
        k = C.c_int(-1)
        torch.cuda.synchronize()
        code = _lib.lib().cc_dev_csp(fc.DTI[c.dt], c.split, c.hid, _lib.ptr(self.xd), *c.x_view, _lib.ptr(out), ocs, oco, c.B, c.H, c.W,
                                     self.wp, self.bp, variant, dbg, C.byref(k), None)
        tag = (c.name, fc.KERNEL_NAMES[want], f"dbg {dbg}")
        assert code == 0, (tag, _err())
        assert k.value == want, (tag, "ran", fc.KERNEL_NAMES[k.value], "not the kernel this case is about")
        o = out.cpu()
        assert bool(torch.isnan(o[c.B]).all()), (tag, "stores past the last image")
        assert bool(torch.isnan(o[:c.B, :, :, :oco]).all()) and bool(torch.isnan(o[:c.B, :, :, oco + c.C2:]).all()), (tag, "channels outside the output view were written")
        view = o[:c.B, :, :, oco:oco + c.C2]
        if dbg == 2:
            assert bool(torch.isnan(view[..., c.hid:]).all()), (tag, "the t dump wrote beyond its hid channels")
            view = view[..., :c.hid]
        assert bool(torch.isfinite(view).all()), (tag, "elements not written or not finite", int((~torch.isfinite(view)).sum()))
        return view.contiguous()


def _check_stage(c, kernel, stage, got_nhwc, y64):
    bars = STAGE_BARS[stage]
    st = rc.check(fc.nchw(got_nhwc.double()), y64, c.dt, enforce=False, **bars)
    print(f"{rc.fmt(f'csp {kernel} {stage:3s} {c.name}', st)}  not faithful {st['not_faithful']}")
    rc.assert_bars(st, f"{c.name} stage {stage} ({kernel})", ulps=None, **bars)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in fc.CSP_CASES])
def test_csp_stages_match_float64_and_kernels_agree(case):
    c = case
    run = CspRun(c)
    (v0, k0), others = c.variants[0], c.variants[1:]
    name0 = fc.KERNEL_NAMES[k0]
    ab, t, ub, out = (run.launch(v0, dbg, k0) for dbg in (1, 2, 3, 0))
    # (a) each stage from the GPU's own previous stage
    n = c.stage_images
    x = fc.nchw(fc.csp_input(c)[:n])
    a64, t64, ub64 = fc.nchw(ab[:n, ..., :c.hid].double()), fc.nchw(t[:n].double()), fc.nchw(ub[:n].double())
    _check_stage(c, name0, "ab", ab[:n], fc.stage_ab(c, x))
    _check_stage(c, name0, "t", t[:n], fc.stage_t(c, a64))
    _check_stage(c, name0, "u", ub[:n, ..., :c.hid], fc.stage_u(c, a64, t64))
    assert torch.equal(_bits(ub[..., c.hid:]), _bits(ab[..., c.hid:])), (c.name, "b of the [u | b] dump is not b of the [a | b] dump")
    _check_stage(c, name0, "out", out[:n], fc.stage_out(c, ub64))
    # (b) the four launches on the same packed weights
    for dbg, got, what in ((1, ab, "[a | b]"), (2, t, "t"), (3, ub, "[u | b]"), (0, out, "out")):
        ref = run.launch(fc.V_LAYERS, dbg, fc.LAYERS)
        diff = _bits(got) != _bits(ref)
        assert not bool(diff.any()), (c.name, name0, what, "differs from the four launches", int(diff.sum()), "first at (b, h, w, c)", diff.nonzero()[0].tolist())
    # (c) every other kernel of this width / split
    for v, k in others:
        dumps = ((1, ab, "[a | b]"), (2, t, "t"), (3, ub, "[u | b]")) if k != fc.TILE else ()
        for dbg, want, what in dumps + ((0, out, "out"),):
            diff = _bits(run.launch(v, dbg, k)) != _bits(want)
            assert not bool(diff.any()), (c.name, fc.KERNEL_NAMES[k], what, "differs from", name0, int(diff.sum()), "first at (b, h, w, c)", diff.nonzero()[0].tolist())
    print(f"csp reached {c.name}: " + ", ".join(fc.KERNEL_NAMES[k] for _, k in c.variants))


def test_launcher_rule_inside_one_process():
    """variant 0 under cc_dev_set("csp_tile"): the production rule picks csp_tile_kernel from 256 tiles on, and under mode 2 always."""
    L = _lib.lib()
    c = next(x for x in fc.CSP_CASES if x.name == "2x17x33-h32-f16-s0-views")
    big = next(x for x in fc.CSP_CASES if x.name == "3x160x320-h32-f16-s0")
    try:
        outs = []
        for mode, want in ((0, fc.RESIDENT), (1, fc.RESIDENT), (2, fc.TILE)):
            _lib.check(L.cc_dev_set(b"csp_tile", mode))
            outs.append(CspRun(c).launch(fc.V_AUTO, 0, want))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))
        _lib.check(L.cc_dev_set(b"csp_tile", 1))
        CspRun(big).launch(fc.V_AUTO, 0, fc.TILE)                    # 300 tiles of 16 x 32
    finally:
        _lib.check(L.cc_dev_set(b"csp_tile", -1))


# ---- letterbox + first conv ------------------------------------------------------------------------------------------------------------
def run_stem(frames_dev, f32, sizes, offsets, res, ragged, dt, cout):
    """-> (info, the output view (B, Ho, Wo, cout) on the host).  The view sits at channels [8, 8 + cout) of a (B + 1, Ho, Wo, cout + 16) NaN buffer."""
    sdt = "f16" if dt == "f16s" else dt
    B = len(sizes)
    nh, nw, py, px = fc.yo.letterbox_geometry(sizes[0][0], sizes[0][1], res)
    Ho, Wo = (nh + 2 * py) // 2, (nw + 2 * px) // 2
    ocs, oco = cout + 16, 8
    out = torch.full((B + 1, Ho, Wo, ocs), NAN, dtype=fc.TORCH_DT[sdt], device="cuda")
    w, b, _ = fc.stem_weights(cout, dt)
    wn, bn = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    hs, ws = np.array([s[0] for s in sizes], np.int32), np.array([s[1] for s in sizes], np.int32)
    off = np.array(offsets, np.int64)
    info = (C.c_int * 3)(-1, -1, -1)
    torch.cuda.synchronize()
    code = _lib.lib().cc_dev_stem(fc.DTI[sdt], int(dt == "f16s"), frames_dev, int(f32), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                  hs.ctypes.data_as(C.POINTER(C.c_int32)), ws.ctypes.data_as(C.POINTER(C.c_int32)), B, res, int(ragged),
                                  _lib.ptr(wn), _lib.ptr(bn), cout, _lib.ptr(out), ocs, oco, info, None)
    tag = (sizes, dt, cout, "ragged" if ragged else "uniform")
    assert code == 0, (tag, _err())
    o = out.cpu()
    assert bool(torch.isnan(o[B]).all()), (tag, "stores past the last image")
    assert bool(torch.isnan(o[:B, :, :, :oco]).all()) and bool(torch.isnan(o[:B, :, :, oco + cout:]).all()), (tag, "channels outside the output view were written")
    view = o[:B, :, :, oco:oco + cout].contiguous()
    assert bool(torch.isfinite(view).all()), (tag, "elements not written or not finite")
    return tuple(info), view


def _check_stem(name, got, y64, sdt):
    st = rc.check(fc.nchw(got.double()), y64, sdt, enforce=False, **rc.BARS)
    print(f"{rc.fmt('stem ' + name, st)}  not faithful {st['not_faithful']}")
    rc.assert_bars(st, name, ulps=None, **rc.BARS)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in fc.STEM_CASES])
def test_stem_matches_float64(case):
    c = case
    frames = fc.stem_frames(c.H, c.W, c.f32, c.B)
    nh, nw, py, px = c.letterboxed
    staging = fc.stem_tile_staging(c.H, c.W, c.res, c.f32, c.big)
    for i, dt in enumerate(fc.STEM_DTYPES):
        # uint8 frames start 0, 3 and 2 bytes into an aligned allocation: the staged dword loads see every alignment of the base pointer
        lead = 0 if c.f32 else (0, 3, 2)[i]
        raw = torch.from_numpy(frames).reshape(-1).view(torch.uint8)
        dev = torch.cat([torch.zeros(lead, dtype=torch.uint8), raw]).cuda()
        for cout in fc.STEM_COUTS:
            info, got = run_stem(_lib.ptr(dev), c.f32, [(c.H, c.W)] * c.B, [lead + b * c.H * c.W * 3 * (4 if c.f32 else 1) for b in range(c.B)],
                                 c.res, False, dt, cout)
            assert info == (nh + 2 * py, nw + 2 * px, int(c.big)), (c.name, info)
            _check_stem(f"{c.name} {dt} c{cout}", got, fc.stem_reference(frames, c.res, cout, dt), "f16" if dt == "f16s" else dt)
    print(f"stem reached {c.name}: {'BIG' if c.big else 'small'} scratch, {sum(staging)} of {len(staging)} tiles staged, "
          f"{'float32' if c.f32 else 'uint8'} frames, uniform, Cout 16 / 32 / 64, f16 / bf16 / split")


@pytest.mark.parametrize("dt,cout", [("f16", 32), ("bf16", 16), ("f16s", 64)])
def test_ragged_stem_equals_each_frame_alone(dt, cout):
    """{64x64, 100x128, 135x240, 270x480} in one packed buffer: byte offsets = 0, 1, 2, 3 (mod 4), the base pointer 3 bytes into its
    allocation, the buffer ending at the last frame's last byte (the staging loads clamp to it)."""
    offs, total = fc.ragged_layout()
    frames = [fc.stem_frames(h, w, False, 1)[0] for h, w in fc.RAGGED_FRAMES]
    packed = np.zeros(3 + total, np.uint8)
    for f, o in zip(frames, offs):
        packed[3 + o:3 + o + f.size] = f.reshape(-1)
    dev = torch.from_numpy(packed).cuda()
    info, got = run_stem(C.c_void_p(dev.data_ptr() + 3), False, list(fc.RAGGED_FRAMES), offs, fc.RAGGED_RES, True, dt, cout)
    assert info == (64, 64, 1), info
    sdt = "f16" if dt == "f16s" else dt
    for b, (f, (h, w)) in enumerate(zip(frames, fc.RAGGED_FRAMES)):
        _check_stem(f"ragged frame {h}x{w} {dt} c{cout}", got[b:b + 1], fc.stem_reference(f[None], fc.RAGGED_RES, cout, dt), sdt)
        alone = torch.from_numpy(f.reshape(-1)).cuda()
        _, one = run_stem(_lib.ptr(alone), False, [(h, w)], [0], fc.RAGGED_RES, False, dt, cout)
        diff = _bits(got[b:b + 1]) != _bits(one)
        assert not bool(diff.any()), (h, w, dt, "the ragged launch differs from the frame's own uniform launch", int(diff.sum()))
    print(f"stem reached ragged {dt} c{cout}: BIG scratch, staged and direct tiles in one launch")
