"""CPU checks of tests/fused_cases.py: the float64 references of the fused RepNCSP and letterbox-stem kernels against torch float32, the
stem cases' geometry against what the case table states, choose_csp through cc_dev_csp_choice, and every refusal of cc_dev_csp /
cc_dev_stem - none of which needs a device (a refusal must come back as an argument error, -22, before the first HIP call)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fused_cases as fc
import restart_check as rc
from clearcam_amd import _lib

U24 = 2.0 ** -24
FAKE_X, FAKE_OUT = 0x10000, 0x20000                     # 16-byte aligned addresses that are never dereferenced: no launch happens here
EINVAL = -22

HOST_CSP = [c for c in fc.CSP_CASES if c.B * c.H * c.W <= 3 * 80 * 160]
CSP_PARAMS = [pytest.param(c, id=c.name) for c in HOST_CSP]
STEM_PARAMS = [pytest.param(c, id=c.name) for c in fc.STEM_CASES]


def _f32_bound(x, w, b, y64, stride=1, res=None):
    """Bound of a float32 evaluation (any summation order, float32 products of float32-rounded weights, expf) around y64: 2 (2K + 8) 2^-24
    sum |x||w| through SiLU (slope at most 1.1) plus 16 * 2^-24 |y64|, as tests/test_gpu_conv_epilogues.f32_bound has it for f32 storage."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    mag = rc.conv_abs64(x, w, b, stride, 1, res)
    return 1.1 * 2.0 * (2 * K + 8) * U24 * mag + 16 * U24 * y64.abs()


def _silu_conv32(x, w, b, stride=1, res=None):
    y = F.silu(F.conv2d(x.float(), w.float(), b, stride=stride, padding=w.shape[-1] // 2))
    return (y if res is None else y + res.float()).double()


@pytest.mark.parametrize("case", CSP_PARAMS)
def test_csp_reference_agrees_with_torch_float32(case):
    """Stage by stage from the reference's own storage values: the float64 stage and torch's float32 one differ by float32 noise only."""
    c = case
    _, b, eff = fc.csp_weights(c.hid, c.dt, c.split)
    x = fc.nchw(fc.csp_input(c))
    ref = fc.csp_reference(c, x)
    a, t = ref["ab"][:, :c.hid], ref["t"]
    b12 = torch.cat([b["cv1"], b["cv2"]])
    stages = [("ab", fc.stage_ab(c, x), _silu_conv32(x, eff["cv12"], b12), _f32_bound(x, eff["cv12"], b12, fc.stage_ab(c, x))),
              ("t", fc.stage_t(c, a), _silu_conv32(a, eff["rep"], b["rep"]), _f32_bound(a, eff["rep"], b["rep"], fc.stage_t(c, a))),
              ("u", fc.stage_u(c, a, t), _silu_conv32(t, eff["bott"], b["bott"], res=a), _f32_bound(t, eff["bott"], b["bott"], fc.stage_u(c, a, t), res=a)),
              ("out", fc.stage_out(c, ref["ub"]), _silu_conv32(ref["ub"], eff["cv3"], b["cv3"]), _f32_bound(ref["ub"], eff["cv3"], b["cv3"], fc.stage_out(c, ref["ub"])))]
    for name, y64, y32, bound in stages:
        ratio = float(((y64 - y32).abs() / bound).max())
        assert ratio <= 1.0, (c.name, name, ratio)
    # the zero padding of a and t is a zero, not SiLU(bias): at these biases the difference is many ulps on every border pixel
    assert ref["ab"].shape == (c.B, c.C2, c.H, c.W) and ref["t"].shape == (c.B, c.hid, c.H, c.W) and ref["out"].shape == (c.B, c.C2, c.H, c.W)
    for v in ref.values():
        assert bool(torch.isfinite(v).all()) and bool((rc.round_storage(v, c.dt) == v).all())


def test_csp_biases_make_a_wrong_halo_visible():
    """SiLU(bias) in place of the zero padding of a: the border rows of t move by far more than a quantum on most elements."""
    c = next(x for x in fc.CSP_CASES if x.name == "2x8x16-h32-f16-s0")
    _, b, eff = fc.csp_weights(c.hid, c.dt, c.split)
    a = fc.csp_reference(c, fc.nchw(fc.csp_input(c)))["ab"][:, :c.hid]
    halo = b["cv1"].double() * torch.sigmoid(b["cv1"].double())
    wrong = F.pad(a, (1, 1, 1, 1)) + F.pad(torch.zeros_like(a), (1, 1, 1, 1), value=1.0) * halo.view(1, -1, 1, 1)
    y_wrong = rc.conv64_ex(wrong, eff["rep"], b["rep"], act=1, pad4=(0, 0, 0, 0))
    y = fc.stage_t(c, a)
    moved = ((y_wrong - y).abs() / rc.quantum(y, c.dt))[:, :, 0, :]
    assert float(moved.median()) > 8.0, float(moved.median())


@pytest.mark.parametrize("case", STEM_PARAMS)
def test_stem_case_geometry_and_reference(case):
    c = case
    L = _lib.lib()
    v = [C.c_int() for _ in range(4)]
    _lib.check(L.cc_letterbox_geometry(c.H, c.W, c.res, *[C.byref(x) for x in v]))
    geo = tuple(x.value for x in v)
    assert geo == c.letterboxed == tuple(fc.yo.letterbox_geometry(c.H, c.W, c.res)), (c.name, geo)
    nh, nw, py, px = geo
    assert (nh + 2 * py) % 32 == 0 and (nw + 2 * px) % 32 == 0
    need = fc.stem_need_bytes(c.H, c.W, nh, nw)
    if c.need is not None:
        assert need == c.need, (c.name, need)
    assert c.big == (not c.f32 and need > fc.SCRATCH_SMALL), (c.name, need)
    st = fc.stem_tile_staging(c.H, c.W, c.res, c.f32, c.big)
    assert {"all": all(st), "none": not any(st), "some": any(st) and not all(st)}[c.staged], (c.name, st)
    # the reference against a float32 chain on the same network input
    frames = fc.stem_frames(c.H, c.W, c.f32, c.B)
    for dt in fc.STEM_DTYPES:
        sdt = "f16" if dt == "f16s" else dt
        w, b, eff = fc.stem_weights(32, dt)
        x = fc.stem_network_input(frames, c.res, sdt)
        assert x.shape == (c.B, 3, nh + 2 * py, nw + 2 * px) and float(x.min()) >= 0.0 and float(x.max()) <= 1.0
        assert bool((x[:, :, :py] == 0).all()) and bool((x[:, :, :, :px] == 0).all())
        y64 = fc.stem_reference(frames, c.res, 32, dt)
        ratio = float(((y64 - _silu_conv32(x, eff, b, stride=2)).abs() / _f32_bound(x, eff, b, y64, stride=2)).max())
        assert ratio <= 1.0, (c.name, dt, ratio)


def test_stem_cases_reach_every_variant():
    u8 = [c for c in fc.STEM_CASES if not c.f32]
    assert any(not c.big and c.staged == "all" for c in u8) and any(c.big and c.staged == "all" for c in u8)
    assert any(c.big and c.staged == "none" for c in u8) and any(c.f32 and c.staged == "none" for c in fc.STEM_CASES)
    offs, total = fc.ragged_layout()
    assert [o % 4 for o in offs] == [0, 1, 2, 3] and total == offs[-1] + fc.RAGGED_FRAMES[-1][0] * fc.RAGGED_FRAMES[-1][1] * 3
    shapes = {(lambda g: (g[0] + 2 * g[2], g[1] + 2 * g[3]))(fc.yo.letterbox_geometry(h, w, fc.RAGGED_RES)) for h, w in fc.RAGGED_FRAMES}
    assert shapes == {(64, 64)}
    # the ragged launch takes the BIG scratch (a frame of the batch needs it); 64x64 and 100x128 alone take the small one
    assert any(fc.stem_need_bytes(h, w, *fc.yo.letterbox_geometry(h, w, fc.RAGGED_RES)[:2]) > fc.SCRATCH_SMALL for h, w in fc.RAGGED_FRAMES)


# ---- the chooser ------------------------------------------------------------------------------------------------------------------------
def _choice(dt, split, hid, B, H, W, variant, dbg):
    k = C.c_int(-1)
    code = _lib.lib().cc_dev_csp_choice(fc.DTI[dt], split, hid, B, H, W, variant, dbg, C.byref(k))
    return code, k.value


@pytest.fixture
def tile_mode():
    L = _lib.lib()
    yield lambda v: _lib.check(L.cc_dev_set(b"csp_tile", v))
    _lib.check(L.cc_dev_set(b"csp_tile", -1))


def test_chooser_returns_the_kernel_every_case_names(tile_mode):
    for mode in (0, 1, 2):
        tile_mode(mode)
        for c in fc.CSP_CASES:
            for variant, want in c.variants + ((fc.V_LAYERS, fc.LAYERS),):
                for dbg in (0, 1, 2, 3):
                    if variant == fc.V_TILE and dbg:
                        continue
                    code, k = _choice(c.dt, c.split, c.hid, c.B, c.H, c.W, variant, dbg)
                    assert code == 0 and k == want == fc.expected_choice(c, variant, dbg, mode), (c.name, variant, dbg, mode, code, k)
            for dbg in (0, 1, 2, 3):
                code, k = _choice(c.dt, c.split, c.hid, c.B, c.H, c.W, fc.V_AUTO, dbg)
                assert code == 0 and k == fc.expected_choice(c, fc.V_AUTO, dbg, mode), (c.name, dbg, mode, k)


def test_chooser_threshold_and_exclusions(tile_mode):
    tile_mode(1)
    # 256 tiles of 16 x 32: one image of 16 x 16 tiles, or 256 images of one ragged tile; 255 stay with csp_fused_kernel
    assert _choice("f16", 0, 32, 1, 256, 512, 0, 0) == (0, fc.TILE)
    assert _choice("f16", 0, 32, 256, 1, 33 - 1, 0, 0) == (0, fc.TILE)
    assert _choice("f16", 0, 32, 255, 16, 32, 0, 0) == (0, fc.RESIDENT)
    assert _choice("f16", 0, 32, 1, 256, 512 - 32, 0, 0) == (0, fc.RESIDENT)
    assert _choice("f16", 0, 32, 6, 160, 160, 0, 0) == (0, fc.TILE) and _choice("f16", 0, 32, 5, 160, 160, 0, 0) == (0, fc.RESIDENT)
    assert _choice("bf16", 0, 32, 6, 160, 160, 0, 0) == (0, fc.TILE) and _choice("f16", 2, 32, 6, 160, 160, 0, 0) == (0, fc.TILE)
    for mode in (1, 2):
        tile_mode(mode)
        big = (64, 160, 160)
        assert _choice("f16", 0, 32, 1, 3, 5, 0, 0) == (0, fc.TILE if mode == 2 else fc.RESIDENT)
        for dbg in (1, 2, 3):
            assert _choice("f16", 0, 32, *big, 0, dbg) == (0, fc.RESIDENT)               # never with dbg
        assert _choice("f16", 0, 32, *big, fc.V_STREAM, 0) == (0, fc.STREAMED)           # ... stream
        assert _choice("f16", 1, 32, *big, 0, 0) == (0, fc.STREAMED)                     # ... split 1
        for split in (0, 1, 2):
            assert _choice("f16", split, 64, *big, 0, 0) == (0, fc.STREAMED)             # ... hidden width 64
        assert _choice("f16", 2, 32, *big, fc.V_FUSED, 0) == (0, fc.STREAMED)            # two planes in the 1x1 convs stream at width 32
    tile_mode(0)
    assert _choice("f16", 0, 32, 64, 160, 160, 0, 0) == (0, fc.RESIDENT)
    assert _choice("f16", 0, 32, 1, 3, 5, fc.V_TILE, 0) == (0, fc.TILE)                  # the variant argument wins over the mode


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _err():
    return _lib.lib().cc_last_error().decode(errors="replace")


def _csp_call(dt="f16", split=0, hid=32, x=FAKE_X, xcs=64, xco=0, out=FAKE_OUT, ocs=64, oco=0, B=1, H=8, W=16, variant=1, dbg=0, nw=5):
    hid_a = max(hid, 8)
    ws = [np.zeros(s, np.float32) for s in ((hid_a, 2 * hid_a), (hid_a, 2 * hid_a), (hid_a, hid_a * 9), (hid_a, hid_a * 9), (2 * hid_a, 2 * hid_a))]
    bs = [np.zeros(2 * hid_a, np.float32) for _ in range(5)]
    wp = (C.c_void_p * 5)(*[a.ctypes.data if i < nw else None for i, a in enumerate(ws)])
    bp = (C.c_void_p * 5)(*[a.ctypes.data for a in bs])
    k = C.c_int(-7)
    code = _lib.lib().cc_dev_csp(fc.DTI.get(dt, 0), split, hid, C.c_void_p(x), xcs, xco, C.c_void_p(out), ocs, oco, B, H, W, wp, bp, variant, dbg, C.byref(k), None)
    return code, k.value


CSP_REFUSALS = {
    "x pointer off by 8 bytes": dict(x=FAKE_X + 8),
    "out pointer off by 2 bytes": dict(out=FAKE_OUT + 2),
    "x_cstride no multiple of 8": dict(xcs=68),
    "out_cstride no multiple of 8": dict(ocs=76, oco=8),
    "x_coff 4": dict(xcs=80, xco=4),
    "out_coff 12": dict(ocs=80, oco=12),
    "view beyond its buffer": dict(xcs=64, xco=8),
    "hid 48": dict(hid=48, xcs=96, ocs=96),
    "hid 16": dict(hid=16, xcs=32, ocs=32),
    "bf16 with split 1": dict(dt="bf16", split=1),
    "bf16 with split 2": dict(dt="bf16", split=2),
    "f32 storage": dict(dt="f32"),
    "split 3": dict(split=3),
    "dbg with csp_tile_kernel": dict(variant=3, dbg=2),
    "csp_tile_kernel at hid 64": dict(variant=3, hid=64, xcs=128, ocs=128),
    "csp_tile_kernel with split 1": dict(variant=3, split=1),
    "dbg 4": dict(dbg=4),
    "variant 5": dict(variant=5),
    "empty batch": dict(B=0),
    "null x": dict(x=0),
    "a conv missing": dict(nw=4),
}


@pytest.mark.parametrize("why", sorted(CSP_REFUSALS))
def test_csp_refusals_come_before_any_hip_call(why):
    code, k = _csp_call(**CSP_REFUSALS[why])
    assert code == EINVAL and _err() and k == -7, (why, code, _err())


def test_csp_choice_refuses_what_the_launch_refuses():
    for kw in (dict(hid=48), dict(dt="bf16", split=1), dict(variant=3, dbg=1), dict(variant=3, hid=64), dict(variant=3, split=1), dict(B=0)):
        a = dict(dt="f16", split=0, hid=32, B=1, H=8, W=16, variant=1, dbg=0)
        a.update(kw)
        code, k = _choice(a["dt"], a["split"], a["hid"], a["B"], a["H"], a["W"], a["variant"], a["dbg"])
        assert code == EINVAL and _err() and k == -1, (kw, code)


def _stem_call(dt="f16", split=0, frames=FAKE_X, f32=0, sizes=((64, 64),), offsets=None, res=64, ragged=0, cout=32, out=FAKE_OUT, ocs=32, oco=0):
    hs = np.array([s[0] for s in sizes], np.int32)
    ws = np.array([s[1] for s in sizes], np.int32)
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum([h * w * 3 * (4 if f32 else 1) for h, w in sizes])[:-1]])
    off = np.array(offsets, np.int64)
    w, b = np.zeros((max(cout, 1), 27), np.float32), np.zeros(max(cout, 1), np.float32)
    info = (C.c_int * 3)(-7, -7, -7)
    code = _lib.lib().cc_dev_stem(fc.DTI.get(dt, 0), split, C.c_void_p(frames), f32, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                  hs.ctypes.data_as(C.POINTER(C.c_int32)), ws.ctypes.data_as(C.POINTER(C.c_int32)), len(sizes), res, ragged,
                                  _lib.ptr(w), _lib.ptr(b), cout, C.c_void_p(out), ocs, oco, info, None)
    return code, tuple(info)


STEM_REFUSALS = {
    "Cout 24": dict(cout=24, ocs=24),
    "Cout 128": dict(cout=128, ocs=128),
    "split weights with bf16": dict(dt="bf16", split=1),
    "f32 storage": dict(dt="f32"),
    "frames that letterbox to different network shapes": dict(sizes=((64, 64), (187, 301)), res=96, ragged=1),
    "a frame that does not letterbox to a multiple of 32": dict(sizes=((100, 100),), res=100),
    "a ragged frame that does not letterbox to a multiple of 32": dict(sizes=((64, 64), (100, 100)), res=100, ragged=1),
    "uniform launch over frames of two sizes": dict(sizes=((64, 64), (100, 128))),
    "uniform launch over frames with a gap": dict(sizes=((64, 64), (64, 64)), offsets=(0, 64 * 64 * 3 + 1)),
    "float32 frame at an odd offset": dict(f32=1, sizes=((64, 64),), offsets=(2,), ragged=1),
    "float32 frames at an odd address": dict(f32=1, frames=FAKE_X + 2),
    "out pointer off by 8 bytes": dict(out=FAKE_OUT + 8),
    "out_coff 4": dict(ocs=40, oco=4),
    "view beyond its buffer": dict(ocs=32, oco=8),
    "null frames": dict(frames=0),
    "negative offset": dict(offsets=(-1,), ragged=1),
}


@pytest.mark.parametrize("why", sorted(STEM_REFUSALS))
def test_stem_refusals_come_before_any_hip_call(why):
    code, info = _stem_call(**STEM_REFUSALS[why])
    assert code == EINVAL and _err() and info == (-7, -7, -7), (why, code, _err())
