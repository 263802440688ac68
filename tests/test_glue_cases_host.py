"""CPU checks of tests/glue_cases.py: the float64 references against torch, the licence for the bit-exact demand on grid inputs, the
pool selection rule through cc_dev_pool_choice, and the refusals - none of which needs a device."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as gc
import restart_check as rc
from clearcam_amd import _lib

FAKE_IN, FAKE_OUT = 0x10000, 0x20000                    # 16-byte aligned addresses that are never dereferenced: no launch happens here

POOL_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in gc.POOL_CASES if not c.refused for dt in c.dtypes]
FUSE_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in gc.FUSE_CASES if not c.refused for dt in c.dtypes]
CONV_PARAMS = [pytest.param(c, dt, id=f"{c.name}-{dt}") for c in gc.CONV_CASES if not c.refused for dt in c.dtypes]


def _nchw(x):
    return torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _torch_pool(c, x, dt):
    t = _nchw(x)
    if c.mode == 0:
        return _nhwc(F.avg_pool2d(t, c.k, c.stride, 0))
    if c.mode == 2:                                     # the model's order: average, round to the storage type, max
        t = torch.from_numpy(gc.storage(F.avg_pool2d(t, 2, 1, 0).numpy(), dt))
    return _nhwc(F.max_pool2d(t, c.k, c.stride, c.pad))


@pytest.mark.parametrize("case,dt", POOL_PARAMS)
def test_pool_reference_agrees_with_torch(case, dt):
    """To 0 on grid inputs (every float64 sum is exact) and on 16-bit normal inputs (four values of at most 11 bits within 2^-24 .. 2^3);
    f32 normal inputs: the float64 sum of four 24-bit values may round, in either order, by 2^-53 of the taps' magnitude."""
    c = case
    for kind in (c.grid_kind, "normal"):
        x, y64, mag = gc.pool_problem(c, dt, kind)
        ref = gc.pool_ref(c, x, dt) if c.mode == 2 else y64
        diff = np.abs(ref - _torch_pool(c, x, dt))
        tol = 2.0 ** -50 * mag if (dt == "f32" and kind == "normal" and c.mode == 0) else 0.0
        assert (diff <= tol).all(), (c.name, dt, kind, float(diff.max()))
        if c.mode == 2:                                 # rounding is monotone: max of the rounded averages = the rounded max of the averages
            assert np.array_equal(ref, gc.storage(y64, dt)), (c.name, dt, kind)


@pytest.mark.parametrize("case,dt", POOL_PARAMS)
def test_pool_grid_cases_are_exact_in_float32(case, dt):
    """numpy float32 in the kernel's summation order gives the float64 value on grid inputs: a kernel rounds once, to the storage type."""
    x, y64, _ = gc.pool_problem(case, dt, case.grid_kind)
    assert np.array_equal(gc.pool_f32_emulation(case, x).astype(np.float64), y64), case.name
    assert np.isfinite(y64).all() and (not case.negative or (y64 < 0).all()), case.name


@pytest.mark.parametrize("case,dt", FUSE_PARAMS)
def test_fuse_reference_agrees_with_torch_and_is_exact_in_float32(case, dt):
    c = case
    for kind in ("grid", "normal"):
        xs, y64, mag = gc.fuse_problem(c, dt, kind)
        acc = torch.zeros(c.B, c.C, c.Ho, c.Wo, dtype=torch.float64)
        for x, s in zip(xs, c.shifts):
            t = _nchw(x)
            if s:
                t = F.interpolate(t, scale_factor=float(1 << s), mode="nearest")
            acc = acc + t[:, :, :c.Ho, :c.Wo]
        diff = np.abs(y64 - _nhwc(acc))
        tol = 2.0 ** -50 * mag if (dt == "f32" and kind == "normal") else 0.0
        assert (diff <= tol).all(), (c.name, dt, kind, float(diff.max()))
        if kind == "grid":
            assert np.array_equal(gc.fuse_f32_emulation(c, xs).astype(np.float64), y64), c.name


@pytest.mark.parametrize("rows,C", gc.AFFINE_SHAPES)
@pytest.mark.parametrize("dt", gc.ALL3)
def test_affine_inputs_license_the_bracket_bar(rows, C, dt):
    x, scale, shift, y64, A = gc.affine_problem(rows, C, dt)
    assert (scale > 0).any() and (scale < 0).any() and (shift > 0).any() and (shift < 0).any()
    assert np.array_equal(gc.storage(x, dt), x)
    assert (np.abs(y64) >= gc.CANCEL * A).all()
    if dt != "f32":                                     # two f32 roundings stay under half a quantum of the storage type at y64
        q = rc.quantum(torch.from_numpy(y64), dt).numpy()
        assert (2.0 ** -23 * A < 0.5 * q).all()
    t = torch.from_numpy(x) * torch.from_numpy(scale).double() + torch.from_numpy(shift).double()
    assert np.array_equal(t.numpy(), y64)


def test_face_frames_and_reference():
    u8 = gc.face_frames(False)
    assert u8.dtype == np.uint8 and u8.shape == (2, 112, 112, 3)
    for b in range(2):
        for ch in range(3):
            assert len(np.unique(u8[b, :, :, ch])) == 256
    ref = gc.face_pre_ref(u8, 8)
    assert ref.dtype == np.float32 and (ref[..., 3:] == 0).all()
    want = (u8[..., ::-1].astype(np.float64) / 255.0 - 0.5) / 0.5                  # the model's expression in float64: the f32 one within 2 ulp of 1
    assert np.abs(ref[..., :3] - want).max() <= 2.0 ** -22
    assert ref[..., :3].min() == -1.0 and ref[..., :3].max() == 1.0
    f32 = gc.face_frames(True)
    assert f32.dtype == np.float32 and (f32 != np.round(f32)).mean() > 0.99


@pytest.mark.parametrize("case,dt", CONV_PARAMS)
def test_conv_reference_agrees_with_torch(case, dt):
    """Nearest F.interpolate / F.avg_pool2d + torch.cat + restart_check.conv64_ex against the module's own materialisation, to 1e-12."""
    c = case
    xs, w, b, x, y64, mag = gc.conv_problem(c.problem_id, dt)
    parts = []
    for s, xv in zip([c.s0] + ([c.s1] if c.s1 else []), xs):
        t = _nchw(xv)
        assert np.array_equal(gc.storage(xv, dt), xv)
        if s.shift > 0:
            t = F.interpolate(t, scale_factor=float(1 << s.shift), mode="nearest")[:, :, :c.H, :c.W]
        elif s.shift < 0:
            t = torch.from_numpy(gc.storage(F.avg_pool2d(t, 2, 1, 0).numpy(), dt))
        parts.append(t)
    xt = torch.cat(parts, 1)
    assert tuple(xt.shape) == (c.B, c.Cin, c.H, c.W) and torch.equal(xt, x)
    w_eff = rc.split_values([w])[0] if dt == "f16s" else w.double()
    if dt != "f16s":
        assert torch.equal(w.to(gc.TORCH_DT[dt]).float(), w)                         # representable: packing keeps the values
    yt = rc.conv64_ex(xt, w_eff, b, c.stride, 1, c.act)
    assert tuple(yt.shape) == (c.B, c.Cout) + c.out_hw
    assert float((yt - y64).abs().max()) <= 1e-12


def _pool_choice(L, c, dt):
    Ho, Wo = c.out_hw
    k = C.c_int(-7)
    code = L.cc_dev_pool_choice(gc.DTI[dt], FAKE_IN, c.ics, c.in_coff, FAKE_OUT, c.ocs, c.out_coff, c.B, c.H, c.W, c.C, Ho, Wo, c.k, c.stride,
                                c.pad, c.mode, C.byref(k))
    return code, k.value


def test_pool_rule_reaches_every_kernel(lib_path):
    """Each case's expected PoolKernel is what the rule returns under the pool_rows value the case sets, and the cases reach all ten."""
    L = _lib.lib()
    reached = set()
    try:
        for c in gc.POOL_CASES:
            if c.refused:
                continue
            _lib.check(L.cc_dev_set(b"pool_rows", -1 if c.pool_rows is None else c.pool_rows))
            for dt in c.dtypes:
                code, k = _pool_choice(L, c, dt)
                assert code == 0, (c.name, dt, L.cc_last_error().decode(errors="replace"))
                assert k == c.expect, (c.name, dt, "rule gives", gc.POOL_NAMES[k], "case expects", gc.POOL_NAMES[c.expect])
                reached.add(k)
    finally:
        _lib.check(L.cc_dev_set(b"pool_rows", -1))
    assert reached == set(range(len(gc.POOL_NAMES))), sorted(set(range(len(gc.POOL_NAMES))) - reached)


def test_pool_rows_override_follows_the_rule(lib_path):
    """8 / 4 / anything else for the average, 1 / anything else for avg-max, -1 back to the default (eight rows, two rows)."""
    L = _lib.lib()
    a = next(c for c in gc.POOL_CASES if c.name == "avg2_67x21")
    m = next(c for c in gc.POOL_CASES if c.name == "avgmax_66x23")
    try:
        for v, ka, km in ((-1, gc.POOL_AVG2_ROWS8, gc.POOL_AVGMAX_ROWS2), (8, gc.POOL_AVG2_ROWS8, gc.POOL_AVGMAX_ROWS2), (4, gc.POOL_AVG2_ROWS4, gc.POOL_AVGMAX_ROWS2),
                          (1, gc.POOL_VEC_AVG2, gc.POOL_AVGMAX), (2, gc.POOL_VEC_AVG2, gc.POOL_AVGMAX_ROWS2)):
            _lib.check(L.cc_dev_set(b"pool_rows", v))
            assert _pool_choice(L, a, "f16") == (0, ka) and _pool_choice(L, m, "f16") == (0, km), v
    finally:
        _lib.check(L.cc_dev_set(b"pool_rows", -1))


def test_refused_cases_are_refused_without_a_device(lib_path):
    L = _lib.lib()
    n = 0
    for c in gc.POOL_CASES:
        if c.refused:
            for dt in c.dtypes:
                Ho, Wo = c.out_hw
                code, _ = _pool_choice(L, c, dt)
                assert code != 0 and L.cc_last_error(), c.name
                code = L.cc_dev_pool(gc.DTI[dt], FAKE_IN, c.ics, c.in_coff, FAKE_OUT, c.ocs, c.out_coff, c.B, c.H, c.W, c.C, Ho, Wo, c.k, c.stride,
                                     c.pad, c.mode, None, None)
                assert code != 0 and b"avg-max" in L.cc_last_error(), c.name
                n += 1
    for c in gc.FUSE_CASES:
        if c.refused:
            for dt in c.dtypes:
                ptrs = (C.c_void_p * c.n)(*[FAKE_IN + 0x1000 * i for i in range(c.n)])
                arr = lambda v: (C.c_int * c.n)(*v)
                code = L.cc_dev_fuse(gc.DTI[dt], c.n, ptrs, arr([c.in_hw(i)[0] for i in range(c.n)]), arr([c.in_hw(i)[1] for i in range(c.n)]),
                                     arr([v[0] for v in c.views]), arr([v[1] for v in c.views]), arr(c.shifts), FAKE_OUT, c.out_view[0], c.out_view[1],
                                     c.B, c.Ho, c.Wo, c.C, None)
                assert code != 0 and b"alignment" in L.cc_last_error(), (c.name, L.cc_last_error())
                n += 1
    for c in gc.CONV_CASES:
        if c.refused:
            for dt in c.dtypes:
                d = _lib.ConvDesc(gc.DTI[dt], c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, 1, c.act, -1, 0, 0, 0, 0, 0, 0, 0, 0, c.variant)
                s0 = _lib.SrcDesc(FAKE_IN, c.s0.H, c.s0.W, c.s0.cs, c.s0.coff, c.s0.C, c.s0.shift)
                w = np.zeros((c.Cout, c.Cin, c.k, c.k), np.float32)
                code = L.cc_dev_conv_src(C.byref(d), C.byref(s0), None, _lib.ptr(w), None, FAKE_OUT, None, None)
                assert code != 0 and b"unsupported shape" in L.cc_last_error(), (c.name, dt, L.cc_last_error())
                n += 1
    assert n >= 6
