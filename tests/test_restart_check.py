"""The float64 restart checker (tests/restart_check.py) on the CPU: a faithful float32 conv passes its bars, and four subtly wrong
results of the same conv - one cell off by an ulp, the epilogue rounded toward zero, round-to-nearest weights where the library rounds
with controlled rounding, one channel's bias dropped - each fail them.  This is what lets the in-situ restart of the detector's plan
(tests/test_gpu_plan_restart.py) tell a faithful kernel from a subtly wrong one."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import restart_check as rc

# torch's CPU f32 conv sums in another blocking than the MFMA kernels, with several times their noise (measured: up to 0.25 % differing,
# p99 midpoint distance up to 0.0074 ulp, against 0.105 % / 0.0009 on the MI355X): the faithful reference gets bars of its own here, and
# each wrong variant must fail even these looser ones
CPU_BARS = dict(R=6e-3, R_cell=2e-2, D=0.02)

# (dtype, k, Cin): K = k*k*Cin from 64 to 2304
CASES = [("f16", 1, 64), ("f16", 3, 256), ("f16", 1, 1024), ("bf16", 3, 64), ("bf16", 1, 512), ("bf16", 3, 256)]


def _case(sdt, k, cin, cout=64, B=2, H=36, W=40, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * k + cin)
    x = torch.randn(B, cin, H, W, generator=g).to(rc.TORCH_T[sdt]).float()          # storage-rounded activations
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.5
    return x, w, b


def _f32_conv(x, w, b, sdt, rounding="nearest"):
    """What a faithful kernel returns: f32 accumulation (torch's own order), f32 epilogue, one rounding."""
    y = F.silu(F.conv2d(x, w, b, padding=w.shape[-1] // 2))
    if rounding == "nearest":
        return y.to(rc.TORCH_T[sdt]).float()
    q = rc.quantum(y.double(), sdt)                                                   # toward zero
    return (torch.trunc(y.double() / q) * q).float()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}_{c[1]}x{c[1]}_cin{c[2]}")
def test_checker_passes_faithful_conv_and_fails_wrong_ones(lib_path, case):
    sdt, k, cin = case
    x, w, b = _case(sdt, k, cin)
    we = rc.effective_weights([w], sdt, split=False)[0]                               # the controlled rounding the library applies
    y64 = rc.conv64(x, we, b)
    good = _f32_conv(x, we.float(), b, sdt)
    st = rc.check(good, y64, sdt, "faithful f32 conv", **CPU_BARS)
    print(rc.fmt(f"{sdt} {k}x{k} cin {cin} faithful", st))
    assert st["differ"] > 0 or sdt == "bf16"                                          # f16: the case is fine enough to see the noise

    def fails(got, why):
        with pytest.raises(AssertionError):
            rc.check(got, y64, sdt, why, **CPU_BARS)
        print(rc.fmt(f"{sdt} {k}x{k} cin {cin} {why}", rc.check(got, y64, sdt, why, enforce=False)))

    nudged = good.clone()                                                             # (a) one 16x16x32 cell one ulp up
    cell = nudged[1, 32:64, 16:32, 16:32]
    cell += rc.quantum(cell.double(), sdt).float()
    fails(nudged, "(a) one cell nudged by an ulp")
    fails(_f32_conv(x, we.float(), b, sdt, rounding="zero"), "(b) epilogue rounded toward zero")
    wn = w.to(rc.TORCH_T[sdt]).float()                                                # (c) round-to-nearest weights
    assert not torch.equal(wn, we.float())
    fails(_f32_conv(x, wn, b, sdt), "(c) nearest-rounded weights")
    b_drop = b.clone()                                                                # (d) one channel's bias dropped
    b_drop[5] = 0.0
    fails(_f32_conv(x, we.float(), b_drop, sdt), "(d) bias of one channel dropped")


def test_split_values_share_one_scale():
    """Convs packed into one launch (cv1 | cv2 of a RepNCSP) share the power of two that puts the LARGEST magnitude of both in
    [2^14, 2^15); a per-tensor scale (what a single-tensor restatement would use) gives the smaller tensor other planes."""
    g = torch.Generator().manual_seed(3)
    a = torch.randn(32, 64, 1, 1, generator=g) * 4.0
    s = torch.randn(32, 64, 1, 1, generator=g) * 0.01
    va, vs = rc.split_values([a, s])
    alone = rc.split_values([s])[0]
    assert torch.equal(va, rc.split_values([a])[0])
    assert not torch.equal(vs, alone)
    e = 14 - int(np.floor(np.log2(float(a.abs().max()))))                             # the scale comes from `a` alone
    hi = (s * 2.0 ** e).half().float()
    assert torch.equal(vs, (hi.double() + (s * 2.0 ** e - hi).half().double()) * 2.0 ** -e)
    assert float((va - a.double()).abs().max() / a.abs().max()) < 2 ** -21


def test_storage_rounding_is_single_and_floored():
    """round_storage rounds float64 once (ties to even) and the quantum is floored at the smallest normal's spacing."""
    x = torch.tensor([1.0 + 2 ** -11 + 2 ** -40, 1.0 + 2 ** -11, 3 * 2 ** -25, 0.0, -2.5e-8], dtype=torch.float64)
    r = rc.round_storage(x, "f16")
    assert r[0] == 1.0 + 2 ** -10 and r[1] == 1.0 and r[2] == 2 * 2 ** -24 and r[3] == 0.0
    assert torch.equal(r.to(torch.float16).double(), r)
    assert float(rc.quantum(torch.tensor([1e-9], dtype=torch.float64), "f16")[0]) == 2 ** -24
    xb = torch.randn(1000, dtype=torch.float64)
    assert torch.equal(rc.round_storage(xb, "bf16"), xb.float().to(torch.bfloat16).double())   # no f32 midpoints in randn draws


def _loops64(x, w, b, stride, groups, act, slope, res, pad4, Ho, Wo):
    """conv64_ex's operation written out: nested loops over plain Python floats (float64), one output element at a time."""
    N, Ci, H, W = x.shape
    Co, cig, k, _ = w.shape
    cog = Co // groups
    top, _, left, _ = pad4
    y = np.zeros((N, Co, Ho, Wo))
    for n in range(N):
        for co in range(Co):
            g = co // cog
            for ho in range(Ho):
                for wo in range(Wo):
                    s = 0.0
                    for c in range(cig):
                        for r in range(k):
                            for q in range(k):
                                ih, iw = ho * stride - top + r, wo * stride - left + q
                                if 0 <= ih < H and 0 <= iw < W:
                                    s += float(x[n, g * cig + c, ih, iw]) * float(w[co, c, r, q])
                    if b is not None:
                        s += float(b[co])
                    if act == 1:
                        s = s / (1.0 + math.exp(-s))
                    elif act == 2:
                        s = 0.5 * s * (1.0 + math.tanh(0.7978845608028654 * (s + 0.044715 * s * s * s)))
                    elif act == 3:
                        s = s if s > 0 else float(slope[co]) * s
                    if res is not None:
                        s += float(res[n, co, ho, wo])
                    if act == 4:
                        s = max(s, 0.0)
                    y[n, co, ho, wo] = s
    return y


# (k, stride, groups, Cout, pad, Ho, Wo) on a 1 x 3 x 5 x 4 input; Ho / Wo None = the symmetric formula
_EX_GEOMS = [
    ("3x3_s1", 3, 1, 1, 4, 1, None, None),
    ("3x3_s2", 3, 2, 1, 4, 1, None, None),
    ("3x3_s2_asym_pad0", 3, 2, 1, 4, 0, 3, 2),           # symmetric formula gives 2 x 1: one extra zero row / column at the bottom / right
    ("5x5_s2_asym_pad1", 5, 2, 1, 2, 1, 3, 2),           # symmetric 2 x 1
    ("3x3_s2_depthwise_asym", 3, 2, 3, 3, 0, 3, 2),
    ("1x1_s2", 1, 2, 1, 5, 0, None, None),
]


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("act", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("geom", _EX_GEOMS, ids=[g[0] for g in _EX_GEOMS])
def test_conv64_ex_matches_nested_loops(geom, act, with_res):
    _, k, stride, groups, Co, pad, Ho, Wo = geom
    H, W, Ci = 5, 4, 3
    g = torch.Generator().manual_seed(31 + 7 * act + k)
    x = torch.randn(1, Ci, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci // groups, k, k, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    slope = torch.rand(Co, generator=g, dtype=torch.float64) * 0.5 - 0.1          # both signs
    Ho = (H + 2 * pad - k) // stride + 1 if Ho is None else Ho
    Wo = (W + 2 * pad - k) // stride + 1 if Wo is None else Wo
    res = torch.randn(1, Co, Ho, Wo, generator=g, dtype=torch.float64) if with_res else None
    pad4 = rc.pads_for(H, W, k, stride, pad, Ho, Wo)
    got = rc.conv64_ex(x, w, b, stride, groups, act, slope, res, pad4)
    want = _loops64(x.numpy(), w.numpy(), b.numpy(), stride, groups, act, slope.numpy(), None if res is None else res.numpy(), pad4, Ho, Wo)
    assert tuple(got.shape) == want.shape
    assert float(np.abs(got.numpy() - want).max()) <= 1e-13 * max(1.0, float(np.abs(want).max()))
    mag = rc.conv_abs64(x, w, b, stride, groups, res, pad4)
    want_mag = _loops64(np.abs(x.numpy()), np.abs(w.numpy()), np.abs(b.numpy()), stride, groups, 0, None,
                        None if res is None else np.abs(res.numpy()), pad4, Ho, Wo)
    assert float(np.abs(mag.numpy() - want_mag).max()) <= 1e-13 * float(want_mag.max())


def test_conv64_ex_order_of_prelu_residual_and_relu():
    """PReLU acts BEFORE the residual, ReLU AFTER it: one element where the two orders differ."""
    x = torch.full((1, 1, 1, 1), -2.0)
    w = torch.ones(1, 1, 1, 1)
    res = torch.full((1, 1, 1, 1), 3.0)
    slope = torch.tensor([0.25])
    assert float(rc.conv64_ex(x, w, None, act=3, slope=slope, res=res, pad4=(0, 0, 0, 0))) == 2.5        # 0.25 * -2 + 3, not prelu(1)
    assert float(rc.conv64_ex(x, w, None, act=4, res=res, pad4=(0, 0, 0, 0))) == 1.0                     # relu(-2 + 3), not relu(-2) + 3
    assert float(rc.conv64_ex(x, w, None, act=4, res=-res, pad4=(0, 0, 0, 0))) == 0.0


def test_conv64_ex_default_equals_conv64():
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(2, 4, 6, 5, generator=g), torch.randn(6, 4, 3, 3, generator=g), torch.randn(6, generator=g)
    res = torch.randn(2, 6, 6, 5, generator=g)
    assert float((rc.conv64_ex(x, w, b, act=1, res=res) - rc.conv64(x, w, b, res=res)).abs().max()) <= 1e-13     # bias added inside / after the conv
    assert float((rc.conv64_ex(x, w, b, act=0) - rc.conv64(x, w, b, act=False)).abs().max()) <= 1e-13
