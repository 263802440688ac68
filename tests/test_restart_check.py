"""The float64 restart checker (tests/restart_check.py) on the CPU: a faithful float32 conv passes its bars, and four subtly wrong
results of the same conv - one cell off by an ulp, the epilogue rounded toward zero, round-to-nearest weights where the library rounds
with controlled rounding, one channel's bias dropped - each fail them.  This is what lets the in-situ restart of the detector's plan
(tests/test_gpu_plan_restart.py) tell a faithful kernel from a subtly wrong one."""
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
