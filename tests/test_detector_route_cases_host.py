"""CPU checks of tests/detector_route_cases.py: the table is consistent and says what the selector says, the new development entries
refuse bad views and residuals before any HIP call, and the committed bars of tests/test_gpu_detector_routes.py have teeth - they reject
the float64 result of a launch that drops the low weight plane (everywhere; in the last K step of the last pixel tile only), leaves one
output row unwritten, or forgets the in-place residual.  None of it needs a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import detector_route_cases as drc
import epilogue_cases as ec
import restart_check as rc
from clearcam_amd import _lib
from test_gpu_detector_routes import bars_of

TWO_PLANE = [c for c in drc.CASES if "f16s" in c.dtypes]
INPLACE = [c for c in drc.CASES if c.res == "inplace16"]


def _err(L) -> bytes:
    return L.cc_last_error()


def test_table_is_consistent(lib_path):
    assert len({c.name for c in drc.CASES}) == len(drc.CASES)
    keys = set()
    for c in drc.CASES:
        M = c.B * c.out_hw[0] * c.out_hw[1]
        assert M % c.pix_tile, (c.name, "M is a whole number of pixel tiles", M, c.pix_tile)
        assert c.res in (None, "storage", "inplace16") and c.act in (0, 1) and not c.out_f32, c.name
        assert all(dt in drc.DTI for dt in c.dtypes) and (c.dtypes == ("f16s",) or "f16s" not in c.dtypes), c.name
        for dt in c.dtypes:
            k = c.ext_key(dt)
            assert len(k) == drc.NKEY and k[len(ec.KEY_FIELDS)] == int(dt == "f16s"), (c.name, k)
            keys.add(k)
    assert len(keys) >= 50                               # many cases, not many names for a few
    # deep-K cases: at least three K steps per plane
    for c in drc.CASES:
        if any(t in c.name for t in ("gen3_", "3x3_256_40", "big128_", "big256_", "phase_", "stream_256")):
            assert c.k * c.k * c.Cin >= 3 * c.kstep, (c.name, c.k * c.k * c.Cin, c.kstep)
    # more tiles than the streaming launcher starts blocks, and the fewest that does it
    two = next(c for c in drc.CASES if c.name == "stream_256_256-two_rounds")
    tiles = -(-two.H * two.W // two.pix_tile)
    assert drc.STREAM_CUS < tiles <= drc.STREAM_CUS + 4


def test_every_case_reaches_the_route_it_names(lib_path):
    """The selector is pure: cc_dev_conv_det_choice gives, without a device, the eight ints the launch will report."""
    L = _lib.lib()
    for c in drc.CASES:
        for dt in c.dtypes:
            code, ch = drc.selector_choice(c, dt)
            assert code == 0, (c.name, dt, _err(L))
            assert ch == c.expect + c.ext, (c.name, dt, "the selector gives", ch, "the case names", c.expect + c.ext)
    # the older tables' cases: what they declare is what the selector gives, so that their extended keys can be taken from it
    for c in ec.CASES:
        if "f16" in c.dtypes:
            code, ch = drc.selector_choice(c, "f16")
            assert code == 0 and ch[:4] == c.expect, (c.name, code, ch, c.expect, _err(L))
    for c in drc.gc.CONV_CASES:
        if not c.refused and c.expect[0] != drc.gc.ADOWN:
            for dt in c.dtypes:
                if dt != "f32":
                    code, ch = drc.glue_selector_choice(c, dt)
                    assert code == 0 and ch[:6] == c.expect, (c.name, dt, code, ch, c.expect, _err(L))


def test_covered_keys_and_merges(lib_path):
    cov = drc.covered_keys()
    assert all(len(k) == drc.NKEY for k in cov)
    for c in drc.CASES:
        assert all(c.ext_key(dt) in cov for dt in c.dtypes)
    assert any(v.startswith("epilogue_cases:") for v in cov.values()) and any(v.startswith("glue_cases:") for v in cov.values())
    for k, (to, why) in drc.MERGED.items():
        assert k not in cov and to in cov and why.strip() and drc.merge_is_legal(k, to), (k, to)
    # the rule itself: a merge may cross the loader's and the K loop's fields, never the kernel, the planes or the epilogue path
    k = next(iter(cov))
    d = dict(zip(drc.KEY_FIELDS, k))
    assert drc.merge_is_legal(drc.key_of(**{**d, "ks": 5, "ns": 3}), k)
    for f in drc.MERGE_FIXED:
        assert not drc.merge_is_legal(drc.key_of(**{**d, f: d[f] + 1}), k), f


def test_new_entries_are_exported(lib_path):
    L = C.CDLL(lib_path)
    for s in ("cc_dev_conv_det", "cc_dev_conv_det_choice"):
        assert s in _lib.SYMBOLS and hasattr(L, s), s


def test_refusals_without_a_device(lib_path):
    """Everything is validated, and the selector asked, before the first HIP call: the error is the entry's own text, not the runtime's."""
    L = _lib.lib()
    IN, OUT, RES = drc.FAKE_IN, drc.FAKE_OUT, drc.FAKE_RES
    w = np.zeros(64 * 64 * 9, np.float32)

    def call(text, res=None, out=OUT, s0=None, s1=None, **kw):
        f = dict(dtype=3, B=2, H=13, W=21, Cin=64, Cout=64, k=3, stride=1, groups=1, act=1, pad=-1, Ho=0, Wo=0, out_f32=0, out_cstride=0,
                 out_coff=0, res_f32=0, res_cstride=0, res_coff=0, variant=0)
        f.update(kw)
        d = _lib.ConvDesc(*[f[n] for n, _ in _lib.ConvDesc._fields_])
        s0 = s0 or _lib.SrcDesc(IN, 13, 21, 64, 0, 64, 0)
        for code in (L.cc_dev_conv_det(C.byref(d), C.byref(s0), C.byref(s1) if s1 else None, _lib.ptr(w), None, res, out, None, None),
                     L.cc_dev_conv_det_choice(C.byref(d), C.byref(s0), C.byref(s1) if s1 else None, res, out, None)):
            assert code != 0 and text in _err(L), (text, kw, code, _err(L))

    call(b"null argument", out=None)
    call(b"dtype must be", dtype=4)
    call(b"bad shape", B=0)
    call(b"groups must divide", groups=3)
    call(b"groups must divide", groups=4, Cout=66)
    call(b"act 0 .. 2", act=5)
    call(b"bad source view", s0=_lib.SrcDesc(IN, 13, 21, 64, 8, 64, 0))                    # the view leaves its buffer
    call(b"bad source view", s0=_lib.SrcDesc(None, 13, 21, 64, 0, 64, 0))
    call(b"smaller than the input", s0=_lib.SrcDesc(IN, 6, 10, 64, 0, 64, 1))              # 6 x 10 upsampled is 12 x 20 < 13 x 21
    call(b"Cin must be the channels", s1=_lib.SrcDesc(IN + 0x1000, 13, 21, 32, 0, 32, 0))
    call(b"bad output view", out_cstride=96, out_coff=40)
    call(b"Ho / Wo beyond", Ho=15)
    call(b"without a residual pointer", res_cstride=64)
    call(b"without a residual pointer", res_f32=1)
    call(b"bad residual view", res=RES, res_cstride=96, res_coff=40)
    call(b"bad residual view", res=RES, res_coff=-8, res_cstride=96)
    call(b"must be the output's own view", res=OUT, res_f32=1)                             # in place, another type
    call(b"must be the output's own view", res=OUT, out_cstride=96, out_coff=8, res_cstride=96, res_coff=16)   # in place, shifted
    call(b"must be the output's own view", res=OUT, out_cstride=96, res_cstride=128)
    call(b"takes no residual", res=RES, s0=_lib.SrcDesc(IN, 14, 22, 128, 64, 64, -1), stride=2)
    call(b"names no kernel", variant=3)
    call(b"weights-stationary 3x3", variant=4)                                             # forced onto a launch it cannot run (two planes)
    # the sibling keeps its contract: no groups, no residual
    d = _lib.ConvDesc(3, 2, 13, 21, 64, 64, 3, 1, 4, 1, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    s0 = _lib.SrcDesc(IN, 13, 21, 64, 0, 64, 0)
    assert L.cc_dev_conv_src(C.byref(d), C.byref(s0), None, _lib.ptr(w), None, OUT, None, None) != 0 and b"one group" in _err(L)
    # and a legal in-place descriptor passes the selector: the residual keeps conv_big's 128-wide tile off the 256 x 256 ones
    ok = next(c for c in drc.CASES if c.name == "big128_3x3_128_128-inplace16")
    assert drc.selector_choice(ok, "f16s") == (0, ok.expect + ok.ext)


# ---- teeth -----------------------------------------------------------------------------------------------------------------------------
def _rejected(st, bars) -> bool:
    try:
        rc.assert_bars(st, "", ulps=None, **bars)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", TWO_PLANE, ids=[c.name for c in TWO_PLANE])
def test_bars_reject_a_dropped_low_plane(case):
    """With the committed bars, restart_check.check passes round_storage(y64) and rejects the three planted faults.  One K step of one
    ragged tile is a small share of a deep sum over a few pixels: where the case's own K moves no output across a rounding midpoint, the
    second fault (drc.faulty_kstep: the last K step wherever that step multiplies more than padding) is planted in the same case with Cin halved until it does (same tile, same loader, same epilogue, same bars)."""
    c = case
    bars = bars_of(c, "f16s")

    def stats(cc, fault):
        prob = drc.problem(cc.problem_id, "f16s")
        y64 = prob[5]
        assert not _rejected(rc.check(rc.round_storage(y64, "f16"), y64, "f16", enforce=False, **bars), bars), (cc.name, cc.Cin)
        st = rc.check(drc.planted(cc, prob, fault), y64, "f16", enforce=False, **bars)
        print(f"{cc.name:40s} Cin {cc.Cin:4d} {fault:12s} differ {100 * st['differ']:.3f} %  max cell {100 * st['max_cell']:.2f} %  "
              f"p99 {st['p99_boundary']:.4f}  not faithful {st['not_faithful']}")
        return st

    for fault in ("no_low", "nan_row"):
        assert _rejected(stats(c, fault), bars), (c.name, fault, "passes the committed bars")
    cc = c
    while True:
        assert bool(drc.kstep_mask(cc, drc.faulty_kstep(cc)).any()), cc.name
        if _rejected(stats(cc, "no_low_last"), bars):
            break
        assert cc.Cin % (2 * 8 * cc.groups) == 0 and cc.cat % 2 == 0, (c.name, "no K shows a low plane missing in one K step of the last tile")
        cc = drc.replace(cc, Cin=cc.Cin // 2, cat=cc.cat // 2)


@pytest.mark.parametrize("case", INPLACE, ids=[c.name for c in INPLACE])
def test_bars_reject_a_forgotten_residual(case):
    c = case
    for dt in c.dtypes:
        bars = bars_of(c, dt)
        prob = drc.problem(c.problem_id, dt)
        y64 = prob[5]
        sdt = drc.SDT[dt]
        assert not _rejected(rc.check(rc.round_storage(y64, sdt), y64, sdt, enforce=False, **bars), bars)
        no_res = rc.round_storage(rc.conv64_ex(prob[0], prob[4], prob[2], c.stride, c.groups, c.act, None, None), sdt)
        assert _rejected(rc.check(no_res, y64, sdt, enforce=False, **bars), bars), (c.name, dt)


def test_planted_faults_are_where_they_claim():
    """no_low_last changes nothing outside the last pixel tile, and there only through the low plane of the last K step."""
    c = next(c for c in drc.CASES if c.name == "gen_3x3_64_80")
    prob = drc.problem(c.problem_id, "f16s")
    y64 = prob[5]
    good, bad = rc.round_storage(y64, "f16"), drc.planted(c, prob, "no_low_last")
    M = y64.shape[0] * y64.shape[2] * y64.shape[3]
    diff = (good != bad).permute(0, 2, 3, 1).reshape(M, -1).any(1)
    first = (M - 1) // 128 * 128
    assert not bool(diff[:first].any()) and bool(diff[first:].any())
    m = drc.last_kstep_mask(c)                            # Ktot 1152 = 18 steps of 64: the last one is the low plane of tap (2, 2)
    assert int(m.sum()) == 64 and bool(m[2, 2].all())
    m8 = drc.last_kstep_mask(next(c for c in drc.CASES if c.name == "ktap_3x3_s2_8_64"))
    assert int(m8.sum()) == 8 and bool(m8[2, 2].all())   # Ktot 144: the fifth 32-element step holds the last tap's two planes, then padding
    # dense() lays groups out block-diagonally
    w = torch.arange(64 * 16 * 9, dtype=torch.float64).reshape(64, 16, 3, 3) + 1
    d = drc.dense(w, 4)
    assert d.shape == (64, 64, 3, 3) and bool((d[:16, 16:] == 0).all()) and torch.equal(d[16:32, 16:32], w[16:32])
    x = torch.randn(1, 64, 5, 6, dtype=torch.float64)
    assert float((rc.conv64_ex(x, w, None, 1, 4) - rc.conv64_ex(x, d, None, 1, 1)).abs().max()) < 1e-6
