"""CPU checks of the plans' K loops at their own depth (tests/plan_route_cases.py, the _DEEP_* tables of tests/epilogue_cases.py and the
committed tests/plan_route_table.py): the table of new cases is consistent and says what the selector says, every extended key the
plans log is covered (or merged legally) by a case deep enough, every new case is the one a logged key needs, and the bars of
tests/test_gpu_conv_epilogues.py have teeth at these depths - they reject the float64 result of a launch that drops one K step of the
last pixel tile, reads a stale ring stage there, adds the f32 in-place residual twice or leaves one output row NaN.  None of it needs a device."""
import pytest
import torch

import detector_route_cases as drc
import epilogue_cases as ec
import plan_route_cases as prc
import restart_check as rc
from clearcam_amd import _lib
from test_gpu_conv_epilogues import BARS, _problem, f32_bound

NEW = prc.NEW_CASES
KIND = {None: None, "storage": "storage", "inplace16": "storage", "f32": "f32", "inplace": "f32"}


def test_table_is_consistent():
    assert len({c.name for c in ec.CASES}) == len(ec.CASES)
    assert 25 <= len(NEW) <= 40 and len({prc.ext_key(c) for c in NEW}) == len(NEW)          # one case per extended key, no spares
    for c in NEW:
        M = c.B * c.out_hw[0] * c.out_hw[1]
        assert M % c.expect[2], (c.name, "M is a whole number of pixel tiles", M, c.expect[2])
        assert c.dtypes == ("f16", "bf16") and c.groups == 1 and len(c.ext) == 4, c.name
        assert len(prc.ext_key(c)) == prc.NKEY
        assert c.expect[0] in prc.RING_KERNELS, c.name
    m1 = [c for c in NEW if c.B * c.out_hw[0] * c.out_hw[1] == 1]
    assert len(m1) == 1 and m1[0].out_f32 and m1[0].res is None and (m1[0].Cin, m1[0].Cout) == (1024, 768)   # the final projection, one valid row
    # every older case keeps its four-int expect; only the new ones name the K loop
    assert all(c.ext is None or c in NEW for c in ec.CASES)


def test_both_conv_entries_are_exported(lib_path):
    """cc_conv2d_ex (four ints of choice) and cc_conv2d_ex_route (eight) are both in the binding and in the library."""
    import ctypes as C
    L = C.CDLL(lib_path)
    for s in ("cc_conv2d_ex", "cc_conv2d_ex_route"):
        assert s in _lib.SYMBOLS and hasattr(L, s), s
    assert _lib.CONV_CHOICE_INTS == 4 + len(NEW[0].ext)


def test_selector_confirms_every_new_case(lib_path):
    """cc_dev_conv_det_choice gives, without a device, exactly the eight ints each new case names (both storage types), and each new
    case stands in covered_cases() under the key it names: one the selector stopped confirming fails here, it does not vanish."""
    L = _lib.lib()
    cov = prc.covered_cases()
    for c in NEW:
        for dt in c.dtypes:
            code, ch = drc.selector_choice(c, dt)
            assert code == 0, (c.name, dt, L.cc_last_error())
            assert ch == c.expect + c.ext, (c.name, dt, "the selector gives", ch, "the case names", c.expect + c.ext)
        assert (f"epilogue_cases:{c.name}", c.ktot) in cov[prc.ext_key(c)], c.name
    assert all(len(k) == prc.NKEY for k in cov)


def test_committed_table_is_covered_at_depth(lib_path):
    cov = prc.covered_cases()
    for k, (to, why) in prc.MERGED.items():
        assert k not in cov and to in cov and why.strip() and prc.merge_is_legal(k, to), (k, to)
    assert tuple(prc.TABLE) == prc.PLANS
    for plan in prc.PLANS:
        table = prc.TABLE[plan]
        assert table and all(len(k) == prc.NKEY and k_plan == prc.field(k, "ks") ** 2 * shape[3] for k, (k_plan, _, shape) in table.items()), plan
        direct, merged, missing, shallow = prc.audit(table, cov)
        print(f"{plan}: {len(table)} extended keys, {len(direct)} covered directly, {len(merged)} merged")
        assert not missing, (plan, [prc.describe(k) for k in missing])
        assert not shallow, (plan, [(prc.describe(k), need, have, who) for k, need, have, who in shallow])
    # the rule itself: a merge may cross the loader's fields, never the kernel, the planes, the epilogue path, the stages or the activation
    k = prc.ext_key(NEW[0])
    d = dict(zip(prc.KEY_FIELDS, k))
    assert prc.merge_is_legal(drc.key_of(**{**d, "ks": 5, "cprw": 4}), k)
    for f in prc.MERGE_FIXED:
        assert not prc.merge_is_legal(drc.key_of(**{**d, f: d[f] + 1}), k), f
    assert {"ns", "act"} <= set(prc.MERGE_FIXED)
    # the depth rule: a ring of ns stages wraps twice after 2 ns + 1 steps; a kernel without a K ring asks nothing
    assert prc.steps_needed(k, 10 ** 6) == 2 * d["ns"] + 1 and prc.steps_needed(k, 8 * d["cprw"] + 1) == 2
    assert prc.steps_needed(drc.key_of(**{**d, "kernel": ec.DIRECT}), 10 ** 6) == 0


def test_every_new_case_is_needed(lib_path):
    """Without any ONE of the new cases some plan's table has a key that is missing or too shallow - that case's own key."""
    cov = prc.covered_cases()
    for c in NEW:
        key, me = prc.ext_key(c), (f"epilogue_cases:{c.name}", c.ktot)
        less = dict(cov)
        less[key] = [e for e in cov[key] if e != me]
        if not less[key]:
            del less[key]
        lost = set()
        for plan in prc.PLANS:
            _, _, missing, shallow = prc.audit(prc.TABLE[plan], less)
            lost |= set(missing) | {s[0] for s in shallow}
        assert lost == {key}, (c.name, [prc.describe(k) for k in lost])


# ---- teeth -----------------------------------------------------------------------------------------------------------------------------
# what restart_check.assert_bars says when bar 1 (NaN counts as neither bracketing value), R, R_cell or D fails
BAR_TEXT = ("neither of the two storage values", "share differing from round(y64)", "cell differs on more than", "flips away from the rounding midpoints")


def _rejected16(got, y64, dt) -> bool:
    st = rc.check(got, y64, dt, enforce=False, **BARS)    # a shape or argument error in here is an error, not teeth
    try:
        rc.assert_bars(st, "", ulps=None, **BARS)
    except AssertionError as e:
        assert any(t in str(e) for t in BAR_TEXT), ("an assertion that names no bar", e)
        return True
    return False


def _rejected32(got, c, dt, y64, mag) -> bool:
    """The f32 branch of test_conv_epilogue_matches_float64."""
    return not bool(torch.isfinite(got).all()) or float(((got - y64).abs() / f32_bound(c, dt, y64, mag)).max()) > 1.0


@pytest.mark.parametrize("case", NEW, ids=[c.name for c in NEW])
def test_bars_reject_planted_faults(case):
    c = case
    assert {"drop_kstep", "nan_row"} <= set(prc.faults_of(c))
    assert ("res_twice" in prc.faults_of(c)) == (c.res == "inplace")
    if c.k == 1 and prc.ksteps(c.ktot, c.ext[2]) > c.ext[3]:
        assert "stale_stage" in prc.faults_of(c), c.name      # wherever the ring wraps in a 1x1 case the stale stage is planted
    for dt in c.dtypes:
        prob = _problem(c.ref_id, dt, KIND[c.res])
        y64, mag = prob[5], prob[6]
        if c.out_f32:
            assert not _rejected32(y64.float().double(), c, dt, y64, mag), (c.name, dt)
        else:
            assert not _rejected16(rc.round_storage(y64, dt), y64, dt), (c.name, dt)
        for fault in prc.faults_of(c):
            bad = prc.planted(c, prob, fault)
            rej = _rejected32(bad.float().double(), c, dt, y64, mag) if c.out_f32 else _rejected16(rc.round_storage(bad, dt), y64, dt)
            assert rej, (c.name, dt, fault, "passes the committed bars")


def test_planted_faults_are_where_they_claim():
    by = {c.name: c for c in NEW}
    # 1x1, K = 1024 on four stages of 64 elements: the last step is 15, its stale stage held step 11
    c = by["clip-deep-g32_4-1x1_k1024-act0"]
    assert prc.faulty_kstep(c) == 15 and int(prc.kstep_mask(c, 15).sum()) == 64 and bool(prc.kstep_mask(c, 15)[960:, 0, 0].all())
    prob = _problem(c.ref_id, "f16", None)
    y64 = prob[5]
    M = y64.shape[0] * y64.shape[2] * y64.shape[3]
    first = (M - 1) // 32 * 32
    for fault in ("drop_kstep", "stale_stage"):
        diff = (prc.planted(c, prob, fault) != y64).permute(0, 2, 3, 1).reshape(M, -1).any(1)
        assert not bool(diff[:first].any()) and bool(diff[first:].all()), fault
    assert not torch.equal(prc.planted(c, prob, "drop_kstep"), prc.planted(c, prob, "stale_stage"))
    x, w = prob[0].double(), prob[1].double()
    px = x.permute(0, 2, 3, 1).reshape(M, -1)[M - 1]
    want = y64.permute(0, 2, 3, 1).reshape(M, -1)[M - 1] - w[:, 960:, 0, 0] @ px[960:] + w[:, 960:, 0, 0] @ px[704:768]
    assert float((prc.planted(c, prob, "stale_stage").permute(0, 2, 3, 1).reshape(M, -1)[M - 1] - want).abs().max()) < 1e-9
    # 3x3: the centre tap's step, never one that multiplies only padding; Cin 8 on 64-byte rows: step 1 holds taps 4 .. 7
    c3 = by["adaface-deep-g32_6-3x3_c512-act3"]
    m = prc.kstep_mask(c3, prc.faulty_kstep(c3))
    assert int(m.sum()) == 64 and bool(m[256:320, 1, 1].all())
    c8 = by["adaface-deep-g128x64_row64-3x3_c8-act3"]
    m8 = prc.kstep_mask(c8, prc.faulty_kstep(c8))
    assert prc.faulty_kstep(c8) == 1 and int(m8.sum()) == 32 and bool(m8[:, 1, 1].all()) and bool(m8[:, 2, 1].all()) and not bool(m8[:, 0, 0].any())
    # the final projection: one pixel, and it is the faulty one
    cm = next(c for c in NEW if c.Cout == 768)
    pm = _problem(cm.ref_id, "bf16", None)
    assert bool(torch.isnan(prc.planted(cm, pm, "nan_row")).all()) and bool((prc.planted(cm, pm, "drop_kstep") != pm[5]).all())
