"""Together on the CPU: the numpy model of tests/near_cases.py against a plain double loop over rows and list entries, the header's
constants and signatures against the binding's, and the preconditions the GPU tests (tests/test_gpu_index_near.py) rely on."""
import ctypes
import os
import re

import numpy as np
import pytest

from clearcam_amd import _lib
from clearcam_amd import objects as O
from near_cases import (CHUNK, DEFAULT_PARTNERS, GROUPS, INT32_MAX, INT32_MIN, MAX_PARTNERS, N_ODD, NO_TS, PARTNERS, VALUES, WITHINS, World, case_table,
                        list_position, near_fold, near_model, near_order, near_timeline_model, ordered, partner_list)
from test_index_terms_host import brute_order
from where_cases import Rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def key(x):
    return ordered(np.float32(x)).item()


def brute_list(Sb, group, ts, cls, partners, cut_b, allowed, b_ts_range, b_classes):
    """The partner list in words: every allowed row with a ts that passes B's filter and the cut, best score first, equal scores by row"""
    rows = []
    for r in range(len(Sb)):
        if ts[r] == NO_TS:
            continue
        if allowed is not None and not (group[r] < len(allowed) and allowed[group[r]]):
            continue
        if b_ts_range is not None and (ts[r] < b_ts_range[0] or ts[r] > b_ts_range[1]):
            continue
        if b_classes is not None and (cls[r] < 0 or cls[r] not in b_classes):
            continue
        if cut_b is not None and Sb[r] < np.float32(cut_b):
            continue
        rows.append(r)
    rows.sort(key=lambda r: (-key(Sb[r]), r))
    return rows[:partners], len(rows)


def brute_fold(Sa, Sb, plist, group, slot, ts, within, value):
    """The join in words, row by row and entry by entry, in Python integers"""
    v, dead, partner = [], [], []
    for r in range(len(Sa)):
        found = -1
        for p in plist:
            if p == r or group[p] != group[r] or ts[r] == NO_TS:
                continue
            if abs(int(ts[p]) - int(ts[r])) > within:
                continue
            if slot[r] >= 0 and slot[p] == slot[r]:
                continue
            found = p
            break
        x = Sa[r]
        if found >= 0 and value == "min" and key(Sb[found]) < key(x):
            x = Sb[found]
        v.append(x); dead.append(found < 0); partner.append(found)
    return np.array(v, np.float32), np.array(dead), np.array(partner, np.int64)


def test_min_follows_the_key_order_and_the_first_entry_wins():
    # one group, no slots, ts all equal: every entry but the row itself qualifies, so the partner is the list's first other row
    Sa = np.array([0.0, -0.0, 0.5, 0.5, -1.0], np.float32)
    Sb = np.array([-0.0, 0.0, 0.7, 0.2, 0.9], np.float32)
    z = np.zeros(5, np.int32)
    plist = [4, 2, 1, 0, 3]
    v, dead, partner = near_fold(Sa, Sb, plist, z, z - 1, z, 0, "min")
    assert partner.tolist() == [4, 4, 4, 4, 2] and not dead.any()
    assert v.tolist() == [0.0, -0.0, 0.5, 0.5, -1.0] and np.signbit(v).tolist() == [False, True, False, False, True]
    v, _, partner = near_fold(Sa, Sb, [0, 1], z, z - 1, z, 0, "min")
    assert partner.tolist() == [1, 0, 0, 0, 0]
    # +0 above -0: min(+0, -0) is -0 whichever side brings it; min(0.5, -0) is -0
    assert np.signbit(v).tolist() == [False, True, True, True, True] and v.tolist() == [0.0, -0.0, -0.0, -0.0, -1.0]
    v, dead, _ = near_fold(Sa, Sb, [0, 1], z, z - 1, z, 0, "a")
    assert np.array_equal(v.view(np.uint32), Sa.view(np.uint32)) and not dead.any()
    # the rules one at a time: another group, too far, the row itself, the same track, no ts
    g = np.array([0, 1, 0, 0, 0], np.int32); t = np.array([10, 10, 13, 10, NO_TS], np.int32); s = np.array([3, 3, 3, -1, -1], np.int32)
    _, dead, partner = near_fold(Sa, Sb, [0], g, s, t, 2, "a")
    assert partner.tolist() == [-1, -1, -1, 0, -1] and dead.tolist() == [True, True, True, False, True]
    _, _, partner = near_fold(Sa, Sb, [0], g, s, t, 3, "a")
    assert partner.tolist() == [-1, -1, -1, 0, -1]                                   # row 2 is near enough now, but of row 0's track
    _, _, partner = near_fold(Sa, Sb, [0, 3], g, s, t, 3, "a")
    assert partner.tolist() == [3, -1, 3, 0, -1]
    # 64-bit differences: the two ends of int32 are 2^32 - 2 apart, not 2 apart
    t = np.array([INT32_MAX, INT32_MIN + 1, 0, 0, 0], np.int32)
    _, _, partner = near_fold(Sa, Sb, [0, 1], z, z - 1, t, INT32_MAX, "a")
    assert partner.tolist() == [-1, -1, 0, 0, 0]


@pytest.mark.parametrize("tracks", [True, False])
def test_model_equals_the_double_loop(tracks):
    w = Rows(n=300, seed=3, queries=2)
    w.E[7] = w.E[3]; w.E[140] = w.E[3]; w.E[141] = w.E[3]                            # ties in both score vectors, whatever the seed drew
    n = w.n
    Sa, Sb = (w.q[:2] @ w.E.T).astype(np.float32)
    allowed = np.array([1, 1, 0, 1, 1], np.uint8)
    for partners in (1, 5, 40, 300):
        for cut_b, b_ts_range, b_classes in ((None, None, None), (float(np.median(Sb)), None, None), (float(Sb[3]), (0, 300), (0, 2, 64, 255))):
            for al in (None, allowed):
                plist, n_partners = partner_list(Sb, w.group, GROUPS, w.ts, w.cls, partners, cut_b, al, b_ts_range, b_classes)
                blist, bn = brute_list(Sb, w.group, w.ts, w.cls, partners, cut_b, al, b_ts_range, b_classes)
                what = (partners, cut_b, b_ts_range, al is None)
                assert plist.tolist() == blist and n_partners == bn and len(blist) == min(partners, bn), what
                for within in (0, 3, 40, 500):
                    for value in sorted(VALUES):
                        v, dead, partner = near_fold(Sa, Sb, plist, w.group, w.slot, w.ts, within, value)
                        bv, bdead, bpartner = brute_fold(Sa, Sb, blist, w.group, w.slot, w.ts, within, value)
                        assert np.array_equal(v.view(np.uint32), bv.view(np.uint32)) and np.array_equal(dead, bdead) and np.array_equal(partner, bpartner), what
                        pos = list_position(plist, partner)
                        assert all((p < 0) == (x < 0) and (p < 0 or plist[p] == x) for p, x in zip(pos.tolist(), partner.tolist()))
                        for cut, ts_range, classes in ((None, None, None), (float(np.median(v)), None, None), (None, (0, 300), (0, 2, 64, 255))):
                            want = brute_order(bv, bdead, w.slot, w.group, w.ts, w.cls, al, tracks, cut, ts_range, classes)
                            got, s = near_order(v, dead, w.slot, w.group, GROUPS, w.ts, w.cls, al, tracks, cut, ts_range, classes)
                            what2 = what + (within, value, cut, ts_range)
                            assert got.tolist() == [r for r, _ in want] and s.tolist() == [x for _, x in want], what2
                            idx, out, total, pr, ps, npart = near_model(Sa, Sb, w.slot, w.group, GROUPS, w.ts, w.cls, within, 2, 9, partners, cut_b, value, al,
                                                                        cut, tracks, ts_range, classes, b_ts_range, b_classes)
                            assert idx.shape == out.shape == pr.shape == ps.shape == (1, 9) and total.tolist() == [len(want)] and npart == bn, what2
                            assert idx[0].tolist() == ([r for r, _ in want][2:11] + [-1] * 9)[:9], what2
                            assert pr.dtype == np.int32 and pr[0].tolist() == [int(bpartner[r]) if r >= 0 else -1 for r in idx[0]], what2
                            assert ps.dtype == np.float32 and ps[0].tolist() == [float(Sb[p]) if p >= 0 else -np.inf for p in pr[0]], what2
                            counts, tot, npart = near_timeline_model(Sa, Sb, w.slot, w.group, GROUPS, w.ts, w.cls, within, -50, 60, 5, partners, cut_b, value,
                                                                     al, cut, tracks, ts_range, classes, b_ts_range, b_classes)
                            hist = [0] * 5
                            for r, _ in want:
                                if w.ts[r] != NO_TS and 0 <= (int(w.ts[r]) + 50) // 60 < 5:
                                    hist[(int(w.ts[r]) + 50) // 60] += 1
                            assert counts.tolist() == [hist] and tot.tolist() == [len(want)] and npart == bn and counts.dtype == np.int64, what2


def _header():
    return open(os.path.join(ROOT, "include", "clearcam_hip.h")).read()


def test_the_header_the_binding_and_the_library_agree(lib_path):
    hdr = _header()
    defs = {k: int(v) for k, v in re.findall(r"#define (CC_NEAR_[A-Z_]+)\s+(\d+)", hdr)}
    assert defs == {"CC_NEAR_MAX_PARTNERS": 16384, "CC_NEAR_DEFAULT_PARTNERS": 4096, "CC_NEAR_VALUE_A": 0, "CC_NEAR_VALUE_MIN": 1}
    assert (_lib.NEAR_MAX_PARTNERS, _lib.NEAR_DEFAULT_PARTNERS) == (defs["CC_NEAR_MAX_PARTNERS"], defs["CC_NEAR_DEFAULT_PARTNERS"]) == (MAX_PARTNERS, DEFAULT_PARTNERS)
    assert _lib.NEAR_VALUE == {"a": defs["CC_NEAR_VALUE_A"], "min": defs["CC_NEAR_VALUE_MIN"]} == VALUES
    assert MAX_PARTNERS % CHUNK == 0 and DEFAULT_PARTNERS <= MAX_PARTNERS
    L = ctypes.CDLL(lib_path)
    for name in ("cc_index_rank_near", "cc_index_timeline_near"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    flat = re.sub(r"\s+", " ", hdr)
    question = ("cc_index* h, const float* qa, int64_t row_a, const float* qb, int64_t row_b, int32_t within, int max_partners, float cut_b, int value, ")
    filters = "const uint8_t* allowed, int n_groups, const cc_row_filter* where_a, const cc_row_filter* where_b, "
    assert ("int cc_index_rank_near(" + question + "int64_t start, int64_t count, float min_score, int flags, " + filters +
            "int32_t* idx, float* score, int32_t* partner, float* partner_score, int64_t* total, int64_t* n_partners, int on_device, void* stream);") in flat
    assert ("int cc_index_timeline_near(" + question + "float min_score, int flags, " + filters +
            "int32_t t0, int32_t bin_seconds, int n_bins, uint32_t* counts, int64_t* total, int64_t* n_partners, int on_device, void* stream);") in flat
    # the binding passes as many arguments as the header declares, 64-bit where it says int64_t
    _lib.lib()
    for name, n_args in (("cc_index_rank_near", 25), ("cc_index_timeline_near", 23)):
        at = getattr(_lib.lib(), name).argtypes
        assert len(at) == n_args and at[2] is ctypes.c_int64 and at[4] is ctypes.c_int64 and at[5] is ctypes.c_int32 and at[7] is ctypes.c_float, name
    import inspect
    sig = inspect.signature(O.EmbeddingIndex.rank_near)
    assert list(sig.parameters)[1:] == ["a", "b", "within", "start", "count", "partners", "cut_b", "value", "allowed", "min_score", "tracks", "ts_range", "classes",
                                        "b_ts_range", "b_classes"]
    assert sig.parameters["partners"].default == DEFAULT_PARTNERS and sig.parameters["value"].default == "min"
    sig = inspect.signature(O.ObjectFinder.together)
    assert list(sig.parameters)[1:] == ["a", "b", "within", "start", "count", "cam_name", "timestamp", "is_face", "min_score", "min_partner", "value", "ts_range",
                                        "classes", "with_classes", "partners"]
    assert (sig.parameters["within"].default, sig.parameters["min_score"].default, sig.parameters["min_partner"].default) == (30, 0.21, 0.21)


def test_together_names_exactly_one_source_per_side():
    f = O.ObjectFinder.__new__(O.ObjectFinder)
    e = np.zeros(768, np.float32)
    assert f._together_source("a white van") == "text" and f._together_source("/cam/objects/2026-01-01/12_3_0.jpg") == "path"
    assert f._together_source(e) == "embedding" and f._together_source(O.Term(path="x")) == "path" and f._together_source(O.Term(text="x.jpg")) == "text"
    for bad in (None, O.Term(), O.Term(text="a", path="b"), O.Term(path="b", embedding=e), O.Term(text="a", embedding=e)):
        with pytest.raises(ValueError):
            f._together_source(bad)
        for args in ((bad, "person"), ("person", bad)):
            with pytest.raises(ValueError):
                f._together_setup(*args, 30, None, None, False, 0.21, 0.21, "min", 4096)
    for kw in (dict(within=-1), dict(within=1 << 31), dict(value="max"), dict(partners=0), dict(partners=MAX_PARTNERS + 1), dict(min_score=float("nan")),
               dict(min_partner=float("nan"))):
        args = dict(within=30, cam_name=None, timestamp=None, is_face=False, min_score=0.21, min_partner=0.21, value="min", partners=4096)
        args.update(kw)
        with pytest.raises(ValueError):
            f._together_setup(e, e, **args)
    for bad in (dict(start=-1), dict(count=0)):
        with pytest.raises(ValueError):
            f.together(e, e, **bad)


def test_the_cases_are_not_vacuous():
    """With numpy scores of the f32 rows, queries 0 and 1 as A and B and no filter: every pair of the case table has both living and
    dead rows (with within <= 1 or at most 5 partners also dead rows that have a ts); with within = 500 and 3000 partners every row with
    a ts lives; the living rows grow with both arguments from a handful to all of them; and
    with 1025 partners and within 0 or 1 some row's first qualifying entry is the list's entry 1024, the first of the second LDS chunk."""
    w = World(N_ODD)
    Sa, Sb = (w.q[:2] @ w.E.T).astype(np.float32)
    has_ts = w.ts != NO_TS
    assert set(case_table()) == {(x, p) for x in WITHINS for p in PARTNERS} and len(case_table()) == 20
    assert 1024 in PARTNERS and 1025 in PARTNERS and max(PARTNERS) > 2 * CHUNK and 500 > int(w.ts[has_ts].max()) - int(w.ts[has_ts].min())
    living = {}
    for within, partners in case_table():
        plist, n_partners = partner_list(Sb, w.group, GROUPS, w.ts, w.cls, partners)
        assert n_partners == int(has_ts.sum()) and len(plist) == partners
        v, dead, partner = near_fold(Sa, Sb, plist, w.group, w.slot, w.ts, within, "min")
        assert not (~dead & ~has_ts).any()
        living[within, partners] = int((~dead).sum())
        assert dead.any() and (~dead).any(), (within, partners)
        if (within, partners) == (500, 3000):
            assert np.array_equal(~dead, has_ts)
        if within <= 1 or partners <= 5:
            assert dead[has_ts].any(), (within, partners)             # not only the rows without a ts are dead
        if partners == 1025 and within in (0, 1):
            assert (list_position(plist, partner) == CHUNK).any(), within
        for tracks in (True, False):
            ans, _ = near_order(v, dead, w.slot, w.group, GROUPS, w.ts, w.cls, None, tracks)
            assert len(ans) >= 1
    for within in WITHINS:
        assert [living[within, p] for p in PARTNERS] == sorted(living[within, p] for p in PARTNERS)
    for p in PARTNERS:
        assert [living[x, p] for x in WITHINS] == sorted(living[x, p] for x in WITHINS)
    assert living[0, 1] < 50 and living[500, 3000] == int(has_ts.sum()) > 7000
