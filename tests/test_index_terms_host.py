"""Compound search on the CPU: the numpy model of tests/terms_cases.py against a brute-force Python loop over rows, the header's
constants against the binding's, and the preconditions the GPU tests (tests/test_gpu_index_terms.py) rely on."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from clearcam_amd import _lib
from clearcam_amd import objects as O
from terms_cases import (COMBINES, GROUPS, N_EVEN, N_ODD, NO_TS, PATTERNS, ROLES, TERM_COUNTS, TERMS_MAX, World, excluded, feasible, fold_terms, median_cuts,
                         ordered, plan, terms_fold, terms_model, terms_order, terms_timeline_model)
from where_cases import Rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(x):
    """Round a Python float to float32, as one f32 operation does"""
    return struct.unpack("f", struct.pack("f", x))[0]


def key(x):
    return ordered(np.float32(x)).item()


def brute_fold(S, roles, weights, cuts, combine):
    """The contract in words, row by row and term by term, in Python floats rounded to float32 after every operation"""
    T, n = S.shape
    v, dead, which = [], [], []
    for r in range(n):
        val, best, wh, d = None, None, -1, False
        for t in range(T):
            x = float(S[t][r])
            if roles[t] == "require":
                d = d or not x >= f32(cuts[t])
            elif roles[t] == "reject":
                d = d or x >= f32(cuts[t])
            elif combine == "sum":
                p = f32(f32(weights[t]) * x)                                         # a double product of two floats is exact: one rounding
                val = f32((0.0 if val is None else val) + p)
                if wh < 0 or key(p) > key(best):
                    best, wh = p, t
            else:
                better = wh < 0 or (key(x) > key(val) if combine == "max" else key(x) < key(val))
                if better:
                    val, wh = x, t
        v.append(val); dead.append(d); which.append(wh)
    return np.array(v, np.float32), np.array(dead), np.array(which)


def brute_order(v, dead, slot, group, ts, cls, allowed, tracks, cut, ts_range, classes):
    """-> [(row, score)] in order, as tests/test_index_like_host.py::brute ranks"""
    n = len(v)
    best, first, loose = {}, {}, []
    for r in range(n):
        if dead[r]:
            continue
        if allowed is not None and not (group[r] < len(allowed) and allowed[group[r]]):
            continue
        if ts_range is not None and (ts[r] == NO_TS or ts[r] < ts_range[0] or ts[r] > ts_range[1]):
            continue
        if classes is not None and (cls[r] < 0 or cls[r] not in classes):
            continue
        t = slot[r]
        if tracks and t >= 0:
            first.setdefault(t, r)
            if t not in best or v[r] > v[best[t]]:
                best[t] = r
        else:
            loose.append(r)
    ans = [(v[r], first[t], r) for t, r in best.items()] + [(v[r], (n + r) if tracks else r, r) for r in loose]
    if cut is not None:
        ans = [a for a in ans if not a[0] < np.float32(cut)]
    ans.sort(key=lambda a: (-a[0], a[1]))
    return [(r, s) for s, _, r in ans]


def same_fold(got, want, what):
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, "v")
    assert np.array_equal(got[1], want[1]), (what, "dead")
    assert np.array_equal(got[2], want[2]), (what, "which")


def test_max_and_min_follow_the_key_order_and_name_the_first_term():
    S = np.array([[-0.0, 0.0, 1.0, -2.0, -0.0, 5.0], [0.0, -0.0, -1.0, -3.0, -0.0, 5.0], [0.0, 0.0, 1.0, -2.0, 0.0, 9.0]], np.float32)
    roles = ["rank", "rank", "reject"]
    v, dead, which = fold_terms(S, roles, None, [None, None, 9.0], "max")
    assert v.tolist() == [0.0, 0.0, 1.0, -2.0, 0.0, 5.0] and np.signbit(v).tolist() == [False, False, False, True, True, False]
    assert which.tolist() == [1, 0, 0, 0, 0, 0] and dead.tolist() == [False] * 5 + [True]    # +0 beats -0; equal keys: the lower term
    v, dead, which = fold_terms(S, roles, None, [None, None, 9.0], "min")
    assert np.signbit(v).tolist() == [True, True, True, True, True, False] and v.tolist() == [-0.0, -0.0, -1.0, -3.0, -0.0, 5.0]
    assert which.tolist() == [0, 1, 1, 1, 0, 0]
    v, _, which = fold_terms(S, ["require", "rank", "rank"], None, [-9.0, None, None], "max")   # the first rank term need not be term 0
    assert v.tolist() == [0.0, 0.0, 1.0, -2.0, 0.0, 9.0] and which.tolist() == [1, 2, 2, 2, 2, 2]
    for combine in COMBINES:
        same_fold(fold_terms(S, roles, [1.0] * 3, [None, None, 9.0], combine), brute_fold(S, roles, [1.0] * 3, [None, None, 9.0], combine), combine)


def test_sum_rounds_twice_per_term_in_term_order():
    # 1 + 2^-24 + 2^-24: from the left both halves are lost (1.0), from the right they add up first (1 + 2^-23): the order matters
    S = np.array([[1.0], [2.0 ** -24], [2.0 ** -24]], np.float32)
    roles, w = ["rank"] * 3, [1.0, 1.0, 1.0]
    assert fold_terms(S, roles, w, [None] * 3, "sum")[0][0] == np.float32(1.0)
    assert fold_terms(S[::-1], roles, w, [None] * 3, "sum")[0][0] == np.float32(1.0) + np.float32(2.0 ** -23)
    # a product that an fma would keep exact: (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 before 2^-24 can meet the -1
    a = np.float32(1.0 + 2.0 ** -12)
    S = np.array([[a], [1.0]], np.float32)
    v, _, which = fold_terms(S, ["rank", "rank"], [float(a), -(1.0 + 2.0 ** -11)], [None, None], "sum")
    assert v[0] == np.float32(0.0) and which[0] == 0
    assert float(a) * float(a) - (1.0 + 2.0 ** -11) == 2.0 ** -24                  # what a fused multiply-add would have returned
    same_fold(fold_terms(S, ["rank", "rank"], [float(a), -(1.0 + 2.0 ** -11)], [None, None], "sum"),
              brute_fold(S, ["rank", "rank"], [float(a), -(1.0 + 2.0 ** -11)], [None, None], "sum"), "fma")
    # which: the largest PRODUCT, so a negative weight turns the order round; ties (equal products, -0 against +0) go to the lower term
    S = np.array([[0.5, 0.5, 0.0, -1.0], [0.9, 0.5, 0.0, 1.0], [0.25, 0.25, -0.0, 0.5]], np.float32)
    v, _, which = fold_terms(S, ["rank"] * 3, [1.0, -1.0, 2.0], [None] * 3, "sum")
    assert which.tolist() == [0, 0, 0, 2] and v.tolist() == [np.float32(0.5) - np.float32(0.9) + np.float32(0.5), 0.5, 0.0, -1.0]
    assert fold_terms(S[:1], ["rank"], [1.0], [None], "sum")[0].tolist() == S[0].tolist()


@pytest.mark.parametrize("combine", sorted(COMBINES))
def test_the_fold_equals_the_brute_force_loop(combine):
    rng = np.random.default_rng(5)
    S = rng.standard_normal((7, 90)).astype(np.float32)
    S[3] = S[1]; S[5, :30] = S[0, :30]; S[:, 40:44] = 0.0; S[2, 40:44] = -0.0           # equal terms, zeros of both signs
    for roles in (["rank"] * 7, ["require", "rank", "reject", "rank", "rank", "reject", "rank"], ["reject", "require", "require", "rank", "reject", "rank", "rank"]):
        w = rng.uniform(-1.5, 1.5, 7).astype(np.float32).tolist()
        cuts = [None if r == "rank" else float(np.float32(np.median(S[t]))) for t, r in enumerate(roles)]
        got = fold_terms(S, roles, w, cuts, combine)
        same_fold(got, brute_fold(S, roles, w, cuts, combine), (combine, roles))
        if roles.count("rank") < 7:
            assert got[1].any() and not got[1].all()
    # a cut of +-0: -0 >= +0 and +0 >= -0 both hold (IEEE compare, not the key order)
    Z = np.array([[1.0, 1.0], [-0.0, 0.0]], np.float32)
    assert fold_terms(Z, ["rank", "require"], [1.0, 1.0], [None, 0.0], combine)[1].tolist() == [False, False]
    assert fold_terms(Z, ["rank", "reject"], [1.0, 1.0], [None, -0.0], combine)[1].tolist() == [True, True]


@pytest.mark.parametrize("tracks", [True, False])
def test_model_equals_the_brute_force_loop(tracks):
    w = Rows(n=60, seed=3, queries=2)
    w.E[7] = w.E[3]; w.E[40] = w.E[3]                                               # ties across tracks, whatever the seed drew
    track = np.flatnonzero((w.slot == w.slot[3]) & (w.group == w.group[3]))
    assert w.slot[3] >= 0
    allowed = np.array([1, 1, 0, 1, 1], np.uint8)
    rows = np.r_[track[:3], 50]
    roles = ["rank", "require", "rank", "rank", "rank", "reject"][:2 + len(rows)]
    roles[-1] = "reject"
    q = w.q[:2]
    S = (np.vstack([q, w.E[rows]]) @ w.E.T).astype(np.float32)
    T = len(S)
    weights = np.linspace(-1.0, 1.5, T).astype(np.float32).tolist()
    cuts = median_cuts(S, roles, np.arange(60))
    for combine in sorted(COMBINES):
        for exclude in (None, "rows", "track"):
            v, dead, which = terms_fold(S, roles, weights, cuts, combine, rows, 2, w.group, w.slot, exclude)
            bv, bdead, bwhich = brute_fold(S, roles, weights, cuts, combine)
            ex = np.zeros(60, bool)
            if exclude == "rows":
                ex[[int(r) for i, r in enumerate(rows) if roles[2 + i] == "rank"]] = True
            elif exclude == "track":
                ex = (w.group == w.group[3]) & (w.slot == w.slot[3])
            same_fold((v, dead, which), (bv, bdead | ex, bwhich), (combine, exclude))
            assert np.array_equal(excluded(60, rows, roles, 2, w.group, w.slot, exclude), ex)
            for al in (None, allowed):
                for cut, ts_range, classes in ((None, None, None), (float(np.median(v)), None, None), (None, (0, 300), (0, 2, 64, 255))):
                    want = brute_order(bv, bdead | ex, w.slot, w.group, w.ts, w.cls, al, tracks, cut, ts_range, classes)
                    got, s = terms_order(v, dead, w.slot, w.group, GROUPS, w.ts, w.cls, al, tracks, cut, ts_range, classes)
                    what = (combine, exclude, al is None, cut, ts_range)
                    assert got.tolist() == [r for r, _ in want] and s.tolist() == [x for _, x in want], what
                    idx, out, total, wh = terms_model(v, dead, which, w.slot, w.group, GROUPS, w.ts, w.cls, 2, 9, al, cut, tracks, ts_range, classes)
                    assert idx.shape == out.shape == wh.shape == (1, 9) and total.shape == (1,) and total[0] == len(want), what
                    assert idx[0].tolist() == ([r for r, _ in want][2:11] + [-1] * 9)[:9], what
                    assert wh[0].tolist() == [int(bwhich[r]) if r >= 0 else -1 for r in idx[0]] and wh.dtype == np.int32, what
                    counts, tot = terms_timeline_model(v, dead, w.slot, w.group, GROUPS, w.ts, w.cls, -50, 60, 5, al, cut, tracks, ts_range, classes)
                    hist = [0] * 5
                    for r, _ in want:
                        if w.ts[r] != NO_TS and 0 <= (int(w.ts[r]) + 50) // 60 < 5:
                            hist[(int(w.ts[r]) + 50) // 60] += 1
                    assert counts.tolist() == [hist] and tot.tolist() == [len(want)] and counts.dtype == np.int64, what


def _header():
    return open(os.path.join(ROOT, "include", "clearcam_hip.h")).read()


def test_the_header_the_binding_and_the_library_agree(lib_path):
    hdr = _header()
    defs = {k: int(v) for k, v in re.findall(r"#define (CC_(?:TERMS?|COMBINE)_[A-Z]+)\s+(\d+)", hdr)}
    assert defs == {"CC_TERMS_MAX": 64, "CC_TERM_RANK": 0, "CC_TERM_REQUIRE": 1, "CC_TERM_REJECT": 2, "CC_COMBINE_MAX": 0, "CC_COMBINE_MIN": 1, "CC_COMBINE_SUM": 2}
    assert (_lib.TERMS_MAX, _lib.TERM_RANK, _lib.TERM_REQUIRE, _lib.TERM_REJECT) == (defs["CC_TERMS_MAX"], defs["CC_TERM_RANK"], defs["CC_TERM_REQUIRE"], defs["CC_TERM_REJECT"])
    assert (_lib.COMBINE_MAX, _lib.COMBINE_MIN, _lib.COMBINE_SUM) == (defs["CC_COMBINE_MAX"], defs["CC_COMBINE_MIN"], defs["CC_COMBINE_SUM"])
    assert TERMS_MAX == _lib.TERMS_MAX and ROLES == O.EmbeddingIndex.TERM_ROLE and COMBINES == O.EmbeddingIndex.COMBINE
    assert "typedef struct { int32_t role; float weight; float cut; } cc_term;" in hdr
    assert ctypes.sizeof(_lib.Term) == 12 and [f[0] for f in _lib.Term._fields_] == ["role", "weight", "cut"]
    L = ctypes.CDLL(lib_path)
    for name in ("cc_index_rank_terms", "cc_index_timeline_terms"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
    flat = re.sub(r"\s+", " ", hdr)
    assert "const cc_term* terms, int combine, int64_t start, int64_t count, float min_score, int flags," in flat
    assert "int32_t* idx, float* score, int32_t* which, int64_t* total, int on_device, void* stream);" in flat


def test_a_term_names_exactly_one_source():
    t = O.Term(text="white van")
    assert t == ("white van", None, None, "rank", 1.0, None) and O.Term._fields == ("text", "path", "embedding", "role", "weight", "cut")
    f = O.ObjectFinder.__new__(O.ObjectFinder)
    e = np.zeros(768, np.float32)
    for bad in ([O.Term()], [O.Term(text="a", path="b")], [O.Term(path="b", embedding=e)], [O.Term(embedding=e, role="must")], [O.Term(embedding=e, role="reject")],
                [O.Term(embedding=e, role="require", cut=float("nan"))], [O.Term(embedding=e, role="reject", cut=0.5)], [], [O.Term(embedding=e)] * 65):
        with pytest.raises(ValueError):
            f._compound_setup(bad, "max", None, None, False, None, None)
    for kw in (dict(combine="mean"), dict(exclude="all"), dict(min_score=float("nan"))):
        args = dict(combine="max", cam_name=None, timestamp=None, is_face=False, min_score=None, exclude=None)
        args.update(kw)
        with pytest.raises(ValueError):
            f._compound_setup([O.Term(embedding=e)], **args)


@pytest.mark.parametrize("n", [N_ODD, N_EVEN])
def test_the_cases_are_not_vacuous(n):
    """With numpy scores of the f32 rows: every case of the GPU tests kills some rows, spares some, and leaves a window at 1030 real
    without tracks and 40 answers with them."""
    w = World(n)
    everyone = np.arange(n)
    for T in TERM_COUNTS:
        for pattern in PATTERNS:
            if not feasible(T, pattern):
                assert (T, pattern) in ((1, "require"), (1, "reject"), (1, "both"), (2, "both"))
                continue
            for combine in sorted(COMBINES):
                q, rows, roles, weights = plan(w, T, pattern, combine, 0)
                n_vec = 0 if q is None else len(q)
                assert n_vec + len(rows) == T and (T == 1 or (n_vec >= 1 and len(rows) >= 1)) and len(set(rows.tolist())) == len(rows)
                assert roles.count("rank") >= 1 and all(np.isfinite(weights))
                V = w.E[rows] if q is None else np.vstack([q, w.E[rows]])
                S = (V @ w.E.T).astype(np.float32)
                cuts = median_cuts(S, roles, everyone)
                v, dead, which = fold_terms(S, roles, weights, cuts, combine)
                assert set(np.unique(which)) <= {t for t in range(T) if roles[t] == "rank"}
                if pattern != "rank":
                    assert dead.any() and (~dead).sum() > 1130, (T, pattern)
                for tracks in (True, False):
                    ans, _ = terms_order(v, dead, w.slot, w.group, GROUPS, w.ts, w.cls, None, tracks)
                    assert len(ans) >= (40 if tracks else 1130), (T, pattern, combine, tracks)
    assert plan(w, 1, "rank", "max", 0)[0] is not None and plan(w, 1, "rank", "max", 1)[0] is None
