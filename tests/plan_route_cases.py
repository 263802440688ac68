"""What tests/test_gpu_plan_routes.py holds the AdaFace, BlazeFace and CLIP L/14 plans to, beyond the case table itself
(tests/epilogue_cases.py): the EXTENDED route key, the committed table of what the plans log, the depth condition and the planted faults
of the teeth test (helper module; not a conftest).  Held on the CPU by tests/test_plan_route_cases_host.py.

The extended key is detector_route_cases' : epilogue_cases' eleven fields plus (split, simple, two, cprw, ns) - the head and the tail of
a route-log record (clearcam_amd/csrc/conv_select.h).  The staged epilogues reuse the K ring's LDS (conv_tile.h), so a launch is wrong
exactly when stores overtake prefetches still in flight, and how many are in flight depends on `ns`: the key keeps (stages x epilogue)
apart.  A merge (MERGED) never crosses detector_route_cases.MERGE_FIXED, and for these plans never `ns` or `act` either.

COVERED.  A key counts as reached by any single launch that is held to float64 under it (covered_cases): a case of epilogue_cases
(through cc_conv2d_ex_route), but also a one-plane case of detector_route_cases or a 16-bit case of glue_cases.CONV_CASES, which run the
same selector and kernels through cc_dev_conv_det / cc_dev_conv_src with weights packed by the detector's pack_convs.  So a key of the
CLIP and face plans may be held by a launch that does not go through cc_conv2d_ex; none of the keys the _DEEP_* cases were added for is
(tests/test_plan_route_cases_host.py, test_every_new_case_is_needed).

DEPTH.  For a key whose kernel walks a K ring (generic, big, phase) a K step is 8 cprw elements.  With S_plan = the largest
ceil(ks ks Cin / (8 cprw)) over the layers the plans log under the key (plan_route_table.TABLE holds that layer), the deepest case that
reaches the key runs at least min(S_plan, 2 ns + 1) steps: the ring wraps twice wherever the plan's own layer makes it wrap.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Set, Tuple

import torch

import detector_route_cases as drc
import epilogue_cases as ec
import glue_cases as gc
import restart_check as rc
from plan_route_table import TABLE

KEY_FIELDS = drc.KEY_FIELDS
NKEY = drc.NKEY
MERGE_FIXED = drc.MERGE_FIXED + ("ns", "act")
RING_KERNELS = (ec.GENERIC, ec.BIG, ec.PHASE)
PLANS = ("adaface", "blazeface", "clip_image", "clip_text")
Key = Tuple[int, ...]
Shape = Tuple[int, ...]                                  # B, H, W, Cin, Cout, Ho, Wo of a logged layer

# Extended keys a plan logs that no case reaches with the same key, and the covered key whose code they run; one line each with the reason.
MERGED: Dict[Key, Tuple[Key, str]] = {}

NEW_CASES: List[ec.Case] = [c for c in ec.CASES if c.ext is not None]       # the cases that name their full route


def field(key: Key, name: str) -> int:
    return key[KEY_FIELDS.index(name)]


def ext_key(c: ec.Case) -> Key:
    """The extended key a case with a declared `ext` names (one weight plane: split 0)."""
    return c.route_key() + (0,) + tuple(c.ext)


def ksteps(ktot: int, cprw: int) -> int:
    return -(-ktot // (8 * cprw))


def merge_is_legal(key: Key, to: Key) -> bool:
    a, b = dict(zip(KEY_FIELDS, key)), dict(zip(KEY_FIELDS, to))
    return len(key) == NKEY and len(to) == NKEY and all(a[f] == b[f] for f in MERGE_FIXED)


@functools.lru_cache(maxsize=None)
def covered_cases() -> Dict[Key, List[Tuple[str, int]]]:
    """extended key -> [(single-launch case, its Ktot)], every case that reaches the key: the 16-bit cases of epilogue_cases, the one-plane
    cases of detector_route_cases and the 16-bit cases of glue_cases.CONV_CASES.  A case that declares `ext` stands under the key it
    NAMES (the host test holds the selector to it, its GPU test the launch), so it cannot vanish silently; the older cases declare
    (kernel, sched, bm, bn) only, the rest of their key is the selector's answer, and one the selector does not confirm is left out (its
    own GPU test fails).  Shared: do not modify."""
    out: Dict[Key, List[Tuple[str, int]]] = {}
    for c in ec.CASES:
        if "f16" not in c.dtypes:
            continue
        if c.ext is not None:
            out.setdefault(ext_key(c), []).append((f"epilogue_cases:{c.name}", c.ktot))
            continue
        code, ch = drc.selector_choice(c, "f16")
        if code == 0 and ch[:4] == c.expect:
            out.setdefault(c.route_key() + (0,) + ch[4:], []).append((f"epilogue_cases:{c.name}", c.ktot))
    for c in drc.CASES:
        for dt in c.dtypes:
            if dt != "f16s":
                out.setdefault(c.ext_key(dt), []).append((f"detector_route_cases:{c.name}", c.ktot))
    for c in gc.CONV_CASES:
        if c.refused or c.expect[0] == gc.ADOWN:
            continue
        for dt in c.dtypes:
            if dt in ("f32", "f16s"):
                continue
            code, ch = drc.glue_selector_choice(c, dt)
            if code == 0 and ch[:6] == c.expect:
                base = c.expect[:4] + (c.k, c.stride, 0, c.act, ec.RES_NONE, 0, int(c.Cout % 8 == 0))
                out.setdefault(base + (0,) + ch[4:], []).append((f"glue_cases:{c.name}", c.k * c.k * c.Cin))
    return out


# ---- the table of what the plans log --------------------------------------------------------------------------------------------------------
def table_of(logs: Dict[int, Dict[Key, Set[Shape]]]) -> Dict[Key, Tuple[int, int, Shape]]:
    """{batch: {extended key: shapes logged}} -> {extended key: (deepest Ktot = ks ks Cin, batch, shape B,H,W,Cin,Cout,Ho,Wo of that
    layer)}; among equally deep layers the smallest batch, then the smallest shape."""
    out: Dict[Key, Tuple[int, int, Shape]] = {}
    for B, log in logs.items():
        for key, shapes in log.items():
            ks = field(key, "ks")
            for s in shapes:
                cand = (ks * ks * s[3], B, tuple(s))
                cur = out.get(key)
                if cur is None or (-cand[0], cand[1], cand[2]) < (-cur[0], cur[1], cur[2]):
                    out[key] = cand
    return out


def format_table(tables: Dict[str, Dict[Key, Tuple[int, int, Shape]]]) -> str:
    """The text of plan_route_table.TABLE for `tables` (what the GPU test prints when the committed table is not what it logs)."""
    lines = ["TABLE = {"]
    for plan in (p for p in PLANS if p in tables):
        lines.append(f'    "{plan}": {{')
        lines += [f"        {k}: ({v[0]}, {v[1]}, {v[2]})," for k, v in sorted(tables[plan].items())]
        lines.append("    },")
    return "\n".join(lines + ["}"])


def steps_needed(key: Key, k_plan: int) -> int:
    """K steps the deepest case of `key` must run; 0 for a kernel without a K ring."""
    if field(key, "kernel") not in RING_KERNELS:
        return 0
    return min(ksteps(k_plan, field(key, "cprw")), 2 * field(key, "ns") + 1)


def audit(table: Dict[Key, Tuple[int, int, Shape]], covered: Dict[Key, List[Tuple[str, int]]], merged=None):
    """(direct keys, merged keys, missing keys, depth shortfalls [(key, steps needed, steps of the deepest case, that case)]) of one plan's table."""
    merged = MERGED if merged is None else merged
    direct, via, missing, shallow = [], [], [], []
    for key, (k_plan, _, _) in sorted(table.items()):
        to = key
        if key in covered:
            direct.append(key)
        elif key in merged and merged[key][0] in covered:
            via.append(key)
            to = merged[key][0]
        else:
            missing.append(key)
            continue
        name, k_case = max(covered[to], key=lambda e: e[1])
        need, have = steps_needed(key, k_plan), ksteps(k_case, field(to, "cprw"))
        if have < need:
            shallow.append((key, need, have, name))
    return direct, via, missing, shallow


def describe(key: Key) -> str:
    return drc.describe(key)


# ---- planted faults of the teeth test ---------------------------------------------------------------------------------------------------------
def pix_tile(c: ec.Case) -> int:
    return c.expect[2]


def faulty_kstep(c: ec.Case) -> int:
    """The K step the teeth test breaks.  A packed row is [tap 0: Cin][tap 1: Cin] ... (net_common.h pack_conv), walked in steps of
    8 cprw elements.  1x1: the last step (every step multiplies real pixels; it is >= ns wherever the ring wraps).  k > 1: the step that
    holds the middle channel of the CENTRE tap - the one tap that multiplies a real pixel for every output, whatever row or column of
    padding the last pixel tile touches (detector_route_cases.faulty_kstep tells the trap)."""
    kstep = 8 * c.ext[2]
    if c.k == 1:
        return (c.ktot - 1) // kstep
    return ((c.k * c.k // 2) * c.Cin + c.Cin // 2) // kstep


def kstep_mask(c: ec.Case, step: int) -> torch.Tensor:
    """(Cin, k, k) bool: the (channel, tap) pairs of K step `step`."""
    kstep = 8 * c.ext[2]
    idx = torch.arange(c.k * c.k * c.Cin).reshape(c.k, c.k, c.Cin)          # K index of (tap row, tap column, channel)
    return (idx // kstep == step).permute(2, 0, 1)


def _last_tile(c: ec.Case, good: torch.Tensor, bad: torch.Tensor) -> torch.Tensor:
    """`good` (NCHW) with the pixels of the last pixel tile taken from `bad`."""
    Bn, Cc, Ho, Wo = good.shape
    M = Bn * Ho * Wo
    first = (M - 1) // pix_tile(c) * pix_tile(c)
    flat = good.permute(0, 2, 3, 1).reshape(M, Cc).clone()
    flat[first:] = bad.permute(0, 2, 3, 1).reshape(M, Cc)[first:]
    return flat.reshape(Bn, Ho, Wo, Cc).permute(0, 3, 1, 2)


def faults_of(c: ec.Case) -> Tuple[str, ...]:
    out = ["drop_kstep", "nan_row"]
    if c.k == 1 and faulty_kstep(c) >= c.ext[3]:          # any stride: the fault shifts channels, not pixels
        out.append("stale_stage")
    if c.res == "inplace":
        out.append("res_twice")
    return tuple(out)


def planted(c: ec.Case, prob, fault: str) -> torch.Tensor:
    """The float64 result (NOT rounded: the caller rounds 16-bit outputs to the storage type) of a launch with `fault` and no other error:
      "drop_kstep"   K step faulty_kstep(c) of the last pixel tile is left out;
      "stale_stage"  1x1: that K step (s >= ns) of the last pixel tile multiplies the activations of step s - ns, the ones its ring stage held before;
      "res_twice"    the f32 in-place residual is added twice;
      "nan_row"      the right result with one pixel's channels NaN in the last pixel tile.
    prob = test_gpu_conv_epilogues._problem(...)."""
    x, w, b, slope, res, y64, _ = prob
    assert c.groups == 1, c.name
    pad4 = rc.pads_for(c.H, c.W, c.k, c.stride, c.padv, *c.out_hw)
    if fault == "res_twice":
        return y64 + res.to(torch.float64)
    if fault == "nan_row":
        Bn, Cc, Ho, Wo = y64.shape
        M = Bn * Ho * Wo
        first = (M - 1) // pix_tile(c) * pix_tile(c)
        flat = y64.permute(0, 2, 3, 1).reshape(M, Cc).clone()
        flat[(first + M) // 2] = float("nan")
        return flat.reshape(Bn, Ho, Wo, Cc).permute(0, 3, 1, 2)
    s = faulty_kstep(c)
    m = kstep_mask(c, s).unsqueeze(0)                                         # (1, Cin, k, k)
    assert bool(m.any()), (c.name, s)
    wb = torch.where(m, torch.zeros_like(w), w).to(torch.float64)
    if fault == "stale_stage":
        assert c.k == 1 and s >= c.ext[3], c.name
        kstep, back = 8 * c.ext[2], c.ext[3] * 8 * c.ext[2]
        lo, hi = s * kstep, min((s + 1) * kstep, c.Cin)
        wb[:, lo - back:hi - back] += w[:, lo:hi].to(torch.float64)           # x[step s - ns] meets the weights of step s
    else:
        assert fault == "drop_kstep", fault
    bad = rc.conv64_ex(x, wb, b, c.stride, 1, c.act, slope, res, pad4)
    return _last_tile(c, y64, bad)
