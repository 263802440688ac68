"""Case table of tests/test_gpu_detector_routes.py: the conv routes of the DETECTOR plans, one launch each through cc_dev_conv_det
(helper module; not a conftest).  Held on the CPU by tests/test_detector_route_cases_host.py.

The detector's default mode "f16h" carries the stem and the backbone's 1x1 convs as TWO f16 weight planes ("f16s": every conv).  Two
planes change the K loop, not the epilogue: the walk visits every tap's channels twice (ConvP::split, common.h), so what can go wrong is
a plane dropped or doubled in one K step of one tile.  A case therefore names, beyond the (kernel, sched, bm, bn) of
tests/epilogue_cases.py, what picks the K-loop instantiation - simple (the incremental-pointer loader), two (the eight-wave kernel's
two-source loader), cprw (16-byte chunks per LDS row: the K step is 8 cprw elements) and ns (LDS stages) - and fails when the selector
lands elsewhere.  The EXTENDED route key is epilogue_cases' eleven fields plus (split, simple, two, cprw, ns): the head and the tail of a
route-log record (clearcam_amd/csrc/conv_select.h).

Shapes are the smallest at which a family can still go wrong: M = B Ho Wo ragged against the family's pixel tile, Cout off the channel
tile where the family allows it, deep-K cases at least three K steps per plane.  All cases run SiLU unless named otherwise.

The selector is pure, so cc_dev_conv_det_choice answers on a machine without a GPU what a case (of this table, of epilogue_cases or of
glue_cases.CONV_CASES) will run: `selector_choice`.  The keys of the older tables' cases are taken from it.
"""
from __future__ import annotations

import ctypes as C
import functools
import zlib
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

import torch

import epilogue_cases as ec
import glue_cases as gc
import restart_check as rc

EXT_FIELDS = ("split", "simple", "two", "cprw", "ns")
KEY_FIELDS = ec.KEY_FIELDS + EXT_FIELDS
NKEY = len(KEY_FIELDS)
# fields a merge may never cross (the kernel instantiation and the epilogue path): the rest is what the kernel does not branch on
MERGE_FIXED = ("kernel", "sched", "bm", "bn", "split", "two", "res", "out_f32")

DIRECT, GENERIC, BIG, PHASE, WS, WAVE, TILE64, STREAM = range(8)
SCHED0, ONE_TILE, BUFFER, PERSIST = range(4)
DTI = {"f16": 1, "bf16": 2, "f16s": 3}
SDT = {"f16": "f16", "bf16": "bf16", "f16s": "f16"}       # the storage type of a mode
FAKE_IN, FAKE_OUT, FAKE_RES = 0x10000, 0x20000, 0x30000  # 16-byte aligned addresses the selector never dereferences


@dataclass(frozen=True)
class DCase(ec.Case):
    """An epilogue_cases.Case run through cc_dev_conv_det: SiLU and two weight planes by default; res None | "storage" | "inplace16"."""
    act: int = 1
    dtypes: Tuple[str, ...] = ("f16s",)
    ext: Tuple[int, int, int, int] = (1, 0, 8, 2)       # simple, two, cprw, ns the launch must report
    pix: int = 0                                        # pixels of one tile where that is not expect[2] (the streaming kernel)
    cat: int = 0                                        # > 0: the input is Concat(Upsample x2 of `cat` channels at half size, Cin - cat channels)

    @property
    def pix_tile(self) -> int:
        return self.pix or self.expect[2]

    @property
    def kstep(self) -> int:
        return 8 * self.ext[2]

    @property
    def planes(self) -> int:
        return 2 if "f16s" in self.dtypes else 1

    def ext_key(self, dtype: str) -> Tuple[int, ...]:
        return self.route_key() + (int(dtype == "f16s"),) + self.ext

    @property
    def problem_id(self):
        return (self.B, self.Cin, self.H, self.W, self.Cout, self.k, self.stride, self.groups, self.act, self.res is not None, self.cat)

    @property
    def half_hw(self) -> Tuple[int, int]:
        return (self.H + 1) // 2, (self.W + 1) // 2


def _build() -> List[DCase]:
    cs: List[DCase] = []
    # ---- generic kernel, 128 x 32 tiles: Cout 80 = 2.5 tiles, M = 546 = 4.27 tiles; 18 virtual taps of one K step each ------------------
    g = DCase("gen_3x3_64_80", 2, 64, 13, 21, 80, 3, (GENERIC, 0, 128, 32), variant=2)
    cs += [g, replace(g, name=g.name + "-slice", out_cstride=96, out_coff=8), replace(g, name=g.name + "-act0", act=0)]
    # ---- 128 x 64 tiles on three LDS stages (Ktot = 2304 >= 2048): the DDetect box branch's entry convs ------------------------------------
    cs.append(DCase("gen3_3x3_128_64", 1, 128, 13, 21, 64, 3, (GENERIC, 0, 128, 64), variant=2, ext=(1, 0, 8, 3)))
    # ---- 64-byte LDS rows (Ktot x 2 <= 512 bytes): a K step is 32 elements, each plane of a 1x1 64 -> n is two of them ---------------------
    cs += [DCase("row64_1x1_64_128", 2, 64, 13, 21, 128, 1, (GENERIC, 0, 128, 128), variant=2, ext=(1, 0, 4, 2)),
           DCase("row64_1x1_64_64", 2, 64, 13, 21, 64, 1, (GENERIC, 0, 128, 64), variant=2, ext=(1, 0, 4, 2))]
    # ---- K-step edges of the virtual-tap walk: Cin = 8 is one 16-byte chunk per virtual tap (a 32-element step spans four of them, the
    #      last step is half padding); Cin = 32: a 64-element step is the high and the low plane of ONE tap ----------------------------------
    cs += [DCase("ktap_3x3_s2_8_64", 2, 8, 19, 23, 64, 3, (GENERIC, 0, 128, 64), stride=2, variant=2, ext=(1, 0, 4, 2)),
           DCase("ktap_3x3_32_32", 2, 32, 13, 21, 32, 3, (GENERIC, 0, 128, 32), variant=2)]
    # ---- few-tile configuration (9) and the small pixel tiles (94 - 97): four and six LDS stages, prefetch distance three and five ----------
    for v, bm, wm_ns in ((9, 128, 6), (94, 64, 6), (95, 64, 4), (96, 32, 6), (97, 32, 4)):
        cs += [DCase(f"small{v}_1x1_64_40", 2, 64, 13, 9, 40, 1, (GENERIC, 0, bm, 32), variant=v, ext=(1, 0, 8, wm_ns)),
               DCase(f"small{v}_3x3_256_40", 1, 256, 9, 11, 40, 3, (GENERIC, 0, bm, 32), variant=v, ext=(1, 0, 8, wm_ns))]     # Ktot 4608: 72 K steps
    # ---- four-wave single-barrier kernel, 128 x 128 tiles (6): plain, RepNBottleneck's in-place residual, into a channel slice ------------
    b = DCase("big128_3x3_128_128", 1, 128, 17, 19, 128, 3, (BIG, 0, 128, 128), variant=6)
    cs += [b, replace(b, name=b.name + "-inplace16", res="inplace16"), replace(b, name=b.name + "-slice", out_cstride=160, out_coff=16)]
    cs.append(DCase("big256_3x3_192_512", 1, 192, 17, 19, 512, 3, (BIG, 0, 256, 256), variant=5))
    # ---- eight-wave kernel (7), its four schedules --------------------------------------------------------------------------------------------
    for tag, pf, sched in (("sched0", 0, SCHED0), ("one_tile", 32, ONE_TILE), ("buffer", 64, BUFFER), ("persist", 512, PERSIST)):
        cs += [DCase(f"phase_{tag}_3x3_192_512", 1, 192, 17, 19, 512, 3, (PHASE, sched, 256, 256), variant=7, phase_flags=pf),
               DCase(f"phase_{tag}_1x1_512_256", 1, 512, 17, 19, 256, 1, (PHASE, sched, 256, 256), variant=7, phase_flags=pf)]
    # 131 x 2 = 262 tiles on at most 256 blocks: some blocks walk two tiles
    cs.append(DCase("persist_gemm_m33300_k64_n512", 1, 64, 185, 180, 512, 1, (PHASE, PERSIST, 256, 256), variant=7, phase_flags=512))
    # ---- streaming 1x1 kernel (10): the three instantiated widths; its tile is (8 / WN) x NP x 16 pixels (conv_stream.hip launch_stream_k) ----
    st = (0, 0, 8, 2)
    cs += [DCase("stream_256_256", 1, 256, 13, 21, 256, 1, (STREAM, 0, 128, 128), variant=10, ext=st, pix=64),
           DCase("stream_128_128", 1, 128, 7, 9, 128, 1, (STREAM, 0, 128, 128), variant=10, ext=st, pix=128),
           DCase("stream_64_64", 1, 64, 33, 17, 64, 1, (STREAM, 0, 128, 128), variant=10, ext=st, pix=256),
           # the launcher starts min(tiles, CUs) blocks: 131 x 127 = 16 637 pixels are 260 tiles of 64 on 256 CUs, four blocks walk two
           DCase("stream_256_256-two_rounds", 1, 256, 131, 127, 256, 1, (STREAM, 0, 128, 128), variant=10, ext=st, pix=64)]
    # ---- grouped: the DDetect box branch's 3x3 with four groups, densified to block-diagonal rows by pack_convs --------------------------------
    cs.append(DCase("grouped4_3x3_64_64", 1, 64, 13, 21, 64, 3, (GENERIC, 0, 128, 64), groups=4, variant=2))
    return cs


# ---- what the detector plans log beyond the families above (tests/test_gpu_detector_routes.py, part b) ------------------------------------
# The selector picks the tile by M = B Ho Wo and by K, so one frame, four frames and 64 frames run the same few loaders (1x1, the 1x1 over
# Concat(Upsample(a), b) of the neck - the non-simple loader -, 3x3, ADown's 3x3 stride 2 over an odd map) and the two epilogues (SiLU;
# SiLU + the in-place 16-bit residual) on most tiles, with one and with two planes.  One small ragged case per extended key they log: the
# tile is forced, the loader and the epilogue are the plan's.   tile -> (variant, phase_flags, Cout, expect, cprw, ns)
_TILES = {
    "g32": (97, None, 40, (GENERIC, 0, 32, 32), 8, 4), "g32_6": (96, None, 40, (GENERIC, 0, 32, 32), 8, 6),
    "g64": (95, None, 40, (GENERIC, 0, 64, 32), 8, 4),
    "g128x32_4": (91, None, 40, (GENERIC, 0, 128, 32), 8, 4), "g128x64_3": (93, None, 64, (GENERIC, 0, 128, 64), 8, 3),
    "g128x64": (2, None, 64, (GENERIC, 0, 128, 64), 8, 2), "g128x128": (2, None, 128, (GENERIC, 0, 128, 128), 8, 2),
    "g128x128_row64": (2, None, 128, (GENERIC, 0, 128, 128), 4, 2),
    "big128": (6, None, 128, (BIG, 0, 128, 128), 8, 2), "one_tile": (7, 32, 256, (PHASE, ONE_TILE, 256, 256), 8, 2),
}
# loader -> (k, stride, Cin, cat)
_LOADERS = {"1x1": (1, 1, 64, 0), "1x1_k128": (1, 1, 128, 0), "1x1_k256": (1, 1, 256, 0), "1x1_k512": (1, 1, 512, 0),
            "1x1cat": (1, 1, 128, 64), "1x1cat_k384": (1, 1, 384, 192), "3x3": (3, 1, 64, 0), "3x3s2": (3, 2, 64, 0)}
# (tile, loader, residual, planes)
_PLAN_ROUTES = [
    ("g32", "1x1cat", None, 2), ("g32", "3x3", None, 1), ("g32_6", "3x3", None, 1), ("g32", "3x3", "inplace16", 1), ("g32", "3x3", "inplace16", 2),
    ("g32", "3x3s2", None, 1), ("g32", "3x3s2", None, 2), ("g32_6", "3x3s2", None, 2),
    ("g64", "1x1cat", None, 1), ("g64", "1x1cat", None, 2), ("g64", "3x3", None, 1), ("g64", "3x3s2", None, 1), ("g64", "3x3s2", None, 2),
    ("g128x32_4", "1x1cat", None, 1), ("g128x32_4", "1x1", None, 1), ("g128x32_4", "1x1cat", None, 2), ("g128x32_4", "1x1", None, 2),
    ("g128x32_4", "3x3", None, 1), ("g128x32_4", "3x3", None, 2), ("g128x32_4", "3x3s2", None, 1), ("g128x32_4", "3x3s2", None, 2),
    ("g128x64_3", "1x1cat", None, 1), ("g128x64_3", "1x1", None, 1), ("g128x64_3", "1x1cat", None, 2), ("g128x64_3", "1x1", None, 2),
    ("g128x64", "3x3", None, 1), ("g128x64_3", "3x3", None, 1), ("g128x64_3", "3x3", "inplace16", 1), ("g128x64_3", "3x3", "inplace16", 2),
    ("g128x64_3", "3x3s2", None, 1), ("g128x64_3", "3x3s2", None, 2),
    ("g128x128", "1x1cat_k384", None, 1), ("g128x128_row64", "1x1_k128", None, 1), ("g128x128", "1x1_k512", None, 1),
    ("g128x128", "1x1cat_k384", None, 2), ("g128x128", "1x1_k256", None, 2), ("g128x128", "3x3s2", None, 1),
    ("big128", "1x1_k256", None, 2), ("big128", "3x3s2", None, 1), ("big128", "3x3s2", None, 2),
    ("one_tile", "3x3s2", None, 1), ("one_tile", "3x3s2", None, 2),
]


def _plan_cases() -> List[DCase]:
    out = []
    for tile, loader, res, planes in _PLAN_ROUTES:
        v, pf, cout, exp, cprw, ns = _TILES[tile]
        k, stride, cin, cat = _LOADERS[loader]
        name = f"plan-{tile}-{loader}" + ("-inplace16" if res else "") + f"-{planes}p"
        out.append(DCase(name, 2, cin, 13, 21, cout, k, exp, stride=stride, variant=v, res=res, phase_flags=pf, cat=cat,
                         ext=(int(cat == 0), 0, cprw, ns), dtypes=("f16s",) if planes == 2 else ("f16", "bf16")))
    return out


CASES: List[DCase] = _build() + _plan_cases()
STREAM_CUS = 256                                        # blocks the streaming launcher starts at most on the MI355X (its CU count)

# Extended route keys a detector plan logs that no case reaches with the same key, and the covered key whose code they run; one line
# each with the reason.  A merge never crosses MERGE_FIXED.
MERGED: Dict[Tuple[int, ...], Tuple[Tuple[int, ...], str]] = {}


def key_of(**kw) -> Tuple[int, ...]:
    return tuple(int(kw[f]) for f in KEY_FIELDS)


def describe(key: Tuple[int, ...]) -> str:
    d = dict(zip(KEY_FIELDS, key))
    d["kernel"] = ec.KERNEL_NAMES[d["kernel"]]
    return " ".join(f"{k}={v}" for k, v in d.items())


# ---- what the selector gives, without a device ---------------------------------------------------------------------------------------------
def _ask(d, s0, s1, res, phase_flags) -> Tuple[int, Tuple[int, ...]]:
    from clearcam_amd import _lib
    L = _lib.lib()
    choice = (C.c_int * 8)(*([-1] * 8))
    try:
        if phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", phase_flags))
        code = L.cc_dev_conv_det_choice(C.byref(d), C.byref(s0), C.byref(s1) if s1 is not None else None, res, FAKE_OUT, choice)
    finally:
        if phase_flags is not None:
            _lib.check(L.cc_dev_set(b"phase_flags", -1))
    return code, tuple(choice)


def desc_of(c: ec.Case, dtype: str):
    """cc_conv_desc of a Case / DCase; an in-place residual reads the output's own view."""
    from clearcam_amd import _lib
    inpl = c.res in ("inplace", "inplace16")
    return _lib.ConvDesc(DTI[dtype], c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, c.groups, c.act, c.pad, c.Ho, c.Wo, int(c.out_f32),
                         c.out_cstride, c.out_coff, int(c.res in ("f32", "inplace")), c.out_cstride if inpl else c.res_cstride,
                         c.out_coff if inpl else c.res_coff, c.variant)


def src_descs(c: ec.Case, ptr0: int, ptr1: int):
    """The one or two cc_src_desc of a Case / DCase over dense buffers at ptr0 (and ptr1)."""
    from clearcam_amd import _lib
    cat = getattr(c, "cat", 0)
    if not cat:
        return _lib.SrcDesc(ptr0, c.H, c.W, c.Cin, 0, c.Cin, 0), None
    hh, hw = c.half_hw
    return _lib.SrcDesc(ptr0, hh, hw, cat, 0, cat, 1), _lib.SrcDesc(ptr1, c.H, c.W, c.Cin - cat, 0, c.Cin - cat, 0)


def selector_choice(c: ec.Case, dtype: str) -> Tuple[int, Tuple[int, ...]]:
    """(return code, (kernel, sched, bm, bn, simple, two, cprw, ns)) the library's selector gives a Case / DCase; no launch, no device."""
    from clearcam_amd import _lib
    s0, s1 = src_descs(c, FAKE_IN, FAKE_IN + 0x1000)
    res = None if c.res is None else (FAKE_OUT if c.res in ("inplace", "inplace16") else FAKE_RES)
    return _ask(desc_of(c, dtype), s0, s1, res, c.phase_flags)


def glue_selector_choice(c: gc.ConvCase, dtype: str) -> Tuple[int, Tuple[int, ...]]:
    from clearcam_amd import _lib
    d = _lib.ConvDesc(DTI[dtype], c.B, c.H, c.W, c.Cin, c.Cout, c.k, c.stride, 1, c.act, -1, 0, 0, 0, 0, 0, 0, 0, 0, c.variant)
    s0 = _lib.SrcDesc(FAKE_IN, c.s0.H, c.s0.W, c.s0.cs, c.s0.coff, c.s0.C, c.s0.shift)
    s1 = None if c.s1 is None else _lib.SrcDesc(FAKE_IN + 0x1000, c.s1.H, c.s1.W, c.s1.cs, c.s1.coff, c.s1.C, c.s1.shift)
    return _ask(d, s0, s1, None, c.phase_flags)


@functools.lru_cache(maxsize=None)
def covered_keys() -> Dict[Tuple[int, ...], str]:
    """extended route key -> the first single-launch case that reaches it: this table, the 16-bit cases of epilogue_cases (one plane) and
    the 16-bit and two-plane cases of glue_cases.CONV_CASES.  The older tables declare (kernel, sched, bm, bn) only; the rest of their keys
    is the selector's answer, and a case whose declared part the selector does not confirm is left out (its own GPU test fails)."""
    out: Dict[Tuple[int, ...], str] = {}
    for c in CASES:
        for dt in c.dtypes:
            out.setdefault(c.ext_key(dt), f"detector_route_cases:{c.name}")
    for c in ec.CASES:
        if "f16" not in c.dtypes:
            continue
        code, ch = selector_choice(c, "f16")
        if code == 0 and ch[:4] == c.expect:
            out.setdefault(c.route_key() + (0,) + ch[4:], f"epilogue_cases:{c.name}")
    for c in gc.CONV_CASES:
        if c.refused or c.expect[0] == gc.ADOWN:           # the averaging kernel bypasses launch_conv_chosen: not in the log
            continue
        for dt in c.dtypes:
            if dt == "f32":
                continue
            code, ch = glue_selector_choice(c, dt)
            if code == 0 and ch[:6] == c.expect:
                base = c.expect[:4] + (c.k, c.stride, 0, c.act, ec.RES_NONE, 0, int(c.Cout % 8 == 0))
                out.setdefault(base + (int(dt == "f16s"),) + ch[4:], f"glue_cases:{c.name}")
    return out


def merge_is_legal(key: Tuple[int, ...], to: Tuple[int, ...]) -> bool:
    a, b = dict(zip(KEY_FIELDS, key)), dict(zip(KEY_FIELDS, to))
    return len(key) == NKEY and len(to) == NKEY and all(a[f] == b[f] for f in MERGE_FIXED)


# ---- inputs and the float64 reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def problem(pid, dtype: str):
    """(x NCHW storage values as the loader sees them, w float32 OIHW as handed to the entry, bias, residual or None, the float64 weights the launch multiplies
    by, y64, A = sum |x||w| + |bias| + |res|, the sources as stored - one tensor, or the half-size and the full-size one of a `cat` case);
    shared by the cases that differ only in the kernel forced and never modified.  N(0,1)
    inputs, weights / sqrt(K) as tests/test_gpu_conv_epilogues._problem draws them; two planes keep the float32 weights as they are, one
    plane takes weights representable in the storage type (controlled rounding keeps those)."""
    B, Cin, H, W, Cout, k, stride, groups, act, has_res, cat = pid
    g = torch.Generator().manual_seed(zlib.crc32(repr(pid).encode()) % (2 ** 31))
    sdt = SDT[dtype]
    t = rc.TORCH_T[sdt]
    if cat:
        half = torch.randn(B, cat, (H + 1) // 2, (W + 1) // 2, generator=g).to(t).float()
        full = torch.randn(B, Cin - cat, H, W, generator=g).to(t).float()
        x = torch.cat([half.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :H, :W], full], 1)
        srcs = (half, full)
    else:
        x = torch.randn(B, Cin, H, W, generator=g).to(t).float()
        srcs = (x,)
    cig = Cin // groups
    w = torch.randn(Cout, cig, k, k, generator=g) / (cig * k * k) ** 0.5
    if dtype != "f16s":
        w = w.to(t).float()
    b = torch.randn(Cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = torch.randn(B, Cout, Ho, Wo, generator=g).to(t).float() if has_res else None
    weff = rc.effective_weights([w], sdt, dtype == "f16s")[0]
    y64 = rc.conv64_ex(x, weff, b, stride, groups, act, None, res)
    mag = rc.conv_abs64(x, weff, b, stride, groups, res)
    return x, w, b, res, weff, y64, mag, srcs


# ---- planted faults of the teeth test (tests/test_detector_route_cases_host.py) -----------------------------------------------------------
def dense(w: torch.Tensor, groups: int) -> torch.Tensor:
    """(Cout, Cin / groups, k, k) -> the block-diagonal (Cout, Cin, k, k) tensor pack_convs lays out."""
    if groups == 1:
        return w
    co, cig = w.shape[0], w.shape[1]
    cog = co // groups
    out = torch.zeros(co, cig * groups, w.shape[2], w.shape[3], dtype=w.dtype)
    for gi in range(groups):
        out[gi * cog:(gi + 1) * cog, gi * cig:(gi + 1) * cig] = w[gi * cog:(gi + 1) * cog]
    return out


def high_plane(w: torch.Tensor) -> torch.Tensor:
    """The value of the HIGH plane alone, float64 (restart_check.split_values without its low plane)."""
    import math
    mx = float(w.abs().max())
    e = 14 - (math.frexp(mx)[1] - 1)
    return (w.to(torch.float32) * 2.0 ** e).to(torch.float16).double() * 2.0 ** -e


def faulty_kstep(c: DCase) -> int:
    """The K step the teeth test drops the low plane in: the last one - unless the last pixel tile lies in the bottom row of the last
    image of a padded 3x3 conv, where the last step (tap (2, 2), the row below) multiplies nothing but padding and no fault in it can
    show; there it is the first step that holds low-plane entries (tap (0, 0), the row above)."""
    Ho, Wo = c.out_hw
    M = c.B * Ho * Wo
    last = (2 * c.k * c.k * c.Cin - 1) // c.kstep
    if c.k > 1 and M - (M - 1) // c.pix_tile * c.pix_tile <= Wo:
        return c.Cin // c.kstep
    return last


def kstep_mask(c: DCase, step: int) -> torch.Tensor:
    """(k, k, Cin) bool: the (tap, channel) pairs whose LOW-plane entry lies in K step `step` of the packed row.  The row is
    [tap 0: hi(Cin) | lo(Cin)] [tap 1: hi | lo] ... (yolo.hip pack_convs), walked in steps of `kstep` elements from 0."""
    kk, cin, ks = c.k * c.k, c.Cin, c.kstep
    m = torch.zeros(kk, cin, dtype=torch.bool)
    for tap in range(kk):
        lo0 = (2 * tap + 1) * cin
        for ch in range(cin):
            m[tap, ch] = (lo0 + ch) // ks == step
    return m.reshape(c.k, c.k, cin)


def last_kstep_mask(c: DCase) -> torch.Tensor:
    return kstep_mask(c, (2 * c.k * c.k * c.Cin - 1) // c.kstep)


def planted(c: DCase, prob, fault: str) -> torch.Tensor:
    """round_storage of the float64 result of a launch with `fault` (what a kernel with that fault and no other error returns):
      "no_low"        the low plane missing everywhere;
      "no_low_last"   the low plane missing in one K step (faulty_kstep: the last one where that can show) of the last pixel tile only;
      "nan_row"       the right result with one pixel's channels NaN in the last pixel tile;
      "no_residual"   the right result without the residual."""
    x, w, b, res, weff, y64 = prob[:6]
    Bn, Cc, Ho, Wo = y64.shape
    M = Bn * Ho * Wo
    first_px = (M - 1) // c.pix_tile * c.pix_tile
    if fault == "no_residual":
        return rc.round_storage(rc.conv64_ex(x, weff, b, c.stride, c.groups, c.act, None, None), "f16")
    if fault == "nan_row":
        flat = rc.round_storage(y64, "f16").permute(0, 2, 3, 1).reshape(M, Cc).clone()
        flat[(first_px + M) // 2] = float("nan")
        return flat.reshape(Bn, Ho, Wo, Cc).permute(0, 3, 1, 2)
    wd, hi = dense(weff, c.groups), dense(high_plane(w), c.groups)
    if fault == "no_low":
        return rc.round_storage(rc.conv64_ex(x, hi, b, c.stride, 1, c.act, None, res), "f16")
    assert fault == "no_low_last", fault
    m = kstep_mask(c, faulty_kstep(c)).permute(2, 0, 1).unsqueeze(0)            # (1, Cin, k, k)
    bad = rc.conv64_ex(x, torch.where(m, hi, wd), b, c.stride, 1, c.act, None, res)
    flat = y64.permute(0, 2, 3, 1).reshape(M, Cc).clone()
    flat[first_px:] = bad.permute(0, 2, 3, 1).reshape(M, Cc)[first_px:]
    return rc.round_storage(flat.reshape(Bn, Ho, Wo, Cc).permute(0, 3, 1, 2), "f16")


assert len({c.name for c in CASES}) == len(CASES)
