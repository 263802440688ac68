"""Case table of tests/test_gpu_conv_epilogues.py and the route keys tests/test_gpu_plan_routes.py holds the production plans to
(helper module; not a conftest).

A case is ONE conv launch through cc_conv2d_ex_route (cc_conv2d_ex's launch; it reports the K loop too).  It names the kernel it must reach - `expect` = (kernel, sched, bm, bn), the ConvChoice
fields the entry reports - and the test fails when the selector lands anywhere else.  A case's ROUTE KEY adds what decides the epilogue
code that runs: (kernel, sched, bm, bn, ks, stride, asym, act, residual kind, out_f32, aligned8), the fields of a route-log record
(clearcam_amd/csrc/conv_select.h) without the layer's shape.

That key does not tell apart instantiations of the generic kernel that differ in LDS stages (`ns`: variants 94 / 95, 96 / 97; the plans
take six stages on 32 x 32 tiles for K >= 4096, four below), chunks per row (`cprw`) or loader (`simple`).  The K loop differs - and the
staged epilogues reuse the K ring's LDS (conv_tile.h), so whether stores overtake prefetches still in flight depends on `ns`.  The plans
are therefore held to the EXTENDED key, the eleven fields plus (split, simple, two, cprw, ns) (tests/plan_route_cases.py): every extended
key AdaFace, BlazeFace and CLIP L/14 log has a case here, and the deepest case of a key runs at least min(S_plan, 2 ns + 1) K steps,
S_plan being the steps of the plans' deepest layer under that key (tests/plan_route_table.py).  The cases added for that (the _DEEP_*
tables) name their full route in `ext` = (simple, two, cprw, ns); the older ones keep asserting (kernel, sched, bm, bn) and take the rest
of their extended key from the selector (cc_dev_conv_det_choice answers without a device).
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Tuple

# ConvKernel (conv_select.h)
DIRECT, GENERIC, BIG, PHASE, WS, WAVE, TILE64, STREAM = range(8)
KERNEL_NAMES = ["direct", "generic", "big", "phase", "ws", "wave", "tile64", "stream"]
# PHASE_* schedules
SCHED0, ONE_TILE, BUFFER, PERSIST = range(4)

KEY_FIELDS = ("kernel", "sched", "bm", "bn", "ks", "stride", "asym", "act", "res", "out_f32", "aligned8")
RES_NONE, RES_STORAGE, RES_F32 = 0, 1, 2


@dataclass(frozen=True)
class Case:
    name: str
    B: int
    Cin: int
    H: int
    W: int
    Cout: int
    k: int
    expect: Tuple[int, int, int, int]
    stride: int = 1
    groups: int = 1
    act: int = 0
    variant: int = 0
    pad: int = -1                       # -1: k // 2
    Ho: int = 0                         # 0: the symmetric formula
    Wo: int = 0
    res: Optional[str] = None           # None | "storage" | "f32" | "inplace" (f32 residual that IS the f32 output buffer) | "inplace16" (a
                                        # storage-type residual that IS the 16-bit output buffer: RepNBottleneck's x + cv2(cv1(x)))
    out_f32: bool = False
    out_cstride: int = 0                # 0: Cout
    out_coff: int = 0
    res_cstride: int = 0
    res_coff: int = 0
    phase_flags: Optional[int] = None   # cc_dev_set("phase_flags") around the launch
    dtypes: Tuple[str, ...] = ("f16", "bf16")
    ext: Optional[Tuple[int, int, int, int]] = None   # (simple, two, cprw, ns) the launch must report too (the deep-K cases name their full route)

    @property
    def padv(self) -> int:
        return self.k // 2 if self.pad < 0 else self.pad

    @property
    def sym_out(self) -> Tuple[int, int]:
        return (self.H + 2 * self.padv - self.k) // self.stride + 1, (self.W + 2 * self.padv - self.k) // self.stride + 1

    @property
    def out_hw(self) -> Tuple[int, int]:
        sh, sw = self.sym_out
        return (self.Ho or sh), (self.Wo or sw)

    @property
    def ocs(self) -> int:
        return self.out_cstride or self.Cout

    def route_key(self) -> Tuple[int, ...]:
        (ho, wo), (sh, sw) = self.out_hw, self.sym_out
        res = RES_NONE if self.res is None else (RES_STORAGE if self.res in ("storage", "inplace16") else RES_F32)
        al8 = int(self.Cout % 8 == 0 and self.out_coff % 8 == 0 and self.ocs % 8 == 0)
        return self.expect + (self.k, self.stride, int(ho > sh or wo > sw), self.act, res, int(self.out_f32), al8)

    @property
    def ktot(self) -> int:
        """Elements of one packed weight row that hold weights: groups are densified (net_common.h pack_conv)."""
        return self.k * self.k * self.Cin

    @property
    def ref_id(self):
        """What the float64 reference depends on: cases that differ only in the kernel forced share one."""
        return (self.B, self.Cin, self.H, self.W, self.Cout, self.k, self.stride, self.groups, self.act, self.padv, self.out_hw,
                self.res is not None)


def _epilogues(base: Case, which: str = "g3rf") -> List[Case]:
    """The four epilogues the issue asks of the wide kernels: g act 2, 3 act 3, r 16-bit residual with act 0, f f32 in-place residual + f32 output."""
    out = []
    if "g" in which:
        out.append(replace(base, name=base.name + "-gelu", act=2))
    if "3" in which:
        out.append(replace(base, name=base.name + "-prelu", act=3))
    if "r" in which:
        out.append(replace(base, name=base.name + "-res16", res="storage"))
    if "f" in which:
        out.append(replace(base, name=base.name + "-res32_inplace", res="inplace", out_f32=True))
    return out


def _build() -> List[Case]:
    cs: List[Case] = []
    # ---- generic kernel (variant 2): 128 x 32 tiles for Cout 80 -----------------------------------------------------------------------
    g = Case("gen_3x3_64_80", 2, 64, 13, 21, 80, 3, (GENERIC, 0, 128, 32), variant=2)
    cs += [replace(g, name=f"{g.name}-staged_act{a}", act=a) for a in (2, 3, 4)]
    cs += [replace(g, name=g.name + "-res16", res="storage"), replace(g, name=g.name + "-res16_relu", res="storage", act=4),
           replace(g, name=g.name + "-res32_inplace", res="inplace", out_f32=True), replace(g, name=g.name + "-out32", out_f32=True),
           replace(g, name=g.name + "-res32_prelu_out16", res="f32", act=3),
           replace(g, name="gen_3x3_64_20-staged_gelu", Cout=20, act=2),                       # Cout % 8 != 0: the register path without residual
           replace(g, name="gen_3x3_64_20-res16_relu", Cout=20, act=4, res="storage"),
           replace(g, name=g.name + "-slice_staged_prelu", act=3, out_cstride=96, out_coff=8),
           replace(g, name=g.name + "-slice_res16", res="storage", out_cstride=96, out_coff=8, res_cstride=96, res_coff=8),
           replace(g, name=g.name + "-slice4_res16", res="storage", out_cstride=92, out_coff=4, res_cstride=84, res_coff=4)]
    s2 = Case("gen_1x1_s2_64_128", 2, 64, 14, 14, 128, 1, (GENERIC, 0, 128, 128), stride=2, pad=0, variant=2)   # AdaFace's shortcut conv
    cs += [s2, replace(s2, name=s2.name + "-res16", res="storage")]
    # ---- few-tile configuration (9) and the small pixel tiles (94-97) -------------------------------------------------------------------
    for v, bm in ((9, 128), (94, 64), (95, 64), (96, 32), (97, 32)):
        f = Case(f"small{v}_1x1_64_40", 2, 64, 13, 9, 40, 1, (GENERIC, 0, bm, 32), variant=v)
        cs += [replace(f, name=f.name + "-staged_prelu", act=3), replace(f, name=f.name + "-res16", res="storage")]
    lin = Case("linear_m3_k25088_n512", 3, 25088, 1, 1, 512, 1, (GENERIC, 0, 32, 32), out_f32=True)      # AdaFace's last linear, chosen as the plan chooses
    cs += [lin, replace(lin, name=lin.name + "-small9", variant=9, expect=(GENERIC, 0, 128, 32))]
    # ---- asymmetric padding: BlazeFace's 5x5 s2 pad (1, 2) and depthwise 3x3 s2 pad (0, 2) ----------------------------------------------
    a5 = Case("asym_5x5_s2_8_24", 2, 8, 20, 20, 24, 5, (GENERIC, 0, 128, 32), stride=2, pad=1, Ho=10, Wo=10, act=4, variant=2)
    a3 = Case("asym_dw3x3_s2_24", 2, 24, 16, 16, 24, 3, (GENERIC, 0, 128, 32), stride=2, groups=24, pad=0, Ho=8, Wo=8, variant=2)
    for a in (a5, a3):
        cs += [a, replace(a, name=a.name + "-small9", variant=9), replace(a, name=a.name + "-direct", variant=1, expect=(DIRECT, 0, 128, 128))]
    cs.append(Case("asym_dw3x3_s2_28-direct", 2, 28, 16, 16, 28, 3, (DIRECT, 0, 128, 128), stride=2, groups=28, pad=0, Ho=8, Wo=8))  # Cin % 8 != 0: the selector's own fallback
    # ---- wide kernels: 128 / 256 tiles on four waves (6, 5), the eight-wave kernel's schedules (7) ---------------------------------------
    for nm, B, Cin, H, W, Cout, k in (("big_1x1", 1, 512, 48, 48, 256, 1), ("big_3x3_odd", 1, 192, 17, 19, 512, 3)):
        for tag, v, exp, pf in (("tile256", 5, (BIG, 0, 256, 256), None), ("tile128", 6, (BIG, 0, 128, 128), None),
                                ("phase_one_tile", 7, (PHASE, ONE_TILE, 256, 256), 32), ("phase_sched0", 7, (PHASE, SCHED0, 256, 256), 0),
                                ("phase_buffer", 7, (PHASE, BUFFER, 256, 256), 64), ("persist", 7, (PHASE, PERSIST, 256, 256), 512)):
            cs += _epilogues(Case(f"{nm}-{tag}", B, Cin, H, W, Cout, k, exp, variant=v, phase_flags=pf))
    # 131 x 2 = 262 tiles on at most 256 blocks: some blocks walk two tiles, the second one's first DMA under the first one's epilogue
    pg = Case("persist_gemm_m33300_k64_n512", 1, 64, 185, 180, 512, 1, (PHASE, PERSIST, 256, 256), variant=7, phase_flags=512)
    cs += _epilogues(pg, "gf")
    cs.append(Case("persist_3x3_s2_128_256-res16", 2, 128, 29, 29, 256, 3, (PHASE, PERSIST, 256, 256), stride=2, res="storage", variant=7, phase_flags=512))
    # ---- narrow 3x3 kernels ---------------------------------------------------------------------------------------------------------------
    for tag, v, exp in (("wave", 8, (WAVE, 0, 128, 128)), ("ws", 4, (WS, 0, 128, 128))):
        cs += _epilogues(Case(f"{tag}_64_64_ragged", 2, 64, 13, 21, 64, 3, exp, variant=v), "3r")
    t64 = Case("tile64_ragged", 3, 64, 13, 41, 64, 3, (TILE64, 0, 128, 128), variant=12, res="storage")
    cs += [replace(t64, name=t64.name + "-res16"), replace(t64, name=t64.name + "-res16_silu", act=1)]
    cs.append(Case("stream_256_256_ragged-gelu", 1, 256, 13, 21, 256, 1, (STREAM, 0, 128, 128), variant=10, act=2))
    # ---- direct kernel --------------------------------------------------------------------------------------------------------------------
    d = Case("direct_1x1_28_32", 2, 28, 9, 11, 32, 1, (DIRECT, 0, 128, 128))
    cs += [replace(d, name=d.name + "-res16_relu", act=4, res="storage"), replace(d, name=d.name + "-gelu", act=2),
           replace(d, name=d.name + "-prelu", act=3),
           Case("direct_1x1_96_2-out32", 2, 96, 9, 11, 2, 1, (DIRECT, 0, 128, 128), out_f32=True),
           Case("direct_1x1_96_6-out32", 2, 96, 9, 11, 6, 1, (DIRECT, 0, 128, 128), out_f32=True)]
    # ---- f32 storage ----------------------------------------------------------------------------------------------------------------------
    gf = replace(g, name="f32_gen_3x3_64_80", dtypes=("f32",))
    cs += [replace(gf, name=f"{gf.name}-act{a}", act=a) for a in (1, 2, 3, 4)]
    cs += [replace(gf, name=gf.name + "-res", res="storage"), replace(gf, name=gf.name + "-res_inplace_relu", res="inplace", act=4),
           replace(lin, name="f32_" + lin.name, dtypes=("f32",), expect=(GENERIC, 0, 128, 128), out_f32=False)]
    return cs


CASES: List[Case] = _build()


# ---- what the production plans reach (tests/test_gpu_plan_routes.py) beyond the cases above ------------------------------------------------
# The selector picks the tile by M = B Ho Wo, so AdaFace at B = 1 .. 256, BlazeFace at B = 1 / 32 and CLIP L/14 at B = 1 .. 64 run each of
# their few epilogues on most tile shapes.  One small case per route key they log: the tile is forced, the loader (ks, stride, padding)
# and the epilogue are the plan's.   tile -> (variant, phase_flags, Cout, expect)
_TILES = {
    "g32": (97, None, 40, (GENERIC, 0, 32, 32)), "g64": (95, None, 40, (GENERIC, 0, 64, 32)), "g128x32": (9, None, 40, (GENERIC, 0, 128, 32)),
    "g128x64": (2, None, 64, (GENERIC, 0, 128, 64)), "g128x128": (2, None, 128, (GENERIC, 0, 128, 128)),       # K < 1024 keeps 128 x 128 off conv_big
    "big128": (6, None, 128, (BIG, 0, 128, 128)), "one_tile": (7, 32, 256, (PHASE, ONE_TILE, 256, 256)), "persist": (7, 512, 256, (PHASE, PERSIST, 256, 256)),
}
# loader -> (k, stride, pad, Cin, H, W, Ho, Wo)
_LOADERS = {
    "1x1": (1, 1, 0, 64, 13, 21, 0, 0), "1x1s2": (1, 2, 0, 64, 14, 14, 0, 0), "3x3": (3, 1, 1, 64, 13, 21, 0, 0), "3x3s2": (3, 2, 1, 64, 13, 21, 0, 0),
    "3x3s2_asym": (3, 2, 0, 24, 16, 16, 8, 8), "5x5s2_asym": (5, 2, 1, 8, 20, 20, 10, 10),
}
# (plan that logs it, tile, loader, act, residual, f32 output)
_PLAN_ROUTES = [
    ("adaface", "g32", "1x1s2", 0, None, False), ("adaface", "g32", "3x3", 0, "storage", False), ("adaface", "g32", "3x3", 3, None, False),
    ("adaface", "g32", "3x3s2", 0, "storage", False), ("adaface", "g64", "1x1s2", 0, None, False), ("adaface", "g64", "3x3", 0, "storage", False),
    ("adaface", "g64", "3x3", 3, None, False), ("adaface", "g64", "3x3s2", 0, "storage", False), ("adaface", "g128x32", "1x1s2", 0, None, False),
    ("adaface", "g128x32", "3x3s2", 0, "storage", False), ("adaface", "g128x64", "1x1s2", 0, None, False), ("adaface", "g128x64", "3x3", 0, "storage", False),
    ("adaface", "g128x64", "3x3", 3, None, False), ("adaface", "g128x64", "3x3s2", 0, "storage", False), ("adaface", "g128x128", "3x3", 3, None, False),
    ("adaface", "big128", "3x3s2", 0, "storage", False), ("adaface", "one_tile", "1x1s2", 0, None, False), ("adaface", "one_tile", "3x3s2", 0, "storage", False),
    ("blazeface", "g32", "1x1", 4, None, False), ("blazeface", "g32", "1x1", 4, "storage", False), ("blazeface", "g32", "3x3", 0, None, False),
    ("blazeface", "g32", "3x3s2_asym", 0, None, False), ("blazeface", "g32", "5x5s2_asym", 4, None, False), ("blazeface", "g64", "3x3s2_asym", 0, None, False),
    ("blazeface", "g128x32", "1x1", 4, "storage", False), ("blazeface", "g128x32", "3x3", 0, None, False),
    ("clip", "g32", "1x1", 0, None, False), ("clip", "g32", "1x1", 2, None, False), ("clip", "g32", "1x1", 0, "inplace", True),
    ("clip", "g64", "1x1", 0, None, False), ("clip", "g128x32", "1x1", 0, None, False), ("clip", "g128x32", "1x1", 2, None, False),
    ("clip", "g128x64", "1x1", 0, "inplace", True), ("clip", "g128x128", "1x1", 0, None, False), ("clip", "big128", "1x1", 0, None, False),
    ("clip", "persist", "1x1", 0, None, False),
]


def _plan_cases() -> List[Case]:
    out = []
    for plan, tile, loader, act, res, o32 in _PLAN_ROUTES:
        v, pf, cout, exp = _TILES[tile]
        k, stride, pad, cin, H, W, Ho, Wo = _LOADERS[loader]
        tag = f"act{act}" + ("" if res is None else "_res16" if res == "storage" else "_res32_inplace")
        out.append(Case(f"{plan}-{tile}-{loader}-{tag}", 2, cin, H, W, cout, k, exp, stride=stride, act=act, variant=v, pad=pad, Ho=Ho, Wo=Wo,
                        res=res, out_f32=o32, phase_flags=pf))
    return out


CASES += _plan_cases()


def _detector_cases() -> List[Case]:
    """The detector's epilogues on the families above that had none of them: SiLU (act 1) wherever a family ran act 0 / 2 / 3 / 4 only, and
    SiLU followed by a 16-bit residual that is the output buffer itself (yolo.hip csp_branch: x1 = x1 + cv2(cv1(x1)) in place) on the
    generic 128 x 32 tile, the four-wave 128 x 128 kernel and the persistent loop."""
    by_name = {c.name: c for c in CASES}
    out = []
    silu_of = ["gen_3x3_64_80-staged_act2", "gen_3x3_64_20-staged_gelu", "gen_3x3_64_80-slice_staged_prelu", "gen_1x1_s2_64_128"]
    silu_of += [f"small{v}_1x1_64_40-staged_prelu" for v in (9, 94, 95, 96, 97)]
    silu_of += [f"{nm}-{tag}-gelu" for nm in ("big_1x1", "big_3x3_odd") for tag in ("tile256", "tile128", "phase_one_tile", "phase_sched0", "phase_buffer", "persist")]
    silu_of += ["persist_gemm_m33300_k64_n512-gelu", "wave_64_64_ragged-prelu", "ws_64_64_ragged-prelu", "stream_256_256_ragged-gelu", "direct_1x1_28_32-gelu"]
    for n in silu_of:
        b = by_name[n]
        out.append(replace(b, name=b.name.rsplit("-", 1)[0] + ("-slice_silu" if b.out_cstride else "-silu"), act=1))
    for n in ("gen_3x3_64_80-res16", "big_3x3_odd-tile128-res16", "big_3x3_odd-persist-res16", "persist_gemm_m33300_k64_n512-gelu"):
        b = by_name[n]
        out.append(replace(b, name=b.name.rsplit("-", 1)[0] + "-silu_inplace16", act=1, res="inplace16"))
    out.append(replace(by_name["tile64_ragged-res16_silu"], name="tile64_ragged-silu", res=None))
    return out


CASES += _detector_cases()


# ---- the plans' K loops at their own depth (tests/plan_route_cases.py, tests/plan_route_table.py) -------------------------------------------
# The EXTENDED key adds (split, simple, two, cprw, ns) to the route key: LDS stages and chunks per row pick another instantiation of the
# generic kernel, and the staged epilogues reuse the K ring's LDS, so (stages x epilogue) is what a launch can get wrong.  One case per
# extended key the plans log that the tables above do not reach - or reach with a single K step where the plan's layer runs tens of them.
# K is the only large dimension: the deepest case of a key runs at least min(S_plan, 2 ns + 1) K steps of 8 cprw elements.  These cases
# name their full route (`ext`), and fail when the selector lands elsewhere.
#   tile -> (variant, phase_flags, Cout, expect, cprw, ns);  91 / 93 / 95 / 96 / 97 force the few-tile configurations the selector picks
#   by M, 2 with Cout 24 / 64 / 128 its plain 128-pixel tiles (64-byte rows where a row of K is at most 512 bytes)
_DEEP_TILES = {
    "g32_4": (97, None, 40, (GENERIC, 0, 32, 32), 8, 4), "g32_6": (96, None, 40, (GENERIC, 0, 32, 32), 8, 6),
    "g64_4": (95, None, 40, (GENERIC, 0, 64, 32), 8, 4), "g128x32_4": (91, None, 40, (GENERIC, 0, 128, 32), 8, 4),
    "g128x32_2": (2, None, 24, (GENERIC, 0, 128, 32), 8, 2), "g128x64_3": (93, None, 64, (GENERIC, 0, 128, 64), 8, 3),
    "g128x64_row64": (2, None, 64, (GENERIC, 0, 128, 64), 4, 2), "g128x128": (2, None, 128, (GENERIC, 0, 128, 128), 8, 2),
    "g128x128_row64": (2, None, 128, (GENERIC, 0, 128, 128), 4, 2), "big128": (6, None, 128, (BIG, 0, 128, 128), 8, 2),
    "one_tile": (7, 32, 256, (PHASE, ONE_TILE, 256, 256), 8, 2), "persist": (7, 512, 256, (PHASE, PERSIST, 256, 256), 8, 2),
}
# loader -> (k, stride, pad, Cin, H, W, Ho, Wo): B = 2 on a 13 x 21 map, M = 546 (stride 2: 154; the asymmetric one: 162) is ragged
# against every pixel tile; Cin 96 / 48 / 24 / 592 leave the last K step partly padding
_DEEP_LOADERS = {
    "1x1_k96": (1, 1, 0, 96, 13, 21, 0, 0), "1x1_k592": (1, 1, 0, 592, 13, 21, 0, 0), "1x1_k1024": (1, 1, 0, 1024, 13, 21, 0, 0),
    "1x1_k4096": (1, 1, 0, 4096, 13, 21, 0, 0), "1x1s2_k256": (1, 2, 0, 256, 13, 21, 0, 0),
    "3x3_c8": (3, 1, 1, 8, 13, 21, 0, 0), "3x3_c24": (3, 1, 1, 24, 13, 21, 0, 0), "3x3_c48": (3, 1, 1, 48, 13, 21, 0, 0),
    "3x3_c256": (3, 1, 1, 256, 13, 21, 0, 0), "3x3_c512": (3, 1, 1, 512, 13, 21, 0, 0), "3x3s2_c256": (3, 2, 1, 256, 13, 21, 0, 0),
    "3x3s2_asym_c96": (3, 2, 0, 96, 18, 18, 9, 9),
}
# (plan that logs the key, tile, loader, act, residual, f32 output)
_DEEP_ROUTES = [
    # 32 x 32, four stages: CLIP's text tower and B = 1 (K 768 .. 3072), BlazeFace's 96-channel blocks, AdaFace's shortcut convs
    ("clip", "g32_4", "1x1_k1024", 0, None, False), ("clip", "g32_4", "1x1_k1024", 2, None, False), ("clip", "g32_4", "1x1_k1024", 0, "inplace", True),
    ("blazeface", "g32_4", "1x1_k96", 4, None, False), ("blazeface", "g32_4", "1x1_k96", 4, "storage", False),
    ("blazeface", "g32_4", "3x3s2_asym_c96", 0, None, False), ("adaface", "g32_4", "1x1s2_k256", 0, None, False),
    # 32 x 32, six stages (K >= 4096): CLIP's mlp c_proj at B = 1, AdaFace's 512-channel layers at B = 1
    ("clip", "g32_6", "1x1_k4096", 0, "inplace", True), ("adaface", "g32_6", "3x3_c512", 3, None, False),
    ("adaface", "g32_6", "3x3_c512", 0, "storage", False), ("adaface", "g32_6", "3x3s2_c256", 0, "storage", False),
    # 64 x 32, four stages
    ("clip", "g64_4", "1x1_k1024", 0, None, False), ("adaface", "g64_4", "1x1s2_k256", 0, None, False),
    # 128 x 32, four stages: the selector's own few-tile choice (variant 9 lands on six)
    ("clip", "g128x32_4", "1x1_k1024", 0, None, False), ("clip", "g128x32_4", "1x1_k1024", 2, None, False),
    ("blazeface", "g128x32_4", "1x1_k96", 4, "storage", False), ("blazeface", "g128x32_4", "3x3_c48", 0, None, False),
    ("adaface", "g128x32_4", "1x1s2_k256", 0, None, False), ("adaface", "g128x32_4", "3x3_c256", 3, None, False),
    ("adaface", "g128x32_4", "3x3_c256", 0, "storage", False), ("adaface", "g128x32_4", "3x3s2_c256", 0, "storage", False),
    # 128 x 32, two stages: BlazeFace's 24-channel layers at B = 32 (too many tiles for the few-tile configurations)
    ("blazeface", "g128x32_2", "1x1_k96", 4, "storage", False), ("blazeface", "g128x32_2", "3x3_c24", 0, None, False),
    # 128 x 64, three stages
    ("clip", "g128x64_3", "1x1_k4096", 0, "inplace", True), ("adaface", "g128x64_3", "1x1s2_k256", 0, None, False),
    ("adaface", "g128x64_3", "3x3_c256", 3, None, False), ("adaface", "g128x64_3", "3x3_c256", 0, "storage", False),
    ("adaface", "g128x64_3", "3x3s2_c256", 0, "storage", False),
    # 64-byte rows: AdaFace's conv0 (Cin padded to 8, K = 72) and its widest shortcut conv (K = 256) at B = 256
    ("adaface", "g128x64_row64", "3x3_c8", 3, None, False), ("adaface", "g128x128_row64", "1x1s2_k256", 0, None, False),
    # 128 x 128, two stages: CLIP's patch GEMM at B = 64 (K = 592 keeps it off the single-barrier kernel)
    ("clip", "g128x128", "1x1_k592", 0, None, False),
    # the wide kernels' plain GEMM at CLIP's K, AdaFace's shortcut conv on the eight-wave kernel
    ("clip", "big128", "1x1_k1024", 0, None, False), ("clip", "persist", "1x1_k1024", 0, None, False),
    ("adaface", "one_tile", "1x1s2_k256", 0, None, False),
    # CLIP's text tower at B = 64 (M = 4928: 180 tiles of 256 x 256): the in_proj GEMM without activation, one tile per block
    ("clip", "one_tile", "1x1_k1024", 0, None, False),
]


def _deep_cases() -> List[Case]:
    out = []
    for plan, tile, loader, act, res, o32 in _DEEP_ROUTES:
        v, pf, cout, exp, cprw, ns = _DEEP_TILES[tile]
        k, stride, pad, cin, H, W, Ho, Wo = _DEEP_LOADERS[loader]
        tag = f"act{act}" + ("" if res is None else "_res16" if res == "storage" else "_res32_inplace")
        out.append(Case(f"{plan}-deep-{tile}-{loader}-{tag}", 2, cin, H, W, cout, k, exp, stride=stride, act=act, variant=v, pad=pad, Ho=Ho, Wo=Wo,
                        res=res, out_f32=o32, phase_flags=pf, ext=(1, 0, cprw, ns)))
    # CLIP's final projection, M = B: ONE valid row in the pixel tile at B = 1, 24 channel tiles, f32 output without a residual
    out.append(Case("clip-deep-g32_4-projection_m1_k1024_n768-out32", 1, 1024, 1, 1, 768, 1, (GENERIC, 0, 32, 32), variant=97, pad=0, out_f32=True,
                    ext=(1, 0, 8, 4)))
    return out


CASES += _deep_cases()

assert len({c.name for c in CASES}) == len(CASES)

# What the production plans log is held to the EXTENDED key: plan_route_cases.covered_cases / MERGED (tests/test_gpu_plan_routes.py).
# The eleven-field view below stays for whoever reads a case table by epilogue alone; nothing may be merged on it any more.
MERGED: Dict[Tuple[int, ...], Tuple[Tuple[int, ...], str]] = {}


def covered_keys() -> Dict[Tuple[int, ...], str]:
    """eleven-field route key -> the name of a 16-bit case that reaches it."""
    out: Dict[Tuple[int, ...], str] = {}
    for c in CASES:
        if "f16" in c.dtypes:
            out.setdefault(c.route_key(), c.name)
    return out


def describe(key: Tuple[int, ...]) -> str:
    d = dict(zip(KEY_FIELDS, key))
    d["kernel"] = KERNEL_NAMES[d["kernel"]]
    return " ".join(f"{k}={v}" for k, v in d.items())
