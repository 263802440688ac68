"""GPU parity tests of the detector, all through the C ABI (libclearcam_hip.so via clearcam_amd).

Tolerances (BASELINE.json north_star: "box coords/classes within 1e-3"):
  * f32 mode is the parity gate.  Box coordinates are compared in image-normalised units
    (|dx| <= 1e-3 * max(H, W), i.e. 0.64 px at 640) and scores within 1e-3, with every oracle detection
    matched one-to-one by class and IoU >= 0.9.  Measured: 0.03 px / 5e-5 — the f32 round-off floor
    of a 144-conv network between two different summation orders.
  * f16/bf16 (speed modes) are checked per layer to storage-rounding tolerance and end to end on the
    well-conditioned synthetic checkpoint (perturbation gain ~1) at B=64 640x640.  f16 - the dtype bench.py
    defaults to - is held to the f32 gate's own yardstick (>= 99 % of the detections matched with boxes within
    1e-3 * max(H, W)); bf16 to its own stated bars; a second run keeps the weights un-rounded (see BARS_16BIT).
    The chaotic checkpoint (gain 30-60x) is kept for the f32 gate, where its ~260 detections per frame
    give top-k / NMS real work; its 16-bit end-to-end test is only a guard against gross breakage.
"""
import ctypes as C
import contextlib
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clearcam_amd import _lib
from conftest import noise_frames
from postprocess_cases import split_value
from oracle import yolov9_oracle as yo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "f16s": torch.float16}
DTI = {"f32": 0, "f16": 1, "bf16": 2, "f16s": 3}


def _yolo(size, res, sd, dtype):
    from clearcam_amd.yolov9 import YOLOv9
    return YOLOv9(size, res, state_dict=sd, dtype=dtype, device=0)


def conv_hip(x_nchw, w, b, stride, groups, act, dtype, force_direct=False):
    """cc_conv2d_nhwc on cuda:0: NCHW f32 torch in -> NCHW f32 torch out (storage dtype in between)."""
    L = _lib.lib()
    xd = x_nchw.permute(0, 2, 3, 1).contiguous().to("cuda", TDT[dtype])
    B, H, W_, Cin = xd.shape
    Cout, k = w.shape[0], w.shape[2]
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W_ + 2 * (k // 2) - k) // stride + 1
    out = torch.full((B, Ho, Wo, Cout), float("nan"), dtype=TDT[dtype], device="cuda")   # NaN, not empty: the caching allocator hands back the last
    wn, bn = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())             # call's (correct) output, which hides a kernel that stores nothing
    torch.cuda.synchronize()
    _lib.check(L.cc_conv2d_nhwc(DTI[dtype], _lib.ptr(xd), B, H, W_, Cin, _lib.ptr(wn), _lib.ptr(bn), Cout, k, stride, groups,
                                act, _lib.ptr(out), int(force_direct), None))
    return out.float().cpu().permute(0, 3, 1, 2)


# (name, B, Cin, H, W, Cout, k, stride, groups) — Appendix A's dominant shapes at reduced spatial size + edge cases
CONV_CASES = [
    ("3x3_256_256", 2, 256, 40, 40, 256, 3, 1, 1),
    ("3x3_128_128", 1, 128, 80, 80, 128, 3, 1, 1),
    ("1x1_1024_512", 2, 1024, 20, 20, 512, 1, 1, 1),
    ("3x3_s2_64_128", 1, 64, 64, 64, 128, 3, 2, 1),
    ("3x3_s2_odd_in", 1, 128, 39, 39, 128, 3, 2, 1),      # ADown: conv over the (H-1)x(W-1) avg-pooled map
    ("1x1_cout80", 1, 256, 20, 20, 80, 1, 1, 1),          # head cls logits (N not a tile multiple)
    ("3x3_grouped", 1, 64, 20, 20, 64, 3, 1, 4),          # head box branch, densified
    ("1x1_grouped", 1, 64, 20, 20, 64, 1, 1, 4),
    ("3x3_32_32", 1, 32, 48, 48, 32, 3, 1, 1),
    ("ragged_m", 1, 64, 13, 7, 64, 3, 1, 1),              # M = 91: not a multiple of the 128-pixel tile
]
# (name, B, Cin, H, W, Cout, variant): the specialised 3x3 kernels, forced through cc_conv2d_nhwc's selector (16-bit modes)
SPECIAL_CASES = [
    ("ws_64_64", 5, 64, 24, 48, 64, 4),                  # more tiles than one block's share: the persistent loop
    ("ws_64_64_ragged", 2, 64, 13, 21, 64, 4),
    ("ws_32_32", 3, 32, 16, 32, 32, 4),
    ("ws_32_64", 1, 32, 20, 30, 64, 4),
    ("ws_64_32", 2, 64, 9, 17, 32, 4),
    ("ws_64_48", 1, 64, 16, 16, 48, 4),                  # Cout not a tile multiple
    ("generic_forced", 1, 64, 16, 16, 64, 2),
    ("small_256_256", 1, 256, 20, 20, 256, 9),           # few-tile configuration: 32-wide channel tiles, four LDS stages, 36 K steps
    ("small_128_320", 1, 128, 40, 40, 320, 9),           # ten channel tiles, ragged last pixel tile (M = 1600)
    ("small_64_80", 2, 64, 13, 21, 80, 9),               # Cout not a tile multiple, M = 546
    ("small_forced_big", 4, 64, 80, 80, 576, 9),         # too many blocks for 32-wide tiles: the 64-wide / three-stage form
    ("wave_64_64", 5, 64, 24, 48, 64, 8),                # more sub-tiles than waves: the persistent loop, patch prefetch under the epilogue
    ("wave_64_64_ragged", 2, 64, 13, 21, 64, 8),         # odd height (half-used 2-row sub-tiles), ragged width
    ("wave_32_32", 3, 32, 16, 32, 32, 8),                # sixteen waves per block, 64-byte rows
    ("wave_32_64", 1, 32, 20, 30, 64, 8),
    ("wave_64_32", 2, 64, 9, 17, 32, 8),
    ("wave_1row", 1, 64, 1, 160, 64, 8),
    ("wave_many", 64, 32, 40, 40, 32, 8),                # 51 200 sub-tiles: every wave walks several
]
TOL = {"f32": 2e-5, "f16": 3e-3, "bf16": 2e-2}            # max |err| / max |ref|


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_layer_matches_torch(case, dtype):
    _, B, Cin, H, W_, Cout, k, stride, groups = case
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin // groups, k, k, generator=g) / (Cin // groups * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    xq = x.to(TDT[dtype]).float()                        # the kernel sees storage-rounded inputs/weights
    wq = w.to(TDT[dtype]).float()
    ref = F.silu(F.conv2d(xq, wq, b, stride=stride, padding=k // 2, groups=groups))
    got = conv_hip(x, w, b, stride, groups, 1, dtype)
    assert got.shape == ref.shape
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err <= TOL[dtype], err


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", SPECIAL_CASES, ids=[c[0] for c in SPECIAL_CASES])
def test_specialised_3x3_kernels_match_torch(case, dtype):
    _, B, Cin, H, W_, Cout, variant = case
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b, padding=1))
    got = conv_hip(x, w, b, 1, 1, 1, dtype, force_direct=variant)
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err <= TOL[dtype], err
    generic = conv_hip(x, w, b, 1, 1, 1, dtype, force_direct=2)      # same products, same f32 accumulation order per k-slab? no: only close
    assert float((got - generic).abs().max() / ref.abs().max()) <= TOL[dtype]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", [("1x1_k256", 1, 256, 40, 40, 256, 1, 1), ("1x1_k1024", 1, 1024, 20, 20, 512, 1, 1), ("3x3_s2", 1, 128, 39, 39, 128, 3, 2),
                                  ("1x1_k64", 1, 64, 80, 80, 64, 1, 1), ("3x3_k288", 1, 32, 48, 48, 32, 3, 1)], ids=lambda c: c[0])
def test_few_tile_configuration_matches_default(case, dtype):
    """Variant 9 (narrow channel tiles, 3-4 LDS stages, the batch-1 path) against torch and against the default selection: the
    K order of the accumulation is the same in every MFMA kernel, so the two agree bit for bit."""
    _, B, Cin, H, W_, Cout, k, stride = case
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b, stride=stride, padding=k // 2))
    got = conv_hip(x, w, b, stride, 1, 1, dtype, force_direct=9)
    assert float((got - ref).abs().max() / ref.abs().max()) <= TOL[dtype]
    assert torch.equal(got, conv_hip(x, w, b, stride, 1, 1, dtype, force_direct=2))


@pytest.mark.parametrize("variant", [94, 95, 96, 97])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", [("3x3_k2304", 1, 256, 40, 40, 256, 3, 1), ("3x3_k4608_c64", 1, 512, 20, 20, 64, 3, 1), ("1x1_k1024", 1, 1024, 20, 20, 512, 1, 1),
                                  ("3x3_s2_ragged", 2, 128, 39, 37, 136, 3, 2), ("1x1_ragged", 1, 64, 13, 9, 40, 1, 1)], ids=lambda c: c[0])
def test_small_pixel_tiles_match_generic(case, dtype, variant):
    """The batch-1 configurations of round 6: 64 x 32 (variants 94 / 95: six / four LDS stages) and 32 x 32 (96 / 97) tiles on 256 threads - half and a
    quarter of the DMA issues per wave and K step, twice / four times the blocks.  Same K order, same MFMA: the generic kernel's bits; ragged pixel
    and channel tiles included."""
    _, B, Cin, H, W_, Cout, k, stride = case
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b, stride=stride, padding=k // 2))
    got = conv_hip(x, w, b, stride, 1, 1, dtype, force_direct=variant)
    assert float((got - ref).abs().max() / ref.abs().max()) <= TOL[dtype]
    assert torch.equal(got, conv_hip(x, w, b, stride, 1, 1, dtype, force_direct=2))


# (name, B, Cin, H, W, Cout, k, stride, groups, variant): every kernel family the split-weight mode selects from
SPLIT_CASES = [
    ("generic_3x3", 1, 64, 16, 16, 64, 3, 1, 1, 2),
    ("generic_1x1_k64_thin", 1, 64, 40, 40, 64, 1, 1, 1, 2),          # K = 128 halfs: the 64-byte-row variant
    ("generic_stem_cin8", 1, 8, 64, 64, 64, 3, 2, 1, 0),              # Cin = one chunk: every chunk of a K step is its own virtual tap
    ("generic_cin32_3x3", 1, 32, 48, 48, 32, 3, 1, 1, 2),             # Cin < K step: a step spans two virtual taps
    ("s2_odd_in", 1, 128, 39, 39, 128, 3, 2, 1, 0),
    ("cout80", 1, 256, 20, 20, 80, 1, 1, 1, 0),
    ("grouped_3x3", 1, 64, 20, 20, 64, 3, 1, 4, 0),
    ("ragged_m", 1, 64, 13, 7, 64, 3, 1, 1, 0),
    ("big128_3x3", 1, 128, 40, 40, 128, 3, 1, 1, 6),                  # single-barrier schedule, 128 x 128 tiles
    ("big256_1x1", 2, 1024, 32, 32, 256, 1, 1, 1, 5),                 # 256 x 256 tiles, four waves
    ("phase_3x3", 2, 64, 32, 32, 256, 3, 1, 1, 7),                    # eight-wave kernel (one tile per block / persistent by the tile rule)
    ("phase_1x1_many_tiles", 4, 256, 80, 80, 256, 1, 1, 1, 7),        # 400 tiles of a 1x1: the persistent loop
    ("phase_s2", 2, 128, 33, 33, 256, 3, 2, 1, 7),
    ("small_256_256", 1, 256, 20, 20, 256, 3, 1, 1, 9),               # few-tile configuration
    ("direct", 1, 64, 12, 12, 64, 3, 1, 1, 1),
    ("auto_3x3_64", 2, 64, 40, 40, 64, 3, 1, 1, 0),                   # where plain f16 takes the wave-autonomous / weights-stationary kernels
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_weight_conv_matches_torch(case):
    """dtype "f16s": f16 activations against weights carried as two f16 planes.  The reference is torch's f32 conv over the
    f16-rounded input and the 22-bit weight value the planes hold; the kernel's f16 output must be THAT value rounded to f16 almost
    everywhere (f32 accumulation order only moves a result across an f16 rounding boundary once in a few hundred), which plain
    f16 weights (11 bits) miss on a large share of the outputs."""
    _, B, Cin, H, W_, Cout, k, stride, groups, variant = case
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin // groups, k, k, generator=g) / (Cin // groups * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    xq = x.half().float()
    ref = F.conv2d(xq, split_value(w), b, stride=stride, padding=k // 2, groups=groups)
    got = conv_hip(x, w, b, stride, groups, 0, "f16s", force_direct=variant)
    assert got.shape == ref.shape
    same = float((got == ref.half().float()).float().mean())
    plain = float((ref.half() == F.conv2d(xq, w.half().float(), b, stride=stride, padding=k // 2, groups=groups).half()).float().mean())
    assert same >= 0.99 and float((got - ref).abs().max() / ref.abs().max()) <= 1e-3, (same, plain)
    assert plain < 0.9                                    # the case can tell the two apart
    if variant != 1:                                      # same accumulation order in every MFMA kernel: bit-identical to the generic one
        assert torch.equal(got, conv_hip(x, w, b, stride, groups, 0, "f16s", force_direct=2))


# (name, B, Cin, H, W, Cout): the weights-resident streaming 1x1 kernel (conv_stream.hip, variant 10), every instantiated shape
STREAM_CASES = [
    ("256_256", 2, 256, 40, 40, 256),                     # 50 tiles of 64 pixels
    ("256_256_long", 16, 256, 80, 80, 256),               # 1600 tiles: several per block, the steady-state counted waits
    ("256_256_ragged", 1, 256, 13, 21, 256),              # M = 273: ragged last tile, fewer tiles than ring slots per block
    ("512_256", 2, 512, 40, 40, 256),                     # 32-pixel tiles (plain modes only: two planes would need K = 1024)
    ("128_128", 3, 128, 40, 40, 128),
    ("128_128_ragged", 1, 128, 7, 9, 128),                # M = 63: one partial tile
    ("64_64", 2, 64, 80, 80, 64),
    ("64_64_long", 64, 64, 80, 80, 64),                   # 1600 tiles of 256 pixels
    ("64_64_ragged", 1, 64, 33, 17, 64),
]


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f16s"])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("case", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_stream_1x1_equals_generic(case, act, dtype):
    """Variant 10 (all weights in registers, pixels streamed through an LDS ring, counted vmcnt over DMA pieces and stores) against torch and,
    bit for bit, against the generic tile kernel: same MFMA, same chunk -> k mapping, same (plane, channel) walk, same epilogue."""
    _, B, Cin, H, W_, Cout = case
    if dtype == "f16s" and Cin == 512:
        pytest.skip("two planes of 512 channels exceed the register-resident weight budget: not an instantiated shape")
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000 + act)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    got = conv_hip(x, w, b, 1, 1, act, dtype, force_direct=10)
    generic = conv_hip(x, w, b, 1, 1, act, dtype, force_direct=2)
    assert torch.equal(got, generic)
    if dtype == "f16s":
        ref = F.conv2d(x.half().float(), split_value(w), b)
        tol = 1e-3
    else:
        ref = F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b)
        tol = TOL[dtype]
    if act:
        ref = F.silu(ref)
    assert float((got - ref).abs().max() / ref.abs().max()) <= tol


# (name, B, H, W): the persistent 3x3 64 -> 64 tile kernel (conv_tile64.hip, variant 12)
TILE64_CASES = [
    ("two_rounds", 8, 64, 64),                            # 128 tiles on 128 blocks
    ("long", 24, 80, 96),                                 # 720 tiles: several per block, both patch buffers, stores under the next K loop
    ("ragged", 3, 13, 41),                                # ragged 8 x 32 tiles on both axes, blocks without a tile
    ("one_tile", 1, 8, 32),
    ("narrow", 2, 40, 7),                                 # maps narrower than a fragment
]


@pytest.mark.parametrize("width", [32, 16])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("act", [1, 0])
@pytest.mark.parametrize("case", TILE64_CASES, ids=[c[0] for c in TILE64_CASES])
def test_tile64_3x3_equals_generic(case, act, dtype, width):
    """Variant 12 (weights resident in LDS in fragment order, double-buffered 10 x 34 patches, hand-pipelined taps, accumulator rows permuted
    for 16-byte stores) against torch and, bit for bit, against the generic tile kernel: same MFMA, same (tap, channel) walk, same epilogue."""
    _, B, H, W_ = case
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000 + act)
    x = torch.randn(B, 64, H, W_, generator=g)
    w = torch.randn(64, 64, 3, 3, generator=g) / 24.0
    b = torch.randn(64, generator=g) * 0.1
    L = _lib.lib()
    _lib.check(L.cc_dev_set(b"tile64_w", width))                       # 8 x 32-pixel tiles / 16 x 16 (the launcher otherwise takes whichever covers the map with fewer)
    try:
        got = conv_hip(x, w, b, 1, 1, act, dtype, force_direct=12)
        wg = torch.randn(64, 16, 3, 3, generator=g) / 12.0
        got_grouped = conv_hip(x, wg, b, 1, 4, act, dtype, force_direct=12)
    finally:
        _lib.check(L.cc_dev_set(b"tile64_w", -1))
    generic = conv_hip(x, w, b, 1, 1, act, dtype, force_direct=2)
    assert torch.equal(got, generic)
    ref = F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b, padding=1)
    if act:
        ref = F.silu(ref)
    assert float((got - ref).abs().max() / ref.abs().max()) <= TOL[dtype]
    # the grouped form DDetect's box branch uses (four groups, densified to block-diagonal weights by the caller)
    assert torch.equal(got_grouped, conv_hip(x, wg, b, 1, 4, act, dtype, force_direct=2))


def test_detect_same_bits_with_and_without_stream_kernel():
    """The detector with the streaming 1x1 kernel on (default) and off (cc_dev_set("stream", 0)): identical rows in every storage mode -
    the kernel reads channel-slice views of the Concat buffers there, which the single-layer entry does not exercise."""
    from clearcam_amd.weights import conditioned_yolov9_state_dict
    L = _lib.lib()
    sd = conditioned_yolov9_state_dict("c", 1234)
    frames = np.random.default_rng(5).integers(0, 256, (16, 480, 640, 3), dtype=np.uint8)
    for dtype in ("f16h", "f16s", "bf16"):
        outs = []
        for on in (1, 0):
            _lib.check(L.cc_dev_set(b"stream", on))
            try:
                m = _yolo("c", 640, sd, dtype)
                outs.append(np.array(m.detect_batch(frames)))
                del m
            finally:
                _lib.check(L.cc_dev_set(b"stream", -1))
        assert np.array_equal(outs[0], outs[1]), dtype


def test_specialised_kernels_refuse_ineligible_shapes():
    from clearcam_amd._lib import CCError
    x, w, b = torch.randn(1, 128, 16, 16), torch.randn(64, 128, 3, 3), torch.zeros(64)
    with pytest.raises(CCError):
        conv_hip(x, w, b, 1, 1, 1, "bf16", force_direct=4)           # Cin = 128: not a narrow layer
    x, w = torch.randn(1, 32, 16, 16), torch.randn(64, 32, 3, 3)
    with pytest.raises(CCError):
        conv_hip(x, w, b, 1, 1, 1, "bf16", force_direct=12)          # Cin = 32: not a 64 -> 64 layer
    for variant in (3, 11):                                           # values that name no kernel
        with pytest.raises(CCError, match="names no kernel"):
            conv_hip(x, w, b, 1, 1, 1, "bf16", force_direct=variant)


_LDS_RACE_SCRIPT = r"""
import threading, numpy as np, torch
from clearcam_amd import _lib
L = _lib.lib()
g = torch.Generator().manual_seed(11)
x = torch.randn(2, 40, 40, 64, generator=g).to("cuda", torch.float16)
w = np.ascontiguousarray((torch.randn(64, 64, 3, 3, generator=g) / 24).numpy())
b = np.ascontiguousarray((torch.randn(64, generator=g) * 0.1).numpy())
outs = [torch.full((2, 40, 40, 64), float("nan"), dtype=torch.float16, device="cuda") for _ in range(2)]
torch.cuda.synchronize()
start, errs = threading.Barrier(2), [None, None]
def run(i):
    start.wait()
    if L.cc_conv2d_nhwc(1, _lib.ptr(x), 2, 40, 40, 64, _lib.ptr(w), _lib.ptr(b), 64, 3, 1, 1, 1, _lib.ptr(outs[i]), 12, None) != 0:
        errs[i] = L.cc_last_error().decode()
threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
for t in threads: t.start()
for t in threads: t.join()
assert errs == [None, None], errs
torch.cuda.synchronize()
assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])
"""


def test_first_launch_from_two_threads():
    """Two host threads make a process's first launch of the 160 KB conv_tile64 kernel at the same time: the dynamic-LDS attribute is set once,
    before either launch, so both calls succeed and return the same output."""
    import subprocess
    import sys
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    subprocess.run([sys.executable, "-c", _LDS_RACE_SCRIPT], check=True, env=env, timeout=300)


def test_conv_direct_fallback_odd_channels():
    """YOLOv9-m widths (60/90) are not 16-byte multiples -> the direct kernel must run and agree."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 90, 20, 20, generator=g)
    w = torch.randn(60, 90, 3, 3, generator=g) / 28.0
    b = torch.randn(60, generator=g) * 0.1
    ref = F.silu(F.conv2d(x, w, b, padding=1))
    got = conv_hip(x, w, b, 1, 1, 1, "f32")
    assert float((got - ref).abs().max()) < 1e-4
    forced = conv_hip(torch.randn(1, 64, 16, 16, generator=g), torch.randn(64, 64, 3, 3, generator=g) / 24, b[:60].repeat(2)[:64], 1, 1, 1, "f32", True)
    assert torch.isfinite(forced).all()


def test_letterbox_uint8_bit_exact(sd_t):
    """Integer path (tinygrad uint8 lerp) must be bit-exact: 540x960 -> 360x640 + 12 px zero pad."""
    frames = noise_frames(6, 1, 540, 960)
    m = _yolo("t", 640, sd_t, "f32")
    m.detect_batch(frames)
    got = m.get_tensor("input")                                           # (1,384,640,3) RGB /255
    lb = yo.letterbox(frames[0], 640)
    ref = lb[..., ::-1].astype(np.float32) / np.float32(255.0)
    assert got.shape == (1, 384, 640, 3)
    assert np.array_equal(got[0], ref)


def test_letterbox_float_frames_exact(sd_t):
    frames = noise_frames(7, 1, 270, 480, np.float32)                     # MOT path: Tensor(im).cast(float32)
    m = _yolo("t", 320, sd_t, "f32")
    m.detect_batch(frames)
    ref = yo.letterbox(frames[0], 320)[..., ::-1] / np.float32(255.0)
    assert np.array_equal(m.get_tensor("input")[0], ref.astype(np.float32))


@pytest.mark.parametrize("size,res,seed,shape", [("t", 640, 1, (2, 640, 640, 3)), ("t", 640, 6, (1, 540, 960, 3)),
                                                  ("c", 640, 1, (1, 640, 640, 3))])
def test_detect_f32_matches_oracle_and_golden(size, res, seed, shape, sd_t, sd_c):
    sd = sd_t if size == "t" else sd_c
    frames = noise_frames(seed, *shape[:3])
    o = yo.YOLOv9Oracle(size, res, sd)
    with torch.no_grad():
        feats = o.features(o.network_input(frames))
        dec_ref = yo.decoded_rows(o.decode(o.head_raw(feats)))
    ref = o.detect_batch(frames)
    m = _yolo(size, res, sd, "f32")
    got = m.detect_batch(frames)
    for name, f in zip(("p3", "p4", "p5"), feats):
        r = f.permute(0, 2, 3, 1).numpy()
        rel = np.sqrt(((m.get_tensor(name) - r) ** 2).mean() / (r ** 2).mean())
        assert rel < 2e-4, (name, rel)
    # continuous parity before the discrete top-k/NMS: every anchor the oracle scores clear of the threshold
    dec = m.get_tensor("decoded")
    tol = 1e-3 * max(shape[1], shape[2])
    sure = dec_ref[..., 4] >= 0.25 + 2e-3
    assert sure.sum() > 0
    assert np.abs(dec[..., :4] - dec_ref[..., :4])[sure].max() <= tol
    assert np.abs(dec[..., 4] - dec_ref[..., 4])[sure].max() <= 1e-3
    assert (dec[..., 5] == dec_ref[..., 5])[sure].mean() >= 0.995       # argmax flips only between near-tied classes
    # end to end: one-to-one matches by class and IoU>=0.9; a detection sitting within f32 noise of the 0.25 / 0.45
    # thresholds may flip (the oracle itself flips between two CPUs), hence 99 % rather than 100 %
    gname = {(640, 1, 2): "yolo_t_640", (640, 6, 1): "yolo_t_640_from_540x960"}.get((res, seed, shape[0])) if size == "t" else "yolo_c_640"
    gold = np.load(os.path.join(GOLD, gname + ".npz"))["det"]
    for b in range(shape[0]):
        for target in (ref[b], gold[b]):
            n_ref, n_got, n_match, box_err, sc_err = yo.match_detections(target, got[b], 0.9)
            assert n_ref > 0 and n_match >= 0.99 * max(n_ref, n_got) - 1, (n_ref, n_got, n_match)
            assert box_err <= tol and sc_err <= 1e-3, (box_err, sc_err)
            assert box_err <= 0.32         # f32 round-off floor actually measured: 0.03-0.17 px


@pytest.mark.parametrize("shift", [0.0, 2.0], ids=["compacted", "radix_select"])
def test_decode_topk_nms_exact_given_same_logits(sd_t, shift):
    """Post-processing isolated: oracle decode+postprocess on the HIP head logits == HIP output row for row.  The class-bias shift
    moves the number of anchors over the 0.25 threshold through the three paths of topk_nms_kernel: fewer than 300 positive anchors
    (zero-score anchors fill the top-300 in index order), 300-512 (all positives sorted), more than 512 (radix select)."""
    from clearcam_amd.weights import shift_class_bias
    sd_t = shift_class_bias(sd_t, shift) if shift else sd_t
    frames = noise_frames(1, 2, 640, 640)
    m = _yolo("t", 640, sd_t, "f32")
    got = m.detect_batch(frames)
    n_pos = (m.get_tensor("decoded")[..., 4] > 0).sum(1)             # positive anchors per frame: the case exercises the path it is named after
    assert ((n_pos > 512).any() if shift else ((n_pos < 300).any() and ((n_pos >= 300) & (n_pos <= 512)).any())), n_pos
    raw = [torch.from_numpy(m.get_tensor(f"raw{i}")).permute(0, 3, 1, 2) for i in range(3)]
    o = yo.YOLOv9Oracle("t", 640, sd_t)
    with torch.no_grad():
        ref = o.scale_boxes((640, 640), o.postprocess(o.decode(raw)), (640, 640)).numpy()
    pos = ref[..., 4] > 0
    assert pos.sum() > 100
    assert np.array_equal(ref[..., 5], got[..., 5])                 # same classes in the same rows
    assert np.abs(ref - got)[pos].max() < 2e-3                      # expf/softmax ulps only
    assert np.array_equal(ref[..., 4] > 0, got[..., 4] > 0)


# End-to-end bars of the 16-bit storage modes on the WELL-CONDITIONED checkpoint (clearcam_amd/weights.py
# conditioned_yolov9_state_dict; measured conditioning in clearcam_amd/assets/synth_cond_report.json), at the bench
# configuration (YOLOv9-C, B=64, 640x640).  The yardstick is the f32 gate's own: a detection is matched only when a detection of
# the same class with IoU >= 0.9 AND all four coordinates within 1e-3 * max(H, W) px exists on the other side
# (oracle.match_detections_strict), and the continuous quantity behind it - the decoded box of one and the same anchor - is held to
# the same 1e-3 * max(H, W) wherever both sides score the anchor over the threshold.
#   f16  (the headline dtype of bench.py): per-anchor boxes within 1e-3 * max(H, W) for EVERY anchor both sides report, scores
#        within 2e-3, P3/P4/P5 within 4e-3 relative RMS - the continuous quantities, met with margin (measured 0.39 px, 1.2e-3,
#        1.5e-3) - and >= 98.5 % of the detections matched.  The detection-level figure rides on discrete decisions (the 0.25
#        threshold, NMS among boxes ~20 strides wide that overlap far beyond 0.45) which flip on score differences far inside the
#        tolerance; on this checkpoint it measures 98.9-99.5 % depending on the frames (64 frames: 99.0 %, smoke's 48: 99.0 %
#        clear of the threshold, the bench's 16: 100 %; CPU emulation of the roundings, 64 frames: 99.2 %), so a 99 % bar sits
#        inside its own sampling noise and the asserted bar is 98.5 %.
#   bf16 cannot meet that yardstick on any network: 8 significant bits are 4e-3 relative per rounding, the bar is 1e-3 of the image
#        for boxes that span most of it.  Emulation: 96.5 % of the IoU pairs within 0.64 px, per-anchor p50 0.13 / p99 1.5 / max
#        4.6 px - and keeping DDetect's box branch in f32 changes nothing (the error arrives with P3..P5).  It stays a speed mode
#        with its own, stated bars: >= 90 % strict matches, >= 95 % IoU matches, per-anchor median within 1e-3 * max(H, W),
#        scores within 1e-2, P3/P4/P5 within 3e-2.
BARS_16BIT = {"bf16": 3e-2, "f16": 4e-3, "f16s": 4e-3, "f16h": 4e-3, "f16c": 4e-3}
MATCH_16BIT = {"bf16": 0.90, "f16": 0.985, "f16s": 0.985, "f16h": 0.985, "f16c": 0.985}
SCORE_16BIT = {"bf16": 1e-2, "f16": 2e-3, "f16s": 2e-3, "f16h": 2e-3, "f16c": 2e-3}


_CASES = {}                                            # the last two f32-oracle runs: parametrised tests share their 64-frame case


def conditioned_case(frames, chunk=8, exact=True, emulate=(), seed=1234):
    """f32 oracle over `frames` in chunks (CPU memory): detections (B,300,6), P3/P4/P5 as NHWC arrays, decoded rows (B,A,6).
    `emulate`: storage types whose rounding emulation (oracle/lowprec_oracle.py) is run on the same frames -> {dtype: (det, dec)}."""
    import hashlib
    key = (frames.shape, hashlib.sha256(frames.tobytes()).hexdigest(), chunk, exact, seed)
    if not emulate and key in _CASES:
        return list(_CASES[key])
    out = _conditioned_case(frames, chunk, exact, emulate, seed)
    if not emulate:
        while len(_CASES) >= 2:
            _CASES.pop(next(iter(_CASES)))
        _CASES[key] = tuple(out)
    return out


def _conditioned_case(frames, chunk, exact, emulate, seed):
    from clearcam_amd.weights import conditioned_yolov9_state_dict
    sd = conditioned_yolov9_state_dict("c", seed, exact=exact)        # seeds 1234, 7, 99: three independently calibrated checkpoints
    res = max(frames.shape[1:3])
    o = yo.YOLOv9Oracle("c", res, sd)
    det, dec, feats = [], [], [[], [], []]
    with torch.no_grad():
        for i in range(0, len(frames), chunk):
            x = o.network_input(frames[i:i + chunk])
            f = o.features(x)
            y = o.decode(o.head_raw(f))
            dec.append(yo.decoded_rows(y))
            det.append(o.scale_boxes(tuple(x.shape[2:]), o.postprocess(y), frames.shape[1:3]).numpy())
            for l in range(3):
                feats[l].append(f[l].permute(0, 2, 3, 1).numpy())
    out = [sd, np.concatenate(det), [np.concatenate(f) for f in feats], np.concatenate(dec)]
    if emulate:
        from oracle.lowprec_oracle import LowPrecOracle
        emu = {}
        for dt in emulate:
            lo = LowPrecOracle("c", res, sd, dt, feedback=True)           # the library's controlled weight rounding (yolo.hip round_controlled)
            d2, c2 = [], []
            with torch.no_grad():
                for i in range(0, len(frames), chunk):
                    x = lo.network_input(frames[i:i + chunk])
                    y = lo.decode(lo.head_raw(lo.features(x)))
                    c2.append(yo.decoded_rows(y))
                    d2.append(lo.scale_boxes(tuple(x.shape[2:]), lo.postprocess(y), frames.shape[1:3]).numpy())
            emu[dt] = (np.concatenate(d2), np.concatenate(c2))
        out.append(emu)
    return out


def check_16bit_against_oracle(m, dtype, frames, ref, feats, dec_ref, min_dets):
    """The bars of the 16-bit modes: features, per-anchor scores and boxes of every candidate, strict one-to-one matches."""
    got = m.detect_batch(frames)
    tol = 1e-3 * max(frames.shape[1:3])
    for name, r in zip(("p3", "p4", "p5"), feats):
        rel = np.sqrt(((m.get_tensor(name) - r) ** 2).mean() / (r ** 2).mean())
        assert rel <= BARS_16BIT[dtype], (dtype, name, rel)
    # scores anchor by anchor, for every anchor either side scores over the threshold (the other side's
    # thresholded score may read 0 when it lands just under 0.25: compare those against the threshold itself)
    dec = m.get_tensor("decoded")
    a, b = dec_ref[..., 4], dec[..., 4]
    cand = (a > 0) | (b > 0)
    same_cls = (dec_ref[..., 5] == dec[..., 5]) | (a == 0) | (b == 0)
    sc_err = np.abs(np.where(a > 0, a, 0.25) - np.where(b > 0, b, 0.25))[cand & same_cls].max()
    assert cand.sum() >= min_dets and sc_err <= SCORE_16BIT[dtype], (dtype, sc_err)
    assert (same_cls[cand]).mean() >= 0.99                                   # argmax flips only between near-tied classes
    # unmatched rows whose own score sits within the mode's score tolerance of the 0.25 threshold are the reference's own
    # discontinuity (where(p >= 0.25, p, 0)), not a coordinate error: they leave the denominator of the strict bar, and the raw
    # fraction (every row counted) is bounded next to it.  This checkpoint puts its scores in 0.25..0.4 on purpose, so ~0.7 % of
    # its detections lie within 5e-4 of the threshold - far more than on a trained detector.
    s = yo.parity_summary(ref, got, tol, dec_ref, dec, score_margin=SCORE_16BIT[dtype])
    assert s["n_ref"] >= min_dets, s
    assert s["match_frac_clear_of_threshold"] >= MATCH_16BIT[dtype] and s["match_frac"] >= MATCH_16BIT[dtype] - 0.01, (dtype, s)
    assert s["match_frac_iou_only"] >= 0.95, (dtype, s)
    if dtype in ("f16s", "f16h"):
        assert yo.tolerance_bars(s)["all"], (dtype, yo.tolerance_bars(s), s)  # 99.9 % of the anchors within tol, none beyond 1.5 tol (oracle.tolerance_bars)
        # ... and the stricter form VERDICT r3 named (EVERY anchor within tol): it holds on the frame sets of these tests (results are
        # deterministic: worst anchor 0.375 / 0.303 / 0.351 px in f16h, 0.629 / 0.124 / 0.187 px in f16s; profiles/r04w_final_modes_*.txt),
        # although the worst anchor of a set is a heavy-tailed draw of the f16 activation rounding ("The tail")
        assert s["anchor_box_err_px_max"] <= tol, (dtype, s)
    elif dtype == "f16c":
        # the calibrated mode, whatever the calibration frames were: the detection and score bars of the tolerance modes, 99 % of the anchors
        # within the tolerance and at most 0.3 % beyond it.  The worst anchor of a frame set is a heavy-tailed draw in EVERY f16-activation
        # mode (profiles/r05n_tail_256.txt: exact-weight f16s reads 19 px on one of 256 frames of this checkpoint), so it is not asserted here
        assert yo.tolerance_bars(s)["detections"], (dtype, yo.tolerance_bars(s), s)
        assert s["anchor_box_err_px_p99"] <= tol and s["anchors_over_tol"] <= 0.003 * s["anchors_both_over_thr"], (dtype, s)
    elif dtype == "f16":
        assert s["anchor_box_err_px_max"] <= tol, (dtype, s)                 # 16-bit-exact weights: the same anchor's box, every anchor both sides report
    else:
        assert s["anchor_box_err_px_p50"] <= tol, (dtype, s)
    return s


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_detect_16bit_modes_match_oracle_at_bench_config(dtype):
    """The speed modes end to end at BASELINE configs[1]: B=64, 640x640, YOLOv9-C."""
    frames = noise_frames(1, 64, 640, 640)
    sd, ref, feats, dec_ref = conditioned_case(frames)
    m = _yolo("c", 640, sd, dtype)
    s = check_16bit_against_oracle(m, dtype, frames, ref, feats, dec_ref, min_dets=500)
    print(f"{dtype}: {s}")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_detect_16bit_modes_with_unrounded_weights(dtype):
    """The same network with its float32 weights NOT pre-rounded to 16-bit-exact values: the speed mode's own rounding of the
    weights is inside the comparison.  Two references: (1) the storage-rounding emulation (what a correct 16-bit implementation
    produces - same controlled weight rounding, f32 accumulation in another order): tight; (2) the f32 oracle: with controlled rounding
    (yolo.hip round_controlled) f16 comes close to the f32 gate's bars - 98.8 % strict matches, per-anchor p99 0.37 px, scores within 2e-3
    over 48 frames in the CPU emulation, where round-to-nearest weights gave 92 % / 1.26 px - but not for EVERY anchor (max ~0.95 px):
    the bars below say so; the mode that holds the 0.64 px bar for every anchor is f16s (next test)."""
    frames = noise_frames(1, 16, 640, 640)
    sd, ref, feats, dec_ref, emu = conditioned_case(frames, exact=False, emulate=(dtype,))
    m = _yolo("c", 640, sd, dtype)
    got = m.detect_batch(frames)
    dec = m.get_tensor("decoded")
    tol = 1e-3 * 640
    vs_emu = yo.parity_summary(emu[dtype][0], got, tol, emu[dtype][1], dec)
    vs_f32 = yo.parity_summary(ref, got, tol, dec_ref, dec, score_margin=2e-3)
    print(f"{dtype} un-rounded weights: vs emulation {vs_emu}\n  vs f32 oracle {vs_f32}")
    assert vs_emu["n_ref"] >= 100
    if dtype == "f16":
        assert vs_emu["match_frac"] >= 0.97 and vs_emu["anchor_box_err_px_p99"] <= tol, vs_emu
        assert vs_f32["match_frac_clear_of_threshold"] >= 0.97 and vs_f32["anchor_box_err_px_p99"] <= tol and vs_f32["anchor_score_err_max"] <= 3e-3, vs_f32
    else:
        assert vs_emu["match_frac_iou_only"] >= 0.93 and vs_emu["anchor_box_err_px_p50"] <= tol, vs_emu
        assert vs_f32["match_frac_iou_only"] >= 0.85 and vs_f32["anchor_box_err_px_p50"] <= tol, vs_f32


@pytest.mark.parametrize("dtype", ["f16h", "f16s"])
def test_detect_split_weight_mode_with_unrounded_weights(dtype):
    """dtype "f16s" (f16 activations, every conv's weights as two f16 planes) and "f16h" (two planes in the backbone's 1x1 convs and the stem, one controlled-rounded
    plane elsewhere - see clearcam_amd/yolov9.py: bench.py's default) on the float32 checkpoint AS IT IS - weights not pre-rounded to 16-bit-exact values,
    which is what a trained checkpoint looks like (detection/yolov9.py:372-373 loads f32 safetensors) - against the F32 ORACLE at the bench
    configuration (64 frames): >= 98.5 % strict matches clear of the threshold, scores within 2e-3, P3..P5 within 4e-3, 99.9 % of the anchors
    within 1e-3 * max(H, W) = 0.64 px and none beyond 1.5x that (oracle.yolov9_oracle.tolerance_bars) - and, as VERDICT r3 asked, EVERY anchor
    within 0.64 px on these 64 frames.  Measured on this frame set: the worst
    anchor reads 0.629 px in f16s (and 0.648 px in f16h's first form, which split every backbone conv and so shared f16s's backbone bits) - one
    anchor of frame 20, an ill-conditioned P5 region where this realisation of the f16 ACTIVATION rounding is amplified 3x over the typical worst
    case; every other frame set measured (tools/dev/hybrid_eval.py, three checkpoints) stays below 0.47 px in both modes."""
    frames = noise_frames(1, 64, 640, 640)
    sd, ref, feats, dec_ref = conditioned_case(frames, exact=False)
    m = _yolo("c", 640, sd, dtype)
    s = check_16bit_against_oracle(m, dtype, frames, ref, feats, dec_ref, min_dets=500)
    print(f"{dtype}, un-rounded weights: {s}")
    # ... and the mode is deterministic and batch-invariant like the others (every kernel it selects walks (tap, hi, lo, channel))
    one = _yolo("c", 640, sd, dtype).detect_batch(frames[:1])
    assert np.array_equal(one[0], m.detect_batch(frames)[0])


@pytest.mark.parametrize("seed", [7, 99])
def test_tolerance_modes_on_other_checkpoints(seed):
    """The same bars on two more conditioned checkpoints: another seed's base filters with its OWN data-dependent calibration
    (tools/calibrate_synth.py cond c --seed N -> assets/synth_cond_c_s<N>.npz), float32 weights un-rounded.  "f16h" decides where the low
    weight plane is needed from measurements on one network; this is the check that the choice is not fitted to that checkpoint."""
    frames = noise_frames(seed, 32, 640, 640)
    sd, ref, feats, dec_ref = conditioned_case(frames, exact=False, seed=seed)
    for dtype in ("f16h", "f16s"):
        m = _yolo("c", 640, sd, dtype)
        s = check_16bit_against_oracle(m, dtype, frames, ref, feats, dec_ref, min_dets=250)
        print(f"checkpoint seed {seed}, {dtype}: {s}")
        m.close()


def calibration_frames(kind, n=4):
    """Calibration inputs for dtype "f16c" that are NOT the test frames: white noise from another seed, or deliberately mismatched
    distributions - heavily blurred noise with stretched contrast ("smooth"), 32x32 constant blocks ("blocks")."""
    fr = np.random.default_rng(4242).integers(0, 256, (n, 640, 640, 3), dtype=np.uint8)
    if kind == "smooth":
        x = torch.from_numpy(fr).float().permute(0, 3, 1, 2)
        for _ in range(3):
            x = F.avg_pool2d(F.pad(x, (8, 8, 8, 8), mode="reflect"), 17, 1)
        x = (x - x.mean((2, 3), keepdim=True)) / x.std((2, 3), keepdim=True) * 50 + 128
        fr = x.clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8).numpy().copy()
    elif kind == "blocks":
        fr = np.ascontiguousarray(np.repeat(np.repeat(fr[:, ::32, ::32], 32, 1), 32, 2))
    return fr


# (the driver gives the GPU suite 20 minutes and the pool's hosts differ: the two extra checkpoints of the calibrated mode - ~40 s of CPU oracle -
#  run under CLEARCAM_TEST_FULL=1 only; they passed on the final round-6 sources, profiles/r06f_pytest_gpu.txt)
_F16C_CASES = [(1234, None), (1234, "noise"), (1234, "smooth"), (1234, "blocks")] + ([(7, None), (99, None)] if os.environ.get("CLEARCAM_TEST_FULL") else [])


@pytest.mark.parametrize("seed,calib", _F16C_CASES)
def test_calibrated_mode_holds_the_tolerance_bars(seed, calib):
    """dtype "f16c" (one f16 plane per conv, two in the stem; the 1x1 convs' weights rounded by the calibration-aware recursion at finalize)
    on the conditioned checkpoints with their float32 weights un-rounded, against the f32 ORACLE on the frame sets of the split-weight tests:
    >= 98.5 % strict matches clear of the threshold, scores within 2e-3, 99 % of the anchors within 0.64 px and at most 0.3 % beyond it
    (matched calibration also holds "f16h"'s 99.9 % / 0.96 px bars on these sets with damping 0.01; the 256-frame record in
    profiles/r05n_tail_256.txt is the better statistic).  calib None = the library's default (seeded noise generated inside cc_yolo_finalize); "noise" = other
    white-noise frames handed over through cc_yolo_calibrate; "smooth" / "blocks" = calibration frames from ANOTHER distribution than the
    test frames.  Plain f16 (the same single plane, controlled rounding) fails these bars on two of the three checkpoints."""
    frames = noise_frames(1, 64, 640, 640) if seed == 1234 else noise_frames(seed, 32, 640, 640)
    sd, ref, feats, dec_ref = conditioned_case(frames, exact=False, seed=seed)
    from clearcam_amd.yolov9 import YOLOv9
    m = YOLOv9("c", 640, state_dict=sd, dtype="f16c", calibration_frames=None if calib is None else calibration_frames(calib))
    done, fallback = m.calibration_info()
    assert done >= 50 and fallback == 0, (done, fallback)
    s = check_16bit_against_oracle(m, "f16c", frames, ref, feats, dec_ref, min_dets=500 if seed == 1234 else 250)
    print(f"f16c checkpoint {seed} calibration {calib}: {s}")
    one = m.detect_batch(frames[:1])
    assert np.array_equal(one[0], m.detect_batch(frames)[0])                  # deterministic and batch-invariant like every other mode
    m.close()


def test_calibrated_mode_is_reproducible_and_refuses_misuse(sd_t):
    """Two handles calibrated on the same frames give identical rows (the recursion is deterministic: fixed sample positions, fixed thread-
    independent arithmetic); cc_yolo_calibrate on a handle of another dtype, or after finalize, is an error."""
    from clearcam_amd._lib import CCError
    from clearcam_amd.yolov9 import YOLOv9
    frames = noise_frames(2, 2, 320, 320)
    cal = noise_frames(9, 2, 320, 320)
    a = YOLOv9("t", 320, state_dict=sd_t, dtype="f16c", calibration_frames=cal)
    b = YOLOv9("t", 320, state_dict=sd_t, dtype="f16c", calibration_frames=cal)
    assert np.array_equal(a.detect_batch(frames), b.detect_batch(frames))
    with pytest.raises(ValueError):
        YOLOv9("t", 320, state_dict=sd_t, dtype="f16h", calibration_frames=cal)
    L = _lib.lib()
    assert L.cc_yolo_calibrate(a._h, _lib.ptr(cal), 2, 320, 320, 0) != 0      # after finalize
    a.close(); b.close()


@pytest.mark.parametrize("stress", ["g3", "g10"])
def test_tolerance_modes_on_stress_checkpoints(stress):
    """How far the tolerance claim reaches: the conditioned construction with a measured f32 perturbation gain of ~3-4 ("g3") and ~8-14 ("g10")
    from the network input to P3..P5 (clearcam_amd/assets/synth_cond_report.json; the benign checkpoints read 1.4-1.9, the chaotic one 30-60),
    float32 weights un-rounded, against the f32 CPU oracle.  g3: every f16-activation mode keeps the median anchor within 0.05 px, 97 % of the
    detections strictly matched and all but at most one frame of the set free of anchors beyond the tolerance (profiles/r05p_stress_128.txt:
    one frame of 128 carries every such anchor, in every mode).  g10: no 16-bit mode holds the tolerance - exact-weight f16s included, so it
    is f16 ACTIVATION rounding amplified by the network - and the test only guards against gross breakage (finite rows, f16s at least as
    close as plain f16).  INTEGRATION.md states this limit next to the modes' claims."""
    from clearcam_amd.weights import conditioned_yolov9_state_dict
    frames = noise_frames(31, 16, 640, 640)
    sd = conditioned_yolov9_state_dict("c", 1234, exact=False, stress=stress)
    o = yo.YOLOv9Oracle("c", 640, sd)
    det, dec = [], []
    with torch.no_grad():
        for i in range(0, len(frames), 4):
            y = o.decode(o.head_raw(o.features(o.network_input(frames[i:i + 4]))))
            dec.append(yo.decoded_rows(y)); det.append(o.scale_boxes((640, 640), o.postprocess(y), (640, 640)).numpy())
    ref, dec_ref = np.concatenate(det), np.concatenate(dec)
    med = {}
    for dtype in ("f16h", "f16s", "f16c", "f16"):
        m = _yolo("c", 640, sd, dtype)
        got = m.detect_batch(frames); d = m.get_tensor("decoded"); m.close()
        assert np.isfinite(got).all()
        s = yo.parity_summary(ref, got, 0.64, dec_ref, d)
        both = (dec_ref[..., 4] > 0) & (d[..., 4] > 0)
        bad_frames = int(((np.where(both, np.abs(dec_ref[..., :4] - d[..., :4]).max(-1), 0.0) > 0.64).sum(1) > 0).sum())
        print(f"stress {stress} {dtype}: frames with anchors beyond 0.64 px {bad_frames}/16", {k: round(float(s[k]), 4) for k in ("match_frac", "anchor_box_err_px_p50", "anchor_box_err_px_p99", "anchor_box_err_px_max")})
        med[dtype] = s["anchor_box_err_px_p50"]
        assert s["anchors_both_over_thr"] >= 500, s
        if stress == "g3" and dtype != "f16":
            assert s["anchor_box_err_px_p50"] <= 0.05 and s["match_frac"] >= 0.97 and bad_frames <= 1, (dtype, bad_frames, s)
    assert med["f16s"] <= 1.1 * med["f16"] + 1e-3, med


def test_natural_statistics_frames():
    """Frames with camera-like second-order statistics (clearcam_amd.streams.natural_frames: 1/f spectrum, a flat region, hard-edged
    rectangles) instead of white noise, through the conditioned construction CALIBRATED ON SUCH FRAMES (stress variant "nat": the
    noise-calibrated tables overflow f16 on them, as a network normalised for one distribution would), un-rounded float32 weights, against
    the f32 CPU oracle (every detector parity test ran on white noise).
      f32 mode: the parity gate's bars - features within 2e-4 relative RMS, every matched box within the tolerance, >= 99 % matched.
      f16h / f16s: features within 4e-3, the median anchor within 0.05 px and 99 % of the anchors within 1.5 px.  The TAIL is not
      asserted: on 2-4 % of such frames this synthetic head decodes boxes with gross errors in EVERY f16-activation mode, exact-weight
      f16s included, with features as accurate as on every other frame (profiles/r06g_tail_natural_256.txt, r06h_natural_bad_frames.txt:
      the same frames in every mode) - the DFL expectation of an out-of-distribution frame, not the library; printed for the record."""
    from clearcam_amd.streams import natural_frames
    from clearcam_amd.weights import conditioned_yolov9_state_dict
    frames = natural_frames(12, 640, 640, seed=41)
    sd = conditioned_yolov9_state_dict("c", 1234, exact=False, stress="nat")
    o = yo.YOLOv9Oracle("c", 640, sd)
    det, dec, feats = [], [], [[], [], []]
    with torch.no_grad():
        for i in range(0, len(frames), 4):
            f = o.features(o.network_input(frames[i:i + 4]))
            y = o.decode(o.head_raw(f))
            dec.append(yo.decoded_rows(y)); det.append(o.scale_boxes((640, 640), o.postprocess(y), (640, 640)).numpy())
            for l in range(3):
                feats[l].append(f[l].permute(0, 2, 3, 1).numpy())
    ref, dec_ref, feats = np.concatenate(det), np.concatenate(dec), [np.concatenate(f) for f in feats]
    assert (dec_ref[..., 4] > 0).sum() >= 500                                  # the comparison has anchors to compare
    for dtype in ("f32", "f16h", "f16s"):
        m = _yolo("c", 640, sd, dtype)
        got = m.detect_batch(frames); d = m.get_tensor("decoded")
        rel = [float(np.sqrt(((m.get_tensor(n) - r) ** 2).mean() / (r ** 2).mean())) for n, r in zip(("p3", "p4", "p5"), feats)]
        m.close()
        assert np.isfinite(got).all()
        s = yo.parity_summary(ref, got, 0.64, dec_ref, d)
        print(f"natural frames {dtype}: features {[round(r, 5) for r in rel]}", {k: round(float(s[k]), 4) for k in ("match_frac", "anchor_box_err_px_p50", "anchor_box_err_px_p99", "anchor_box_err_px_max", "anchors_over_tol", "anchors_both_over_thr")})
        if dtype == "f32":
            assert max(rel) < 2e-4 and s["match_frac"] >= 0.99 and s["anchor_box_err_px_max"] <= 0.64 and s["anchor_score_err_max"] <= 1e-3, s
        else:
            assert max(rel) <= 4e-3 and s["anchor_box_err_px_p50"] <= 0.05 and s["anchor_box_err_px_p99"] <= 1.5, (dtype, rel, s)


def test_conditioned_checkpoint_f32_mode():
    """The conditioned checkpoint through the f32 parity mode: the tight f32 bars hold on it too (restored in round 5: the 16-bit
    tolerance modes are judged against the oracle, and this pins the library's own f32 mode to the same oracle on the same network)."""
    frames = noise_frames(3, 8, 640, 640)
    sd, ref, feats, _ = conditioned_case(frames)
    m = _yolo("c", 640, sd, "f32")
    got = m.detect_batch(frames)
    for name, r in zip(("p3", "p4", "p5"), feats):
        assert np.sqrt(((m.get_tensor(name) - r) ** 2).mean() / (r ** 2).mean()) < 2e-4, name
    tot = [0, 0, 0]
    for b in range(8):
        a, c, k, be, se = yo.match_detections(ref[b], got[b], 0.9)
        tot[0] += a; tot[1] += c; tot[2] += k
        assert be <= 0.64 and se <= 1e-3, (be, se)
    assert tot[0] > 50 and tot[2] >= 0.99 * max(tot[0], tot[1]) - 1, tot


@pytest.mark.parametrize("dtype,min_match,feat_rel", [("f16", 0.85, 0.08), ("f16h", 0.85, 0.08), ("f16s", 0.85, 0.08), ("bf16", 0.55, 0.5)])
def test_detect_16bit_modes_on_the_chaotic_checkpoint(dtype, min_match, feat_rel, sd_c):
    """The chaotic seeded checkpoint (perturbation gain 30-60x, clearcam_amd/assets/synth_cond_report.json) amplifies storage rounding: no
    16-bit mode can hold the tolerance bars on it (INTEGRATION.md says so); this guards against gross breakage there - finite rows, features
    within a loose relative bar, most detections found - for every 16-bit mode including the default.  The tight bars are the tests above."""
    frames = noise_frames(1, 2, 640, 640)
    o = yo.YOLOv9Oracle("c", 640, sd_c)
    ref = o.detect_batch(frames)
    with torch.no_grad():
        p3 = o.block_outputs[15].permute(0, 2, 3, 1).numpy()
    m = _yolo("c", 640, sd_c, dtype)
    got = m.detect_batch(frames)
    rel = np.sqrt(((m.get_tensor("p3") - p3) ** 2).mean() / (p3 ** 2).mean())
    assert rel < feat_rel, rel
    for b in range(2):
        n_ref, n_got, n_match, _, _ = yo.match_detections(ref[b], got[b], 0.5)
        assert n_match >= min_match * n_ref and abs(n_got - n_ref) <= 0.15 * n_ref, (n_ref, n_got, n_match)
    assert np.isfinite(got).all()


def test_backbone_split_boundary(monkeypatch, sd_t):
    """dtype "f16h" is "f16s" in some convs and "f16" in the others, nothing else: with every conv up to the last block carrying the low plane
    its rows are f16s's bit for bit, with none plain f16's (development switches CLEARCAM_SPLIT_ALL_LAST / CLEARCAM_SPLIT_1X1_LAST, read when
    the handle is created); the default (the stem conv and the backbone's 1x1 convs) gives rows of its own."""
    frames = noise_frames(5, 2, 320, 320)
    rows = {}
    for name, dt, last in (("f16s", "f16s", None), ("f16", "f16", None), ("all", "f16h", ("99", "99")), ("none", "f16h", ("-1", "-1")), ("default", "f16h", None)):
        for k, env in enumerate(("CLEARCAM_SPLIT_ALL_LAST", "CLEARCAM_SPLIT_1X1_LAST")):
            if last is None:
                monkeypatch.delenv(env, raising=False)
            else:
                monkeypatch.setenv(env, last[k])
        m = _yolo("t", 320, sd_t, dt)
        m.detect_batch(frames)
        rows[name] = np.concatenate([m.get_tensor("decoded")[..., :4].ravel(), m.get_tensor("p5").ravel()])    # every anchor's box + the P5 map
        m.close()
    assert np.array_equal(rows["all"], rows["f16s"]) and np.array_equal(rows["none"], rows["f16"])
    assert not np.array_equal(rows["default"], rows["f16s"]) and not np.array_equal(rows["default"], rows["f16"])


@pytest.mark.parametrize("dtype", ["f16", "bf16", "f16s", "f16h"])
def test_batch_invariance_and_determinism(sd_c, dtype):
    """Size-independent properties at the bench configuration (B=64, 640x640; f16 = the bench's dtype, and bf16)."""
    frames = noise_frames(11, 64, 640, 640)
    m = _yolo("c", 640, sd_c, dtype)
    a = m.detect_batch(frames)
    b = m.detect_batch(frames)
    assert np.array_equal(a, b)                                     # deterministic replay
    one = m.detect_batch(frames[17:18])
    assert np.array_equal(one[0], a[17])                            # a frame's result does not depend on its batch
    dev = m.detect_batch(torch.from_numpy(frames).cuda())           # device-resident frames == host frames
    assert np.array_equal(dev, a)
    s = a[..., 4]
    assert (a[..., :4] >= 0).all() and (a[..., [0, 2]] <= 640).all() and (a[..., [1, 3]] <= 640).all()
    assert ((a[..., 5] >= 0) & (a[..., 5] < 80)).all() and (a[..., 5] == np.floor(a[..., 5])).all()
    for i in range(64):                                             # surviving rows are in descending score order
        nz = s[i][s[i] > 0]
        assert (np.diff(nz) <= 0).all() and (nz >= 0.25).all()
    dead = s == 0
    assert (a[dead][:, :4].max() if dead.any() else 0) <= 640


def test_f16_range_overflow_is_reported(sd_t):
    """f16 activations saturate at 65504; past it they become inf -> NaN logits, which every threshold silently turns into "no detection".
    A checkpoint that does this must be REPORTED: host-output calls fail with a message naming the remedy, device-output calls leave a
    count behind (cc_yolo_nonfinite); bf16 / f32 storage run the same checkpoint fine."""
    from clearcam_amd._lib import CCError
    sd = {k: np.array(v, copy=True) for k, v in sd_t.items()}
    sd["model.list.0.conv.weight"] = sd["model.list.0.conv.weight"] * np.float32(3e5)       # first conv's outputs far beyond 65504
    frames = noise_frames(3, 2, 320, 320)
    for dt in ("f16", "f16s", "f16h"):
        m = _yolo("t", 320, sd, dt)
        with pytest.raises(CCError, match="non-finite"):
            m.detect_batch(frames)
        out = torch.empty(2, 300, 6, device="cuda")
        m.detect_batch_device(torch.from_numpy(frames).cuda(), out)
        torch.cuda.synchronize()
        assert m.nonfinite() > 0 and m.nonfinite() == 0                                      # reported once, then cleared
        m.close()
    for dt in ("bf16", "f32"):
        m = _yolo("t", 320, sd, dt)
        assert np.isfinite(m.detect_batch(frames)).all() and m.nonfinite() == 0
        m.close()
    ok = _yolo("t", 320, sd_t, "f16")                                                         # the unmodified checkpoint: nothing to report
    ok.detect_batch(frames)
    assert ok.nonfinite() == 0


def test_reference_call_surface(sd_t):
    """clearcam.py:582-583 / run_mot.py:33-34 call shapes, through the shims."""
    from clearcam_amd.helpers import Tensor, jit_infer
    m = _yolo("t", 640, sd_t, "f32")
    frame = noise_frames(1, 1, 640, 640)[0]
    cache = {}
    preds = jit_infer(m, Tensor(frame), cache).numpy()
    assert preds.shape == (300, 6) and preds.dtype == np.float32
    mot = m(Tensor(frame).cast("float32")).numpy()
    assert np.array_equal(mot, preds)                               # same integers as floats, identity resize
    boxes, scores, cls = preds[:, :4], preds[:, 4], preds[:, 5].astype(int)   # ocsort.py:194-196
    assert boxes.shape == (300, 4) and scores.max() <= 1 and cls.max() < 80


def test_yolov9_e_graph_matches_oracle():
    """The 43-block "e" graph (CBLinear / CBFuse auxiliary branch, yolov9.py:328-371), f32 parity."""
    from clearcam_amd.weights import synthetic_yolov9_state_dict
    sd = synthetic_yolov9_state_dict("e", 1234)
    frames = noise_frames(1, 1, 640, 640)
    o = yo.YOLOv9Oracle("e", 640, sd)
    with torch.no_grad():
        feats = o.features(o.network_input(frames))
    ref = o.detect_batch(frames)
    m = _yolo("e", 640, sd, "f32")
    got = m.detect_batch(frames)
    for name, f in zip(("p3", "p4", "p5"), feats):
        r = f.permute(0, 2, 3, 1).numpy()
        assert np.sqrt(((m.get_tensor(name) - r) ** 2).mean() / (r ** 2).mean()) < 2e-4, name
    n_ref, n_got, n_match, box_err, sc_err = yo.match_detections(ref[0], got[0], 0.9)
    assert n_ref > 50 and n_match >= 0.99 * max(n_ref, n_got) - 1 and box_err <= 0.64 and sc_err <= 1e-3, (n_ref, n_got, n_match, box_err)
    bf = _yolo("e", 640, sd, "bf16").detect_batch(frames)
    assert np.isfinite(bf).all() and (bf[..., 4] > 0).sum() > 0


def test_small_model_sizes_run(sd_t):
    from clearcam_amd.weights import synthetic_yolov9_state_dict
    for size in ("s", "m"):
        sd = synthetic_yolov9_state_dict(size, 1234)
        frames = noise_frames(2, 1, 640, 640)
        ref = yo.YOLOv9Oracle(size, 640, sd).detect_batch(frames)
        got = _yolo(size, 640, sd, "f32").detect_batch(frames)
        n_ref, n_got, n_match, box_err, sc_err = yo.match_detections(ref[0], got[0], 0.9)
        assert n_match >= 0.99 * max(n_ref, n_got) - 1 and box_err <= 0.64 and sc_err <= 1e-3, (size, n_ref, n_got, n_match)


@pytest.mark.parametrize("size,res", [("t", 320), ("s", 320), ("m", 320), ("e", 320)])
def test_split_weight_mode_all_sizes(size, res):
    """dtypes "f16s" / "f16h" through every graph variant: ELAN1 / AConv (t, s), channel counts off the 16-byte grid -> the direct kernel (m), the
    43-block graph with CBLinear / CBFuse (e).  The seeded checkpoints of these sizes are chaotic (perturbation gain 30-60x), so the check
    is relative: split weights must not be further from the f32 oracle's P3..P5 than plain f16 (whose weights carry 11 bits), and the
    run is finite, deterministic and batch-invariant."""
    from clearcam_amd.weights import synthetic_yolov9_state_dict
    sd = synthetic_yolov9_state_dict(size, 1234)
    frames = noise_frames(7, 2, res, res)
    o = yo.YOLOv9Oracle(size, res, sd)
    with torch.no_grad():
        feats = [f.permute(0, 2, 3, 1).numpy() for f in o.features(o.network_input(frames))]
    rel = {}
    for dt in ("f16s", "f16h", "f16c", "f16"):                # f16c (round 5): the calibration pass through every graph variant as well
        m = _yolo(size, res, sd, dt)
        got = m.detect_batch(frames)
        assert np.isfinite(got).all()
        rel[dt] = [float(np.sqrt(((m.get_tensor(n) - r) ** 2).mean() / (r ** 2).mean())) for n, r in zip(("p3", "p4", "p5"), feats)]
        if dt == "f16c":
            done, fallback = m.calibration_info()
            assert done >= 10 and fallback == 0, (size, done, fallback)
        if dt != "f16":
            assert np.array_equal(got, m.detect_batch(frames)) and np.array_equal(got[1], m.detect_batch(frames[1:2])[0])
        m.close()
    print(size, rel)
    assert all(a <= 1.1 * b + 1e-4 for a, b in zip(rel["f16s"], rel["f16"])), (size, rel)
    assert all(a <= 1.1 * b + 1e-4 for a, b in zip(rel["f16h"], rel["f16"])), (size, rel)
    assert all(a <= 1.5 * b + 1e-4 for a, b in zip(rel["f16c"], rel["f16"])), (size, rel)     # one plane like f16: same ballpark on a chaotic net


BIG_CASES = [
    ("big_1x1", 1, 512, 48, 48, 256, 1),                 # 9 m-tiles of 256 pixels, ragged last tile, 8 K steps
    ("big_1x1_k64", 2, 64, 16, 16, 512, 1),              # a single K step: prologue-only pipeline
    ("big_1x1_k128", 1, 128, 32, 40, 256, 1),            # two K steps
    ("big_3x3", 1, 128, 24, 24, 256, 3),                 # im2col loader with halo taps, 18 K steps
    ("big_3x3_odd", 1, 192, 17, 19, 512, 3),             # K = 1728 = 27 steps (odd), ragged pixels, two channel tiles
]


@pytest.mark.parametrize("variant", [5, 6, 7], ids=["tile256", "tile128", "pingpong256"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", BIG_CASES, ids=[c[0] for c in BIG_CASES])
def test_big_tile_kernel_matches_torch(case, dtype, variant):
    """256x256-tile, four-wave, single-barrier kernel (variant 5) against torch, with and without activation/bias."""
    _, B, Cin, H, W_, Cout, k = case
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.silu(F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b, padding=k // 2))
    got = conv_hip(x, w, b, 1, 1, 1, dtype, force_direct=variant)        # 5: 256x256 tiles, 6: 128x128 tiles, same schedule; 7: eight-wave two-group kernel
    assert float((got - ref).abs().max() / ref.abs().max()) <= TOL[dtype]


PERSIST_CASES = BIG_CASES + [
    ("persist_many_tiles", 40, 256, 48, 48, 512, 1),     # 360 x 2 = 720 tiles on 256 blocks: every block walks 2-3 tiles (next tile's DMA under the epilogue)
    ("persist_3x3_many", 24, 64, 40, 40, 256, 3),        # 150 tiles... one round, 9 K steps of one tap each (retarget every step)
    ("persist_k64_many", 64, 64, 32, 32, 256, 1),        # single K step per tile, 256 tiles
    ("tiles_400", 25, 64, 64, 64, 256, 1),               # M = 102400 (the 40x40 maps of a 64-frame batch): 1.56 rounds of tiles
    ("tiles_400_3x3", 25, 64, 64, 64, 256, 3),
    ("tiles_800_two_channel_tiles", 25, 128, 64, 64, 512, 1),
]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("case", PERSIST_CASES, ids=[c[0] for c in PERSIST_CASES])
def test_persistent_eight_wave_kernel_matches_torch(case, dtype):
    """conv_persist_kernel (persistent tile loop, wave-private LDS-staged epilogue; conv_persist.hip), forced for every shape through
    cc_dev_set("phase_flags", 512), against torch (SiLU and no activation) and, bit for bit, against the one-tile-per-block kernel
    (same accumulation order).  The v_mfma_f32_32x32x16 instantiation (development build, measured slower) passed the same cases in
    rounds r03b / r03d."""
    from clearcam_amd import _lib as lib_
    L = lib_.lib()
    _, B, Cin, H, W_, Cout, k = case
    g = torch.Generator().manual_seed(zlib.crc32(case[0].encode()) % 1000)
    x = torch.randn(B, Cin, H, W_, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    lin = F.conv2d(x.to(TDT[dtype]).float(), w.to(TDT[dtype]).float(), b, padding=k // 2)
    try:
        lib_.check(L.cc_dev_set(b"phase_flags", 512))
        for act, ref in ((1, F.silu(lin)), (0, lin)):
            got = conv_hip(x, w, b, 1, 1, act, dtype, force_direct=7)
            assert float((got - ref).abs().max() / ref.abs().max()) <= TOL[dtype], (case[0], act)
        again = conv_hip(x, w, b, 1, 1, 0, dtype, force_direct=7)
        assert torch.equal(again, got)                                      # deterministic (no race between a tile's epilogue and the next tile's DMA)
        lib_.check(L.cc_dev_set(b"phase_flags", 32))                        # one tile per block, block-wide staged epilogue
        assert torch.equal(conv_hip(x, w, b, 1, 1, 0, dtype, force_direct=7), got)
    finally:
        lib_.check(L.cc_dev_set(b"phase_flags", -1))


_STEM_SCRIPT = r"""
import sys, numpy as np
from clearcam_amd.weights import synthetic_yolov9_state_dict
from clearcam_amd.yolov9 import YOLOv9
size, res, dtype, H, W, f32 = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
frames = np.random.default_rng(5).integers(0, 256, (2, H, W, 3), dtype=np.uint8)
if f32: frames = frames.astype(np.float32)
m = YOLOv9(size, res, state_dict=synthetic_yolov9_state_dict(size, 1234), dtype=dtype, device=0)
if len(sys.argv) > 8:                                  # device frames that start at an odd byte address
    import torch
    raw = torch.zeros(frames.size + 8, dtype=torch.uint8, device="cuda")
    off = int(sys.argv[8])
    raw[off:off + frames.size] = torch.from_numpy(frames.reshape(-1)).cuda()
    det = m.detect_batch(raw[off:off + frames.size].view(frames.shape))
else:
    det = m.detect_batch(frames)
np.savez(sys.argv[7], stem=m.get_tensor("stem"), inp=m.get_tensor("input"), det=det)
"""


@pytest.mark.parametrize("size,res,dtype,H,W,f32", [("t", 320, "bf16", 270, 480, 0), ("c", 640, "bf16", 640, 640, 0), ("s", 320, "f16", 320, 200, 1),
                                                    ("t", 640, "bf16", 1080, 1920, 0),      # 3x downscale: 100-row source rectangles staged in LDS
                                                    ("t", 320, "f16", 199, 301, 0),         # W*3 % 4 != 0: every source row starts at another byte offset
                                                    ("s", 640, "bf16", 2160, 3840, 0),      # 6x downscale: rectangle too large for LDS, direct loads
                                                    ("t", 320, "bf16", 90, 160, 0),         # upscale
                                                    ("c", 640, "f16s", 640, 640, 0),        # split weights: a second MFMA on the low plane
                                                    ("t", 320, "f16s", 270, 480, 0)])
def test_fused_letterbox_stem_equals_unfused(tmp_path, size, res, dtype, H, W, f32):
    """stem_fused_kernel (letterbox + first conv from the frames) against the unfused path (preprocess_kernel -> generic conv)
    and against the oracle's first layer: same inputs rounded the same way, one MFMA K step instead of two, so at most a
    last-place difference of the 16-bit result; the "input" tap is rebuilt on demand and must be identical."""
    import subprocess
    import sys
    outs = []
    for fuse in ("0", "1"):
        path = str(tmp_path / f"stem{fuse}.npz")
        env = dict(os.environ, CLEARCAM_FUSE_STEM=fuse, CLEARCAM_TAP_STEM="1",
                   PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        extra = ["3"] if (H, W) == (199, 301) else []                          # that case also hands over a misaligned device pointer
        subprocess.run([sys.executable, "-c", _STEM_SCRIPT, size, str(res), dtype, str(H), str(W), str(f32), path] + extra, check=True, env=env)
        outs.append(np.load(path))
    a, b = outs
    assert np.array_equal(a["inp"], b["inp"])                                  # the tap is the same tensor in both modes
    ulp = 2.0 ** -7 if dtype == "bf16" else 2.0 ** -10                         # spacing of the storage type relative to |x| (upper bound)
    d = np.abs(a["stem"] - b["stem"])
    assert (d <= ulp * np.maximum(np.abs(a["stem"]), 2.0 ** -6) * 1.01).all(), float(d.max())   # one unit in the last place at most
    assert (d > 0).mean() < 0.02                                               # and rarely that
    # first layer of the oracle on the same (rounded) input: SiLU(conv3x3 s2)
    from clearcam_amd.weights import synthetic_yolov9_state_dict
    sd = synthetic_yolov9_state_dict(size, 1234)
    x = torch.from_numpy(b["inp"]).permute(0, 3, 1, 2)
    wq = torch.from_numpy(sd["model.list.0.conv.weight"])
    wq = split_value(wq) if dtype == "f16s" else wq.to(TDT[dtype]).float()
    ref = F.silu(F.conv2d(x, wq, torch.from_numpy(sd["model.list.0.conv.bias"]), stride=2, padding=1)).permute(0, 2, 3, 1).numpy()
    assert np.abs(b["stem"] - ref).max() <= 2 * ulp * max(1.0, float(np.abs(ref).max()))
    n0, n1, nm, _, _ = yo.match_detections(a["det"][0], b["det"][0], 0.5)
    assert nm >= 0.7 * max(n0, n1, 1) - 1                                      # end to end the two modes stay the same detector


_CSP_SCRIPT = r"""
import sys, numpy as np
from clearcam_amd.weights import conditioned_yolov9_state_dict, synthetic_yolov9_state_dict
from clearcam_amd.yolov9 import YOLOv9
size, res, dtype, H, W, B, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), sys.argv[7]
frames = np.random.default_rng(5).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
sd = conditioned_yolov9_state_dict(size, 1234) if size == "c" else synthetic_yolov9_state_dict(size, 1234)
m = YOLOv9(size, res, state_dict=sd, dtype=dtype, device=0)
d = {"det": m.detect_batch(frames)}
def grab(n):                                             # B > 16: a digest of every frame (several GB as float32) + the last two frames
    if B <= 16: return m.get_tensor(n)
    import hashlib
    h = hashlib.sha256()
    for b0 in range(0, B, 8): h.update(m.get_tensor(n, (b0, min(8, B - b0))).tobytes())
    d[n + "_last"] = m.get_tensor(n, (B - 2, 2))
    return np.frombuffer(h.digest(), np.uint8)
for k in range(16):
    try: d[f"csp{k}_u"] = grab(f"csp{k}_u")
    except Exception: pass
for n in ("p3", "p4", "p5"): d[n] = grab(n)
d["launches"] = np.array(m.profile(iters=1)["conv_launches"])
np.savez(out, **d)
"""


@pytest.mark.parametrize("size,res,dtype,H,W,B,level,fused", [
    # round 6: csp_tile_kernel (hidden width 32: weights resident in LDS in fragment order, 16 x 32 tiles, register-chained 1x1 convs) is taken
    # from one round of tiles on (256 tiles: B >= 6 at 160 x 160); level "1t" / "2t" force it at these small batches (CLEARCAM_CSP_TILE=2)
    ("c", 640, "bf16", 640, 640, 3, "1t", 2),     # one weight plane, bf16; three frames: blocks with one tile and blocks with none
    ("c", 640, "f16h", 640, 640, 1, "2t", 6),     # two planes in the 1x1 convs (68 KB of weights resident); 50 tiles on 48 blocks
    ("c", 608, "f16h", 608, 608, 2, "2t", 6),     # 152 x 152 maps: ragged 16 x 32 tiles on both axes
    ("c", 640, "f16", 270, 480, 2, "2t", 6),      # letterboxed 384 x 640: 96 x 160 maps
    ("m", 320, "f16", 320, 320, 2, "1t", 2),      # YOLOv9-m: hidden width 32 at 80 x 80
    ("c", 640, "f16h", 640, 640, 6, "2", 6),      # 300 tiles: the kernel by its own rule
    ("c", 640, "bf16", 640, 640, 3, "1", 2),      # the bench plan's shapes: hidden width 32 at 160x160 (weights resident, persistent blocks)
    ("c", 640, "f16", 640, 640, 1, "2", 6),       # + hidden width 64 at 80x80 (weights streamed); a single frame: fewer tiles than CUs
    ("c", 608, "bf16", 608, 608, 2, "2", 6),      # 152 x 152 and 76 x 76 maps: ragged 8 x 16 tiles on both axes
    ("c", 640, "bf16", 270, 480, 2, "2", 6),      # letterboxed 384 x 640: non-square maps
    ("m", 320, "f16", 320, 320, 2, "1", 2),       # YOLOv9-m: one bottleneck per RepNCSP, hidden width 32 at 80x80
    ("c", 640, "f16s", 640, 640, 1, "2", 6),      # split weights: both widths stream their two planes (tap, plane, channel order)
    ("c", 608, "f16s", 608, 608, 2, "2", 6),      # ... ragged tiles
    ("c", 640, "f16h", 640, 640, 1, "2", 6),      # round 5: two planes in the 1x1 convs only (the four backbone blocks), one plane everywhere (the two neck blocks)
    ("c", 608, "f16h", 608, 608, 2, "2", 6),      # ... ragged tiles
    ("c", 640, "f16h", 640, 640, 11, "2", 2),     # round 6: from one round of conv_tile64's tiles on (25 per frame at 80 x 80: B >= 11) level 2 leaves hidden width 64 to the four launches ...
    ("c", 640, "f16h", 640, 640, 11, "3", 6),     # ... level 3 fuses it at every batch size
    ("c", 640, "f16h", 640, 640, 64, "2", 2),     # the bench batch: csp_tile_kernel at 160 x 160 (1600 tiles), hidden width 64 left to the four launches
])
def test_fused_csp_equals_unfused(tmp_path, size, res, dtype, H, W, B, level, fused):
    """csp_fused_kernel (cv1|cv2, RepConvN 3x3, 3x3 + shortcut, cv3 of a RepNCSP in one launch, intermediates in LDS) against the
    four launches it replaces: every intermediate is rounded where the layer-at-a-time path stores it and every accumulation runs
    in the same K order, so block outputs, P3-P5 and the detections are IDENTICAL, bit for bit."""
    import subprocess
    import sys
    outs = []
    for lv in ("0", level):
        path = str(tmp_path / f"csp{lv}.npz")
        env = dict(os.environ, CLEARCAM_FUSE_CSP=lv.rstrip("t"), CLEARCAM_CSP_TILE="2" if lv.endswith("t") else "1", CLEARCAM_TAP_CSP="1",
                   PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", _CSP_SCRIPT, size, str(res), dtype, str(H), str(W), str(B), path], check=True, env=env)
        outs.append(np.load(path))
    a, b = outs
    assert int(a["launches"]) - int(b["launches"]) == 3 * fused                # four launches became one, `fused` times
    names = [n for n in a.files if n.startswith("csp")]
    assert len(names) >= fused
    for n in names + ["p3", "p4", "p5", "det"]:
        assert np.array_equal(a[n], b[n]), n
    p3 = a["p3_last"] if "p3_last" in a.files else a["p3"]
    assert np.abs(p3).max() > 0.05 and np.isfinite(p3).all()


def test_tile64_in_the_detector_same_bits(tmp_path):
    """The persistent 3x3 64 -> 64 tile kernel inside the detector (eleven frames: one round of its tiles at 80 x 80 and 160 x 160), layer at a time so that
    it also takes the RepNBottleneck convs that carry the shortcut (16-bit residual added after the activation), against the same plan with
    CLEARCAM_TILE64=0 (wave-autonomous kernel, register epilogue): block outputs, P3-P5 and detections identical."""
    import subprocess
    import sys
    outs = []
    for t64 in ("0", "1"):
        path = str(tmp_path / f"t64_{t64}.npz")
        env = dict(os.environ, CLEARCAM_TILE64=t64, CLEARCAM_FUSE_CSP="0", CLEARCAM_TAP_CSP="1", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", _CSP_SCRIPT, "c", "640", "f16h", "640", "640", "11", path], check=True, env=env)
        outs.append(np.load(path))
    a, b = outs
    for n in [n for n in a.files if n.startswith("csp")] + ["p3", "p4", "p5", "det"]:
        assert np.array_equal(a[n], b[n]), n
    assert (a["det"][..., 4] > 0).sum() > 10


def test_pool_rows_per_thread_same_bits(tmp_path):
    """ADown's pools with eight / four output rows per thread (2x2 average; the avg-max kernel takes two) against one row per thread
    (CLEARCAM_POOL_ROWS, read once per process): every output sums its taps in the same order, so features and detections are IDENTICAL -
    on maps whose height is not a multiple of the rows per thread (270 x 480 frames: 152 x 160 letterboxed maps at stride 4 -> 79, 39, 19 rows)."""
    import subprocess
    import sys
    outs = []
    for rows in ("1", "4", "8"):
        path = str(tmp_path / f"pool{rows}.npz")
        env = dict(os.environ, CLEARCAM_POOL_ROWS=rows, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", _CSP_SCRIPT, "c", "640", "f16", "270", "480", "3", path], check=True, env=env)
        outs.append(np.load(path))
    for other in outs[1:]:
        for n in ("p3", "p4", "p5", "det"):
            assert np.array_equal(outs[0][n], other[n]), n
    assert (outs[0]["det"][..., 4] > 0).sum() > 10


@pytest.mark.parametrize("dtype", ["f16", "f16s"])
def test_head_entry_split_equals_single_launch(tmp_path, dtype):
    """DDetect's two entry convs per level (box 64 + class 256 channels over the same map) as two launches - the class conv on the
    eight-wave 256-wide kernel - against the single 320-channel launch (CLEARCAM_HEAD_SPLIT=0): every channel's K walk is the same, so
    the detections are IDENTICAL; three more conv launches per plan."""
    import subprocess
    import sys
    outs = []
    for on in ("0", "1"):
        path = str(tmp_path / f"head{on}.npz")
        env = dict(os.environ, CLEARCAM_HEAD_SPLIT=on, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", _CSP_SCRIPT, "c", "640", dtype, "640", "640", "3", path], check=True, env=env)
        outs.append(np.load(path))
    a, b = outs
    assert int(b["launches"]) - int(a["launches"]) == 3
    assert np.array_equal(a["det"], b["det"]) and (a["det"][..., 4] > 0).sum() > 10


@pytest.mark.parametrize("size,res,dtype,shape", [
    ("c", 640, "f16", (3, 640, 640, 3)),          # the bench network: class branch 256 wide; 3 frames: ragged 64-pixel tiles at 20x20
    ("c", 640, "bf16", (2, 270, 480, 3)),         # letterboxed 384 x 640: non-square maps
    ("s", 320, "f16", (5, 320, 320, 3)),          # class branch 128 wide
    ("e", 640, "bf16", (1, 640, 640, 3)),         # the 43-block graph's head (model.list.42)
    ("c", 640, "f16s", (3, 640, 640, 3)),         # split weights: rows [hi | lo] in LDS, the pixel fragments walked twice
    ("s", 320, "f16s", (2, 200, 320, 3)),         # ... class branch 128 wide, non-square maps
])
def test_fused_ddetect_tail_equals_unfused(size, res, dtype, shape):
    """head_tail_kernel (DDetect's last 1x1 convs of both branches + DFL + dist2bbox + sigmoid + class max in one launch, the 144
    logits per anchor never written) against the three launches per level + decode_kernel it replaces: same MFMA accumulation order,
    decode_kernel's own arithmetic -> the decoded rows of every anchor and the detections are IDENTICAL, bit for bit."""
    from clearcam_amd.weights import conditioned_yolov9_state_dict, synthetic_yolov9_state_dict
    sd = conditioned_yolov9_state_dict("c", 1234) if size == "c" else synthetic_yolov9_state_dict(size, 1234)
    frames = noise_frames(4, *shape[:3])
    res_ = {}
    for label, env in (("unfused", "0"), ("fused", "1")):
        os.environ["CLEARCAM_FUSE_HEAD"] = env                                # read when the plan is built (first call of a shape)
        try:
            m = _yolo(size, res, sd, dtype)
            det = m.detect_batch(frames)
            dec = m.get_tensor("decoded")
            os.environ["CLEARCAM_PROFILE_CSV"] = "/tmp/_tail_profile.csv"
            prof = m.profile(iters=1)
            has_raw = True
            try:
                m.get_tensor("raw0")
            except Exception:                                                 # noqa: BLE001
                has_raw = False
            res_[label] = (det, dec, prof["conv_launches"], has_raw)
            m.close()
        finally:
            os.environ.pop("CLEARCAM_FUSE_HEAD", None); os.environ.pop("CLEARCAM_PROFILE_CSV", None)
    (d0, c0, n0, raw0), (d1, c1, n1, raw1) = res_["unfused"], res_["fused"]
    assert raw0 and not raw1                                                  # the logits are not materialised any more
    assert n0 - n1 == 6                                                       # two conv launches per level became part of the tail
    assert np.array_equal(c0, c1)                                             # every anchor's decoded row
    assert np.array_equal(d0, d1)
    assert (c1[..., 4] > 0).sum() > 0 and np.isfinite(c1).all()


@pytest.mark.parametrize("size,res,dtype,shape", [
    ("c", 640, "f16", (3, 640, 640, 3)),          # the bench network
    ("c", 640, "f32", (2, 270, 480, 3)),          # f32: the unfused DDetect tail (five launches per level + decode) on its lanes
    ("t", 320, "bf16", (4, 320, 320, 3)),         # ELAN1 + AConv graph (no pooled ADown half)
    ("e", 640, "f16", (1, 640, 640, 3)),          # the 43-block graph: CBLinear / CBFuse between the lanes' producers
])
def test_concurrent_lanes_equal_one_chain(size, res, dtype, shape):
    """The captured plan with independent chains on their own streams (each DDetect level on a lane, ADown's pooled half on another:
    CLEARCAM_LANES=3, every fork the builder knows) against the same launches as ONE chain (CLEARCAM_LANES=0).  The kernels are the
    same and deterministic, so detections and every decoded row must be IDENTICAL - a missing dependency edge or a buffer shared
    between two launches that may now overlap would show as a difference (or as NaNs) on some replay; three replays each."""
    from clearcam_amd.weights import conditioned_yolov9_state_dict, synthetic_yolov9_state_dict
    sd = conditioned_yolov9_state_dict("c", 1234) if size == "c" else synthetic_yolov9_state_dict(size, 1234)
    frames = noise_frames(9, *shape[:3])
    got = {}
    for label, env in (("chain", "0"), ("lanes", "3"), ("one_head_lane", "5")):
        os.environ["CLEARCAM_LANES"] = env                                    # read when the plan is built (first call of a shape)
        try:
            m = _yolo(size, res, sd, dtype)
            runs = []
            for _ in range(3):
                det = m.detect_batch(frames)
                runs.append((det, m.get_tensor("decoded"), m.get_tensor("p3"), m.get_tensor("p5")))
            got[label] = runs
            m.close()
        finally:
            os.environ.pop("CLEARCAM_LANES", None)
    ref = got["chain"][0]
    assert (ref[1][..., 4] > 0).sum() > 0 and np.isfinite(ref[1]).all()
    for label, runs in got.items():
        for det, dec, p3, p5 in runs:
            assert np.array_equal(det, ref[0]) and np.array_equal(dec, ref[1]), label
            assert np.array_equal(p3, ref[2]) and np.array_equal(p5, ref[3]), label


@pytest.mark.parametrize("size,res,dtype", [("c", 640, "f16"), ("t", 320, "bf16"), ("s", 320, "f32")])
def test_batches_in_flight_equal_detect(size, res, dtype):
    """cc_yolo_set_in_flight / cc_yolo_submit / cc_yolo_wait: batches queued round robin on the handle's slots (own stream, arena and
    graph each, so consecutive batches overlap on the GPU) give exactly the rows cc_yolo_detect gives for the same frames - for
    every depth, for batch shapes that change between submissions (a plan per slot and shape), with the wait on a torch stream or
    on the host, and with cc_yolo_detect calls in between."""
    import torch
    from clearcam_amd.weights import conditioned_yolov9_state_dict, synthetic_yolov9_state_dict
    sd = conditioned_yolov9_state_dict("c", 1234) if size == "c" else synthetic_yolov9_state_dict(size, 1234)
    m = _yolo(size, res, sd, dtype)
    shapes = [(3, res, res), (2, 270, 480), (3, res, res), (1, 360, 640), (2, 270, 480), (3, res, res), (3, res, res)]
    frames = [torch.from_numpy(noise_frames(20 + i, *shp)).cuda() for i, shp in enumerate(shapes)]
    ref = [m.detect_batch(f) for f in frames]
    assert sum(int((r[..., 4] > 0).sum()) for r in ref) > 0
    for depth in (1, 2, 3, 4):
        m.set_in_flight(depth)
        for rnd in range(3):                                   # 0: submissions and waits on a torch side stream, 1: host waits,
            host = rnd == 2                                     # 2: pinned host frames and rows (upload and download on the slot's stream)
            outs = [torch.full((f.shape[0], 300, 6), -1.0, device="cpu" if host else "cuda") for f in frames]
            if host:
                outs = [o.pin_memory() for o in outs]
            src = [f.cpu().pin_memory() for f in frames] if host else frames
            torch.cuda.synchronize()
            tickets = []
            with (torch.cuda.stream(torch.cuda.Stream()) if rnd == 0 else contextlib.nullcontext()):
                for i, f in enumerate(src):
                    while len(tickets) - sum(t is None for t in tickets) > depth - 1:      # at most `depth` unwaited submissions
                        j = next(k for k, t in enumerate(tickets) if t is not None)
                        m.wait(tickets[j], host=bool(rnd)); tickets[j] = None
                    tickets.append(m.submit(f, outs[i]))
                    if i == 3:
                        assert np.array_equal(m.detect_batch(frames[0]), ref[0])           # the synchronous call between submissions
                for t in tickets:
                    if t is not None:
                        m.wait(t, host=bool(rnd))
                torch.cuda.current_stream().synchronize()
            for i in range(len(frames)):
                assert np.array_equal(outs[i].cpu().numpy(), ref[i]), (depth, rnd, i)
    with pytest.raises(ValueError):
        m.submit(frames[0].cpu(), torch.empty(3, 300, 6).pin_memory())                 # pageable host frames
    with pytest.raises(RuntimeError):
        m.wait(10 ** 9)                                                                # no such submission
    with pytest.raises(RuntimeError):
        m.set_in_flight(0)
    m.set_in_flight(1)
    assert np.array_equal(m.detect_batch(frames[1]), ref[1])
    m.close()


_ADOWN_SCRIPT = r"""
import csv, os, sys, numpy as np
from clearcam_amd.weights import conditioned_yolov9_state_dict, synthetic_yolov9_state_dict
from clearcam_amd.yolov9 import YOLOv9
size, res, dtype, H, W, B, out = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), sys.argv[7]
frames = np.random.default_rng(6).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
sd = conditioned_yolov9_state_dict(size, 1234) if size == "c" else synthetic_yolov9_state_dict(size, 1234)
m = YOLOv9(size, res, state_dict=sd, dtype=dtype, device=0)
d = {"det": m.detect_batch(frames)}
for n in ("p3", "p4", "p5"): d[n] = m.get_tensor(n)
os.environ["CLEARCAM_PROFILE_CSV"] = out + ".csv"
m.profile(iters=1)
kinds = [r["kind"] for r in csv.DictReader(open(out + ".csv"))]
d["avg_pools"] = np.array(sum(k == "pool0_k2_s1" for k in kinds)); d["avg_convs"] = np.array(sum(k == "conv_avg" for k in kinds))
np.savez(out, **d)
"""


@pytest.mark.parametrize("size,res,dtype,H,W,B,fused", [
    ("c", 640, "bf16", 640, 640, 2, 5),      # the bench plan's five ADown blocks: 128- and 256-channel halves, 160x160 ... 40x40 sources
    ("c", 640, "f16", 270, 480, 1, 5),       # letterboxed 384 x 640: non-square maps, a single frame (fewer tiles than CUs)
    ("c", 608, "bf16", 608, 608, 3, 5),      # 152 x 152 -> 76 x 76 -> 38 x 38 -> 19 x 19: odd averaged maps, ragged last tiles
    ("e", 320, "bf16", 320, 320, 1, 8),      # YOLOv9-e: the ADown blocks of both branches
])
def test_fused_adown_equals_unfused(tmp_path, size, res, dtype, H, W, B, fused):
    """conv_avg_s2_kernel (ADown's 2x2 stride-1 average computed in the stride-2 conv's loader) against the two launches it replaces:
    the averages are summed, scaled and rounded exactly as pool_vec_kernel does and the accumulation runs in the same K order, so
    P3-P5 and the detections are IDENTICAL, bit for bit, and the averaged map is never materialised (no 2x2 average launches left)."""
    import subprocess
    import sys
    outs = []
    for lv in ("0", "1"):
        path = str(tmp_path / f"adown{lv}.npz")
        env = dict(os.environ, CLEARCAM_FUSE_ADOWN=lv, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        subprocess.run([sys.executable, "-c", _ADOWN_SCRIPT, size, str(res), dtype, str(H), str(W), str(B), path], check=True, env=env)
        outs.append(np.load(path))
    a, b = outs
    assert int(a["avg_pools"]) == fused and int(a["avg_convs"]) == 0
    assert int(b["avg_pools"]) == 0 and int(b["avg_convs"]) == fused
    for n in ("p3", "p4", "p5", "det"):
        assert np.array_equal(a[n], b[n]), n
    assert np.abs(a["p3"]).max() > 0.05 and np.isfinite(a["p3"]).all()
