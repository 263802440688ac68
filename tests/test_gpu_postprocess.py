"""The kernels that turn logits into detections, ONE launch each through the cc_dev_* entries, on the crafted inputs of
tests/postprocess_cases.py (whose conditions tests/test_postprocess_host.py holds on the CPU): decode_kernel and head_tail_kernel against
float64, topk_nms_kernel and blaze_post_kernel bit for bit against the oracle's own float32 rule on inputs with exact arithmetic.
Every output buffer is NaN before the launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import postprocess_cases as pc
from clearcam_amd import _lib
from clearcam_amd.weights import blazeface_anchors

pytestmark = pytest.mark.gpu
DTI = {"f16": 1, "bf16": 2, "f16s": 3}
NAN = float("nan")


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).contiguous().to("cuda")


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data for t in ts])


def _hw(levels):
    return (C.c_int * 3)(*[h for h, _ in levels]), (C.c_int * 3)(*[w for _, w in levels])


def run_decode(raws, dfl_w, conf=pc.CONF):
    """cc_dev_decode -> ((B,A,6) rows, nonfinite count)."""
    d = [_dev(r) for r in raws]
    B, levels = raws[0].shape[0], [r.shape[1:3] for r in raws]
    H, W = _hw(levels)
    out = torch.full((B, sum(h * w for h, w in levels), 6), NAN, device="cuda")
    nf, dfl = C.c_int(-1), np.ascontiguousarray(dfl_w, np.float32)            # host arrays stay referenced across the call
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_decode(_ptrs(d), H, W, B, _lib.ptr(dfl), C.c_float(conf), _lib.ptr(out), C.byref(nf), None))
    return out.cpu().numpy(), nf.value


def run_head_tail(c: pc.TailCase, dtype, bx=None, conf=pc.CONF):
    """cc_dev_head_tail -> ((B,A,6) rows, nonfinite count)."""
    t = pc.TORCH_DT[dtype]
    bxd = [_dev(x, t) for x in (bx or c.bx)]
    cld = [_dev(x, t) for x in c.cl]
    H, W = _hw(c.levels)
    out = torch.full((c.B, sum(h * w for h, w in c.levels), 6), NAN, device="cuda")
    nf = C.c_int(-1)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_head_tail(DTI[dtype], c.ch, _ptrs(bxd), _ptrs(cld), _ptrs(c.w2), _ptrs(c.b2), _ptrs(c.w3), _ptrs(c.b3), H, W, c.B,
                                           _lib.ptr(c.dfl_w), C.c_float(conf), _lib.ptr(out), C.byref(nf), None))
    return out.cpu().numpy(), nf.value


def run_unfused(c: pc.TailCase, dtype):
    """The unfused chain through existing entries: per level two cc_conv2d_ex launches writing float32 into channels 0..63 and 64..143
    of a (B,H,W,144) buffer, then cc_dev_decode.  The convs get the values the detector's packing rounds the weights to (the face nets'
    packing keeps representable values as they are)."""
    L, t = _lib.lib(), pc.TORCH_DT[dtype]
    raws = []
    for l, (h, w) in enumerate(c.levels):
        raw = torch.full((c.B, h, w, 144), NAN, device="cuda")
        for x, wt, b, cin, cout, groups, coff in ((c.bx[l], c.w2[l], c.b2[l], 64, 64, 4, 0), (c.cl[l], c.w3[l], c.b3[l], c.ch, 80, 1, 64)):
            d = _lib.ConvDesc(DTI[dtype], c.B, h, w, cin, cout, 1, 1, groups, 0, -1, 0, 0, 1, 144, coff, 0, 0, 0, 0)
            xd, wk = _dev(x, t), np.ascontiguousarray(pc.kernel_weights(dtype, wt))
            torch.cuda.synchronize()
            _lib.check(L.cc_conv2d_ex(C.byref(d), _lib.ptr(xd), _lib.ptr(wk), _lib.ptr(b), None, None, _lib.ptr(raw), None, None))
        raws.append(raw.cpu().numpy())
    assert all(np.isfinite(r).all() for r in raws)
    return run_decode(raws, c.dfl_w)


# ---- decode_kernel ---------------------------------------------------------------------------------------------------------------
def test_decode_kernel_against_float64():
    """Non-square ragged levels, random DFL weights and the planted edges (uniform / saturated sides, exact class ties, first and last
    cells) in one launch.  Bars: boxes 2e-3 px (the project's bar for this stage), scores 1e-6 (sigmoid <= 1, a few float32 ulps), the
    class on every anchor (the case has no top-two gap inside (0, 1e-6) and no score within 1e-6 of the threshold)."""
    c = pc.decode_case()
    ref = pc.decode_np(c.raws, c.dfl_w)
    f32 = pc.decode_np(c.raws, c.dfl_w, np.float32)
    got, nf = run_decode(c.raws, c.dfl_w)
    assert got.shape == (3, 315, 6) and np.isfinite(got).all() and nf == 0
    rows = pc.rows_of(ref)
    frac = (rows[..., 4] > 0).mean()
    assert 1 / 3 <= frac <= 2 / 3 and not ((ref.gap > 0) & (ref.gap < 1e-6)).any() and not (np.abs(ref.score - pc.CONF) <= 1e-6).any()
    box_err, sc_err = np.abs(got[..., :4] - rows[..., :4]).max(), np.abs(got[..., 4] - rows[..., 4]).max()
    print(f"decode_kernel vs float64: box {box_err:.3g} px, score {sc_err:.3g}; float32 NumPy restatement: box "
          f"{np.abs(f32.box - ref.box).max():.3g} px, score {np.abs(f32.score - ref.score).max():.3g}")
    assert box_err <= 2e-3 and sc_err <= 1e-6
    assert np.array_equal(got[..., 5], rows[..., 5])
    assert np.array_equal(got[..., 4] > 0, rows[..., 4] > 0)
    for name, (b, a) in c.planted.items():                                    # each planted edge on its own, for the failure message
        assert np.abs(got[b, a, :4] - rows[b, a, :4]).max() <= 2e-3 and got[b, a, 4] > 0 and got[b, a, 5] == rows[b, a, 5], name
    for name, pair in zip(("tie_7_42", "tie_0_79", "tie_3_4"), pc.TIE_CLASSES):
        b, a = c.planted[name]
        assert got[b, a, 5] == pair[0], name


def test_decode_kernel_counts_nonfinite_logits():
    c = pc.decode_case()
    raws = [r.copy() for r in c.raws]
    raws[0][1, 3, 4, :64] = np.inf                                            # one anchor's box logits
    raws[2][2, 1, 1, 64:] = np.nan                                            # another's class logits
    _, nf = run_decode(raws, c.dfl_w)
    assert nf == 2, nf
    _, nf = run_decode(c.raws, c.dfl_w)
    assert nf == 0


# ---- head_tail_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch", [128, 256])
@pytest.mark.parametrize("dtype", ["f16", "bf16", "f16s"])
def test_head_tail_kernel(dtype, ch):
    """Both shapes of the case table.  (a) f16 / bf16: every row bit-equal to the unfused chain.  (b) against float64 over the stored
    activations and the weight values the kernel multiplies by: the class outside a top-two gap of 1e-4 (at most 1 % of the anchors),
    class TIE_PAIR[0] wherever the tied pair is on top, scores within 1e-5, boxes within 4x the deviation of a float32 NumPy evaluation
    of the same reference (the kernel's K order and MFMA accumulation differ from NumPy's)."""
    for small in (False, True):
        c = pc.tail_case(dtype, ch, small)
        got, nf = run_head_tail(c, dtype)
        A = sum(h * w for h, w in c.levels)
        assert got.shape == (c.B, A, 6) and np.isfinite(got).all() and nf == 0
        if not small:
            assert [c.B * h * w for h, w in c.levels] == [720, 180, 45]       # ragged tile, ragged fragment, blk1 = 2, blk2 = 3
        if dtype != "f16s":
            chain, nf2 = run_unfused(c, dtype)
            assert nf2 == 0 and np.array_equal(got, chain), np.abs(got - chain).max()
        ref = pc.decode_np(pc.tail_logits(c, dtype), c.dfl_w)
        f32 = pc.decode_np(pc.tail_logits(c, dtype, np.float32), c.dfl_w, np.float32)
        rows = pc.rows_of(ref)
        near = (ref.gap > 0) & (ref.gap < 1e-4)
        tie = ref.gap == 0
        assert near.mean() <= 0.01 and tie.sum() >= 1 and not (np.abs(ref.score - pc.CONF) <= 1e-5).any()
        assert (got[..., 5][tie] == pc.TIE_PAIR[0]).all()                      # the cross-lane tie rule
        assert np.array_equal(got[..., 5][~near], rows[..., 5][~near])
        assert np.array_equal(got[..., 4] > 0, rows[..., 4] > 0)
        floor = np.abs(f32.box - ref.box).max()
        box_err, sc_err = np.abs(got[..., :4] - rows[..., :4]).max(), np.abs(got[..., 4] - rows[..., 4]).max()
        print(f"head_tail_kernel {dtype} ch {ch} {'small' if small else 'main'}: box {box_err:.3g} px (float32 NumPy floor {floor:.3g}), "
              f"score {sc_err:.3g} (floor {np.abs(f32.score - ref.score).max():.3g}), {int(near.sum())} near-ties, {int(tie.sum())} ties")
        assert sc_err <= 1e-5
        assert box_err <= 4 * floor, (box_err, floor)


def test_head_tail_kernel_counts_nonfinite_activations():
    c = pc.tail_case("f16", 128, small=True)
    bx = [x.copy() for x in c.bx]
    bx[1][0, 2, 3, 17] = np.inf
    _, nf = run_head_tail(c, "f16", bx=bx)
    assert nf > 0
    _, nf = run_head_tail(c, "f16")
    assert nf == 0


# ---- topk_nms_kernel -------------------------------------------------------------------------------------------------------------
def run_nms(rows, geom, ragged):
    B, A = rows.shape[:2]
    d = _dev(rows)
    out = torch.full((B, pc.MAX_DET, 6), NAN, device="cuda")
    g = np.ascontiguousarray(geom, np.float32)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_topk_nms(_lib.ptr(d), B, A, C.c_float(0.45), _lib.ptr(g), int(ragged), _lib.ptr(out), None))
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def nms_cases():
    return pc.nms_launches()


@pytest.mark.parametrize("launch", ["a2100", "a189", "a525"])
def test_topk_nms_kernel_equals_oracle(nms_cases, launch):
    """Every selection path (compaction + zero fill, 512-key sort, radix select down to the anchor bytes), the boundaries nz = 299 / 300 /
    301 and 511 / 512 / 513, A < 300 and A < 1024, the NMS edge rules and scale_boxes with a letterbox geometry: all six columns equal
    to postprocess_rows + scale_boxes, one image per scenario in one launch."""
    names, rows = nms_cases[launch]
    nz = (rows[..., 4] > 0).sum(1)
    if launch == "a2100":
        want = {"nz0": 0, "nz1": 1, "nz299": 299, "nz300": 300, "nz301": 301, "nz511": 511, "nz512": 512, "nz513": 513, "nz2100": 2100,
                "all_equal": 2100, "seven_values": 700, "low_byte": 600, "head200": 200, "tail40": 40, "identical300": 300, "trio0": 300}
        assert all(nz[names.index(k)] == v for k, v in want.items()), dict(zip(names, nz))
    ref = pc.nms_expected(rows, [pc.UNIFORM_SRC])
    got = run_nms(rows, pc.geometry(pc.UNIFORM_SRC), False)
    for i, n in enumerate(names):
        assert np.array_equal(got[i], ref[i]), (launch, n, np.argwhere(got[i] != ref[i])[:5])
    if launch == "a2100":
        i = names.index("all_equal")
        alive = got[i][:, 4] > 0
        assert alive.sum() > 50 and np.array_equal(got[i][alive, 4:], rows[i][:300][alive, 4:])        # anchors 0..299 in order


def test_topk_nms_kernel_ragged_geometry(nms_cases):
    """The ragged launcher: image b scaled and clipped with its own (pad, gain, source size), computed as Builder::head_finish does."""
    names, rows = nms_cases["a2100"]
    srcs = [pc.RAGGED_SRCS[i % len(pc.RAGGED_SRCS)] for i in range(len(rows))]
    ref = pc.nms_expected(rows, srcs)
    got = run_nms(rows, np.stack([pc.geometry(s) for s in srcs]), True)
    for i, n in enumerate(names):
        assert np.array_equal(got[i], ref[i]), (n, srcs[i], np.argwhere(got[i] != ref[i])[:5])
    one = run_nms(rows[:1], pc.geometry(srcs[0])[None], True)                 # B = 1 through the ragged launcher
    assert np.array_equal(one[0], ref[0])


def test_dev_entries_refuse_bad_arguments():
    L = _lib.lib()
    rows = _dev(np.zeros((1, 8, 6), np.float32))
    out = torch.zeros((1, 300, 6), device="cuda")
    g = pc.geometry(pc.UNIFORM_SRC)
    assert L.cc_dev_topk_nms(None, 1, 8, C.c_float(0.45), _lib.ptr(g), 0, _lib.ptr(out), None) != 0
    assert L.cc_dev_topk_nms(_lib.ptr(rows), 0, 8, C.c_float(0.45), _lib.ptr(g), 0, _lib.ptr(out), None) != 0
    assert L.cc_dev_topk_nms(_lib.ptr(rows), 1, 0, C.c_float(0.45), _lib.ptr(g), 0, _lib.ptr(out), None) != 0
    assert b"bad shape" in L.cc_last_error()
    c = pc.tail_case("f16", 128, small=True)
    H, W = _hw(c.levels)
    nf = C.c_int(0)
    raws = [_dev(np.zeros((1, h, w, 144), np.float32)) for h, w in c.levels]
    det = torch.zeros((1, 84, 6), device="cuda")
    bad = (C.c_void_p * 3)(raws[0].data_ptr() + 4, raws[1].data_ptr(), raws[2].data_ptr())                  # misaligned for float4 loads
    assert L.cc_dev_decode(bad, H, W, 1, _lib.ptr(c.dfl_w), C.c_float(0.25), _lib.ptr(det), C.byref(nf), None) != 0
    assert L.cc_dev_decode(_ptrs(raws), H, W, 0, _lib.ptr(c.dfl_w), C.c_float(0.25), _lib.ptr(det), C.byref(nf), None) != 0
    bxd, cld = [_dev(x, torch.float16) for x in c.bx], [_dev(x, torch.float16) for x in c.cl]
    args = (_ptrs(bxd), _ptrs(cld), _ptrs(c.w2), _ptrs(c.b2), _ptrs(c.w3), _ptrs(c.b3), H, W, 1, _lib.ptr(c.dfl_w), C.c_float(0.25), _lib.ptr(det), C.byref(nf), None)
    assert L.cc_dev_head_tail(0, 128, *args) != 0                             # f32 storage has no fused tail
    assert L.cc_dev_head_tail(1, 80, *args) != 0                              # nor has ch = 80
    assert L.cc_dev_head_tail(2, 128, *args[:-6], 0, *args[-5:]) != 0         # B = 0
    assert L.cc_dev_blaze_post(None, None, None, None, 1, None, C.c_float(1.0), 0, 0, None, None, None, None) != 0


# ---- blaze_post_kernel -----------------------------------------------------------------------------------------------------------
def run_blaze(anchors, L: pc.BlazeLaunch, sel=None):
    raw, score = (L.raw, L.score) if sel is None else (L.raw[sel:sel + 1], L.score[sel:sel + 1])
    n = len(raw)
    parts = [_dev(p) for p in pc.blaze_split(raw, score)]
    out = torch.full((n, 896, 17), NAN, device="cuda")
    first = torch.full((n, 17), NAN, device="cuda")
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    anc = np.ascontiguousarray(anchors, np.float32)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_blaze_post(*[_lib.ptr(p) for p in parts], n, _lib.ptr(anc), C.c_float(L.scale), L.pad_top, L.pad_left,
                                            _lib.ptr(out), _lib.ptr(first), _lib.ptr(idx), None))
    return out.cpu().numpy(), first.cpu().numpy(), idx.cpu().numpy()


def test_blaze_post_kernel_equals_oracle():
    """Crafted images (dyadic coordinates: columns 0..15 bit-equal to the oracle's decode / postprocess / back-map, the same rows alive, the
    first-row pick) and two random ones (the same rows alive, columns within the bars of test_blazeface_f32_matches_oracle); the batch
    of six against six single launches, bit for bit."""
    anchors = blazeface_anchors()
    launches = pc.blaze_launches(anchors)
    for key, L in launches.items():
        ref, rfirst, ridx = pc.blaze_expected(anchors, L)
        got, first, idx = run_blaze(anchors, L)
        assert np.isfinite(got).all() and np.isfinite(first).all()
        assert np.array_equal(idx, ridx), (key, idx, ridx)
        for i, n in enumerate(L.names):
            assert np.array_equal(got[i][:, 16] != 0, ref[i][:, 16] != 0), n
            assert np.abs(got[i][:, 16] - ref[i][:, 16]).max() <= 1e-5 * 256 / L.scale, n
            if n.startswith("random"):
                ds, di = pc.blaze_margins(anchors, L.raw[i], L.score[i])
                assert ds > 1e-5 and di > 1e-5
                err = np.abs(got[i][:, :16] - ref[i][:, :16]).max()
                print(f"blaze_post_kernel {n}: columns 0..15 within {err:.3g} px of the oracle, {(ref[i][:, 16] != 0).sum()} rows alive")
                assert err <= 2e-3 / L.scale
            else:
                assert np.array_equal(got[i][:, :16], ref[i][:, :16]), (n, np.argwhere(got[i][:, :16] != ref[i][:, :16])[:5])
            assert np.array_equal(first[i], got[i][idx[i]] if idx[i] >= 0 else np.zeros(17, np.float32)), n
            assert np.array_equal(first[i][:16], rfirst[i][:16]) or n.startswith("random"), n
        if key == "padded":
            by = {n: i for i, n in enumerate(L.names)}
            assert len(L.names) == 6 and idx[by["none_alive_padded"]] == 0 and idx[by["ymin_zero"]] == 1
            i = by["all_score_one"]
            assert (got[i][got[i][:, 16] != 0, 16] == np.float32(256) / np.float32(L.scale)).all()
            for i in range(len(L.names)):                                     # image i of the batch == the single launch of image i
                o1, f1, i1 = run_blaze(anchors, L, sel=i)
                assert np.array_equal(o1[0], got[i]) and np.array_equal(f1[0], first[i]) and i1[0] == idx[i], L.names[i]
        else:
            assert idx[0] == -1 and not first.any()
