"""Ragged batches on the GPU: frames of different source sizes that letterbox to one network shape run as ONE batch of that shape's plan
(cc_yolo_detect_ragged, YOLOv9.detect_frames / submit_frames, MixedStreamPipeline).  The yardstick is the bar the project already holds
for batches (test_batch_invariance_and_determinism, test_pipeline_equals_frame_by_frame_loop): a frame's rows do not depend on its batch,
so every row must equal the existing single-frame call bit for bit - no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

from conftest import noise_frames
from oracle import yolov9_oracle as yo

pytestmark = pytest.mark.gpu

SIZES_320 = [(270, 480), (135, 240), (360, 640), (1080, 1920)]       # all -> 192 x 320 at res 320


def _yolo(size, res, sd, dtype):
    from clearcam_amd.yolov9 import YOLOv9
    return YOLOv9(size, res, state_dict=sd, dtype=dtype)


def _frame(seed, h, w, dtype=np.uint8):
    return noise_frames(seed, 1, h, w, dtype)[0]


def _scene(seed, h, w):
    """A noise frame with four flat rectangles (what streams.SyntheticCamera draws): white noise alone, scaled down to 192 x 320, gives the
    synthetic checkpoint almost nothing to detect, and a comparison of empty rows would show nothing."""
    f = noise_frames(seed, 1, h, w)[0].copy()
    r = np.random.default_rng(1000 + seed)
    for _ in range(4):
        rh, rw = max(2, h // int(r.integers(3, 7))), max(2, w // int(r.integers(4, 9)))
        y, x = int(r.integers(0, h - rh + 1)), int(r.integers(0, w - rw + 1))
        f[y:y + rh, x:x + rw] = r.integers(0, 256, 3)
    return f


def _singles(m, frames):
    return [m(f).numpy() for f in frames]


@pytest.mark.parametrize("fdtype", [np.uint8, np.float32])
def test_ragged_letterbox_bit_exact(sd_t, fdtype):
    """Every frame of one ragged call is letterboxed exactly as the oracle letterboxes it alone (the uint8 path is integer arithmetic)."""
    frames = [_frame(20 + i, h, w, fdtype) for i, (h, w) in enumerate(SIZES_320)]
    m = _yolo("t", 320, sd_t, "f32")
    assert {m.network_shape(h, w) for h, w in SIZES_320} == {(192, 320)}
    m.detect_frames(frames)
    got = m.get_tensor("input")
    assert got.shape == (4, 192, 320, 3)
    for i, f in enumerate(frames):
        ref = yo.letterbox(f, 320)[..., ::-1] / np.float32(255.0)
        assert np.array_equal(got[i], ref.astype(np.float32)), f"frame {i} {f.shape}"
    assert m.last_gpu_ms() > 0 and m.nonfinite() == 0
    m.close()


@pytest.mark.parametrize("dtype", ["f32", "f16h", "f16", "bf16", "f16s"])
def test_ragged_detections_equal_single_frame_calls(sd_t, dtype):
    """8 uint8 frames (noise with flat rectangles) of 4 sizes in shuffled order: detect_frames, submit_frames with three batches in flight, and device-resident
    frames all give each frame the rows of its own single-frame call."""
    import torch
    order = np.random.default_rng(5).permutation(8)
    sizes = [SIZES_320[j % 4] for j in order]
    frames = [_scene(40 + i, h, w) for i, (h, w) in enumerate(sizes)]
    m = _yolo("t", 320, sd_t, dtype)
    ref = _singles(m, frames)
    for hw in SIZES_320:                                             # not vacuous: every size has a frame with a detection
        assert any((ref[i][:, 4] > 0).any() for i in range(8) if sizes[i] == hw), hw
    got = m.detect_frames(frames)
    assert got.shape == (8, 300, 6) and got.dtype == np.float32
    for i in range(8):
        assert np.array_equal(got[i], ref[i]), f"frame {i} {sizes[i]}"
    # the 16-bit modes rebuild "input" with the ragged letterbox kernel: same bits as the f32 path stores, rounded to the storage type
    assert m.get_tensor("input").shape == (8, 192, 320, 3)
    dev = m.detect_frames([torch.from_numpy(f).cuda() for f in frames])
    for i in range(8):
        assert np.array_equal(dev[i], ref[i]), f"device frame {i} {sizes[i]}"
    m.set_in_flight(3)
    perms = [np.random.default_rng(60 + k).permutation(8) for k in range(3)]
    tickets = [m.submit_frames([frames[i] for i in p]) for p in perms]           # three batches in flight, one per slot
    for p, t in zip(perms, tickets):
        rows = m.wait(t, host=True)
        for k, i in enumerate(p):
            assert np.array_equal(rows[k], ref[i]), f"in flight: frame {i} {sizes[i]}"
    assert m.nonfinite() == 0
    m.close()


def test_several_network_shapes_in_one_call(sd_t):
    sizes = [(360, 640), (480, 640), (270, 480), (240, 320), (720, 1280), (600, 800)]
    frames = [_scene(70 + i, h, w) for i, (h, w) in enumerate(sizes)]
    m = _yolo("t", 640, sd_t, "f16h")
    assert [m.network_shape(h, w) for h, w in sizes] == [(384, 640), (480, 640)] * 3
    ref = _singles(m, frames)
    got = m.detect_frames(frames)
    for i in range(len(frames)):
        assert np.array_equal(got[i], ref[i]), f"frame {i} {sizes[i]}"
    assert sum((r[:, 4] > 0).sum() for r in ref) > 0
    m.close()


def _stage_bytes(h, w, nh, nw):
    """The stem kernel's bound on the source bytes a 33 x 33-pixel tile can need (stem_needs_big in detect.hip)."""
    nr, nc = (33 * h + nh - 1) // nh + 2, (33 * w + nw - 1) // nw + 2
    return nr * ((nc * 3 + 6) // 4) * 4


def test_production_shape_mixed_site(sd_c):
    """YOLOv9-C 640 f16h, B = 8: 3 x 1080p, 3 x 720p, 1 x 4K, 1 x 360x640 in one ragged batch.  The 4K frame's tiles do not fit even the
    36 KB stage (direct reads), the 1080p frames need the 36 KB stage and the 720p frames fit the 18 KB one: all three branches of the
    stem's source staging run in this one launch."""
    sizes = [(1080, 1920), (720, 1280), (2160, 3840), (1080, 1920), (360, 640), (720, 1280), (1080, 1920), (720, 1280)]
    small, big = 128 * 72 * 2, 256 * 72 * 2
    geo = {hw: yo.letterbox_geometry(*hw, 640) for hw in set(sizes)}
    assert _stage_bytes(2160, 3840, *geo[(2160, 3840)][:2]) > big
    assert small < _stage_bytes(1080, 1920, *geo[(1080, 1920)][:2]) <= big
    assert _stage_bytes(720, 1280, *geo[(720, 1280)][:2]) <= small
    frames = [_scene(80 + i, h, w) for i, (h, w) in enumerate(sizes)]
    m = _yolo("c", 640, sd_c, "f16h")
    assert {m.network_shape(h, w) for h, w in sizes} == {(384, 640)}
    got = m.detect_frames(frames)
    for i, f in enumerate(frames):
        ref = m(f).numpy()
        assert (ref[:, 4] > 0).any()
        assert np.array_equal(got[i], ref), f"frame {i} {sizes[i]}"
    m.close()


def test_mixed_pipeline_equals_frame_by_frame_loop(sd_t):
    """2 x 270x480 and 2 x 135x240 cameras (interleaved) through MixedStreamPipeline: detections and track rows of 6 ticks equal the
    reference's per-frame loop detect -> tracker.update, camera by camera."""
    from clearcam_amd.ocsort import OCSort
    from clearcam_amd.streams import MixedCameraBank, MixedStreamPipeline
    sizes, T, depth = [(270, 480), (135, 240), (270, 480), (135, 240)], 6, 2
    N = len(sizes)
    model = _yolo("t", 320, sd_t, "f32")
    cams = MixedCameraBank(sizes, ring=4)
    pipe = MixedStreamPipeline(model, sizes, depth=depth, n_threads=2)
    assert len(pipe.groups) == 1 and len(pipe.trackers) == N
    got = []
    for _ in range(depth - 1):
        pipe.submit(cams.read_all())
    for _ in range(T - depth + 1):
        pipe.submit(cams.read_all())
        preds, rows = pipe.collect()
        got.append((preds.copy(), rows))
    for _ in range(depth - 1):
        preds, rows = pipe.collect()
        got.append((preds.copy(), rows))
    assert len(got) == T
    with pytest.raises(RuntimeError):
        pipe.collect()
    trackers = [OCSort(max_age=100) for _ in range(N)]
    for t in range(T):
        for i, c in enumerate(cams):
            frame = np.ascontiguousarray(c.frames[t % c.ring].numpy())
            assert frame.shape == sizes[i] + (3,)
            p = model(frame).numpy()
            assert np.array_equal(p, got[t][0][i]), f"detections differ at frame {t} camera {i}"
            np.testing.assert_array_equal(trackers[i].update_rows(p, 0.25), got[t][1][i])
    assert sum(len(r) for _, rows in got for r in rows) > 0
    # per-camera uploads give the same rows as the single upload of the flat buffer
    pipe.submit([c.frames[0] for c in cams])
    preds, _ = pipe.collect()
    assert np.array_equal(preds, got[0][0])
    stats = pipe.run(cams, 3, warmup=1)
    assert stats["frames_per_sec"] > 0 and stats["cameras"] == N and not stats["frames_resident"]
    pipe.close()
    model.close()


def test_two_network_shapes_in_a_mixed_pipeline(sd_t):
    """Cameras of two network shapes (192x320 and 256x320 at res 320), interleaved: two ragged batches per tick, rows back in camera order."""
    from clearcam_amd.streams import MixedCameraBank, MixedStreamPipeline
    sizes = [(240, 320), (270, 480), (120, 160), (135, 240), (240, 320)]
    model = _yolo("t", 320, sd_t, "f16h")
    cams = MixedCameraBank(sizes, ring=3)
    pipe = MixedStreamPipeline(model, sizes, depth=2, track=False)
    assert sorted(len(g[0]) for g in pipe.groups) == [2, 3]
    pipe.submit(cams.read_all())
    preds, rows = pipe.collect()
    assert rows is None
    for i, c in enumerate(cams):
        assert np.array_equal(preds[i], model(np.ascontiguousarray(c.frames[0].numpy())).numpy()), f"camera {i}"
    pipe.close()
    model.close()


def _ragged_call(m, pixels, offsets, heights, widths, out):
    from clearcam_amd import _lib
    o, h, w = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(heights, np.int32), np.ascontiguousarray(widths, np.int32)
    i32p = C.POINTER(C.c_int32)
    return _lib.lib().cc_yolo_detect_ragged(m._h, _lib.ptr(pixels), o.ctypes.data_as(C.POINTER(C.c_int64)), h.ctypes.data_as(i32p), w.ctypes.data_as(i32p),
                                            len(o), 0, 0, _lib.ptr(out), 0, None)


def _plans_built(m):
    from clearcam_amd import _lib
    n = C.c_int()
    _lib.check(_lib.lib().cc_yolo_plans_built(m._h, C.byref(n)))
    return n.value


def test_ragged_abi_errors_offsets_and_plan_reuse(sd_t):
    from clearcam_amd import _lib
    m = _yolo("t", 320, sd_t, "f16h")
    a, b = _scene(90, 270, 480), _scene(91, 240, 320)               # 192x320 and 256x320: two network shapes
    out = np.zeros((2, 300, 6), np.float32)
    rc = _ragged_call(m, np.concatenate([a.ravel(), b.ravel()]), [0, a.size], [270, 240], [480, 320], out)
    err = _lib.lib().cc_last_error().decode()
    assert rc == -22 and "frame 1" in err and "256x320" in err and "192x320" in err, err
    rc = _ragged_call(m, np.zeros(8 * 4000 * 3, np.uint8), [0], [8], [4000], out)
    err = _lib.lib().cc_last_error().decode()
    assert rc == -22 and "frame 0" in err and "multiple of 32" in err, err
    # frames at arbitrary byte offsets (1 and 3 modulo 4, a gap between them, slack at the end): the stem stages source rows with aligned
    # dword loads, so the row misalignment comes from the frame's offset
    f0, f1, f2 = _scene(92, 135, 240), _scene(93, 270, 480), _scene(94, 135, 240)
    offs = [1, 1 + f0.size + 6, 1 + f0.size + 6 + f1.size + 1]
    assert [o % 4 for o in offs] == [1, 3, 0] and f0.size % 4 == 0
    packed = np.zeros(offs[2] + f2.size + 5, np.uint8)
    for o, f in zip(offs, (f0, f1, f2)):
        packed[o:o + f.size] = f.ravel()
    out = np.zeros((3, 300, 6), np.float32)
    n0 = _plans_built(m)
    assert _ragged_call(m, packed, offs, [135, 270, 135], [240, 480, 240], out) == 0, _lib.lib().cc_last_error().decode()
    assert _plans_built(m) == n0 + 1
    ref = _singles(m, (f0, f1, f2))
    n1 = _plans_built(m)
    for i in range(3):
        assert np.array_equal(out[i], ref[i]), f"frame {i}"
    # a camera changes resolution: the same B with other source sizes reuses the plan (no new arena, no new graph capture)
    g0, g1, g2 = _scene(95, 360, 640), _scene(96, 1080, 1920), _scene(97, 270, 480)
    offs = [0, g0.size, g0.size + g1.size]
    assert _ragged_call(m, np.concatenate([g0.ravel(), g1.ravel(), g2.ravel()]), offs, [360, 1080, 270], [640, 1920, 480], out) == 0
    assert _plans_built(m) == n1
    ref = _singles(m, (g0, g1, g2))
    for i in range(3):
        assert np.array_equal(out[i], ref[i]), f"frame {i} after the resolution change"
    # the profilers refuse a ragged plan with a message instead of replaying a stem launch without its records
    assert _ragged_call(m, np.concatenate([g0.ravel(), g1.ravel(), g2.ravel()]), offs, [360, 1080, 270], [640, 1920, 480], out) == 0
    with pytest.raises(_lib.CCError, match="ragged"):
        m.profile(1)
    m.close()
