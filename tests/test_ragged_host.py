"""Ragged batches, host side (no GPU): the letterbox geometry helper of the library, the grouping of camera sizes by network shape, and
the packing / regrouping that YOLOv9.detect_frames does around the GPU call."""
import ctypes as C

import numpy as np
import pytest

from oracle import yolov9_oracle as yo

# the sixteen camera sizes of the grouping table, by the network shape they letterbox to at res 640
CLASSES_640 = {
    (384, 640): [(1080, 1920), (720, 1280), (2160, 3840), (1440, 2560), (360, 640), (270, 480), (135, 240)],
    (480, 640): [(480, 640), (1536, 2048), (600, 800), (960, 1280), (240, 320)],
    (544, 640): [(576, 704), (288, 352)],
    (640, 384): [(1920, 1080)],
    (640, 640): [(640, 640)],
}
SIXTEEN = [hw for sizes in CLASSES_640.values() for hw in sizes]


@pytest.fixture(scope="module")
def L(lib_path):
    from clearcam_amd import _lib
    return _lib.lib()


def test_sixteen_sizes():
    assert len(SIXTEEN) == 16 and len(set(SIXTEEN)) == 16


def test_letterbox_geometry_equals_oracle(L):
    sweep = set(SIXTEEN) | {(1920, 1080), (135, 240), (288, 352), (1, 1), (2, 4096), (4096, 2), (719, 1279), (1081, 1921), (333, 777), (31, 33)}
    sweep |= {(h, w) for h in range(97, 1300, 97) for w in range(113, 2100, 131)}
    rng = np.random.default_rng(0)
    sweep |= {(int(h), int(w)) for h, w in rng.integers(1, 4400, (300, 2))}
    v = [C.c_int() for _ in range(4)]
    for res in (320, 640, 960):
        for h, w in sorted(sweep):
            assert L.cc_letterbox_geometry(h, w, res, *[C.byref(x) for x in v]) == 0
            assert tuple(x.value for x in v) == yo.letterbox_geometry(h, w, res), (h, w, res)
    assert L.cc_letterbox_geometry(0, 10, 640, *[C.byref(x) for x in v]) != 0
    assert L.cc_letterbox_geometry(10, 10, 0, *[C.byref(x) for x in v]) != 0


def test_network_shape_groups_the_sixteen_sizes(L):
    from clearcam_amd.yolov9 import YOLOv9, group_frames, network_shape
    m = YOLOv9.__new__(YOLOv9)                       # network_shape needs nothing of the model but its res (no GPU handle here)
    m.res = 640
    got = {}
    for hw in SIXTEEN:
        assert m.network_shape(*hw) == network_shape(*hw, 640)
        got.setdefault(m.network_shape(*hw), []).append(hw)
    assert {k: sorted(v) for k, v in got.items()} == {k: sorted(v) for k, v in CLASSES_640.items()}
    # the same classes out of the grouping detect_frames uses (shapes only: zero-strided stand-ins, no 4K allocation)
    frames = [np.broadcast_to(np.uint8(0), hw + (3,)) for hw in SIXTEEN]
    groups = group_frames(frames, 640)
    assert {g.shape: sorted(SIXTEEN[i] for i in g.index) for g in groups} == {k: sorted(v) for k, v in CLASSES_640.items()}


def _tagged(i, h, w, dtype):
    """A frame whose content names it: every pixel of frame i is i + 1."""
    return np.full((h, w, 3), i + 1, dtype=dtype)


def test_packing_and_input_order(L):
    """Shuffled mixed inputs: every frame lands at its offset of its group's packed buffer, untouched, and rows computed per group come
    back in input order."""
    from clearcam_amd.yolov9 import MAX_DET, group_frames, pack_group, scatter_rows
    sizes = [(270, 480), (240, 320), (135, 240), (360, 640), (120, 160), (270, 480), (480, 640), (135, 240)]
    order = np.random.default_rng(3).permutation(len(sizes))
    frames = [_tagged(i, *sizes[j], np.uint8) for i, j in enumerate(order)]
    frames[2] = frames[2].astype(np.float32)                                    # a float32 frame never shares a batch with uint8 ones
    groups = group_frames(frames, 320)
    assert sorted(i for g in groups for i in g.index) == list(range(len(frames)))
    outs = []
    for g in groups:
        assert len({(frames[i].dtype == np.float32) for i in g.index}) == 1 and g.index == sorted(g.index)
        for i in g.index:
            nh, nw, py, px = yo.letterbox_geometry(*frames[i].shape[:2], 320)
            assert (nh + 2 * py, nw + 2 * px) == g.shape
        buf = np.full(g.nbytes + 7, 255, np.uint8)
        pack_group(frames, g, buf)
        assert (buf[g.nbytes:] == 255).all()                                    # nothing written past the packed size
        es = 4 if g.f32 else 1
        end = 0
        rows = np.zeros((len(g.index), MAX_DET, 6), np.float32)
        for k, i in enumerate(g.index):
            h, w = frames[i].shape[:2]
            assert (g.heights[k], g.widths[k]) == (h, w) and g.offsets[k] == end   # back to back, in input order
            got = buf[end:end + h * w * 3 * es].view(frames[i].dtype).reshape(h, w, 3)
            assert np.array_equal(got, frames[i])
            end += h * w * 3 * es
            rows[k] = got[0, 0, 0]                                              # stand-in for the detector: a row that names its frame
        assert end == g.nbytes
        assert g.offsets.dtype == np.int64 and g.heights.dtype == np.int32 and g.widths.dtype == np.int32
        outs.append(rows)
    out = scatter_rows(groups, outs, len(frames))
    assert out.shape == (len(frames), MAX_DET, 6)
    for i in range(len(frames)):
        assert (out[i] == i + 1).all()
    assert group_frames([], 320) == []


@pytest.mark.parametrize("bad,msg", [
    (np.zeros((270, 480), np.uint8), "(H,W,3)"),
    (np.zeros((270, 480, 4), np.uint8), "(H,W,3)"),
    (np.zeros((1, 270, 480, 3), np.uint8), "(H,W,3)"),
    (np.zeros((270, 480, 3), np.int16), "uint8 or float32"),
    (np.zeros((270, 480, 3), np.float64), "uint8 or float32"),
    (np.zeros((0, 480, 3), np.uint8), "(H,W,3)"),
    (np.zeros((8, 4000, 3), np.uint8), "multiple of 32"),                       # letterboxes to 1 x 320 + 0 padding: not a network shape
])
def test_bad_frames_raise_with_the_frame_index(L, bad, msg):
    from clearcam_amd.yolov9 import group_frames
    good = np.zeros((270, 480, 3), np.uint8)
    with pytest.raises(ValueError) as e:
        group_frames([good, good, bad, good], 320)
    assert "frame 2" in str(e.value) and msg in str(e.value)


def test_parse_mix():
    from clearcam_amd.streams import parse_mix
    sizes = parse_mix("1080x1920:32,720x1280:16,2160x3840:8,480x640:8")
    assert len(sizes) == 64 and sizes[0] == (1080, 1920) and sizes[32] == (720, 1280) and sizes[48] == (2160, 3840) and sizes[-1] == (480, 640)
    assert parse_mix("270x480") == [(270, 480)]
    for bad in ("", "1080:3", "ax1920:2", "1080x1920:x"):
        with pytest.raises(ValueError):
            parse_mix(bad)
