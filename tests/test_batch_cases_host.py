"""tests/batch_cases.py held on the CPU: the pattern that places four distinct inputs over a batch has the properties the GPU test leans
on, check_rows catches every planted fault under every bar, and the oracle tells the four inputs of each model apart - a case whose
inputs the oracle cannot separate proves nothing.  (The CLIP L/14 oracle is too heavy for a host test: CLIP tiny stands in here, and
tests/test_gpu_plan_batches.py makes the same separation assertion on the L/14 oracle's outputs before it compares anything.)"""
import numpy as np
import pytest
import torch

import batch_cases as bc
from clearcam_amd.arch import CLIP_TINY
from clearcam_amd.weights import synthetic_adaface_state_dict, synthetic_blazeface_state_dict, synthetic_clip_state_dict
from oracle.adaface_oracle import AdaFaceOracle
from oracle.blazeface_oracle import BlazeFaceOracle
from oracle.clip_oracle import OpenCLIPOracle

EMBEDDERS = ("clip_image", "clip_text", "adaface")
BAR_OF = {"clip_image": "clip", "clip_text": "clip", "adaface": "adaface", "blazeface": "blazeface"}


@pytest.fixture(scope="module")
def blaze_oracle():
    return BlazeFaceOracle(synthetic_blazeface_state_dict(555))


@pytest.fixture(scope="module")
def want(blaze_oracle):
    """The oracle's outputs for the four inputs of each model (CLIP tiny for CLIP).  Shared: do not modify."""
    clip = OpenCLIPOracle(synthetic_clip_state_dict(CLIP_TINY, 4321), CLIP_TINY)
    face = AdaFaceOracle(synthetic_adaface_state_dict(777))
    return {"clip_image": clip.precompute_embedding(bc.clip_images(CLIP_TINY.image_size)),
            "clip_text": clip.encode_tokens(bc.text_tokens(CLIP_TINY)),
            "adaface": np.concatenate([face(f) for f in bc.face_crops()]),
            "blazeface": np.stack([blaze_oracle(f) for f in bc.blaze_images()])}


# ---- the pattern ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", bc.ALL_B)
def test_pattern_has_its_properties(B):
    p = bc.pattern(B)
    assert p.shape == (B,) and p[0] == 0 and np.array_equal(p, bc.pattern(B))          # deterministic from B
    assert bc.pattern_faults(p) == []
    assert p[-1] != p[-2] and p[-1] != p[0]
    assert np.bincount(p, minlength=bc.K).min() >= 2 or (B <= 2 * bc.K and np.bincount(p).max() >= 2)   # condition (b) needs copies to compare


def test_pattern_below_k_and_the_teeth_of_its_audit():
    assert [bc.pattern(B).tolist() for B in (1, 2, 3, 4)] == [[0], [0, 1], [0, 1, 2], [0, 1, 2, 3]]
    assert any("periodic with period 4" in f for f in bc.pattern_faults(np.arange(64) % 4))
    assert any("periodic with period 16" in f for f in bc.pattern_faults(np.tile(bc.pattern(16), 4)))
    assert "two neighbours are the same input" in bc.pattern_faults(np.array([0, 1, 1, 2, 3, 0, 2, 1, 3]))
    assert "an input does not occur" in bc.pattern_faults(np.array([0, 1, 2, 1, 0, 2, 0, 1, 2, 0, 2]))
    assert len({bc.pattern(B)[:8].tobytes() for B in bc.ALL_B}) > 1                  # another batch size, another placement


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
def test_inputs_have_four_structures():
    for imgs in (bc.face_crops().astype(np.float64) / 256, (bc.clip_images(56).transpose(0, 2, 3, 1).astype(np.float64) + 1) / 2):
        noise, grad, blocks, quarter = imgs
        step = lambda v: np.abs(np.diff(v, axis=1)).mean()
        assert step(grad) < 0.05 < step(noise)                                       # smooth against rough
        flat = np.abs(np.diff(blocks, axis=1)).max(-1)
        assert (flat == 0).mean() > 0.7 and flat.max() > 0.5                         # flat colour (at most 13 edges in 55 steps), hard edges
        assert quarter.max() < 0.25 + 1e-6 and noise.max() > 0.9
    t = bc.text_tokens(CLIP_TINY)
    assert t.shape == (4, CLIP_TINY.t_ctx) and len(set(t.argmax(1).tolist())) == 4   # the EOT position differs from row to row
    assert sorted(t.argmax(1).tolist())[0] == 1 and sorted(t.argmax(1).tolist())[-1] == CLIP_TINY.t_ctx - 1   # the empty and the full-length prompt


@pytest.mark.parametrize("model", EMBEDDERS)
def test_the_oracle_separates_the_inputs(model, want):
    """Pairwise more than 10 x the f32 bar apart, or a swapped row would pass condition (a) in f32."""
    w = want[model]
    assert np.allclose(np.linalg.norm(w, axis=1), 1, atol=1e-5)
    sep = bc.separation(w)
    print(f"{model}: the closest two oracle rows differ by {sep:.3g} (10 x the f32 bar: {10 * bc.F32_ABS_BAR[BAR_OF[model]]:g})")
    assert sep > 10 * bc.F32_ABS_BAR[BAR_OF[model]]


def test_blazeface_inputs_keep_rows_in_the_oracle(blaze_oracle, want):
    for kind, img, det in zip(bc.KINDS, bc.blaze_images(), want["blazeface"]):
        alive = int((det[:, 16] != 0).sum())
        _, c = blaze_oracle.raw(img)
        margin = float((torch.sigmoid(c.clamp(-100, 100)) - 0.85).abs().min())
        print(f"blazeface {kind}: {alive} surviving rows, the closest score is {margin:.3g} away from the 0.85 test")
        assert alive > 10
        assert margin > 100 * 1e-5                     # 100 x the f32 score bar (test_gpu_blazeface.py:35, network units): the same rows pass the test on the device
    assert bc.separation(want["blazeface"]) > 10 * 2e-3 / 0.4                        # 10 x the f32 box bar at 640 -> 256


# ---- check_rows ----------------------------------------------------------------------------------------------------------------------------
def _cases():
    for model in EMBEDDERS + ("blazeface",):
        for dtype in ("f32", "f16", "bf16"):
            for B in bc.BATCHES["clip_image" if model == "clip_text" else model] + ((300,) if model != "blazeface" else ()):
                yield pytest.param(model, dtype, B, id=f"{model}-{dtype}-{B}")


def _flip_last_bit(a, i):
    a.reshape(len(a), -1).view(np.uint32)[i, 0] ^= 1


def planted(good: np.ndarray, w: np.ndarray, p: np.ndarray):
    """(name, faulty batch) for each planted fault; `good` is left as it is."""
    B, k = len(p), len(w)
    mid = B // 2
    g = good.copy(); g[mid] = good[mid + 1]
    yield "one row replaced by its neighbour's", g
    yield "all rows shifted by one position", np.roll(good, 1, axis=0)
    g = good.copy(); g[-1] = 0
    yield "the last row zeroed", g
    # CLIP's M = 257 B rows: the last 256-row tile begins inside the last image for every batch size here; a batch above 256 rows has a
    # whole tail past the last multiple of 256
    for start in sorted({B - 1, (B - 1) // 256 * 256} - {0}):
        g = good.copy(); g[start:] = w[(p[start:] + 1) % k]
        yield f"every row from {start} onwards replaced by another input's row", g
    twice = [i for i in range(B) if (p == p[i]).sum() >= 2]                         # at B = 8 two inputs stand once: no copy to differ from
    g = good.copy(); _flip_last_bit(g, twice[-1])
    yield "one copy changed in its last mantissa bit", g


@pytest.mark.parametrize("model,dtype,B", _cases())
def test_check_rows_catches_every_planted_fault(model, dtype, B, want):
    w, p, bar = want[model], bc.pattern(B), bc.BARS[(BAR_OF[model], dtype)]
    good = bc.expand(w, p)
    assert bc.check_rows(good, w, p, bar) < 0.1                   # not 0: the oracle rows are unit vectors to float32 only
    names = []
    for name, bad in planted(good, w, p):
        assert not np.array_equal(bad.view(np.uint32), good.view(np.uint32)), name
        with pytest.raises(AssertionError, match=r"position \d+"):
            bc.check_rows(bad, w, p, bar)
        names.append(name)
    assert len(names) >= 5
    with pytest.raises(AssertionError, match=f"position {B - 1} "):
        bc.check_rows(np.concatenate([good[:-1], np.zeros_like(good[:1])]), w, p, bar)       # the offending position is named
    assert np.array_equal(good, bc.expand(w, p))


@pytest.mark.parametrize("model", EMBEDDERS)
def test_condition_a_alone_catches_what_bit_equality_cannot_see(model, want):
    """Faults that change every copy of an input alike leave condition (b) blind: the f32 bar has to catch them."""
    w, p, bar = want[model], bc.pattern(40), bc.BARS[(BAR_OF[model], "f32")]
    off = w.copy(); off[2, 7] += 3e-5                                               # 1.5 x the bar, in every copy of input 2
    with pytest.raises(AssertionError, match="misses the bar"):
        bc.check_rows(bc.expand(off, p), w, p, bar)
    with pytest.raises(AssertionError, match="position 0 "):
        bc.check_rows(bc.expand(w, (p + 1) % bc.K), w, p, bar)                       # every input swapped for the next one, consistently
    near = w.copy(); near[2, 7] += 5e-6                                             # a quarter of the bar passes, and is reported as such
    assert 0.2 < bc.check_rows(bc.expand(near, p), w, p, bar) < 0.3
