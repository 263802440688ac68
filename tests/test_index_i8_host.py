"""The int8 storage rule of the embedding index on the host: the numpy restatement of tests/i8_cases.py yields the hand-written
codes on the edges of the rule, its scores stay inside the derived bound, and the Python wrapper and the header name the mode."""
import os
import re

import numpy as np
import pytest

from i8_cases import GROUP, crafted_rows, decode, outlier_rows, quantise, score_bound, unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("dim", [256, 768])
def test_restatement_yields_the_hand_written_codes(dim):
    E, expected = crafted_rows(dim)
    codes, scales = quantise(E)
    assert codes.dtype == np.int8 and scales.dtype == np.float32 and codes.shape == E.shape and scales.shape == (len(E), dim // GROUP)
    assert len(expected) >= dim // GROUP + 8
    for row, g, want, s in expected:
        assert scales[row, g] == s and scales[row, g].tobytes() == np.float32(s).tobytes(), (row, g)
        assert np.array_equal(codes[row, g * GROUP:(g + 1) * GROUP], want), (row, g)
    assert np.abs(codes.astype(np.int32)).max() == 127 and codes.min() >= -127
    # every live group reaches +-127 somewhere, and decoding gives back amax there to within one rounding
    D = decode(codes, scales)
    live = scales > 0
    top = np.abs(codes.astype(np.int32)).reshape(len(E), -1, GROUP).max(axis=2)
    assert (top[live] == 127).all() and (top[~live] == 0).all()
    amax = np.abs(E).reshape(len(E), -1, GROUP).max(axis=2)
    assert np.allclose(np.abs(D).reshape(len(E), -1, GROUP).max(axis=2)[live], amax[live], rtol=2e-7, atol=0)
    # the row of mixed magnitudes: every group keeps its own precision (one scale per row would zero the small groups)
    err = np.abs(D[6].astype(np.float64) - E[6]).reshape(-1, GROUP).max(axis=1)
    assert (err <= (0.5 + 127 * 2.0 ** -23) * scales[6]).all()


def test_scores_of_the_decoded_rows_stay_inside_the_bound():
    rng = np.random.default_rng(22)
    E = unit(rng.standard_normal((2000, 768)))
    Q = unit(rng.standard_normal((11, 768)))
    for rows in (E, outlier_rows(500, 768, 23)):             # (a flushed group, scale 0, loses up to 127 * 2^-126 per element instead)
        codes, scales = quantise(rows)
        D = decode(codes, scales).astype(np.float64)
        err = np.abs(Q.astype(np.float64) @ D.T - Q.astype(np.float64) @ rows.astype(np.float64).T)
        bound = score_bound(Q, scales)
        assert bound.shape == err.shape and (err <= bound).all()
    # unit Gaussian rows: the bound itself is below 1e-2 and the error well inside it
    codes, scales = quantise(E)
    assert score_bound(Q, scales).max() <= 1e-2


def test_the_wrapper_and_the_header_name_the_mode():
    from clearcam_amd.objects import EmbeddingIndex
    assert EmbeddingIndex.STORAGE == {"f32": 0, "bf16": 2, "i8": 8}
    with open(os.path.join(ROOT, "include", "clearcam_hip.h")) as f:
        header = f.read()
    assert re.search(r"^#define\s+CC_INDEX_I8\s+8\s*$", header, re.M)
