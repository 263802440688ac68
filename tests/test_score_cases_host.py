"""tests/score_cases.py on the host: the checker that holds the f32 and bf16 scoring kernels of the embedding index to float64
(tests/test_gpu_index_scores.py) passes a float32 restatement of every summation shape those kernels have, and rejects each of a
list of subtly wrong kernels, on every row maker.  No GPU."""
import numpy as np
import pytest

from score_cases import (BAR, BF16_EDGES, bf16_bits, bf16_edge_rows, bf16_round, bf16_storage_bound, cancelling_rows, check, exact,
                         expected_path, gamma, one_hot, order_free_bound, scaled_rows, scored_queries, stored, unit_rows, with_duplicates)

DIMS = (36, 256, 768)
N, NQ = 41, 3


def fma32(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32, which differs
    from one rounding only where the float64 sum lies within 2^-29 ulp of a float32 tie"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def lanes_then_tree(Q, E, lanes, vec):
    """The scan kernels' order: lane l of `lanes` owns the slots of `vec` elements l, l + lanes, l + 2 lanes, ... of a row and
    accumulates them in ascending order with fma from zero; the lane sums are then added as an xor butterfly, lanes / 2 first.
    scan_kernel: 16 lanes x 4; scan_bf16_kernel: 16 x 8; scores_kernel: 64 x 4 (lanes past the end of a short row hold zero)."""
    Q, E = np.atleast_2d(Q), np.asarray(E)
    n, dim = E.shape
    pad = -dim % (lanes * vec)
    Er = np.pad(E, ((0, 0), (0, pad))).reshape(n, -1, lanes, vec)
    Qr = np.pad(Q, ((0, 0), (0, pad))).reshape(len(Q), -1, lanes, vec)
    out = np.empty((len(Q), n), np.float32)
    idx = np.arange(lanes)
    for c in range(len(Q)):
        acc = np.zeros((n, lanes), np.float32)
        for t in range(Er.shape[1]):
            for k in range(vec):
                acc = fma32(Er[:, t, :, k], Qr[c, t, :, k][None, :], acc)
        o = lanes // 2
        while o:
            acc = acc + acc[:, idx ^ o]
            o //= 2
        out[c] = acc[:, 0]
    return out


def matmul32(Q, E):
    """a plain float32 matmul, for the GEMM: exact products, float32 sums in an order of the library's choosing"""
    return np.atleast_2d(Q).astype(np.float32) @ np.asarray(E, np.float32).T


SHAPES = {"16x4": lambda Q, E: lanes_then_tree(Q, E, 16, 4), "16x8": lambda Q, E: lanes_then_tree(Q, E, 16, 8),
          "64x4": lambda Q, E: lanes_then_tree(Q, E, 64, 4), "matmul": matmul32}


def makers(dim):
    q = unit_rows(NQ, dim, 100 + dim)
    ce, cq = cancelling_rows(N, dim, NQ, 300 + dim)
    return {"unit": (unit_rows(N, dim, 1 + dim), q), "scaled": (scaled_rows(N, dim, 2 + dim), q), "cancelling": (ce, cq)}


def faithful(Q, E, storage, path, shape="16x4"):
    """scores as a correct kernel of that storage and path would give them"""
    return SHAPES["matmul" if path else shape](scored_queries(Q, storage, path), stored(E, storage))


# ---- the faithful restatements pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_summation_shape_passes(shape, storage, dim):
    path = int(shape == "matmul")
    for name, (E, Q) in makers(dim).items():
        bad, worst = check(faithful(Q, E, storage, path, shape), Q, E, storage, path)
        assert not bad, (name, bad)
        assert worst < 1.0, (name, worst)


@pytest.mark.parametrize("dim", DIMS)
def test_cancelling_rows_cancel(dim):
    E, Q = cancelling_rows(N, dim, NQ, 300 + dim)
    rel = np.abs(exact(Q, E)) / (np.abs(Q.astype(np.float64)) @ np.abs(E.astype(np.float64)).T)
    assert 2e-5 < rel.min() and rel.max() < 5e-4, (rel.min(), rel.max())


@pytest.mark.parametrize("dim", DIMS)
def test_bf16_scores_stay_within_the_storage_bound_of_the_exact_rows(dim):
    for name in ("unit", "scaled"):
        E, Q = makers(dim)[name]
        for path in (0, 1):
            got = faithful(Q, E, "bf16", path)
            lim = bf16_storage_bound(Q, E, queries_rounded=bool(path)) + order_free_bound(scored_queries(Q, "bf16", path), bf16_round(E))
            assert (np.abs(got - exact(Q, E)) <= lim).all(), (name, path)


# ---- the mutants are rejected -------------------------------------------------------------------------------------------------
def drop_last4(Q, E, storage, path):
    S = stored(E, storage).copy()
    S[:, -4:] = 0
    return SHAPES["matmul" if path else "16x4"](scored_queries(Q, storage, path), S)


def drop_middle_slot(Q, E, storage, path):
    S = stored(E, storage).copy()
    m = E.shape[1] // 8 * 4
    S[:, m:m + 4] = 0
    return SHAPES["matmul" if path else "16x4"](scored_queries(Q, storage, path), S)


def row_answered_with_last(Q, E, storage, path):
    got = faithful(Q, E, storage, path)
    got[:, 5] = got[:, -1]
    return got


def query_answered_with_next(Q, E, storage, path):
    got = faithful(Q, E, storage, path)
    got[1] = got[2]
    return got


def truncated_bf16(Q, E, storage, path):
    S = (np.ascontiguousarray(E, np.float32).view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    return SHAPES["matmul" if path else "16x8"](scored_queries(Q, storage, path), S)


MUTANTS = {"last 4 elements dropped": drop_last4, "a 16-byte slot dropped": drop_middle_slot, "row answered with row n-1": row_answered_with_last,
           "query answered with the next": query_answered_with_next}


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_is_rejected(mutant, storage, path, dim):
    for name, (E, Q) in makers(dim).items():
        bad, _ = check(MUTANTS[mutant](Q, E, storage, path), Q, E, storage, path)
        assert bad, (mutant, name)


@pytest.mark.parametrize("dim", [256, 768])
@pytest.mark.parametrize("path", [0, 1])
def test_truncation_in_place_of_rounding_is_rejected(path, dim):
    for name, (E, Q) in makers(dim).items():
        bad, _ = check(truncated_bf16(Q, E, "bf16", path), Q, E, "bf16", path)
        assert bad, name


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_a_duplicate_off_by_one_bit_is_rejected(storage, path, dim):
    for name, (E, Q) in makers(dim).items():
        D = with_duplicates(E, (2, 9, N - 1))
        # a fixed order on both paths: the host library's matmul gives equal rows scores that differ in the last bit at the edge of its tiles
        got = SHAPES["16x8"](scored_queries(Q, storage, path), stored(D, storage))
        bad, _ = check(got, Q, D, storage, path)
        assert not bad, (name, bad)
        got[1, N - 1] = np.nextafter(got[1, N - 1], np.float32(np.inf))
        bad, _ = check(got, Q, D, storage, path)
        assert len(bad) == 1 and "byte-equal" in bad[0], (name, bad)                   # nothing but the tie rule sees one bit


def test_wrong_shape_and_non_finite_scores_are_rejected():
    E, Q = makers(36)["unit"]
    got = faithful(Q, E, "f32", 0)
    assert check(got[:, :-1], Q, E, "f32", 0)[0] and check(got.astype(np.float64), Q, E, "f32", 0)[0]
    got[0, 3] = np.nan
    assert check(got, Q, E, "f32", 0)[0]


# ---- one-hot queries read the stored matrix back ------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 36, 256])
def test_one_hot_scores_are_the_stored_columns_in_every_shape(dim):
    E = np.concatenate([scaled_rows(9, dim, 5), bf16_edge_rows(dim)[0]])
    for storage in ("f32", "bf16"):
        S = stored(E, storage)
        for shape, f in SHAPES.items():
            got = f(one_hot(dim, np.arange(dim)), S)
            assert np.array_equal(got, S.T), (storage, shape)


# ---- bf16_round ---------------------------------------------------------------------------------------------------------------
def test_bf16_round_is_torchs_rounding_bit_for_bit():
    import torch
    rng = np.random.default_rng(9)
    bits = rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits >> 23) & 0xff != 0xff]                                        # NaN and inf are out of scope
    bits = bits[(bits & 0x7fffffff) < 0x7F7F8000]                                   # and so is what rounds to inf
    x = np.concatenate([bits.view(np.float32), rng.standard_normal(100000).astype(np.float32),
                        (bits[:20000] & np.uint32(0xffff0000) | np.uint32(0x8000)).view(np.float32)])   # a fifth of them exact ties
    x = x[np.abs(x) < 3.38e38]
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bf16_bits(x), want)
    assert np.array_equal(bf16_round(x).view(np.uint32), torch.from_numpy(x).to(torch.bfloat16).float().numpy().view(np.uint32))


@pytest.mark.parametrize("dim", [4, 36, 256, 768])
def test_bf16_round_gives_the_hand_written_bits(dim):
    E, expected = bf16_edge_rows(dim)
    assert len(expected) == len(BF16_EDGES)
    B = bf16_bits(E)
    for r, c, f32, b16 in expected:
        assert E.view(np.uint32)[r, c] == f32 and B[r, c] == b16, (r, c, hex(f32), hex(int(B[r, c])), hex(b16))
    assert np.isfinite(bf16_round(E)).all()
    halfway = [(f, b) for f, b in BF16_EDGES if f & 0xffff == 0x8000]
    assert any((f >> 16) & 1 == 0 and b == f >> 16 for f, b in halfway) and any((f >> 16) & 1 and b == (f >> 16) + 1 for f, b in halfway)
    assert any((f >> 23) != (b >> 7) for f, b in BF16_EDGES)                         # a carry into the exponent


# ---- the dispatch table -------------------------------------------------------------------------------------------------------
def test_expected_path_at_its_boundaries():
    P = expected_path
    assert (P("f32", 768, 64, 16), P("f32", 768, 64, 17), P("f32", 768, 65, 17), P("f32", 768, 66, 17)) == (0, 1, 0, 0)
    assert (P("f32", 4096, 64, 17), P("f32", 4352, 64, 17), P("f32", 4352, 64, 5), P("f32", 4352, 64, 4)) == (1, 1, 1, 0)
    assert (P("f32", 96, 64, 4), P("f32", 96, 64, 5), P("f32", 96, 66, 5)) == (0, 1, 0)
    assert (P("f32", 100, 64, 5), P("f32", 100, 64, 64), P("f32", 36, 64, 64), P("f32", 4, 64, 64)) == (0, 0, 0, 0)
    assert (P("bf16", 256, 64, 16), P("bf16", 256, 64, 17), P("bf16", 256, 68, 17), P("bf16", 256, 60, 64)) == (0, 1, 0, 0)
    with pytest.raises(ValueError):
        P("i8", 256, 64, 1)


def test_the_bound_is_the_textbook_one():
    assert gamma(768) == 768 * 2.0 ** -24 / (1 - 768 * 2.0 ** -24)
    E, Q = makers(36)["scaled"]
    assert np.array_equal(order_free_bound(Q, E), gamma(36) * (np.abs(Q.astype(np.float64)) @ np.abs(E.astype(np.float64)).T))
    assert BAR == 2e-6
