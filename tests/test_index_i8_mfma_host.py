"""The arithmetic of the int8 index's MFMA kernel on the host (tests/i8_mfma_cases.py): the three bf16 planes of a query sum back to
it bit for bit, and the group-wise float32 sum of their exact products stays inside the bars the GPU tests hold the device to, on
the inputs of those tests.  The sum inside a group is taken sequentially here, which is pessimistic: the bars of the device tests
(2e-6 absolute on unit rows, 1e-6 relative to sum |q_i d_i|) leave a factor of five and more above what is read here."""
import numpy as np
import pytest

from i8_cases import decode, quantise
from i8_mfma_cases import abs_dot, bf16_round, crafted_world, group_sum_scores, split_planes, unit_world


def planes_sum(q):
    hi, mid, lo = (p.astype(np.float64) for p in split_planes(q))
    return hi + mid + lo                                              # exact in float64: three 8-bit values inside one 24-bit window


def query_sets():
    rng = np.random.default_rng(3)
    mag = np.float32(2.0) ** rng.integers(-100, 101, (64, 256)).astype(np.float32)
    return {"unit": unit_world(768, 1, 65)[1], "eye": np.eye(256, dtype=np.float32),
            "2^-100 .. 2^100": rng.standard_normal((64, 256)).astype(np.float32) * mag,
            "zeros": np.zeros((3, 256), np.float32), "crafted": crafted_world(768)[1]}


@pytest.mark.parametrize("name", ["unit", "eye", "2^-100 .. 2^100", "zeros", "crafted"])
def test_three_planes_sum_back_to_the_query_bit_for_bit(name):
    q = query_sets()[name]
    planes = split_planes(q)
    for p in planes:
        assert np.array_equal(p, bf16_round(p))                      # each plane is a bf16 value
        assert not (p.view(np.uint32) & 0xFFFF).any()
    assert np.array_equal(planes_sum(q), q.astype(np.float64))
    s32 = ((planes[0] + planes[1]).astype(np.float32) + planes[2]).astype(np.float32)
    assert np.array_equal(s32.view(np.uint32) << 1, q.view(np.uint32) << 1)          # and in float32 (the sign of a zero aside)
    if name == "eye":
        assert np.array_equal(planes[0], q) and not planes[1].any() and not planes[2].any()


def test_two_planes_are_not_enough():
    q = query_sets()["unit"]
    hi, mid = split_planes(q, 2)
    left = np.abs(q.astype(np.float64) - hi - mid)
    assert left.max() > 0 and (left <= 2.0 ** -16 * np.abs(q)).all()


def test_group_sum_on_unit_rows_stays_within_the_absolute_bar():
    E, Q, D, scales = unit_world()
    codes = quantise(E)[0]
    dec = Q.astype(np.float64) @ D.astype(np.float64).T
    got = group_sum_scores(Q, codes, scales)
    err = np.abs(got - dec).max()
    print(f"unit rows, three planes: max |score - dec| = {err:.3g}")
    assert err <= 5.9e-8


def test_group_sum_on_crafted_rows_stays_within_the_relative_bar():
    E, Q = crafted_world()
    codes, scales = quantise(E)
    D = decode(codes, scales)
    dec = Q.astype(np.float64) @ D.astype(np.float64).T
    scale = abs_dot(Q, D)
    got = group_sum_scores(Q, codes, scales)
    err = np.abs(got - dec)
    live = scale > 0
    print(f"crafted rows, three planes: max |score - dec| / sum |q d| = {(err[live] / scale[live]).max():.3g}")
    assert (err <= 1.8e-7 * scale).all()
    assert not got[:, ~D.any(axis=1)].any() and not got[18].any()    # all-zero rows and the zero query score exactly 0
    two = np.abs(group_sum_scores(Q, codes, scales, planes=2) - dec)
    print(f"crafted rows, two planes: {(two[live] / scale[live]).max():.3g}")
    assert (two[live] / scale[live]).max() > 1e-6                    # with two planes the device bar itself would be out of reach


def test_one_hot_queries_return_the_decoded_rows():
    E = crafted_world(256)[0]
    codes, scales = quantise(E)
    got = group_sum_scores(np.eye(256, dtype=np.float32), codes, scales)
    assert np.array_equal(got, decode(codes, scales).T)
