"""The arithmetic of the MFMA kernel for batches of queries on int8 index rows (clearcam_amd/csrc/index_i8_mfma.hip) restated in
numpy, with the inputs its tests share: tests/test_index_i8_mfma_host.py checks the restatement on the host,
tests/test_gpu_index_i8_mfma.py holds the device to the same bars on the same inputs.

A query stays float32 and is split into three bf16 planes, hi = bf16(q), mid = bf16(q - hi), lo = bf16(q - hi - mid), whose sum is q
bit for bit.  An int8 code is exact in bf16, so every product plane x code is exact in float32.  Per scale group of 32 elements the
products of the three planes are added into a fresh float32 partial, then acc = fma(partial, scale, acc) in float32."""
import numpy as np

from i8_cases import GROUP, crafted_rows, decode, outlier_rows, quantise, unit


def bf16_round(x):
    """float32 -> the nearest bf16 value (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def split_planes(q, planes=3):
    """float32 -> `planes` arrays of bf16 values (as float32): each is the bf16 rounding of what the ones before it left over"""
    rest = np.ascontiguousarray(q, dtype=np.float32)
    out = []
    for _ in range(planes):
        p = bf16_round(rest)
        out.append(p)
        rest = (rest - p).astype(np.float32)                        # exact: the leftover has fewer significant bits than float32 holds
    return out


def group_sum_scores(q, codes, scales, planes=3):
    """(Q, dim) float32 queries, (n, dim) int8 codes, (n, dim / 32) float32 scales -> (Q, n) float32.  Inside a group the products
    are added one after the other in float32, smallest plane first: an order that is at least as bad as any the hardware may take."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    P = split_planes(q, planes)[::-1]
    c = codes.astype(np.float32)
    acc = np.zeros((q.shape[0], codes.shape[0]), np.float32)
    for g in range(codes.shape[1] // GROUP):
        part = np.zeros_like(acc)
        for p in P:
            for k in range(g * GROUP, (g + 1) * GROUP):
                part = (part + p[:, k, None] * c[None, :, k]).astype(np.float32)       # the product is exact in float32
        # fma: the product of two float32 is exact in float64, the sum is rounded once to float64 and once to float32
        acc = (part.astype(np.float64) * scales[None, :, g].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def abs_dot(q, D):
    """sum_i |q_i d_i| in float64, (Q, n): the scale of a score's rounding error"""
    return np.abs(np.atleast_2d(q).astype(np.float64)) @ np.abs(D.astype(np.float64)).T


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------
def unit_world(dim=768, n=1000, nq=65, seed=11):
    """Unit rows and unit queries; for dim 768 the rows and the first 17 queries are those of test_gpu_index_i8.py's fixture.
    -> E, Q, decoded rows, scales"""
    rng = np.random.default_rng(seed)
    E = unit(rng.standard_normal((n, dim)))
    Q = unit(rng.standard_normal((nq, dim)))
    codes, scales = quantise(E)
    return E, Q, decode(codes, scales), scales


def stored_rows_37(dim):
    """The 37 rows of test_gpu_index_i8.py's first test: the crafted rows among random rows of several magnitudes"""
    crafted, _ = crafted_rows(dim)
    rng = np.random.default_rng(7)
    rand = rng.standard_normal((30, dim)).astype(np.float32) * (10.0 ** rng.integers(-3, 3, (30, 1))).astype(np.float32)
    return np.concatenate([crafted[:1], rand[:8], crafted[1:], rand[8:]])


def crafted_world(dim=768):
    """Rows on the edges of the storage rule (zero groups, a scale at the smallest normal, groups from 1e-6 to 1e3 in one row), rows
    with outliers, and queries of several magnitudes: unit ones and larger.  None is smaller, because the score of a unit query with
    the row whose scale is the smallest normal number is already at the edge of float32's normal range, and below it a float32 has an
    absolute precision (2^-149), which no bar relative to sum |q_i d_i| can describe.  -> E, Q"""
    E = np.concatenate([crafted_rows(dim)[0], outlier_rows(40, dim, 17), np.zeros((1, dim), np.float32)])
    rng = np.random.default_rng(21)
    Q = unit(rng.standard_normal((20, dim)))
    Q[16] *= np.float32(37.0); Q[17] *= np.float32(1e3); Q[18] = 0
    Q[19] = (rng.standard_normal(dim) * 10.0 ** rng.integers(0, 5, dim)).astype(np.float32)
    return E, Q
