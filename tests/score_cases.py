"""The score matrix of an f32 or bf16 embedding index (compute_scores in clearcam_amd/csrc/index.hip) held to float64: the storage
rule, the dispatch contract, the error bounds, the row makers and the checker, in plain numpy.  Shared by
tests/test_score_cases_host.py (where the checker is shown to reject subtly wrong kernels and to pass faithful ones) and
tests/test_gpu_index_scores.py (where the device is held to it).

Every tolerance here is derived: `order_free_bound` from the float32 format alone, `bf16_storage_bound` from the bf16 format, and
bit equality wherever the arithmetic is exact.  The one bare figure is BAR, the project's existing 2e-6 for unit rows on the scan
path (tests/test_gpu_clip.py, tests/test_gpu_index_i8.py)."""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of float32
BAR = 2e-6                        # the project's bar for unit rows against unit queries on the scan path


# ---- storage ------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> the 16 bits of the nearest bf16, ties to even: the rule, on the bits.  bf16 keeps the upper half of a float32.
    With b the lowest kept bit, adding 0x7fff + b to the word carries into the kept half exactly when the dropped half is above
    0x8000, or is 0x8000 (halfway) and b is 1; a carry out of an all-ones mantissa lands in the exponent, which is the right
    answer too.  NaN and inf are out of scope."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_round(E):
    """float32 -> bf16 -> float32: what a bf16 index holds of E"""
    return (bf16_bits(E).astype(np.uint32) << 16).view(np.float32)


def stored(E, storage):
    E = np.ascontiguousarray(E, dtype=np.float32)
    return bf16_round(E) if storage == "bf16" else E


def scored_queries(Q, storage, path):
    """The queries as the kernel multiplies them: the bf16 GEMM (bf16 rows, path 1) rounds them to bf16, nothing else does."""
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    return bf16_round(Q) if (storage == "bf16" and path == 1) else Q


# ---- the reference and its bounds ---------------------------------------------------------------------------------------------
def exact(Q, E):
    """(Q, dim), (n, dim) -> (Q, n) float64"""
    return np.atleast_2d(np.asarray(Q, np.float64)) @ np.asarray(E, np.float64).T


def gamma(d):
    return d * U / (1.0 - d * U)


def order_free_bound(Q, E):
    """(Q, n) float64: gamma(dim) * (|Q| @ |E|.T), gamma(d) = d u / (1 - d u), u = 2^-24.

    The float32 products of a score are formed exactly (fma, or the f32 MFMA) and every product then passes through at most dim
    roundings on its way into the sum, whatever the order of the additions (sequential, a tree, lanes then a butterfly, MFMA
    blocks): the computed sum is sum_i e_i q_i (1 + t_i) with |t_i| <= (1 + u)^dim - 1 <= gamma(dim) (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.1).  So it holds for every path of compute_scores.  For bf16 rows it is applied
    to bf16_round(E), on the bf16 GEMM also to bf16_round(Q): the error of the arithmetic, not of the storage."""
    Q = np.atleast_2d(np.asarray(Q, np.float64))
    E = np.asarray(E, np.float64)
    return gamma(E.shape[1]) * (np.abs(Q) @ np.abs(E).T)


def bf16_storage_bound(Q, E, queries_rounded):
    """(Q, n) float64: the figure a bf16-mode score is allowed to differ from the exact-row score by, on top of
    order_free_bound of the stored values.

    A stored element is e (1 + d) and the score differs from the exact one by sum_i q_i e_i d_i, at most D * (|Q| @ |E|.T) with
    D the largest |d_i|.  With the queries rounded too (the bf16 GEMM) the factor is (1 + d)(1 + d') - 1 <= 2 D + D^2.  The
    issue that asked for these tests sets D = 2^-9: 2^-9 for rounded rows, 2^-8 + 2^-18 with rounded queries.  bf16 keeps 8
    significant bits, so a single element can be off by up to 2^-8 / (1 + 2^-8) of itself (1 + 2^-8 is stored as 1): 2^-9 is
    NOT the worst case of one element but what a row of elements that do not all sit at halfway points stays within (the mean
    |d| of a rounding is a quarter of an ulp, 2^-9 at the bottom of a binade and 2^-10 at its top).  It is therefore applied to
    random rows only, never to bf16_edge_rows, and kept as set: a kernel that truncates, or rounds twice, doubles the mean and
    is caught by it."""
    D = 2.0 ** -9
    f = (2 * D + D * D) if queries_rounded else D
    return f * (np.abs(np.atleast_2d(np.asarray(Q, np.float64))) @ np.abs(np.asarray(E, np.float64)).T)


# ---- the dispatch contract ----------------------------------------------------------------------------------------------------
def expected_path(storage, dim, n, Q):
    """What last_scores_path() must say: 0 scan passes, 1 the MFMA GEMM.  f32: the GEMM iff Q > T and n % 4 == 0 and
    dim % 32 == 0, with T = 16 where scan_kernel serves (dim % 256 == 0 and dim <= 4096) and 4 where scores_kernel does.  bf16: the
    GEMM iff Q > 16 and n % 8 == 0.  (The 16-byte alignment the GEMM also asks of the row matrix holds for every dim an index accepts.)"""
    if storage == "f32":
        T = 16 if (dim % 256 == 0 and dim <= 4096) else 4
        return int(Q > T and n % 4 == 0 and dim % 32 == 0)
    if storage == "bf16":
        return int(Q > 16 and n % 8 == 0)
    raise ValueError(storage)


# ---- row makers ---------------------------------------------------------------------------------------------------------------
def unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def unit_rows(n, dim, seed):
    return unit(np.random.default_rng(seed).standard_normal((n, dim)))


def scaled_rows(n, dim, seed):
    """unit rows times 10^k, k drawn from -3..3 per row"""
    rng = np.random.default_rng(seed)
    E = unit(rng.standard_normal((n, dim))).astype(np.float64)
    return (E * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(np.float32)


def cancelling_rows(n, dim, nq, seed):
    """-> (E (n, dim), Q (nq, dim)), unit rows and unit queries with every exact score about 1e-4 of sum_i |e_i q_i|: a row is drawn
    in the orthogonal complement of the queries and then given 1e-4 * 0.64 of each query (0.64 ~ 2 / pi is what sum |e_i q_i| comes
    to for unit Gaussian directions).  The large terms of such a score cancel, so an error in any one of them shows in full."""
    assert dim > nq
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((nq, dim))
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    basis, _ = np.linalg.qr(Q.T)                                   # (dim, nq): an orthonormal basis of the queries' span
    G = rng.standard_normal((n, dim))
    G -= (G @ basis) @ basis.T
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    G += 0.64e-4 * rng.choice([-1.0, 1.0], (n, nq)) @ Q
    return G.astype(np.float32), Q.astype(np.float32)


# (float32 bits, bf16 bits) written down by hand.  A bf16 is the upper 16 bits; the lower 16 decide the rounding: below 0x8000 down,
# above up, 0x8000 to the even neighbour.
BF16_EDGES = (
    (0x3F808000, 0x3F80),       # 1 + 2^-8: halfway, the kept mantissa 0x00 is even -> stays 1.0
    (0x3F818000, 0x3F82),       # 1 + 2^-7 + 2^-8: halfway, kept mantissa 0x01 is odd -> up to 1 + 2^-6
    (0x3F828000, 0x3F82),       # the next halfway: even again -> down, the same bf16 as the one before
    (0x3F808001, 0x3F81),       # one bit above halfway -> up
    (0x3F807FFF, 0x3F80),       # one bit below halfway -> down
    (0xBF808000, 0xBF80),       # the same four with the sign set: rounding is on the magnitude
    (0xBF818000, 0xBF82),
    (0xBF808001, 0xBF81),
    (0xBF807FFF, 0xBF80),
    (0x3FFFFFFF, 0x4000),       # 2 - 2^-23, mantissa all ones: the carry runs into the exponent -> 2.0
    (0x3FFF8000, 0x4000),       # 2 - 2^-8: halfway with an odd, all-ones kept mantissa -> 2.0 as well
    (0x3FFF7FFF, 0x3FFF),       # just below: stays 2 - 2^-7, the largest bf16 under 2
    (0xC0FFC000, 0xC100),       # -(8 - 2^-7): above halfway, carries into the exponent -> -8.0
    (0x7F7F7FFF, 0x7F7F),       # the largest float32 that still rounds to a finite bf16 (0x7F7F8000 would go to inf)
    (0xFF7F7FFF, 0xFF7F),
    (0x7F7F0000, 0x7F7F),       # the largest bf16 itself
    (0x00808000, 0x0080),       # halfway, even, at the smallest normal exponent: stays 2^-126
    (0x0D818000, 0x0D82),       # a halfway case far down the range (about 8e-31): odd -> up
    (0x00000000, 0x0000),       # +0
    (0x80000000, 0x8000),       # -0 keeps its sign in storage (a score reads it back as a zero of either sign)
    (0x3F800000, 0x3F80),       # exact values stay: 1.0
    (0xC2F70000, 0xC2F7),       # -123.5
)


def bf16_edge_rows(dim, seed=3):
    """-> (E (rows, dim) float32, expected): rows of a few magnitudes with the BF16_EDGES values laid into them, up to eight per row
    in columns spread from the first to the last.  expected lists (row, col, float32 bits, bf16 bits).  The rows are for one-hot
    queries only: beside 3.4e38 no other sum means anything."""
    assert dim >= 4
    per = min(dim, 8)
    cols = np.unique(np.linspace(0, dim - 1, per).astype(int))
    assert len(cols) == per
    rows = -(-len(BF16_EDGES) // per)
    rng = np.random.default_rng(seed)
    E = (unit(rng.standard_normal((rows, dim))).astype(np.float64) * 10.0 ** rng.integers(-2, 3, (rows, 1))).astype(np.float32)
    expected = []
    for k, (f32, b16) in enumerate(BF16_EDGES):
        r, c = k // per, int(cols[k % per])
        E[r, c] = np.array([f32], np.uint32).view(np.float32)[0]
        expected.append((r, c, f32, b16))
    return E, expected


def with_duplicates(E, positions):
    """A copy of E with the row at positions[0] copied, byte for byte, to every other position"""
    E = np.array(E, dtype=np.float32)
    E[list(positions[1:])] = E[positions[0]]
    return E


def one_hot(dim, cols):
    Q = np.zeros((len(cols), dim), np.float32)
    Q[np.arange(len(cols)), cols] = 1.0
    return Q


# ---- the checker --------------------------------------------------------------------------------------------------------------
def equal_row_groups(E):
    """lists of row ids (two or more) whose rows are byte-equal"""
    b = np.ascontiguousarray(E, dtype=np.float32).view(np.uint32)
    _, inv, cnt = np.unique(b, axis=0, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    return [np.flatnonzero(inv == g) for g in np.flatnonzero(cnt > 1)]


def is_unit(A):
    return bool((np.abs(np.linalg.norm(np.asarray(A, np.float64), axis=-1) - 1.0) < 1e-3).all())


def check(got, Q, E, storage, path, find_copies=None):
    """got (Q, n) against queries Q (Q, dim) and the rows E (n, dim) as they were GIVEN to an index of `storage` ("f32" / "bf16") that
    answered on `path` (0 scan, 1 GEMM).  -> (violations, worst): a list of strings, empty when all is well, and the largest
    |got - exact| / order_free_bound.

    Checked: shape; finiteness; |got - exact(stored)| <= order_free_bound(stored) elementwise (stored: what the kernel multiplies:
    bf16_round of the rows of a bf16 index, and of the queries on its GEMM); BAR on the scan path where rows and queries are unit
    vectors; and that byte-equal rows have bit-equal scores under every query (looked for up to 4096 rows unless find_copies says)."""
    Q = np.ascontiguousarray(np.atleast_2d(Q), dtype=np.float32)
    E = np.ascontiguousarray(E, dtype=np.float32)
    got = np.asarray(got)
    bad = []
    if got.shape != (Q.shape[0], E.shape[0]) or got.dtype != np.float32:
        return [f"shape {got.shape} {got.dtype}, expected {(Q.shape[0], E.shape[0])} float32"], float("inf")
    if not np.isfinite(got).all():
        bad.append(f"{(~np.isfinite(got)).sum()} scores are not finite, first at {tuple(np.argwhere(~np.isfinite(got))[0])}")
    S, Qs = stored(E, storage), scored_queries(Q, storage, path)
    want, bound = exact(Qs, S), order_free_bound(Qs, S)
    err = np.abs(np.where(np.isfinite(got), got, np.inf).astype(np.float64) - want)
    over = err > bound
    if over.any():
        c, r = np.argwhere(over)[0]
        bad.append(f"{over.sum()} scores outside the order-free bound, first (query {c}, row {r}): got {got[c, r]!r}, exact {want[c, r]!r}, "
                   f"bound {bound[c, r]:.3g}")
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    if path == 0 and is_unit(E) and is_unit(Q) and (err > BAR).any():
        c, r = np.argwhere(err > BAR)[0]
        bad.append(f"{(err > BAR).sum()} unit-row scores off by more than {BAR}, first (query {c}, row {r}): {err[c, r]:.3g}")
    if find_copies if find_copies is not None else E.shape[0] <= 4096:
        for ids in equal_row_groups(E):
            col = got[:, ids].view(np.uint32)
            if (col != col[:, :1]).any():
                c, k = np.argwhere(col != col[:, :1])[0]
                bad.append(f"rows {ids[0]} and {ids[k]} are byte-equal but score {got[c, ids[0]]!r} and {got[c, ids[k]]!r} under query {c}")
    return bad, worst
