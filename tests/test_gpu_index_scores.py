"""EmbeddingIndex.scores on f32 and bf16 rows, held to float64 at every edge of compute_scores (clearcam_amd/csrc/index.hip):
scores_kernel, scan_kernel<1..8>, scan_bf16_kernel<1..8>, the f32 and bf16 MFMA GEMM and to_bf16_kernel.

Every search feature is tested against the index's own score matrix, so this file is what that matrix stands on.  The tolerances
are those of tests/score_cases.py: the derived order-free bound, the bf16 storage bound, the project's 2e-6 for unit rows on the
scan path, and bit equality wherever the arithmetic is exact (one-hot queries, batch splits on the scan path, equal rows).  Every
case asserts the path it meant to run (last_scores_path against the dispatch table `expected_path`).  The worst error-to-bound
ratio per storage and path is printed when the module is done (pytest -s)."""
import functools

import numpy as np
import pytest

from score_cases import (bf16_edge_rows, bf16_round, bf16_storage_bound, check, exact, expected_path, one_hot, order_free_bound, scaled_rows,
                         scored_queries, stored, unit_rows, with_duplicates)

pytestmark = pytest.mark.gpu

WORST = {}                                                          # (storage, path) -> the largest |error| / order_free_bound seen


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    for (storage, path), w in sorted(WORST.items()):
        print(f"\n[index scores] {storage} path {path}: worst |error| / order-free bound = {w:.4f}", end="")
    print()


def build(storage, E, capacity=None):
    """an index of E's rows, added in two uneven pieces (one where there is a single row) to a capacity that makes it grow"""
    from clearcam_amd.objects import EmbeddingIndex
    n, dim = E.shape
    cut = n // 3
    ix = EmbeddingIndex(dim, capacity if capacity else max(cut, 1), storage=storage)
    if cut:
        ix.add(E[:cut])
    ix.add(E[cut:])
    assert len(ix) == n
    return ix


def scores_on(ix, Q, want_path=None):
    """scores(Q) with the path asserted: the dispatch table's, and `want_path` where the case means to run one in particular"""
    Q = np.atleast_2d(Q)
    got = ix.scores(Q)
    path = expected_path(ix.storage, ix.dim, len(ix), len(Q))
    assert ix.last_scores_path() == path, (ix.storage, ix.dim, len(ix), len(Q), ix.last_scores_path())
    assert want_path is None or path == want_path, (ix.storage, ix.dim, len(ix), len(Q), path)
    return got, path


def held(ix, Q, E, want_path=None, find_copies=None):
    """scores(Q), checked against float64 with the bound of the path that ran"""
    got, path = scores_on(ix, Q, want_path)
    bad, worst = check(got, Q, E, ix.storage, path, find_copies)
    assert not bad, (ix.storage, ix.dim, len(ix), len(np.atleast_2d(Q)), bad)
    WORST[(ix.storage, path)] = max(WORST.get((ix.storage, path), 0.0), worst)
    return got, path


@functools.lru_cache(maxsize=None)
def rows(kind, dim, n=65):
    """(E (n, dim), Q (17, dim)), made once per module; nobody writes to them"""
    E = {"unit": unit_rows, "scaled": scaled_rows}[kind](n, dim, 7 + dim)
    Q = unit_rows(17, dim, 1007 + dim)
    E.setflags(write=False)
    Q.setflags(write=False)
    return E, Q


def probe_cols(dim):
    """every column up to dim 256; beyond, the first and the last 20 and one column in each 16-byte slot of the first 256"""
    if dim <= 256:
        return np.arange(dim)
    return np.unique(np.concatenate([np.arange(20), np.arange(dim - 20, dim), 4 * np.arange(64) + np.arange(64) % 4]))


def assert_reads_back(ix, S, cols, want_path, rows_sel=None):
    """one-hot queries: every product but one is an exact zero, so the scores ARE the stored columns (a zero's sign apart)"""
    got, _ = scores_on(ix, one_hot(ix.dim, cols), want_path)
    want = S.T[cols]
    if rows_sel is not None:
        got, want = got[:, rows_sel], want[:, rows_sel]
    assert got.shape == want.shape and np.array_equal(got, want), (ix.storage, ix.dim, len(ix), np.argwhere(got != want)[:8])


SCAN_DIMS = [("f32", 256), ("f32", 768), ("f32", 36), ("f32", 100), ("bf16", 256), ("bf16", 768)]


# a ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,dim", [("f32", 4), ("f32", 36), ("f32", 100), ("f32", 256), ("f32", 768), ("f32", 4352), ("bf16", 256), ("bf16", 768)])
def test_one_hot_queries_read_the_stored_rows_back_bit_for_bit(storage, dim):
    """37 rows of seven magnitudes and the bf16 edge rows; on the scan path in one call of up to 256 queries (passes of every
    width down to the remainder) and in a call of 3; padded to 40 rows, the same through the GEMM wherever it is reachable."""
    edge = bf16_edge_rows(dim)[0]
    E = np.concatenate([scaled_rows(40 - len(edge), dim, 11 + dim), edge])
    assert len(E) == 40
    cols = probe_cols(dim)
    ix = build(storage, E[:37])
    assert_reads_back(ix, stored(E[:37], storage), cols, 0)
    assert_reads_back(ix, stored(E[:37], storage), cols[-3:], 0)
    ix.close()
    ix = build(storage, E)
    gemm = expected_path(storage, dim, 40, len(cols))
    assert gemm == int(dim in (256, 768, 4352))                     # the GEMM takes every dim with dim % 32 == 0 here (17 or more queries)
    assert_reads_back(ix, stored(E, storage), cols, gemm)
    assert_reads_back(ix, stored(E, storage), cols[:3], 0)
    ix.close()


# b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("storage,dim", SCAN_DIMS)
def test_row_count_edges_within_the_float64_bound(storage, dim, n):
    """every tail of the four lane groups (and of the bf16 kernel's a / b halves): three queries against n rows"""
    for kind in ("unit", "scaled"):
        E, Q = rows(kind, dim)
        ix = build(storage, E[:n])
        held(ix, Q[:3], E[:n], 0)
        ix.close()


# c ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 40])
@pytest.mark.parametrize("storage,dim", SCAN_DIMS)
def test_every_pass_width_scores_like_single_queries(storage, dim, n):
    """The order of the additions of one query does not depend on QB or nq in any of the three scan kernels: a batch on the scan path
    is bit-equal to its queries one at a time, wherever in the batch they stand.  n = 33 keeps every batch on the scan path; at
    n = 40 the 17th query moves an index of dim % 32 == 0 to the GEMM, which is held to the bound."""
    E, Q = rows("unit", dim)
    E = E[:n]
    ix = build(storage, E)
    single = np.concatenate([held(ix, Q[i], E, 0)[0] for i in range(17)])
    for nq in range(1, 18 if dim % 256 == 0 else 10):
        got, path = held(ix, Q[:nq], E)
        if path == 0:
            assert np.array_equal(got, single[:nq]), (nq, np.argwhere(got != single[:nq])[:4])
    assert n != 33 or path == 0
    assert not (n == 40 and dim % 256 == 0) or path == 1
    got, _ = held(ix, Q[3:12], E, 0)
    assert np.array_equal(got, single[3:12])
    ix.close()


# d ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,dim,n,nq,path", [
    ("f32", 768, 64, 16, 0), ("f32", 768, 64, 17, 1), ("f32", 768, 65, 17, 0),
    ("f32", 96, 64, 4, 0), ("f32", 96, 64, 5, 1), ("f32", 96, 66, 5, 0),
    ("f32", 100, 64, 4, 0), ("f32", 100, 64, 5, 0), ("f32", 100, 64, 17, 0),
    ("bf16", 256, 64, 16, 0), ("bf16", 256, 64, 17, 1), ("bf16", 256, 68, 17, 0)])
def test_dispatch_boundaries(storage, dim, n, nq, path):
    """the thresholds of the two GEMMs and the fallbacks when the row count is no multiple of 4 (f32) or 8 (bf16)"""
    E, _ = rows("unit", dim, 68)
    E = E[:n]
    Q = unit_rows(nq, dim, 55 + dim)
    ix = build(storage, E)
    got, _ = held(ix, Q, E, path)
    if storage == "bf16":                                            # and against the rows as they were given: the storage error on top
        lim = bf16_storage_bound(Q, E, queries_rounded=bool(path)) + order_free_bound(scored_queries(Q, storage, path), bf16_round(E))
        assert (np.abs(got - exact(Q, E)) <= lim).all(), float((np.abs(got - exact(Q, E)) / lim).max())
    ix.close()


# e ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,dim,n,nq,path", [
    ("f32", 256, 301, 3, 0), ("f32", 256, 301, 17, 0), ("f32", 256, 304, 17, 1),
    ("f32", 36, 301, 3, 0), ("f32", 36, 304, 9, 0), ("f32", 96, 304, 5, 1),
    ("bf16", 256, 301, 3, 0), ("bf16", 256, 301, 17, 0), ("bf16", 256, 304, 17, 1)])
def test_equal_rows_score_equal_and_rank_by_row_id(storage, dim, n, nq, path):
    """Copies of one row in each of the four lane groups (0..3), in the b half of the bf16 kernel (4..7), at 16 and 17, at 40 and in
    the last row (a partial group at n = 301; at n = 304 more than 256 rows, so another output tile of the GEMM, from the first):
    bit-equal scores under every query (`check` looks for byte-equal rows), and `search` lists them by ascending row id."""
    E, _ = rows("unit", dim, 304)
    pos = (0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 40, n - 1)
    E = with_duplicates(E[:n], pos)
    Q = np.concatenate([E[:1], unit_rows(nq - 1, dim, 77 + dim)])    # the first query is the copied row itself: the copies lead its ranking
    ix = build(storage, E)
    got, _ = held(ix, Q, E, path, find_copies=True)
    assert len(np.unique(got[:, list(pos)].view(np.uint32), axis=1).T) == 1
    idx, sc = ix.search(Q, len(pos) + 3)
    assert ix.last_scores_path() == path
    assert idx[0, :len(pos)].tolist() == list(pos), idx[0]
    assert np.array_equal(sc[0, :len(pos)], got[0, list(pos)]) and sc[0, len(pos)] < sc[0, 0]
    ix.close()


# f ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage,dim,trip", [("f32", 256, 32768), ("bf16", 256, 65536), ("f32", 36, 16384)])
def test_grid_stride_wrap(storage, dim, trip):
    """The smallest row counts at which a wave of scan_kernel (2048 blocks x 4 waves x 4 rows), scan_bf16_kernel (x 8 rows) and
    scores_kernel (4096 blocks x 4 waves x 1 row) takes a second trip, plus 5 rows: the bound everywhere, and the stored values
    read back exactly across the wrap and in the last 40 rows."""
    n = trip + 5
    E = unit_rows(n, dim, 21 + dim)
    Q = unit_rows(2, dim, 22 + dim)
    ix = build(storage, E, capacity=n)
    held(ix, Q, E, 0, find_copies=False)
    sel = np.concatenate([np.arange(trip - 20, trip + 5), np.arange(n - 40, n)])
    assert_reads_back(ix, stored(E, storage), np.arange(dim), 0, np.unique(sel))
    ix.close()


# g ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2048, 2304, 4096])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_wide_rows(storage, dim):
    """Rows whose pass of eight queries asks for more than 64 KB of LDS (from dim 2304 on; 128 KB at 4096): eight queries at once
    within the bound, the stored values read back exactly, and a batch of nine bit-equal to single queries."""
    E, Q = rows("scaled", dim, 37)
    ix = build(storage, E)
    held(ix, Q[:8], E, 0)
    assert_reads_back(ix, stored(E, storage), probe_cols(dim), 0)
    U, _ = rows("unit", dim, 37)
    ux = build(storage, U)
    got, _ = held(ux, Q[:9], U, 0)
    assert np.array_equal(got, np.concatenate([held(ux, Q[i], U, 0)[0] for i in range(9)]))
    ix.close()
    ux.close()


@pytest.mark.parametrize("dim", [5120, 5376, 8192, 16384, 40960])
def test_bf16_rows_too_wide_for_a_pass_of_eight(dim):
    """A bf16 index has no f32-style limit of 4096 on its rows, so the pass width has to give way: the queries of a pass fill the 160 KB
    of a CU at dim 5120 (eight), 8192 (five) and 40960 (one, the widest row an index takes); 5376 takes seven, 16384 two.  Nine
    queries, so every dim cuts at least two passes: within the bound and bit-equal to single queries."""
    E, Q = rows("scaled", dim, 5)
    ix = build("bf16", E)
    got, _ = held(ix, Q[:9], E, 0)
    assert np.array_equal(got, np.concatenate([ix.scores(Q[i]) for i in range(9)]))
    assert_reads_back(ix, stored(E, "bf16"), probe_cols(dim), 0)
    ix.close()


def test_a_bf16_index_too_wide_for_one_query_is_refused_at_create_or_works():
    """dim 65536: a single query is 256 KB, more LDS than a CU has.  Either the index is refused where it is created, with a message
    that names the limit, or it scores; failing at the first search is not acceptable."""
    from clearcam_amd.objects import EmbeddingIndex
    dim = 65536
    try:
        ix = EmbeddingIndex(dim, 3, storage="bf16")
    except RuntimeError as e:
        assert "bf16" in str(e) and "dim" in str(e), str(e)
        return
    E, Q = rows("scaled", dim, 3)
    ix.add(E)
    held(ix, Q[:1], E, 0)
    ix.close()


# h ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("dim", [256, 768])
def test_to_bf16_rounds_the_edge_values_to_the_hand_written_bits(dim, on_device):
    """ties to even on both sides of zero, the carry into the exponent, the largest value that stays finite, zeros: each read back
    through a one-hot query and compared with the bits written down by hand in score_cases.BF16_EDGES"""
    import torch
    E, expected = bf16_edge_rows(dim)
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(dim, 2, storage="bf16")
    ix.add(torch.from_numpy(E[:1]).cuda() if on_device else E[:1])
    ix.add(torch.from_numpy(E[1:]).cuda() if on_device else E[1:])
    cols = sorted({c for _, c, _, _ in expected})
    got, _ = scores_on(ix, one_hot(dim, cols), 0)
    bits = got.view(np.uint32)
    for r, c, f32, b16 in expected:
        have = int(bits[cols.index(c), r])
        if b16 & 0x7fff == 0:
            assert have & 0x7fffffff == 0, (hex(f32), hex(have))                      # a zero; its sign does not survive the sum
        else:
            assert have == b16 << 16, (hex(f32), hex(have), hex(b16 << 16))
    ix.close()
