"""Batches of queries on int8 index rows through the MFMA kernel (clearcam_amd/csrc/index_i8_mfma.hip), forced with
cc_dev_set("index_i8_mfma", 1) so that every batch size reaches it, and the default rule that chooses between it and the scan.

Bars (dec = the float64 product with the rows decoded by i8_cases.decode):
  unit rows   |score - dec| <= 2e-6, the bar test_gpu_index_i8.py holds the scan to, and |score - exact| <= score_bound + 2e-6;
  any rows    |score - dec| <= 1e-6 * sum |q_i d_i|, five times what the sequential restatement of tests/i8_mfma_cases.py reads on
              the host; the forced scan is held to it in the same test.
Every product is exact, so a one-hot query must return the decoded matrix bit for bit, and a (query, row) score may depend on nothing
but that pair: those comparisons are np.array_equal."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from i8_cases import decode, quantise, score_bound, unit
from i8_mfma_cases import abs_dot, crafted_world, stored_rows_37, unit_world
from rank_cases import rank_model
from test_gpu_index_remove import assert_same_answers, fresh, slab_rows

pytestmark = pytest.mark.gpu

TILE = 256                                                            # rows per workgroup tile of the kernel, 64 per wave


@contextlib.contextmanager
def mfma_from(value):
    """cc_dev_set("index_i8_mfma"): 1 = every batch on the MFMA kernel, 0 = never, -1 = the default rule (restored on the way out)"""
    from clearcam_amd import _lib
    _lib.check(_lib.lib().cc_dev_set(b"index_i8_mfma", value))
    try:
        yield
    finally:
        _lib.check(_lib.lib().cc_dev_set(b"index_i8_mfma", -1))


def i8_index(dim, rows, *more):
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(dim, max(len(rows), 1), storage="i8")
    ix.add(rows, *more)
    return ix


def mfma_scores(ix, q):
    with mfma_from(1):
        s = ix.scores(q)
        assert ix.last_scores_path() == 2
    return s


def scan_scores(ix, q):
    with mfma_from(0):
        s = ix.scores(q)
        assert ix.last_scores_path() == 0
    return s


@pytest.fixture(scope="module")
def world():
    E, Q, D, scales = unit_world()
    return E, Q, D, scales, Q.astype(np.float64) @ D.astype(np.float64).T, Q.astype(np.float64) @ E.astype(np.float64).T


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257, 1000])
def test_tile_edges(world, n):
    E, Q, D, scales, dec, exact = world
    ix = i8_index(768, E[:n])
    for nq in (1, 15, 16, 17, 33, 64, 65):
        got = mfma_scores(ix, Q[:nq])
        assert got.shape == (nq, n)
        err = np.abs(got - dec[:nq, :n]).max()
        print(f"n {n} Q {nq}: max |score - dec| = {err:.3g}")
        assert err <= 2e-6, (n, nq)
        assert (np.abs(got - exact[:nq, :n]) <= score_bound(Q[:nq], scales[:n]) + 2e-6).all(), (n, nq)
    ix.close()


@pytest.mark.parametrize("dim", [256, 1024])
def test_other_widths(dim):
    E, Q, D, scales = unit_world(dim, 129, 33, seed=100 + dim)
    ix = i8_index(dim, E)
    got = mfma_scores(ix, Q)
    assert np.abs(got - Q.astype(np.float64) @ D.astype(np.float64).T).max() <= 2e-6
    assert (np.abs(got - Q.astype(np.float64) @ E.astype(np.float64).T) <= score_bound(Q, scales) + 2e-6).all()
    ix.close()


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [256, 768])
def test_one_hot_queries_return_the_decoded_rows_bit_for_bit(dim):
    E = stored_rows_37(dim)
    ix = i8_index(dim, E)
    want = decode(*quantise(E))
    got = mfma_scores(ix, np.eye(dim, dtype=np.float32))
    assert got.shape == (dim, 37)
    assert np.array_equal(got, want.T), np.argwhere(got != want.T)[:8]
    ix.close()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_crafted_and_outlier_rows_on_both_paths():
    E, Q = crafted_world()
    D = decode(*quantise(E))
    dec, scale = Q.astype(np.float64) @ D.astype(np.float64).T, abs_dot(Q, D)
    ix = i8_index(768, E)
    live = scale > 0
    for name, got in (("mfma", mfma_scores(ix, Q)), ("scan", scan_scores(ix, Q))):
        err = np.abs(got - dec)
        print(f"{name}: max |score - dec| / sum |q d| = {(err[live] / scale[live]).max():.3g}")
        assert (err <= 1e-6 * scale).all(), name
        assert not got[:, ~D.any(axis=1)].any() and not got[18].any(), name      # all-zero rows (and the zero query) score exactly 0
    ix.close()


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_score_depends_on_its_pair_alone(world):
    E, Q, D, scales, dec, exact = world
    rows = E[:600].copy()
    n = len(rows)
    last = n - n % TILE                                                # first row of the last, partial tile
    copies = {}
    for r in (3, 100, 300):
        copies[r] = (r + 1, r + 16, r + 64, last + 7 + len(copies))
        for c in copies[r]:
            rows[c] = rows[r]
    ix = i8_index(768, rows)
    q = Q[:64]
    full = mfma_scores(ix, q)
    assert np.array_equal(mfma_scores(ix, q), full)                   # a second call
    perm = np.random.default_rng(4).permutation(64)
    assert np.array_equal(mfma_scores(ix, q[perm]), full[perm])
    part = np.sort(np.random.default_rng(5).choice(64, 40, replace=False))
    assert np.array_equal(mfma_scores(ix, q[part]), full[part])
    for r, cs in copies.items():
        for c in cs:
            assert np.array_equal(full[:, c], full[:, r]), (r, c)
    ix.close()


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_loops():
    """The grid is two workgroups per CU and a workgroup takes TILE = 256 rows at a time: one sweep covers 2 * CUs * 256 rows, 131 072
    on 256 CUs.  n = two sweeps, three more tiles and 77 rows (262 989 on 256 CUs), so some workgroups loop three times and the last
    tile is partial.  The rows are copies of 4 099 unit rows (a prime: a copy lands in another lane, wave and tile every time)."""
    import torch
    dim, nq, base = 256, 32, 4099
    E, Q, D, _ = unit_world(dim, base, nq, seed=41)
    n = 2 * (2 * torch.cuda.get_device_properties(0).multi_processor_count * TILE) + 3 * TILE + 77
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(dim, n, storage="i8")
    Ed = torch.from_numpy(E).cuda()
    for a in range(0, n, base):
        ix.add(Ed[:min(base, n - a)])
    assert len(ix) == n
    src = np.arange(n) % base
    got = mfma_scores(ix, Q)
    scan = scan_scores(ix, Q)
    assert np.array_equal(got, got[:, :base][:, src])                 # every copy scores as its original
    assert np.abs(got[:, :base].astype(np.float64) - Q.astype(np.float64) @ D.astype(np.float64).T).max() <= 2e-6
    assert np.abs(got - scan).max() <= 4e-6
    ix.close()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_default_rule(world):
    E, Q, D, scales, dec, exact = world
    ix = i8_index(768, E[:300])
    with mfma_from(-1):
        single = np.concatenate([ix.scores(Q[i]) for i in range(17)])
        assert ix.last_scores_path() == 0
        got = ix.scores(Q[:17])
        assert ix.last_scores_path() == 0 and np.array_equal(got, single)
        got = ix.scores(Q[:64])
        assert ix.last_scores_path() == 2 and np.abs(got - dec[:64, :300]).max() <= 2e-6
    with mfma_from(0):
        got = ix.scores(Q[:64])
        assert ix.last_scores_path() == 0 and np.array_equal(got[:17], single)
    ix.close()
    wide = 4096 + 256                                                  # above the kernel's limit of 4096: the scan, whatever the batch
    Ew, Qw, Dw, _ = unit_world(wide, 5, 64, seed=43)
    ix = i8_index(wide, Ew)
    for key in (-1, 1):
        with mfma_from(key):
            got = ix.scores(Qw)
            assert ix.last_scores_path() == 0
            assert np.abs(got - Qw.astype(np.float64) @ Dw.astype(np.float64).T).max() <= 2e-6
    ix.close()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_everything_above_the_scores():
    """The RankWorld pattern of test_gpu_index_i8.py at 3 000 rows: a crowd near the queries, exact duplicates, groups and track
    slots.  Every search of a 40-query batch is the model of tests/rank_cases.py fed with the index's own scores."""
    rng = np.random.default_rng(12)
    n, dim = 3000, 256
    u = unit(rng.standard_normal(dim))
    E = unit(rng.standard_normal((n, dim)))
    hot = rng.choice(n, 400, replace=False)
    E[hot] = unit(u + 0.08 * rng.standard_normal((400, dim)))
    for r in rng.choice(np.arange(1, n), 300, replace=False):
        E[r] = E[rng.integers(0, r)]
    E[hot[1]] = E[hot[2]] = E[hot[0]]
    group = rng.integers(0, 5, n).astype(np.int32)
    slot = rng.integers(0, 150, n).astype(np.int32)
    slot[rng.random(n) < 0.1] = -1
    allowed = np.array([1, 0, 1, 0, 1], np.uint8)
    q = unit(u + 0.05 * rng.standard_normal((40, dim)))
    ix = i8_index(dim, E, group, slot)

    def same(got, want, what):
        assert ix.last_scores_path() == 2, what
        for g, w in zip(got, want):
            assert np.array_equal(g, w), what

    with mfma_from(1):
        sc = ix.scores(q)
        assert ix.last_scores_path() == 2
        top = np.sort(sc, axis=1)[:, ::-1]
        assert (top[:, :1024] == np.roll(top, 1, axis=1)[:, :1024]).any()            # exact ties among the answers
        for al in (None, allowed):
            for k in (1, 100, 1024):
                same(ix.search(q, k, al), rank_model(sc, slot, group, 0, k, al, None, tracks=False)[:2], ("search", k, al is not None))
            for k in (10, 1024):
                same(ix.search_tracks(q, k, al), rank_model(sc, slot, group, 0, k, al, None, tracks=True)[:2], ("search_tracks", k, al is not None))
            for tracks in (False, True):
                for start, count in ((0, 10), (100 if tracks else 1500, 50)):    # the second window lies deep in the order
                    same(ix.rank(q, start, count, al, None, tracks), rank_model(sc, slot, group, start, count, al, None, tracks),
                         ("rank", tracks, start, al is not None))
    ix.close()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_after_removal_and_growth():
    rng = np.random.default_rng(13)
    n, dim = 5000, 256
    E = unit(rng.standard_normal((n + 300, dim)))
    for r in rng.choice(np.arange(1, n), 500, replace=False):
        E[r] = E[rng.integers(0, r)]
    group = rng.integers(0, 8, n + 300).astype(np.int32)
    slot = rng.integers(-1, 120, n + 300).astype(np.int32)
    q = unit(E[:40] + 0.2 * rng.standard_normal((40, dim)))
    allowed = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
    rows = np.arange(n)
    drop = rows % 3 == 0
    with slab_rows(256), mfma_from(1):
        ix = i8_index(dim, E[:n], group[:n], slot[:n])
        assert ix.remove(drop) == int(drop.sum())
        live = np.flatnonzero(~drop)
        ref = fresh(E[live], group[live], slot[live], "i8", dim)
        assert_same_answers(ix, ref, q, allowed, "removal")
        assert ix.last_scores_path() == 2 and ref.last_scores_path() == 2
        ref.close()
        more = np.arange(n, n + 300)
        ix.add(E[more], group[more], slot[more])
        live = np.concatenate([live, more])
        ref = fresh(E[live], group[live], slot[live], "i8", dim)
        assert_same_answers(ix, ref, q, allowed, "removal, then 300 rows")
        assert ix.last_scores_path() == 2
        assert np.array_equal(ix.scores(np.eye(dim, dtype=np.float32)[:40]), decode(*quantise(E[live])).T[:40])
        ref.close(); ix.close()


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_device_queries_on_a_caller_stream(world):
    import torch
    from clearcam_amd import _lib
    E, Q, D, scales, dec, exact = world
    n, nq = 300, 33
    ix = i8_index(768, E[:n])
    want = mfma_scores(ix, Q[:nq])
    qd = torch.from_numpy(Q[:nq]).cuda()
    out = torch.zeros((nq, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with mfma_from(1):
        _lib.check(_lib.lib().cc_index_scores(ix._h, _lib.ptr(qd), nq, _lib.ptr(out), 1, C.c_void_p(stream.cuda_stream)))
        assert ix.last_scores_path() == 2
    stream.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    ix.close()
