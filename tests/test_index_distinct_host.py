"""The numpy model of cc_index_distinct (tests/distinct_cases.py) held to a plain Python double loop, and the conditions the seeded
worlds must meet for the GPU tests (tests/test_gpu_index_distinct.py) to compare exactly.  No GPU."""
import numpy as np
import pytest

from distinct_cases import CHAIN, DIMS, LEVELS, SAME_AT, crafted_rows, distinct_model, greedy, mask_rule, threshold_margins, world
from like_cases import stored

STORAGES = ("f32", "bf16", "i8")


def loop_distinct(lst, score, G_of, same_at, start, count, size):
    """One list, entry by entry, nothing vectorised -> (idx, score, dups) lists of `count` and the total"""
    present = [(p, int(r)) for p, r in enumerate(lst) if 0 <= int(r) < size]
    kept, dups = [], []
    if present:
        G = np.asarray(G_of(np.array([r for _, r in present], np.int64)), np.float32)
        for j in range(len(present)):
            owner = None
            for slot, i in enumerate(kept):
                if G[i][j] >= np.float32(same_at):
                    owner = slot
                    break
            if owner is None:
                kept.append(j)
                dups.append(0)
            else:
                dups[owner] += 1
    oi, os_, od = [-1] * count, [-np.inf] * count, [0] * count
    for k in range(start, min(start + count, len(kept))):
        p, r = present[kept[k]]
        oi[k - start], od[k - start] = r, dups[k]
        if score is not None:
            os_[k - start] = score[p]
    return oi, os_, od, len(kept)


def host_lists(w, D, depth, Q=3):
    """Q ranked lists of `depth` rows by float32 scores of w.q against the stored rows D, with absent entries scattered in"""
    S = (w.q[:Q] @ D.T).astype(np.float32)
    idx = np.argsort(-S, axis=1, kind="stable")[:, :depth].astype(np.int64)
    sc = np.take_along_axis(S, idx, axis=1)
    idx[:, 3::11] = -1
    idx[:, 5::17] = w.n + 2
    return idx, sc


@pytest.mark.parametrize("dim", DIMS)
def test_the_model_is_the_double_loop(dim):
    w = world(dim)
    D = stored(w.E, "f32")
    G_of = lambda rows: (D[rows] @ D[rows].T).astype(np.float32)            # noqa: E731
    for depth in (1, 2, 65, 200):
        idx, sc = host_lists(w, D, depth)
        if depth == 65:
            idx[2] = -1                                                         # an all-absent list
        for same_at in SAME_AT + (np.inf, -np.inf):
            for start, count in ((0, depth), (0, 1), (depth // 3, 7), (depth, 4)):
                for score in (sc, None):
                    got = distinct_model(idx, score, G_of, same_at, start, count, w.n)
                    for q in range(len(idx)):
                        oi, os_, od, total = loop_distinct(idx[q], None if score is None else score[q], G_of, same_at, start, count, w.n)
                        assert got[0][q].tolist() == oi and got[2][q].tolist() == od and int(got[3][q]) == total, (dim, depth, same_at, start, count, q)
                        if score is None:
                            assert got[1] is None
                        else:
                            assert np.array_equal(got[1][q], np.asarray(os_, np.float32))
    # a ranking's head really is full of near-duplicates: the model drops most of it, and keeps more the higher the threshold
    idx, sc = host_lists(w, D, 300)
    totals = [int(distinct_model(idx[:1], None, G_of, t, 0, 300, w.n)[3][0]) for t in SAME_AT]
    present = int(((idx[0] >= 0) & (idx[0] < w.n)).sum())
    assert totals[0] >= totals[1] >= totals[2] and totals[0] < present and totals[0] > totals[2]


@pytest.mark.parametrize("dim", DIMS)
def test_dups_sum_to_what_was_dropped(dim):
    w = world(dim)
    D = stored(w.E, "f32")
    G_of = lambda rows: (D[rows] @ D[rows].T).astype(np.float32)            # noqa: E731
    idx, sc = host_lists(w, D, 500, Q=4)
    for same_at in SAME_AT:
        oi, _, od, total = distinct_model(idx, sc, G_of, same_at, 0, 500, w.n)
        present = ((idx >= 0) & (idx < w.n)).sum(axis=1)
        assert np.array_equal(od.sum(axis=1), present - total) and (od[oi < 0] == 0).all() and (total > 0).all()


@pytest.mark.parametrize("dim", DIMS)
def test_the_chains_tell_the_greedy_rule_from_the_mask_rule(dim):
    w = world(dim)
    for storage in STORAGES:
        D = stored(w.E, storage).astype(np.float64)
        for a, b, c in w.chains:
            G = (D[[a, b, c]] @ D[[a, b, c]].T).astype(np.float32)
            assert abs(G[0, 1] - CHAIN) < 5e-3 and abs(G[1, 2] - CHAIN) < 5e-3 and abs(G[0, 2] - (2 * CHAIN ** 2 - 1)) < 5e-3
            for same_at in SAME_AT:
                keep, owner = greedy(G, same_at)
                assert keep.tolist() == [True, False, True] and owner.tolist() == [-1, 0, -1]
                assert mask_rule(G, same_at).tolist() == [True, False, False]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("storage", STORAGES)
def test_no_pair_of_stored_rows_comes_near_a_threshold(dim, storage):
    """The condition on the inputs under which a comparison with same_at cannot depend on the order of a float32 summation: for every
    pair of stored rows the float64 similarity is further from each threshold than order_free_bound can reach."""
    w = world(dim)
    margins, bound = threshold_margins(stored(w.E, storage), SAME_AT)
    assert bound < 1e-4
    for same_at, m in zip(SAME_AT, margins):
        assert m > 10 * bound, (dim, storage, same_at, m, bound)
    assert min(abs(l - t) for l in LEVELS + (CHAIN, 2 * CHAIN ** 2 - 1, 1.0) for t in SAME_AT) >= 0.01 - 1e-12


@pytest.mark.parametrize("dim", DIMS)
def test_the_crafted_rows_are_exact_in_every_storage(dim):
    E, same_at = crafted_rows(dim)
    for storage in STORAGES:
        D = stored(E, storage)
        assert np.array_equal(D, E), storage                                     # bf16 and int8 hold them as they are
    G = E.astype(np.float64) @ E.astype(np.float64).T
    assert np.array_equal(G.astype(np.float32).astype(np.float64), G) and G.max() < 1.0
    rng = np.random.default_rng(1)
    for _ in range(5):                                                         # a float32 sum in any order is the exact one
        order = rng.permutation(dim)
        acc = np.zeros((4, 4), np.float32)
        for k in order[np.flatnonzero(E[:, order].any(axis=0))]:
            acc = (acc + np.outer(E[:, k], E[:, k]).astype(np.float32)).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64), G)
    up, down = np.nextafter(same_at, np.float32(2)), np.nextafter(same_at, np.float32(0))
    assert np.float32(G[0, 1]) == same_at and np.float32(G[0, 2]) == down and np.float32(G[0, 3]) == up
    keep, owner = greedy(G, same_at)
    assert keep.tolist() == [True, False, True, False] and owner.tolist() == [-1, 0, -1, 0]
