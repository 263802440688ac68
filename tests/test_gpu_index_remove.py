"""cc_index_remove_rows / cc_index_remove_groups on the GPU: rows leave by stable compaction in place, and every answer afterwards
equals, bit for bit, that of a fresh index built with `add` from the surviving host rows in their order.

The kernels only move bytes, so nothing here has a tolerance: scores, row ids and score arrays are compared with np.array_equal.
The fresh index numbers its track slots densely by first appearance among the survivors, the compacted one keeps its old slots
(some of them empty now): the answers must not depend on that.

The world is the one of test_gpu_index_tracks.py, rebuilt here (40 000 x 256, 8 groups, one dominant track of 6 000 rows, 300
ordinary tracks, 5 % slot-less rows, 20 % exact duplicates of earlier rows so that ties decide, a slot-less tail), in f32 and bf16
storage.  cc_dev_set("index_slab_rows", 4096) makes the index span ten slabs with a ragged last one (a slab is bounced until
1 024 rows are gone before it, then slabs are moved directly); one more pattern runs at the default slab size with dim 768."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, N_GROUPS, DOMINANT, PLAIN_TAIL, SLAB = 40000, 256, 8, 6000, 1500, 4096
EXTRA = N + 3000                                                   # rows kept ready for the appends after a removal
STORAGES = ("f32", "bf16")


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


class World:
    def __init__(self):
        rng = np.random.default_rng(31)
        u = unit(rng.standard_normal(DIM))
        total = N + EXTRA
        E = unit(rng.standard_normal((total, DIM), dtype=np.float32))
        slot = rng.integers(1, 301, total).astype(np.int32)
        slot[rng.random(total) < 0.05] = -1
        dom = rng.choice(N - PLAIN_TAIL, DOMINANT, replace=False)
        slot[dom] = 0
        E[dom] = unit(u + 0.02 * rng.standard_normal((DOMINANT, DIM)))        # cosine ~0.95 with u: above every other row
        dup = np.flatnonzero(rng.random(total) < 0.20); dup = dup[dup > 0]
        for r in dup:                                                         # copies of EARLIER rows, whatever their track
            E[r] = E[rng.integers(0, r)]
        E[dom[1]] = E[dom[2]] = E[dom[0]]                                     # ties inside the dominant track, for certain
        slot[N - PLAIN_TAIL:N] = -1                                           # the slot-less tail
        slot[N:][rng.random(EXTRA) < 0.3] += 300                              # the appended rows also bring tracks of their own
        self.E, self.slot, self.dom = E, slot, dom
        self.group = rng.integers(0, N_GROUPS, total).astype(np.int32)
        self.q = unit(u + 0.03 * rng.standard_normal((3, DIM)))
        self.allowed = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
        self.rng = rng

    def patterns(self):
        rng = np.random.default_rng(32)
        rows = np.arange(N)
        return {"nothing": np.zeros(N, bool), "everything": np.ones(N, bool), "row 0": rows == 0, "the last row": rows == N - 1,
                "one group": self.group[:N] == 3, "run 4095..8193": (rows >= SLAB - 1) & (rows <= 2 * SLAB + 1),
                "every other row": rows % 2 == 0, "random 90 %": rng.random(N) < 0.9}


@pytest.fixture(scope="module")
def world():
    return World()


@contextlib.contextmanager
def slab_rows(value):
    from clearcam_amd import _lib
    _lib.check(_lib.lib().cc_dev_set(b"index_slab_rows", value))
    try:
        yield
    finally:
        _lib.check(_lib.lib().cc_dev_set(b"index_slab_rows", -1))


def dense(slot):
    """Track slots renumbered by first appearance: what a caller that only ever saw the survivors would hand to add()."""
    out = np.full(len(slot), -1, np.int32)
    seen = {}
    for i, s in enumerate(slot.tolist()):
        if s >= 0:
            out[i] = seen.setdefault(s, len(seen))
    return out


def fresh(E, group, slot, storage, dim=DIM):
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(dim, max(len(E), 1), storage=storage)
    if len(E):
        ix.add(E, group, dense(slot))
    return ix


def assert_same_answers(ix, ref, q, allowed, what):
    assert len(ix) == len(ref), what
    assert np.array_equal(ix.scores(q), ref.scores(q)), what
    for Q in (1, 3):
        for al in (None, allowed):
            a, b = ix.search(q[:Q], 100, al), ref.search(q[:Q], 100, al)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, "search", Q, al is not None)
    for k in (1, 10, 1024):
        for al in (None, allowed):
            a, b = ix.search_tracks(q, k, al), ref.search_tracks(q, k, al)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (what, "search_tracks", k, al is not None)


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("pattern", ["nothing", "everything", "row 0", "the last row", "one group", "run 4095..8193", "every other row",
                                     "random 90 %"])
def test_removal_equals_an_index_built_from_the_survivors(world, storage, pattern):
    from clearcam_amd.objects import EmbeddingIndex
    w = world
    drop = w.patterns()[pattern]
    with slab_rows(SLAB):
        ix = EmbeddingIndex(DIM, N, storage=storage)
        ix.add(w.E[:N], w.group[:N], w.slot[:N])
        cap = ix.capacity
        assert ix.remove(drop) == int(drop.sum())
        live = np.flatnonzero(~drop)
        assert len(ix) == len(live) and ix.capacity == cap
        ref = fresh(w.E[live], w.group[live], w.slot[live], storage)
        assert_same_answers(ix, ref, w.q, w.allowed, pattern)
        ref.close()
        # growth after compaction: the appends run 3 000 rows past the old capacity
        more = np.arange(N, N + cap - len(live) + 3000)
        ix.add(w.E[more], w.group[more], w.slot[more])
        live = np.concatenate([live, more])
        assert len(ix) == cap + 3000 and ix.capacity > cap
        ref = fresh(w.E[live], w.group[live], w.slot[live], storage)
        assert_same_answers(ix, ref, w.q, w.allowed, pattern + ", grown")
        ref.close()
        # a second removal on the same handle: every third row, and a run across the seam between old and appended rows
        pos = np.arange(len(live))
        drop2 = (pos % 3 == 1) | ((pos >= cap - 700) & (pos < cap + 700))
        cap2 = ix.capacity
        assert ix.remove(drop2) == int(drop2.sum())
        live = live[~drop2]
        assert ix.capacity == cap2
        ref = fresh(w.E[live], w.group[live], w.slot[live], storage)
        assert_same_answers(ix, ref, w.q, w.allowed, pattern + ", second removal")
        ref.close(); ix.close()


@pytest.mark.parametrize("storage", STORAGES)
def test_default_slab_size_dim_768(storage):
    """The default slab size on 768-d rows (three 16-byte pieces per lane and row), half of the rows dropped at random: the head
    of the matrix goes through the bounce buffer, the rest is moved directly."""
    from clearcam_amd.objects import EmbeddingIndex
    rng = np.random.default_rng(33)
    n, dim = 50001, 768
    E = unit(rng.standard_normal((n, dim), dtype=np.float32))
    E[rng.integers(1, n, 4000)] = E[0]                                        # ties
    group = rng.integers(0, N_GROUPS, n).astype(np.int32)
    slot = rng.integers(-1, 200, n).astype(np.int32)
    q = unit(E[:3] + 0.1 * rng.standard_normal((3, dim)))
    drop = rng.random(n) < 0.5
    ix = EmbeddingIndex(dim, n, storage=storage)
    ix.add(E, group, slot)
    assert ix.remove(drop) == int(drop.sum())
    ref = fresh(E[~drop], group[~drop], slot[~drop], storage, dim)
    assert_same_answers(ix, ref, q, np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8), "default slab")


def test_a_mask_of_the_wrong_length_is_refused_and_changes_nothing(world):
    from clearcam_amd._lib import CCError
    w = world
    n = 9000
    with slab_rows(SLAB):
        ix = fresh(w.E[:n], w.group[:n], w.slot[:n], "f32")
        ref = fresh(w.E[:n], w.group[:n], w.slot[:n], "f32")
        for bad in (np.ones(n - 1, bool), np.ones(n + 1, np.uint8), np.ones(0, bool)):
            with pytest.raises(CCError):
                ix.remove(bad)
            assert len(ix) == n
        with pytest.raises(IndexError):
            ix.remove(np.array([0, n]))
        assert_same_answers(ix, ref, w.q, w.allowed, "after refused masks")


def test_empty_index_and_empty_masks(world):
    from clearcam_amd.objects import EmbeddingIndex
    ix = EmbeddingIndex(DIM, 16)
    assert ix.remove(np.zeros(0, bool)) == 0 and ix.remove(np.zeros(0, np.int64)) == 0
    assert ix.remove_groups(np.ones(4, np.uint8)) == 0 and len(ix) == 0
    ix.add(world.E[:10], world.group[:10])
    assert ix.remove(np.zeros(10, bool)) == 0 and ix.remove_groups(np.zeros(N_GROUPS, np.uint8)) == 0 and len(ix) == 10
    assert ix.remove(np.ones(10, bool)) == 10 and len(ix) == 0
    assert ix.scores(world.q).shape == (3, 0)
    ix.add(world.E[:10], world.group[:10])                                      # and it takes rows again
    assert np.array_equal(ix.scores(world.q), fresh(world.E[:10], world.group[:10], np.full(10, -1), "f32").scores(world.q))


@pytest.mark.parametrize("storage", STORAGES)
def test_row_numbers_and_group_tables_equal_the_mask(world, storage):
    w = world
    n = 3 * SLAB + 77
    E, group, slot = w.E[:n], w.group[:n], w.slot[:n]
    mask = np.random.default_rng(34).random(n) < 0.3
    with slab_rows(SLAB):
        a, b = fresh(E, group, slot, storage), fresh(E, group, slot, storage)
        assert a.remove(mask) == b.remove(np.flatnonzero(mask)[::-1]) == int(mask.sum())      # row numbers in any order
        assert_same_answers(b, a, w.q, w.allowed, "row numbers")
        # a group table: the flags come from the group ids on the device.  The bitmap is shorter than the group count: groups 3.. stay
        c, d = fresh(E, group, slot, storage), fresh(E, group, slot, storage)
        table = np.array([0, 1, 1], np.uint8)
        gm = (group == 1) | (group == 2)
        assert c.remove_groups(table) == d.remove(gm) == int(gm.sum())
        assert_same_answers(c, d, w.q, w.allowed, "group table")
        assert_same_answers(c, fresh(E[~gm], group[~gm], slot[~gm], storage), w.q, w.allowed, "group table against the survivors")
        long_table = np.zeros(64, np.uint8); long_table[[5, 40]] = 1                          # longer than the ids in use
        g5 = group[~gm] == 5
        assert c.remove_groups(long_table) == int(g5.sum()) and len(c) == int((~gm).sum() - g5.sum())
