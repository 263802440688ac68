"""The world of tests/slot_cases.py on the CPU: it has the collisions tests/test_gpu_index_slots.py needs, and every ranking that file
asks for tells each of three wrong track reductions, under both extremes of the race for a table entry, from the right one.  Scores
are q @ E.T in float32; the ties come from copied rows, so they survive.

Without this file the GPU file could pass for the reason every earlier track test passes: no two slots in one table entry."""
import numpy as np
import pytest

import near_cases
import slot_cases as S
import terms_cases
from like_cases import like_model
from rank_cases import full_order, rank_model, window
from where_cases import FILTERS, Rows, rank_where_model, timeline_model


@pytest.fixture(scope="module")
def world():
    return S.World()


@pytest.fixture(scope="module")
def host(world):
    return S.HostIndex(world.E)


def per_block(mask):
    return [int(mask[b * S.BLOCK:(b + 1) * S.BLOCK].sum()) for b in range(4)]


def test_the_shape_and_the_slot_range(world):
    w = world
    assert w.n == 3 * 2048 + 137 and w.E.shape == (w.n, 256) and w.slot.dtype == np.int32
    assert 1 << 20 < w.slot.max() < S.SLOT_CAP                          # T about 2 M: best[] costs 16 MB a query
    assert 0.04 < (w.slot < 0).mean() < 0.06
    assert len(np.unique(w.slot[w.slot >= 0])) > 2300                   # deep pages exist
    m = np.unique(w.slot[w.slot >= 0] // S.TABLE)
    assert set(S.MULTS) <= set(m.tolist())
    fam = w.slot[np.r_[0:S.BLOCK, 2 * S.BLOCK:w.n]]
    assert 30 <= len(np.unique(fam[fam >= 0] & (S.TABLE - 1))) <= 48     # a few dozen residues
    b = w.E.view(np.uint32)
    _, inv, cnt = np.unique(b, axis=0, return_inverse=True, return_counts=True)
    copied = np.flatnonzero(cnt[inv.reshape(-1)] > 1)
    assert len(copied) > 0.25 * w.n                                     # a fifth of the rows copy another
    mates = {}
    for r in copied:                                                    # equal rows that sit in one (block, bucket) under two slots
        if w.slot[r] >= 0:
            mates.setdefault((b[r].tobytes(), r // S.BLOCK, w.slot[r] & (S.TABLE - 1)), set()).add(int(w.slot[r]))
    assert sum(len(v) > 1 for v in mates.values()) >= 10                # exact ties cross bucket mates


def test_colliders_in_every_block(world):
    for pick in S.PICKS:
        hit = per_block(S.colliders(world.slot, pick))
        assert min(hit[:3]) >= 1024, (pick, hit)
        assert hit[1] >= 2000 and hit[3] > 40, (pick, hit)


def test_block_1_is_one_bucket_with_a_slot_per_row(world):
    s = world.slot[S.BLOCK:2 * S.BLOCK]
    assert (s & (S.TABLE - 1) == S.ONE_BUCKET).all() and len(np.unique(s)) == S.BLOCK and s.min() >= 0
    for pick in S.PICKS:
        assert per_block(S.colliders(world.slot, pick))[1] == S.BLOCK - 1    # every row but the owner's takes the global path


def test_spanning_slots(world):
    w = world
    assert w.blocks_of(S.SPAN_ALL) == [0, 1, 2, 3]
    assert S.PAIR_A & (S.TABLE - 1) == S.PAIR_B & (S.TABLE - 1) == S.PAIR_RES
    assert w.blocks_of(S.PAIR_A) == w.blocks_of(S.PAIR_B) == [0, 2, 3]
    assert set(np.unique(w.slot[(w.slot >= 0) & (w.slot & (S.TABLE - 1) == S.PAIR_RES)]).tolist()) == {S.PAIR_A, S.PAIR_B}
    for pick in S.PICKS:                                                # each owns one block and collides in another, whoever wins
        own = S.owners(w.slot, pick)
        for s in (S.PAIR_A, S.PAIR_B):
            rows = np.flatnonzero(w.slot == s)
            mine = {int(r // S.BLOCK) for r in rows[own[rows] == s]}
            assert mine and mine != {0, 2, 3}, (pick, s, mine)


def test_the_query_track_has_a_bucket_mate_beside_it(world):
    w = world
    assert w.qslot >= S.TABLE and S.MATE >= S.TABLE and S.MATE != w.qslot and S.MATE & (S.TABLE - 1) == w.qslot & (S.TABLE - 1)
    assert len(w.track) >= 36 and (w.slot[w.track] == w.qslot).all() and (w.group[w.track] == w.qgroup).all()
    mate = np.flatnonzero((w.slot == S.MATE) & (w.group == w.qgroup))
    assert np.unique(w.track // S.BLOCK).tolist() == np.unique(mate // S.BLOCK).tolist() == [0, 2, 3]
    assert np.flatnonzero(w.slot == w.qslot)[0] == w.track[0]           # excluding the track kills the row that places the slot
    assert ((w.slot == w.qslot) & (w.group != w.qgroup)).any()          # and the slot goes on answering from other groups
    rows = w.query_rows(S.LIKE_ROWS)
    assert len(set(rows.tolist())) == S.LIKE_ROWS and np.isin(rows, w.track).all()


def test_the_first_row_filter_removes_a_colliding_track_s_first_row(world):
    w = world
    al, r = S.first_row_filter(w)
    rows = np.flatnonzero(w.slot == w.slot[r])
    assert rows[0] == r and al[w.group[r]] == 0 and S.colliders(w.slot, "low")[r] and S.colliders(w.slot, "high")[r]
    assert (al[w.group[rows]] != 0).any()                               # the track goes on answering, placed by a later row


def test_every_ranking_tells_every_wrong_reduction_from_the_right_one(world, host):
    asked = S.rankings(world, host)
    names = [a[0] for a in asked]
    assert len(set(names)) == len(names)
    for entry in ("search_tracks", "rank", "timeline", "rank_like", "rank_terms", "timeline_terms", "rank_near", "timeline_near"):
        assert any(n[0] == entry for n in names), entry
    for name, questions, view in asked:
        for i, (v, g, al, cut) in enumerate(questions):
            told = S.told_apart(world.slot, world.ts, v, g, al, cut, view)
            assert all(told.values()), (name, i, [k for k, x in told.items() if not x])


def test_a_world_without_collisions_tells_nothing_apart():
    """The check above can fail: where_cases.Rows has 40 slots, and there every wrong reduction is the right one"""
    w = Rows()
    sc = S.HostIndex(w.E).scores(w.q[:1])[0]
    for pick in S.PICKS:
        assert not S.colliders(w.slot, pick).any()
    told = S.told_apart(w.slot, w.ts, sc, w.group, None, None, ("window", 0, 1024))
    assert not any(told.values())


def test_the_reduced_questions_are_the_models_the_device_is_held_to(world, host):
    """`rankings` hands the reduction (v, group, allowed, cut) and a view; the GPU file calls the existing models.  The same thing."""
    w = world
    sc = host.scores(w.q[:S.RANK_Q])
    by_name = {a[0]: a for a in S.rankings(w, host)}

    def mine(name):
        _, questions, view = by_name[name]
        return [S.answer(v, w.slot, g, al, cut, view, w.ts) for v, g, al, cut in questions]

    for name in FILTERS:
        ts_range, classes, allowed = FILTERS[name]
        want = rank_where_model(sc, *w.cols(), 0, 1024, allowed, None, True, ts_range, classes)
        for i, got in enumerate(mine(("rank", name, 0, 1024, None))):
            assert np.array_equal(got[0], want[0][i]) and np.array_equal(got[1], want[1][i]) and got[2] == want[2][i]
        counts, total = timeline_model(sc, *w.cols(), *S.TIMELINE_BINS, allowed, None, True, ts_range, classes)
        for i, got in enumerate(mine(("timeline", name, None))):
            assert np.array_equal(got[0], counts[i]) and got[1] == total[i]
    rows, Sm, _, _, _ = S.like_question(w, host)
    for start, count in S.LIKE_WINDOWS:
        want = like_model(Sm, *w.cols(), rows, start, count, None, None, True, "track")
        got = mine(("rank_like", start, count))[0]
        assert np.array_equal(got[0], want[0][0]) and np.array_equal(got[1], want[1][0]) and got[2] == want[2][0]
    ask, v, dead, which, _, _ = S.terms_question(w, host)
    want = terms_cases.terms_model(v, dead, which, *w.cols(), *S.TERMS["window"])
    got = mine(("rank_terms",))[0]
    assert np.array_equal(got[0], want[0][0]) and got[2] == want[2][0] and 40 < got[2] < w.n and dead.any()
    ask, Sa, Sb, v, dead, _, _ = S.near_question(w, host)
    want = near_cases.near_model(Sa, Sb, *w.cols(), S.NEAR["within"], *S.NEAR["window"], partners=S.NEAR["partners"], value=S.NEAR["value"])
    got = mine(("rank_near",))[0]
    assert np.array_equal(got[0], want[0][0]) and got[2] == want[2][0] and got[2] > 1024 and dead.any()
    counts, total, _ = near_cases.near_timeline_model(Sa, Sb, *w.cols(), S.NEAR["within"], *S.NEAR["bins"], partners=S.NEAR["partners"], value=S.NEAR["value"])
    got = mine(("timeline_near",))[0]
    assert np.array_equal(got[0], counts[0]) and got[1] == total[0]


def test_the_rank_windows_reach_every_edge(world, host):
    w = world
    sc = host.scores(w.q[:1])[0]
    rows, s = full_order(sc, w.slot, w.group, None, True, None)
    assert len(rows) > 2500
    wins = S.rank_windows(s)
    assert wins[0] == (0, 1024, None) and 0 < wins[1][0] < 1024 < wins[2][0] and wins[2][0] + wins[2][1] <= len(rows)
    start = wins[3][0]
    assert s[start - 1] == s[start]                                     # a window that begins inside a run of equal scores
    start, count, cut = wins[4]
    left = int((s >= np.float32(cut)).sum())
    assert (s == np.float32(cut)).sum() >= 2 and start < left < start + count and left < len(rows)    # the cut's edge is in the window


def test_a_filter_takes_a_track_s_first_row_and_another_track_s_best_row(world, host):
    """Rows that fail a row filter must neither answer nor set first[]: for every entry of FILTERS some track that still answers has
    lost the row that placed it, and some track its best row - both among colliders, so the global path is held to it too."""
    w = world
    sc = host.scores(w.q[:1])[0]
    for name in FILTERS:
        lost_first, lost_best = S.filter_losses(w, sc, name)
        assert lost_first >= 3 and lost_best >= 3, (name, lost_first, lost_best)


def test_removal_keeps_the_collisions(world, host):
    w = world
    g = S.removal_groups(w)
    gone = np.unique(w.slot[g == S.GONE_GROUP])
    assert len(gone) >= 30 and not np.isin(w.slot[g != S.GONE_GROUP], gone).any()       # the group holds every row of these slots
    assert all(((w.slot >= 0) & (w.slot & (S.TABLE - 1) == s & (S.TABLE - 1)) & (g != S.GONE_GROUP)).any() for s in gone)   # their mates stay
    keep = np.flatnonzero(g != S.GONE_GROUP)
    for round_ in range(2):
        slot, group = w.slot[keep], w.group[keep]
        sc = S.HostIndex(w.E[keep]).scores(w.q[:S.REMOVAL_Q])
        for name, questions, view in S.plain_rankings("removal", sc, group, S.REMOVAL_KS, S.REMOVAL_WINDOWS):
            for i, (v, gg, al, cut) in enumerate(questions):
                told = S.told_apart(slot, w.ts[keep], v, gg, al, cut, view)
                assert all(told.values()), (round_, name, i)
        if round_ == 0:
            rows = S.second_removal(sc[0], slot)
            assert len(rows) >= 50 and np.isin(np.array(S.PLANTED), slot[rows]).all()
            keep = np.delete(keep, rows)
            assert np.isin(np.array(S.PLANTED), w.slot[keep]).all()                     # the tracks go on, with their next best row


def test_growth_reaches_past_the_table_in_the_second_round():
    w = S.GrowthWorld()
    assert w.slot[:3000].max() < 300 and w.slot[3000:].max() >= 3 * S.TABLE
    for pick in S.PICKS:
        assert not S.colliders(w.slot[:3000], pick).any()
        hit = S.colliders(w.slot, pick)
        assert hit[3000:].sum() > 1000
        assert pick == "low" or hit[S.BLOCK:3000].sum() > 100                            # the block both rounds share: old rows collide too
    sc = S.HostIndex(w.E).scores(w.q[:S.GROWTH_Q[1]])
    for name, questions, view in S.plain_rankings("growth", sc, w.group, S.GROWTH_KS, S.GROWTH_WINDOWS):
        for i, (v, g, al, cut) in enumerate(questions):
            told = S.told_apart(w.slot, w.ts, v, g, al, cut, view)
            assert all(told.values()), (name, i, [k for k, x in told.items() if not x])


def test_the_top_of_the_slot_range():
    w = S.TopWorld()
    assert w.slot.max() == (1 << 24) - 1 and {5, 1029} <= set(w.slot.tolist()) and len(np.unique(w.slot[w.slot >= 0])) == 7
    assert len({int(s) & (S.TABLE - 1) for s in w.slot if s >= 0}) == 2
    sc = S.HostIndex(w.E).scores(w.q[:1])
    for name, questions, view in S.plain_rankings("top", sc, w.group, S.TOP_KS, S.TOP_WINDOWS):
        v, g, al, cut = questions[0]
        told = S.told_apart(w.slot, w.ts, v, g, al, cut, view)
        assert all(told.values()), (name, [k for k, x in told.items() if not x])


def test_the_models_of_the_wrong_reductions():
    """Two blocks by hand.  Block 0: slots 5, 1029, 5 in bucket 5.  Block 1: slot 1029 alone."""
    slot = np.full(S.BLOCK + 1, -1, np.int64)
    slot[[0, 1, 2, S.BLOCK]] = (5, 1029, 5, 1029)
    group = np.zeros(len(slot), np.int64)
    assert S.owners(slot, "low")[[0, 1, 2, S.BLOCK]].tolist() == [5, 5, 5, 1029]
    assert S.owners(slot, "high")[[0, 1, 2, S.BLOCK]].tolist() == [5, 5, 5, 1029]
    slot[3] = 1029
    assert S.owners(slot, "high")[[0, 1, 2, 3]].tolist() == [1029] * 4
    assert np.flatnonzero(S.colliders(slot, "low")).tolist() == [1, 3] and np.flatnonzero(S.colliders(slot, "high")).tolist() == [0, 2]
    s, g, al = S.wrong_reduction("flushed by bucket", slot, group, None, "high")
    assert s[[0, 1, 2, 3, S.BLOCK]].tolist() == [5, 5, 5, 5, 5] and al is None            # the owners, 1029, land on entry 5's own number
    s, g, al = S.wrong_reduction("merged into the owner", slot, group, None, "low")
    assert s[[0, 1, 2, 3, S.BLOCK]].tolist() == [5, 5, 5, 5, 1029]
    s, g, al = S.wrong_reduction("colliders dropped", slot, group, None, "low")
    assert np.array_equal(s, slot) and g[[0, 1, 2, 3, S.BLOCK]].tolist() == [0, 1, 0, 1, 0] and al.tolist() == [1, 0]
    allowed = np.array([0], np.uint8)                                   # nothing competes: nothing owns, nothing changes
    for kind in S.WRONG:
        s, g, al = S.wrong_reduction(kind, slot, group, allowed, "low")
        assert np.array_equal(s, slot) and (g == 0).all()
    v = np.linspace(1, 0, len(slot)).astype(np.float32)
    idx, _, total = rank_model(v[None], slot, group, 0, 2)
    assert idx[0].tolist() == [0, 1] and total[0] == 2 + (slot < 0).sum()
    idx, _, total = rank_model(v[None], *S.wrong_reduction("merged into the owner", slot, group, None, "low")[:2], 0, 2)
    assert idx[0].tolist() == [0, 4] and total[0] == 2 + (slot < 0).sum()                 # row 1 answers no more: slot 5 took it in
