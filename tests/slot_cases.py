"""Track slots past the reduction's table: the seeded world, the race's two extremes and three wrong reductions, for
tests/test_slot_cases_host.py (where the world is shown to tell a wrong reduction from the right one) and
tests/test_gpu_index_slots.py (where the device is held to the unchanged models on that world).

track_reduce_kernel reduces each block of BLOCK contiguous rows in a table of TABLE entries keyed by slot & (TABLE - 1) and tagged
with the slot.  The first competing row to reach an entry makes its slot the entry's owner; a row of another slot in the same entry (a
collider) goes to global memory on its own, and the table is flushed to the owners' slots at the end of the block.  With fewer than
TABLE slots no entry ever has two slots.  This world has them everywhere.

Which row reaches an entry first is a race, so `owners` models both extremes: the owner of a (block, bucket) is the slot of its lowest
competing row ("low") or of its highest ("high").  The wrong reductions are transforms of (slot, group, allowed) in front of the
unchanged `rank_cases.full_order`, as `where_cases.disguise` is for a row filter."""
import numpy as np

import near_cases
import terms_cases
from like_cases import dead_rows, fold
from rank_cases import allowed_rows, full_order, run_bounds, window
from where_cases import DIM, FILTERS, GROUPS, NO_TS, Rows, disguise, passing  # noqa: F401

BLOCK, TABLE = 2048, 1024                                        # kTrkRows, kTrkTab
N = 3 * BLOCK + 137                                              # three full blocks and a ragged fourth
SEED = 5
MULTS = (0, 1, 2, 3, 5, 8, 37, 100, 511, 1023, 2047)             # slot = residue + TABLE * one of these
ONE_BUCKET = 7                                                   # block 1: row i has slot 7 + TABLE * i, 2048 slots in one entry
SPAN_ALL = ONE_BUCKET + TABLE * 37                               # planted in blocks 0, 2 and 3; block 1 has it at row 37
QRES, QGROUP = 5, 1
QSLOT, MATE = QRES + TABLE * 5, QRES + TABLE                     # the query track's slot (5125) and a bucket mate (1029) beside it
PAIR_RES = 600                                                   # a bucket that only these two slots use, in blocks 0, 2 and 3
PAIR_A, PAIR_B = PAIR_RES + TABLE, PAIR_RES + TABLE * 100
SLOT_CAP = 1 << 21
PICKS = ("low", "high")
WRONG = ("flushed by bucket", "merged into the owner", "colliders dropped")


class World(Rows):
    """where_cases.Rows (E with a fifth of the rows copied, q, group, ts, cls) at N rows, with its own slots: families
    residue + TABLE * m over 36 residues, about 5 % slot-less rows, block 1 in one bucket with a slot per row (7 + TABLE * i, so that
    the 2048 slots stay below SLOT_CAP), and the planted slots named above.  Rows' eight triples of equal rows stay slot-less outside
    block 1."""

    def __init__(self, seed=SEED, queries=20):
        super().__init__(n=N, seed=seed, queries=queries)
        rng = np.random.default_rng(1000 + seed)
        n = self.n
        free = np.array([c for c in range(TABLE) if c not in (ONE_BUCKET, QRES, PAIR_RES)])
        self.residues = np.r_[rng.choice(free, 34, replace=False), ONE_BUCKET, QRES]
        slot = rng.choice(self.residues, n) + TABLE * rng.choice(np.array(MULTS), n)
        slot[rng.random(n) < 0.075] = -1
        tied = 11 + np.arange(24) * (n // 24)                    # as Rows placed them
        slot[tied] = -1
        slot[BLOCK:2 * BLOCK] = ONE_BUCKET + TABLE * np.arange(BLOCK)
        group = self.group
        planted = []

        def plant(block, offsets, s, g=None):
            rows = block * BLOCK + np.asarray(offsets)
            assert rows.max() < n and not np.isin(rows, tied).any() and not np.isin(rows, planted).any()
            planted.extend(rows.tolist())
            slot[rows] = s
            if g is not None:
                group[rows] = g

        for b in (0, 2, 3):
            plant(b, (1, 30, 31, 64, 65, 100, 101, 102, 120, 121, 125, 126), QSLOT, QGROUP)       # the query track
            plant(b, (2, 40, 90, 124), MATE, QGROUP)                                             # its bucket mate, same group, same blocks
            plant(b, (50, 110), QSLOT, (QGROUP + 1) % GROUPS)                                    # the slot goes on answering with the track dead
            plant(b, (3, 70, 128), SPAN_ALL)
        plant(0, (20, 2040), PAIR_A); plant(0, (500, 900), PAIR_B)                               # A owns block 0 and block 3 under both picks,
        plant(2, (20, 2040), PAIR_B); plant(2, (500, 900), PAIR_A)                               # B block 2: each collides where the other owns
        plant(3, (6, 130), PAIR_A); plant(3, (60,), PAIR_B)
        self.slot = slot.astype(np.int32)
        self.qslot, self.qgroup = QSLOT, QGROUP
        self.track = np.flatnonzero((self.slot == QSLOT) & (self.group == QGROUP))

    def query_rows(self, k):
        """k rows of the query track, spread over it, in ascending order (like_cases.World.query_rows)"""
        return self.track[np.linspace(0, len(self.track) - 1, k).round().astype(int)]

    def cols(self):
        return self.slot, self.group, GROUPS, self.ts, self.cls

    def blocks_of(self, s):
        return np.unique(np.flatnonzero(self.slot == s) // BLOCK).tolist()


class HostIndex:
    """`scores` and `fetch` of an f32 index in numpy: q @ E.T in float32.  Copied rows score equally, so the ties survive."""

    def __init__(self, E):
        self.E = np.ascontiguousarray(E, dtype=np.float32)

    def scores(self, q):
        return (np.asarray(q, np.float32).reshape(-1, self.E.shape[1]) @ self.E.T).astype(np.float32)

    def fetch(self, rows):
        return self.E[np.asarray(rows, np.int64)]


# ---- the race's two extremes ----------------------------------------------------------------------------------------------------------
def competing(group, allowed):
    ok = np.zeros(len(group), bool)
    ok[allowed_rows(len(group), np.asarray(group), allowed)] = True
    return ok


def owners(slot, pick, ok=None):
    """Per row the slot that owns the row's (block, bucket), -1 for a row that takes no part (no slot, or not in `ok`).  The owner is
    the slot of the lowest ("low") or the highest ("high") row of the block that takes part and falls into the bucket."""
    assert pick in PICKS
    slot = np.asarray(slot, np.int64)
    n = len(slot)
    rows = np.flatnonzero(slot >= 0 if ok is None else (slot >= 0) & np.asarray(ok, bool))
    if pick == "high":
        rows = rows[::-1]
    key = (rows // BLOCK) * TABLE + (slot[rows] & (TABLE - 1))
    _, lead = np.unique(key, return_index=True)                  # the first occurrence of every key
    own = np.full((n // BLOCK + 1) * TABLE, -1, np.int64)
    own[key[lead]] = slot[rows[lead]]
    out = np.full(n, -1, np.int64)
    out[rows] = own[key]
    return out


def colliders(slot, pick, ok=None):
    """Bool per row: the row meets an entry owned by another slot and goes to global memory on its own"""
    own = owners(slot, pick, ok)
    return (own >= 0) & (own != np.asarray(slot, np.int64))


# ---- three wrong reductions -----------------------------------------------------------------------------------------------------------
def wrong_reduction(kind, slot, group, allowed, pick):
    """(slot, group, allowed) as the right model takes them -> the same for a wrong kernel.  Only competing rows reach the table.
    "flushed by bucket": the flush goes to best[i], not best[tag[i]] - owner rows are relabelled slot & (TABLE - 1).
    "merged into the owner": no tag compare - every row of a (block, bucket) takes the owner's slot.
    "colliders dropped": no else branch - collider rows move to a forbidden group."""
    assert kind in WRONG
    slot, group = np.asarray(slot, np.int64), np.asarray(group, np.int64)
    own = owners(slot, pick, competing(group, allowed))
    part, hit = own >= 0, (own >= 0) & (own != slot)
    if kind == "flushed by bucket":
        return np.where(part & ~hit, slot & (TABLE - 1), slot), group, allowed
    if kind == "merged into the owner":
        return np.where(part, own, slot), group, allowed
    G = int(group.max()) + 1 if allowed is None else len(allowed)
    al = np.ones(G, np.uint8) if allowed is None else np.asarray(allowed, np.uint8)
    return slot, np.where(hit, G, group), np.r_[al, np.uint8(0)]


# ---- what a call sees: one (v, group, allowed, cut) per query, and the view it compares -----------------------------------------------
def bins_of(rows, ts, t0, bin_seconds, n_bins):
    """where_cases.timeline_model's counting of one full order -> (counts (n_bins,), total)"""
    t = np.asarray(ts, np.int64)[rows]
    b = (t - int(t0)) // int(bin_seconds)
    b = b[(t != NO_TS) & (b >= 0) & (b < n_bins)]
    return np.bincount(b, minlength=n_bins).astype(np.int64), len(rows)


def answer(v, slot, group, allowed, cut, view, ts):
    """One question's answer in the compared view: ("window", start, count) -> (idx, score, total); ("bins", t0, bin_seconds, n_bins)
    -> (counts, total)"""
    rows, s = full_order(v, slot, group, allowed, True, cut)
    if view[0] == "window":
        return window(rows, s, view[1], view[2])
    return bins_of(rows, ts, *view[1:])


def differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def told_apart(slot, ts, v, group, allowed, cut, view):
    """{(kind, pick): the wrong reduction's answer differs from the right one's in the compared view}"""
    right = answer(v, slot, group, allowed, cut, view, ts)
    return {(kind, pick): differs(answer(v, *wrong_reduction(kind, slot, group, allowed, pick), cut, view, ts), right)
            for kind in WRONG for pick in PICKS}


def first_row_filter(w):
    """A group bitmap that removes the first row of a track whose first row is a collider under both picks (the lowest such row)"""
    hit = colliders(w.slot, "low") & colliders(w.slot, "high")
    first = np.full(int(w.slot.max()) + 1, w.n, np.int64)
    rows = np.flatnonzero(w.slot >= 0)
    np.minimum.at(first, w.slot[rows], rows)
    r = int(min(f for f in first[first < w.n] if hit[f] and (w.slot == w.slot[f]).sum() > 1))
    al = np.ones(GROUPS, np.uint8); al[w.group[r]] = 0
    return al, r


def search_filters(w):
    return {"none": None, "without a colliding track's first row": first_row_filter(w)[0], "nothing": np.zeros(GROUPS, np.uint8)}


def filter_parts(name):
    return FILTERS[name] if name else (None, None, None)


def where_groups(w, name, dead=None):
    """-> (group, allowed) of where_cases.disguise for a FILTERS entry (None: no filter) and a dead-row mask"""
    ts_range, classes, allowed = filter_parts(name)
    ok = passing(w.ts, w.cls, ts_range, classes)
    if dead is not None:
        ok &= ~dead
    if name is None and dead is None:
        return w.group, None
    return disguise(w.group, GROUPS, ok, allowed)


def tied_start(s, lo=0):
    """A position inside a run of equal scores of a descending list, at or past `lo` (its second element)"""
    runs = [r for r in run_bounds(s) if r[0] >= lo]
    assert runs, "no equal scores among the answers"
    return runs[len(runs) // 2][0] + 1


def tied_cut(s):
    runs = run_bounds(s)
    assert runs, "no equal scores among the answers"
    return float(s[runs[len(runs) // 2][0]])


def rank_windows(s):
    """The windows of the grouped ranking, from the score list of query 0's full order -> [(start, count, cut)]: the first 1024; a start
    inside the order; a start past 1024; a window that begins inside a run of equal scores; a cut equal to a tied score, seen at its
    edge (the whole run stays, nothing below it)."""
    cut = tied_cut(s)
    left = int((s >= np.float32(cut)).sum())
    return [(0, 1024, None), (300, 200, None), (1100, 300, None), (tied_start(s), 100, None), (max(left - 60, 0), 80, cut)]


RANK_Q = 3
TIMELINE_BINS = (-50, 19, 24)                                    # where_cases' BINS[1]: every ts of the world in 24 bins
LIKE_ROWS, LIKE_WINDOWS = 9, ((0, 1024), (1030, 200))
TERMS = dict(roles=["rank", "require", "rank", "rank", "reject"], n_vec=2, n_rows=3, combine="sum", weights=[1.0, 1.0, -0.4, 0.8, 1.0],
             exclude="track", window=(0, 1024))
NEAR = dict(within=7, partners=3000, value="min", window=(0, 1024), bins=(-50, 30, 15))


def like_question(w, ix):
    """-> (rows, S, v, group, allowed) of rank_like(rows = nine crops of the query track, exclude="track")"""
    rows = w.query_rows(LIKE_ROWS)
    S = ix.scores(ix.fetch(rows))
    g, al = where_groups(w, None, dead_rows(w.n, rows, w.group, w.slot, "track"))
    return rows, S, fold(S), g, al


def terms_question(w, ix):
    """-> (ask, v, dead, which, group, allowed): the keyword arguments of rank_terms / timeline_terms and the fold behind them"""
    q, rows = w.q[4:4 + TERMS["n_vec"]], w.query_rows(TERMS["n_rows"]).astype(np.int64)
    S = ix.scores(np.vstack([q, ix.fetch(rows)]))
    cuts = terms_cases.median_cuts(S, TERMS["roles"], np.arange(w.n))
    v, dead, which = terms_cases.terms_fold(S, TERMS["roles"], TERMS["weights"], cuts, TERMS["combine"], rows, TERMS["n_vec"], w.group, w.slot, TERMS["exclude"])
    ask = dict(q=q, rows=rows, roles=TERMS["roles"], weights=TERMS["weights"], cuts=cuts, combine=TERMS["combine"], exclude=TERMS["exclude"])
    return ask, v, dead, which, *where_groups(w, None, dead)


def near_question(w, ix):
    """-> (ask, Sa, Sb, v, dead, group, allowed) of rank_near / timeline_near(a = q[0], b = q[1])"""
    S = ix.scores(w.q[:2])
    plist, _ = near_cases.partner_list(S[1], w.group, GROUPS, w.ts, w.cls, NEAR["partners"])
    v, dead, _ = near_cases.near_fold(S[0], S[1], plist, w.group, w.slot, w.ts, NEAR["within"], NEAR["value"])
    ask = dict(a=w.q[0], b=w.q[1], within=NEAR["within"], partners=NEAR["partners"], value=NEAR["value"])
    return ask, S[0], S[1], v, dead, *where_groups(w, None, dead)


def filtered_windows(s):
    """The windows of a ranking behind a FILTERS entry, from the score list of query 0's full order -> [(start, count, cut)]: the first
    1024, the end of the order, and the first 1024 above a cut equal to a tied score"""
    return [(0, 1024, None), (max(len(s) - 40, 0), 100, None), (0, 1024, tied_cut(s))]


def rankings(w, ix):
    """Every grouped ranking tests/test_gpu_index_slots.py asks of the main world, as the reduction sees it ->
    [(name, [(v, group, allowed, cut)] one per query, view)].  `ix` gives the scores: a HostIndex here, the device's own there."""
    out = []
    sc = ix.scores(w.q)
    for fname, allowed in search_filters(w).items():
        if fname == "nothing":
            continue                                             # no row competes: nothing for a reduction to get wrong
        for Q in (1, 3, 20):
            for k in (100, 1024):
                out.append((("search_tracks", fname, Q, k), [(sc[i], w.group, allowed, None) for i in range(Q)], ("window", 0, k)))
    for name in (None,) + tuple(FILTERS):
        g, al = where_groups(w, name)
        _, s = full_order(sc[0], w.slot, g, al, True, None)
        windows = rank_windows(s) if name is None else filtered_windows(s)
        for start, count, cut in windows:
            out.append((("rank", name, start, count, cut), [(sc[i], g, al, cut) for i in range(RANK_Q)], ("window", start, count)))
        for cut in (None,) if name is None else (None, tied_cut(s)):
            out.append((("timeline", name, cut), [(sc[i], g, al, cut) for i in range(RANK_Q)], ("bins",) + TIMELINE_BINS))
    _, S, v, g, al = like_question(w, ix)
    for start, count in LIKE_WINDOWS:
        out.append((("rank_like", start, count), [(v, g, al, None)], ("window", start, count)))
    out.append((("rank_like", "nothing excluded"), [(fold(S), w.group, None, None)], ("window", 0, 1024)))
    _, v, _, _, g, al = terms_question(w, ix)
    out.append((("rank_terms",), [(v, g, al, None)], ("window",) + TERMS["window"]))
    out.append((("timeline_terms",), [(v, g, al, None)], ("bins",) + TIMELINE_BINS))
    _, _, _, v, _, g, al = near_question(w, ix)
    out.append((("rank_near",), [(v, g, al, None)], ("window",) + NEAR["window"]))
    out.append((("timeline_near",), [(v, g, al, None)], ("bins",) + NEAR["bins"]))
    return out


def plain_rankings(tag, sc, group, ks, windows):
    """search_tracks at every k and rank at every window of a (Q, n) score matrix, without a filter, in the form of `rankings`"""
    qs = [(v, group, None, None) for v in sc]
    return ([((tag, "search_tracks", k), qs, ("window", 0, k)) for k in ks] +
            [((tag, "rank", start, count), qs, ("window", start, count)) for start, count in windows])


# ---- removal --------------------------------------------------------------------------------------------------------------------------
GONE_GROUP, GONE_MULT = GROUPS, 3                                # a sixth group that holds every row of the slots c + TABLE * 3
REMOVAL_Q, REMOVAL_KS, REMOVAL_WINDOWS = 3, (100, 1024), ((0, 1024), (1100, 300))
PLANTED = (QSLOT, MATE, SPAN_ALL, PAIR_A, PAIR_B)


def removal_groups(w):
    """The world's groups with every row of the slots c + TABLE * 3 (some forty slots, each with bucket mates that stay) in
    GONE_GROUP, for remove_groups to take"""
    g = w.group.copy()
    g[(w.slot >= 0) & (w.slot // TABLE == GONE_MULT)] = GONE_GROUP
    return g


def best_rows(v, slot, slots):
    """The best row (equal scores: the lowest) of each of `slots` under one score vector"""
    rows, _ = full_order(v, slot, np.zeros(len(slot), np.int64), None, True, None)
    rows = rows[slot[rows] >= 0]
    return np.sort(rows[np.isin(slot[rows], slots)])


def leading_slots(v, slot, m):
    """The slots of the m best tracks under one score vector"""
    rows, _ = full_order(v, slot, np.zeros(len(slot), np.int64), None, True, None)
    return slot[rows[slot[rows] >= 0][:m]]


def filter_losses(w, v, name):
    """How many tracks that still answer behind FILTERS[name] lost to it the row that placed them, and how many their best row under
    the score vector v - counting only lost rows that are colliders under both picks -> (lost_first, lost_best)"""
    ts_range, classes, allowed = FILTERS[name]
    ok = passing(w.ts, w.cls, ts_range, classes)
    if allowed is not None:
        ok &= np.asarray(allowed)[w.group] != 0
    hit = colliders(w.slot, "low") & colliders(w.slot, "high")
    rows = np.flatnonzero(w.slot >= 0)
    T = int(w.slot.max()) + 1
    first, alive = np.full(T, w.n, np.int64), np.zeros(T, bool)
    np.minimum.at(first, w.slot[rows], rows)
    alive[w.slot[rows[ok[rows]]]] = True
    best = best_rows(v, w.slot, np.flatnonzero(alive))
    first = first[np.flatnonzero(alive)]
    return int((~ok[first] & hit[first]).sum()), int((~ok[best] & hit[best]).sum())


def second_removal(v, slot):
    """The rows remove(rows) takes after remove_groups, from query 0's scores of the surviving rows: the best rows of the planted slots
    and of the fifty leading tracks"""
    return best_rows(v, slot, np.r_[np.array(PLANTED), leading_slots(v, slot, 50)])


# ---- the smaller worlds ---------------------------------------------------------------------------------------------------------------
TOP_KS, TOP_WINDOWS = (100,), ((0, 100), (3, 50))
GROWTH_KS, GROWTH_WINDOWS, GROWTH_Q = (100, 1024), ((0, 1024), (1030, 100)), (3, 8)
TOP_SLOT = (1 << 24) - 1


class TopWorld:
    """The top of the slot range: 300 rows of DIM whose slots are 5, 1029 and 2^24 - 1 - TABLE * j (j = 0 .. 3 and 16383, which is
    1023), so T = 2^24.  5 and 1029 share bucket 5, the others bucket 1023; the first and the last row of either bucket belong to
    a slot past TABLE, so that an owner flushed by bucket lands on a slot that has rows of its own.  A tenth of the rows slot-less, a
    fifth copied."""

    def __init__(self, seed=SEED):
        base = Rows(n=300, seed=seed, queries=1)
        rng = np.random.default_rng(2000 + seed)
        self.n, self.E, self.q, self.group = 300, base.E, base.q, base.group
        slots = np.array([5, 1029] + [TOP_SLOT - TABLE * j for j in (0, 1, 2, 3, 16383)])
        slot = rng.choice(slots, self.n)
        slot[rng.random(self.n) < 0.1] = -1
        slot[:7] = slots[::-1]                                   # every slot present
        slot[:2] = (TOP_SLOT, 1029)
        slot[-2:] = (TOP_SLOT - TABLE, 1029)
        self.slot = slot.astype(np.int32)
        self.ts = np.full(self.n, NO_TS, np.int32)


class GrowthWorld:
    """Two rounds of 3000 rows: slots below 300 first, then slots c + TABLE * m that reach past TABLE and share buckets with the old
    ones (c below 300, m from 0 to 3, so the old slots keep gaining rows too)."""

    def __init__(self, seed=SEED):
        base = Rows(n=6000, seed=seed, queries=8)
        rng = np.random.default_rng(3000 + seed)
        self.n, self.E, self.q, self.group = 6000, base.E, base.q, base.group
        slot = rng.integers(0, 300, 6000)
        slot[3000:] += TABLE * rng.integers(0, 4, 3000)
        slot[rng.random(6000) < 0.05] = -1
        self.slot = slot.astype(np.int32)
        self.ts = np.full(self.n, NO_TS, np.int32)
