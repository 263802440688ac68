"""The contract of cc_index_gram / cc_index_distinct as a numpy model, and the seeded worlds both new test files use
(tests/test_index_distinct_host.py, where the model is held to a plain double loop, and tests/test_gpu_index_distinct.py, where the
device is held to the model).

Thinning a ranked list is a walk over the Gram matrix of its present entries: an entry is kept unless a KEPT entry before it is at
least `same_at` similar (the greedy rule; under the detector's mask rule a suppressed entry would still suppress).  The GPU tests run
the model on the device's own `ix.gram(list)`, so every comparison is exact; `gram` itself is held to float64 with
score_cases.order_free_bound.

Random unit rows are all mutually dissimilar, so the worlds here are new (DupWorld): clusters of 1 to 40 rows around shared centres,
byte-equal copies, and chains a ~ b, b ~ c, a !~ c.  The similarity inside a cluster is one of LEVELS exactly (up to the rounding of
the storage, about 1e-3): a member is cos(t) * centre + sin(t) * u_k with the u_k orthonormal and orthogonal to the centre, so two
members meet at cos(t)^2.  The thresholds the tests use (SAME_AT) lie 0.01 and more from every level, from the two chain values and
from 1, and rows of different clusters meet near 0: no pair comes near a threshold, which tests/test_index_distinct_host.py
checks on the stored rows of all three storages."""
import numpy as np

from like_cases import stored
from score_cases import U, exact, gamma, order_free_bound            # noqa: F401  (re-exported for the two test files)
from where_cases import GROUPS, Rows, unit

MAX_DEPTH, MAX_Q = 1024, 64                                      # CC_DISTINCT_MAX_DEPTH, CC_DISTINCT_MAX_Q
N = 2 * 4096 + 37                                                # 8229, as like_cases.N_ODD
DIMS = (768, 256)                                                # CLIP's width, and the smallest the bf16 / i8 storages take
LEVELS = (0.99, 0.97, 0.93, 0.91)                                # the similarity inside a cluster
CHAIN = 0.96                                                     # a.b = b.c = 0.96, a.c = 2 * 0.96^2 - 1 = 0.8432
SAME_AT = (0.95, 0.92, 0.90)                                     # splits the levels 2 : 2, 3 : 1, 4 : 0; a chain is a chain under all three
DEPTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1024)                 # the word and row boundaries of the bit matrix


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def greedy(G, same_at):
    """(n, n) similarities of a list's present entries -> (keep (n,) bool, owner (n,) int64): entry j is kept iff no kept i < j has
    G[i][j] >= same_at (float32); owner[j] is the first such i of a dropped j and -1 of a kept one.  Written as the walk the device
    does: a kept entry marks what it newly drops."""
    G = np.asarray(G, np.float32)
    n = len(G)
    t = np.float32(same_at)
    keep, owner = np.zeros(n, bool), np.full(n, -1, np.int64)
    dropped = np.zeros(n, bool)
    for j in range(n):
        if dropped[j]:
            continue
        keep[j] = True
        hit = (G[j] >= t) & ~dropped
        hit[:j + 1] = False
        owner[hit] = j
        dropped |= hit
    return keep, owner


def mask_rule(G, same_at):
    """The detector's rule (a suppressed entry still suppresses) -> keep (n,) bool.  NOT what cc_index_distinct does."""
    G = np.asarray(G, np.float32)
    hit = np.triu(G >= np.float32(same_at), 1)
    return ~hit.any(axis=0)


def distinct_model(idx, score, G_of, same_at, start, count, size):
    """idx (Q, depth) -> what EmbeddingIndex.distinct returns: (idx (Q, count) int32, score (Q, count) f32 or None, dups (Q, count)
    int32, total (Q,) int64).  G_of(rows) gives the Gram matrix of a list of row numbers; size is the number of rows in the index."""
    idx = np.atleast_2d(np.asarray(idx, np.int64))
    Q, depth = idx.shape
    sc = None if score is None else np.asarray(score, np.float32).reshape(Q, depth)
    oi, od = np.full((Q, count), -1, np.int32), np.zeros((Q, count), np.int32)
    os_ = None if sc is None else np.full((Q, count), -np.inf, np.float32)
    total = np.zeros(Q, np.int64)
    for q in range(Q):
        at = np.flatnonzero((idx[q] >= 0) & (idx[q] < size))
        if not len(at):
            continue
        keep, owner = greedy(G_of(idx[q, at]), same_at)
        dups = np.bincount(owner[owner >= 0], minlength=len(at))
        k = np.flatnonzero(keep)
        total[q] = len(k)
        win = k[start:start + count]
        oi[q, :len(win)] = idx[q, at[win]]
        od[q, :len(win)] = dups[win]
        if sc is not None:
            os_[q, :len(win)] = sc[q, at[win]]
    return oi, os_, od, total


# ---- the worlds ---------------------------------------------------------------------------------------------------------------------
def cluster(rng, dim, size, level):
    """`size` unit rows that meet pairwise at `level` exactly (in exact arithmetic)"""
    basis, _ = np.linalg.qr(rng.standard_normal((dim, size + 1)))          # orthonormal columns: the centre and one direction per member
    c, s = np.sqrt(level), np.sqrt(1.0 - level)
    return (c * basis[:, :1] + s * basis[:, 1:]).T


def chain(rng, dim):
    """a, b, c in one plane, b between the other two: a.b = b.c = CHAIN, a.c = 2 CHAIN^2 - 1"""
    basis, _ = np.linalg.qr(rng.standard_normal((dim, 2)))
    th = np.arccos(CHAIN)
    return np.stack([np.cos(k * th) * basis[:, 0] + np.sin(k * th) * basis[:, 1] for k in range(3)])


class DupWorld(Rows):
    """where_cases.Rows (groups, track slots, ts, classes) with its embeddings replaced: clusters of 1 to 40 rows at one of LEVELS,
    scattered over the row numbers; a tenth of the rows byte-equal copies of an earlier row; eight chains at known rows (self.chains,
    each (a, b, c) ascending); the last row of the index a member of a cluster.  18 queries: members-to-be of the first clusters
    with fresh noise, so that a ranking's head is full of near-duplicates."""

    def __init__(self, dim, n=N, seed=41):
        super().__init__(n=n, seed=seed)
        rng = np.random.default_rng(seed + dim)
        rows, centres = [], []
        while len(rows) < n:
            size = int(rng.integers(1, 41)) if rows else 12
            C = cluster(rng, dim, size, LEVELS[int(rng.integers(0, len(LEVELS)))])
            centres.append(C.mean(axis=0))
            rows.extend(C)
        order = rng.permutation(n)
        p = int(np.flatnonzero(order == n - 1)[0])
        order[[0, p]] = order[[p, 0]]                                      # rows[k] lands at order[k]: row n - 1 is a member of the first cluster
        E = np.empty((n, dim), np.float32)
        E[order] = np.asarray(rows[:n], np.float32)
        self.chains = []
        for k in range(8):
            at = 100 + 1000 * k + np.array([0, 7, 301])
            E[at] = chain(rng, dim).astype(np.float32)
            self.chains.append(tuple(int(r) for r in at))
        taken = {r for c in self.chains for r in c} | {n - 1}
        for i in np.flatnonzero(rng.random(n) < 0.1):
            if i and int(i) not in taken:
                E[i] = E[rng.integers(0, i)]
        self.E, self.dim = E, dim
        self.q = unit(np.stack(centres[:18]) + 0.3 * unit(rng.standard_normal((18, dim))))


_worlds = {}


def world(dim):
    if dim not in _worlds:
        _worlds[dim] = DupWorld(dim)
    return _worlds[dim]


def threshold_margins(D, thresholds, block=1024):
    """-> ([min over all pairs of stored rows D of |<a, b> - t| in float64, per t], the largest order_free_bound can get for such
    rows: gamma(dim) * max ||a||^2, since |a|.|b| <= ||a|| ||b|| (Cauchy-Schwarz)).  One pass over the Gram matrix for all t."""
    D = np.asarray(D, np.float64)
    ts = [float(np.float32(t)) for t in thresholds]
    worst = [np.inf] * len(ts)
    for a in range(0, len(D), block):
        S = D[a:a + block] @ D.T
        worst = [min(w, float(np.abs(S - t).min())) for w, t in zip(worst, ts)]
    return worst, gamma(D.shape[1]) * float((D * D).sum(axis=1).max())


# ---- rows whose products are exact in every storage and every order of summation -----------------------------------------------------
def crafted_rows(dim):
    """-> (E (4, dim) float32, same_at float32): rows A, B=, B-, B+ with A.B= == same_at, A.B- one ulp below it, A.B+ one ulp above.

    Group 0 (columns 0 .. 31) holds multiples of 2^-8, group 1 (columns 32 .. 63) multiples of 2^-12, in both the largest value is 127
    steps: the int8 scale is the step itself and the codes are the multipliers, and no value has more than 7 significant bits, so
    bf16 keeps it.  A product of group 0 is a multiple of 2^-16, one of group 1 of 2^-24, every dot product below 1: all partial sums,
    in any order, are multiples of 2^-24 below 1 and therefore float32 numbers.  A.Bx = (3 * 127^2 + 127 * 100) 2^-16 + x 2^-24 =
    0.93211... + x 2^-24, in [0.5, 1) where one ulp is 2^-24."""
    def row(g0, g1):
        v = np.zeros(dim)
        for c, m in g0:
            v[c] = m * 2.0 ** -8
        for c, m in g1:
            v[32 + c] = m * 2.0 ** -12
        return v
    A = row([(0, 127), (1, 127), (2, 127), (3, 127)], [(0, 127), (1, 1)])
    B = [row([(0, 127), (1, 127), (2, 127), (3, 100)], [(1, x), (2, 127)]) for x in (64, 63, 65)]
    E = np.stack([A] + B).astype(np.float32)
    t = (3 * 127 * 127 + 127 * 100) * 2.0 ** -16 + 64 * 2.0 ** -24
    same_at = np.float32(t)
    assert float(same_at) == t and np.array_equal(E.astype(np.float64), np.stack([A] + B))
    return E, same_at
