"""The int8 storage rule of the embedding index (include/clearcam_hip.h, CC_INDEX_I8) restated in numpy, shared by
tests/test_index_i8_host.py (where it is checked against hand-written codes and against its own error bound) and
tests/test_gpu_index_i8.py (where the device bytes are held to it bit for bit).

A row is dim int8 codes and dim / 32 float32 scales, one per group of 32 consecutive elements.  Per group, all in float32:
a = max |x|, s = a / 127 (correctly rounded), s zero or subnormal -> s = 0 and every code 0, otherwise
code = clip(rint(x / s), -127, 127) with ties to even.  The decoded element is float32(code) * s."""
import numpy as np

GROUP = 32
F32_MIN = np.float32(np.finfo(np.float32).tiny)                  # the smallest normal float32


def quantise(E):
    """(n, dim) float32 -> (codes (n, dim) int8, scales (n, dim / 32) float32)"""
    E = np.ascontiguousarray(E, dtype=np.float32)
    n, dim = E.shape
    assert dim % GROUP == 0
    x = E.reshape(n, dim // GROUP, GROUP)
    a = np.abs(x).max(axis=2)
    s = (a / np.float32(127.0)).astype(np.float32)
    s[~(s >= F32_MIN)] = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.rint(x / s[:, :, None])                             # float32 division, round half to even
    c = np.where(s[:, :, None] > 0, np.clip(c, -127, 127), 0)
    return c.astype(np.int8).reshape(n, dim), s


def decode(codes, scales):
    """-> (n, dim) float32: what the index holds"""
    n, dim = codes.shape
    return (codes.astype(np.float32).reshape(n, dim // GROUP, GROUP) * scales[:, :, None]).astype(np.float32).reshape(n, dim)


def score_bound(q, scales):
    """(Q, dim) queries, (n, dim / 32) scales -> (Q, n) float64: sum over groups of (s_g / 2) * ||q_g||_1, the most a score of the
    decoded rows can differ from the exact one.  The half step is widened by 127 * 2^-23 of a step: x / s is rounded to float32
    before rint (at most 127 * 2^-24 off) and code * s once more in `decode`."""
    q = np.atleast_2d(np.asarray(q, np.float64))
    l1 = np.abs(q).reshape(q.shape[0], -1, GROUP).sum(axis=2)                      # (Q, groups)
    return (0.5 + 127.0 * 2.0 ** -23) * l1 @ np.asarray(scales, np.float64).T


def crafted_rows(dim, seed=5):
    """-> (E (7, dim) float32, expected): rows that sit on the edges of the rule.  expected lists (row, group, codes (32,), scale)
    written down by hand for the groups whose answer can be."""
    assert dim % 256 == 0
    rng = np.random.default_rng(seed)
    G = dim // GROUP
    E = np.zeros((7, dim), np.float32)
    expected = []

    def put(row, group, values):
        E[row, group * GROUP:group * GROUP + len(values)] = np.asarray(values, np.float32)

    def zeros_but(pairs):
        c = np.zeros(GROUP, np.int8)
        for i, v in pairs:
            c[i] = v
        return c

    # row 0: all zero
    expected += [(0, g, zeros_but([]), np.float32(0)) for g in range(G)]
    # row 1: a live row with a zero group inside
    E[1] = 0.05 * rng.standard_normal(dim).astype(np.float32)
    put(1, 2, np.zeros(GROUP))
    expected.append((1, 2, zeros_but([]), np.float32(0)))
    # row 2: scales at the edge of the normal range.  group 0: amax is subnormal itself; group 1: amax is normal, amax / 127 is
    # subnormal; group 2: amax = 127 * 2^-126, the scale is the smallest normal number and is kept
    put(2, 0, [1e-40, -3e-41, 2e-42])
    put(2, 1, [1e-36, -5e-37, 1.4e-36])
    put(2, 2, np.array([127, -64, 1, 0, 2, -127], np.float32) * F32_MIN)
    expected.append((2, 0, zeros_but([]), np.float32(0)))
    expected.append((2, 1, zeros_but([]), np.float32(0)))
    expected.append((2, 2, zeros_but([(0, 127), (1, -64), (2, 1), (4, 2), (5, -127)]), F32_MIN))
    # row 3: amax exactly 127 -> scale 1: halves round to even
    put(3, 0, [127, 0.5, 1.5, 2.5, -0.5, -1.5, 3.5, -2.5, 126.5, -126.5])
    expected.append((3, 0, zeros_but([(0, 127), (1, 0), (2, 2), (3, 2), (4, 0), (5, -2), (6, 4), (7, -2), (8, 126), (9, -126)]), np.float32(1)))
    # row 4: -amax at the first and +amax at the last element of a group (and the reverse in the last group of the row)
    put(4, 1, [-0.25, 0.1] + [0.0] * 29 + [0.25])
    put(4, G - 1, [0.25] + [0.0] * 30 + [-0.25])
    expected.append((4, 1, zeros_but([(0, -127), (1, 51), (31, 127)]), np.float32(0.25 / 127.0)))          # 0.1 / (0.25 / 127) = 50.8
    expected.append((4, G - 1, zeros_but([(0, 127), (31, -127)]), np.float32(0.25 / 127.0)))
    # row 5: one huge outlier beside tiny values: step 1000 / 127 = 7.87
    put(5, 3, [1e-3] * 5 + [1000.0, -3.0, 4.0, -12.0] + [-1e-3] * 23)
    expected.append((5, 3, zeros_but([(5, 127), (7, 1), (8, -2)]), np.float32(1000.0 / 127.0)))
    # row 6: groups of very different magnitude in one row, 1e-6 .. 1e3
    mag = (10.0 ** (np.arange(G) % 10 - 6)).astype(np.float32)
    E[6] = (rng.standard_normal((G, GROUP)).astype(np.float32) * mag[:, None]).reshape(dim)
    return E, expected


def unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def outlier_rows(n, dim, seed):
    """Unit Gaussian rows with two dimensions of about 0.4 each: what one scale per row would handle badly."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((n, dim))
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    E *= np.sqrt(1 - 2 * 0.4 ** 2)
    for r in range(n):
        i = rng.choice(dim, 2, replace=False)
        E[r, i] = 0.4 * rng.choice([-1.0, 1.0], 2)
    return E.astype(np.float32)
