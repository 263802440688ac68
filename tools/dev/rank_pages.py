"""Latency of paging through search results at depth (docs/measurement.md, "Paging the search"):

    python tools/dev/rank_pages.py [--rows N] [--calls C] [--warmup W] [--worlds a,b,a16] [--no-parent] [--limit SECONDS]

Worlds of N x 768 crops (default 1 M) in 20 camera/day folders, filled on the device, one after the other in one process:
  a    50 k tracks of about 20 crops, 5 % of the rows without a track id, f32 rows
  b    as a, but one track owns 10 % of the rows and they score above everything else
  a16  as a with bf16 rows
Timed per world, wall clock with the answer on the host, p50 of C calls after W warm-up calls:
  EmbeddingIndex.search_tracks(k=100)                       the first page as it is today: the yardstick of the same run
  EmbeddingIndex.rank(start, 100), start 0 / 1000 / 10 000  pages of the track order
  EmbeddingIndex.rank(100 000, 100, tracks=False)           a page of the row order
  EmbeddingIndex.rank(0, 5000)                              five windows in one call
  ObjectFinder.search_page(start=1000, count=100, min_score=0.21)
  ObjectFinder.search(top_k=1100) over an index that hides `rank`: the candidate-list loop + score download + Python loop over
  the rows, which is what every page past the tenth cost before (two calls only: they take seconds)
The script ends itself after --limit seconds (default 600).  Kernel split: put it behind `rocprofv3 --kernel-trace --stats --`
with --no-parent --calls 10 --warmup 2.  One JSON line out."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from clearcam_amd.objects import EmbeddingIndex, ObjectFinder, _RowTable

DIM = 768


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


class WithoutRank:
    """The same index with `rank` hidden: ObjectFinder.search then takes the path it took before the index could rank."""

    def __init__(self, index):
        self._index, self.dim = index, index.dim
        self.search, self.search_tracks, self.scores = index.search, index.search_tracks, index.scores

    def __len__(self):
        return len(self._index)


def build(n, dominant, storage, gen, q0):
    rng = np.random.default_rng(1)
    track = rng.integers(1, max(n // 20, 1) + 1, n)
    loose = rng.random(n) < 0.05
    E = unit(torch.randn((n, DIM), generator=gen, device="cuda"))
    if dominant:
        rows = rng.choice(n, n // 10, replace=False)
        track[rows], loose[rows] = 0, False
        r = torch.as_tensor(rows, device="cuda")
        E[r] = unit(q0 + 0.5 * torch.randn((len(rows), DIM), generator=gen, device="cuda") / DIM ** 0.5)     # cosine ~0.9 with q0
    cams, days = rng.integers(0, 4, n), rng.integers(1, 6, n)
    paths = [f"data/cameras/cam{c}/objects/2026-01-0{d}/" + (f"snap{i}.jpg" if s else f"{1700000000 + i}.0_{t}_2.jpg")
             for i, (c, d, t, s) in enumerate(zip(cams, days, track, loose))]
    index, table = EmbeddingIndex(DIM, n, storage=storage), _RowTable()
    groups = table.extend(paths)
    index.add(E, groups, table.slots())
    del E
    torch.cuda.empty_cache()
    f = ObjectFinder("nowhere")
    f._dev["store"] = (index, table)
    f._attached = True
    return f, index, table


def timed(fn, queries, calls, warmup):
    for i in range(warmup):
        fn(queries[i % len(queries)])
    ms = []
    for i in range(calls):
        t0 = time.perf_counter()
        fn(queries[i % len(queries)])                     # every call ends in a stream synchronise: the answer is on the host
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"p50_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worlds", default="a,b,a16")
    ap.add_argument("--no-parent", action="store_true")
    ap.add_argument("--limit", type=int, default=600)
    a = ap.parse_args()
    signal.alarm(a.limit)                                 # the default action of SIGALRM ends the process
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    q0 = unit(torch.randn(DIM, generator=gen, device="cuda"))
    queries = unit(q0 + 0.2 * torch.randn((8, DIM), generator=gen, device="cuda") / DIM ** 0.5).cpu().numpy()
    res = {"what": "rank_pages", "rows": a.rows, "calls": a.calls}
    kinds = {"a": (False, "f32"), "b": (True, "f32"), "a16": (False, "bf16")}
    deep_rows = min(100_000, max(a.rows - 100, 0))
    for name in a.worlds.split(","):
        dominant, storage = kinds[name]
        f, index, table = build(a.rows, dominant, storage, gen, q0)
        t = lambda fn, calls=a.calls, warmup=a.warmup: timed(fn, queries, calls, warmup)
        idx, sc, total = index.rank(queries[0], 0, 100)
        first = index.search_tracks(queries[0], 100)
        assert np.array_equal(idx, first[0]) and np.array_equal(sc, first[1])                 # the same first page
        out = {"answers": int(total[0]), "search_tracks_k100": t(lambda q: index.search_tracks(q, 100))}
        for start in (0, 1000, 10_000):
            out[f"rank_{start}_100"] = t(lambda q: index.rank(q, start, 100))
        out[f"rank_rows_{deep_rows}_100"] = t(lambda q: index.rank(q, deep_rows, 100, tracks=False))
        out["rank_0_5000"] = t(lambda q: index.rank(q, 0, 5000))
        out["search_tracks_k100_again"] = t(lambda q: index.search_tracks(q, 100))           # the yardstick once more: the spread of this run
        out["finder_page_1000_100_cut"] = t(lambda q: f.search_page(start=1000, count=100, text_embedding=q, min_score=0.21))
        out["finder_top_1100"] = t(lambda q: f.search(top_k=1100, text_embedding=q))
        if not a.no_parent:
            new = f.search(top_k=1100, text_embedding=queries[0])
            f._dev["store"] = (WithoutRank(index), table)
            old = f.search(top_k=1100, text_embedding=queries[0])
            out["same_as_before"] = new == old
            out["finder_top_1100_without_rank"] = timed(lambda q: f.search(top_k=1100, text_embedding=q), queries, 2, 0)
        res[name] = out
        print(json.dumps({name: out}), flush=True)
        index.close()
        del f, index, table
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
