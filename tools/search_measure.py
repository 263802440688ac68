"""Latency of ObjectFinder.search on a large index (docs/measurement.md): python tools/search_measure.py [--rows N] [--calls C] [--warmup W]

Two worlds of N x 768 f32 crops (default 1 M) in 20 camera/day folders, one after the other in one process:
  a  ordinary:   50 k tracks of about 20 crops each
  b  degenerate: one track owns 10 % of the rows and they score above everything else (a parked car, one crop every 10 s);
                 the rest as in a
Timed per world: ObjectFinder.search(top_k=10), p50 of C calls after W warm-up calls (wall clock, the answer is on the host).
On world a also EmbeddingIndex.search and, where the index has it, EmbeddingIndex.search_tracks at k = 160.
Runs on a tree without search_tracks as well (it then times what exists).  One JSON line out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearcam_amd.objects import EmbeddingIndex, ObjectFinder, _RowTable

DIM = 768
HAS_TRACKS = hasattr(EmbeddingIndex, "search_tracks")


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def build(n, dominant, gen, q0):
    """ObjectFinder with an attached device matrix of n rows, filled on the device (no 3 GB host copy, no per-crop dict)."""
    rng = np.random.default_rng(1)
    track = rng.integers(1, max(n // 20, 1) + 1, n)
    E = unit(torch.randn((n, DIM), generator=gen, device="cuda"))
    if dominant:
        rows = rng.choice(n, n // 10, replace=False)
        track[rows] = 0
        r = torch.as_tensor(rows, device="cuda")
        E[r] = unit(q0 + 0.5 * torch.randn((len(rows), DIM), generator=gen, device="cuda") / DIM ** 0.5)     # cosine ~0.9 with q0
    cams, days = rng.integers(0, 4, n), rng.integers(1, 6, n)
    paths = [f"data/cameras/cam{c}/objects/2026-01-0{d}/{1700000000 + i}.0_{t}_2.jpg" for i, (c, d, t) in enumerate(zip(cams, days, track))]
    index, table = EmbeddingIndex(DIM, n), _RowTable()
    groups = table.extend(paths)
    if HAS_TRACKS:
        index.add(E, groups, table.slots())
    else:
        index.add(E, groups)
    f = ObjectFinder("nowhere")
    f._dev["store"] = (index, table)
    f._attached = True
    return f, index


def timed(fn, queries, calls, warmup):
    for i in range(warmup):
        fn(queries[i % len(queries)])
    ms = []
    for i in range(calls):
        t0 = time.perf_counter()
        fn(queries[i % len(queries)])
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"p50_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    q0 = unit(torch.randn(DIM, generator=gen, device="cuda"))
    queries = unit(q0 + 0.2 * torch.randn((8, DIM), generator=gen, device="cuda") / DIM ** 0.5).cpu().numpy()
    res = {"what": "search_measure", "rows": a.rows, "calls": a.calls, "search_tracks": HAS_TRACKS}
    for name, dominant in (("a", False), ("b", True)):
        f, index = build(a.rows, dominant, gen, q0)
        hits = f.search(top_k=10, text_embedding=queries[0])
        out = {"tracks_in_top10": len({p.split("_")[-2] for p, _ in hits}), "top1_track": hits[0][0].split("_")[-2],
               "finder_top10": timed(lambda q: f.search(top_k=10, text_embedding=q), queries, a.calls, a.warmup)}
        if not dominant:
            out["search_k160"] = timed(lambda q: index.search(q, 160), queries, a.calls, a.warmup)
            if HAS_TRACKS:
                out["search_tracks_k160"] = timed(lambda q: index.search_tracks(q, 160), queries, a.calls, a.warmup)
        res[name] = out
        index.close()
        del f, index
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
