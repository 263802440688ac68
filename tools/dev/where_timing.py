"""What the row filters and the timeline cost on the device (docs/measurement.md, "Row filters and timeline"):

    python tools/dev/where_timing.py [--rows N] [--storage f32,i8] [--calls C] [--rounds R] [--warmup W] [--tree DIR] [--limit SECONDS]

One world per storage of N x 768 crops (default 1 M) filled on the device: 50 k tracks of about 20 crops, 5 % of the rows without a
track id, 20 groups, ts uniform over a day, six classes.  Timed with hipEvents on the stream the calls run on, results left on the
device and no total asked for, so a call waits for nothing on the host; R rounds that alternate the calls, C calls each
after W warm-up calls, per call the median over all rounds and the span of the round medians:
  A  rank(0, 100)                                                     no filter: the launches of the parent commit
  B  rank(0, 100, ts_range=(14 h, 16 h), classes=three of the six)    the filter inside track_reduce_kernel and rank_keys_kernel
  C  timeline(24 bins of an hour)                                     scan, reduction, keys, timeline_kernel; no select
  D  rank(0, 100, tracks=False)                                       every row an answer: the yardstick of E
  E  timeline(24 bins of an hour, tracks=False)                       one LDS atomic per row into 24 bins: the contended case
--tree DIR imports clearcam_amd from another checkout (one built from the parent commit): it has no filter, so only A runs.
One JSON line out."""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys

import numpy as np
import torch

DIM = 768


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--storage", default="f32,i8")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    ap.add_argument("--limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.limit)                                 # the default action of SIGALRM ends the process
    sys.path.insert(0, os.path.abspath(a.tree))
    from clearcam_amd import _lib
    from clearcam_amd.objects import EmbeddingIndex
    new = hasattr(EmbeddingIndex, "timeline")
    n = a.rows
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    rng = np.random.default_rng(1)
    q = unit(torch.randn((8, DIM), generator=gen, device="cuda"))
    slot = rng.integers(0, max(n // 20, 1), n).astype(np.int32)
    slot[rng.random(n) < 0.05] = -1
    group = rng.integers(1, 21, n).astype(np.int32)
    ts = rng.integers(0, 86400, n).astype(np.int32)
    cls = rng.choice(np.array([0, 2, 7, 63, 64, 255]), n).astype(np.int32)
    window, classes = (14 * 3600, 16 * 3600), (2, 7, 64)
    stream = torch.cuda.Stream()
    res = {"what": "where_timing", "tree": "this" if new else "parent", "rows": n, "calls": a.calls, "rounds": a.rounds}
    for storage in a.storage.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        for lo in range(0, n, 1 << 18):                   # in pieces: the f32 staging of an i8 index stays small
            hi = min(n, lo + (1 << 18))
            E = unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda"))
            if new:
                ix.add(E, group[lo:hi], slot[lo:hi], ts=ts[lo:hi], classes=cls[lo:hi])
            else:
                ix.add(E, group[lo:hi], slot[lo:hi])
            del E
        torch.cuda.empty_cache()
        counts = torch.zeros((1, 24), dtype=torch.int32, device="cuda")

        def timeline(qi, flags=1):
            _lib.check(_lib.lib().cc_index_timeline(ix._h, _lib.ptr(qi), 1, float("-inf"), flags, None, 0, None, 0, 3600, 24, _lib.ptr(counts), None, 1,
                                                    C.c_void_p(stream.cuda_stream)))

        calls = {"A_rank": lambda qi: ix.rank_device(qi, 0, 100, with_total=False)}
        if new:
            calls["B_rank_where"] = lambda qi: ix.rank_device(qi, 0, 100, with_total=False, ts_range=window, classes=classes)
            calls["C_timeline"] = timeline
            calls["D_rank_rows"] = lambda qi: ix.rank_device(qi, 0, 100, tracks=False, with_total=False)
            calls["E_timeline_rows"] = lambda qi: timeline(qi, 0)
            host = ix.rank(q[:1].cpu().numpy(), 0, 100, ts_range=window, classes=classes)
            res.setdefault("answers", {})[storage] = {"unfiltered": int(ix.rank(q[:1].cpu().numpy(), 0, 1)[2][0]), "filtered": int(host[2][0])}
        per_round = {k: [] for k in calls}
        every = {k: [] for k in calls}
        with torch.cuda.stream(stream):
            for r in range(a.rounds):
                for name, fn in calls.items():            # A, B, C, ..., A, B, C, ...: drift hits all of them alike
                    for i in range(a.warmup):
                        fn(q[i % 8:i % 8 + 1])
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
                    for i, (e0, e1) in enumerate(ev):
                        e0.record(stream)
                        fn(q[i % 8:i % 8 + 1])
                        e1.record(stream)
                    stream.synchronize()
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
                    per_round[name].append(statistics.median(ms))
                    every[name] += ms
        if new:
            assert int(counts.sum()) == n                 # the last call was E: every row has a ts inside the day
        res[storage] = {k: {"p50_ms": round(statistics.median(every[k]), 4), "round_p50_min_ms": round(min(per_round[k]), 4),
                            "round_p50_max_ms": round(max(per_round[k]), 4), "min_ms": round(min(every[k]), 4)} for k in calls}
        print(json.dumps({storage: res[storage]}), flush=True)
        ix.close()
        del ix
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
