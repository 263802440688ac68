"""What a search by a stored crop, or by its whole track, costs on the device (docs/measurement.md, "Search by stored crop"):

    python tools/dev/like_timing.py [--rows N] [--storage f32,bf16,i8] [--calls C] [--rounds R] [--warmup W] [--limit SECONDS]

One world per storage of N x 768 crops (default 1 M) filled on the device: 50 k tracks of about 20 crops, 5 % of the rows without a
track id, 20 groups, and one planted track of 64 crops in one group.  Timed with hipEvents on the stream the calls run on, results
left on the device and no total asked for, so a call waits for nothing on the host; R rounds that alternate the calls, C calls each
after W warm-up calls, per call the median over all rounds and the span of the round medians:
  A  rank(0, 100), one query on the device                       the yardstick: the launches of the parent commit
  B  rank_like([row], 0, 100)                                    a gather of one row instead of a 3 KB copy, no fold
  C  rank(0, 100), 64 queries on the device                      64 separate answer lists
  D  rank_like(the 64 rows of the track, 0, 100, exclude=track)  the same scoring launch, one fold, ONE reduction and select
  S  scores of D's 64 queries into a device buffer               D - S is about what fold, keys and select cost (S also copies the
                                                                 (64, N) matrix once, device to device, which D does not)
  E  fetch of the 64 rows, left on the device
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
    ap.add_argument("--storage", default="f32,bf16,i8")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=420)
    a = ap.parse_args()
    signal.alarm(a.limit)                                 # the default action of SIGALRM ends the process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from clearcam_amd import _lib
    from clearcam_amd.objects import EmbeddingIndex
    n = a.rows
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    rng = np.random.default_rng(1)
    q = unit(torch.randn((8, DIM), generator=gen, device="cuda"))
    n_tracks = max(n // 20, 1)
    slot = rng.integers(0, n_tracks, n).astype(np.int32)
    slot[rng.random(n) < 0.05] = -1
    group = rng.integers(1, 21, n).astype(np.int32)
    track = (1000 + (n - 2000) // 64 * np.arange(64)).astype(np.int64)   # the planted track: 64 crops of one folder, spread over the matrix
    slot[track], group[track] = n_tracks, 1
    stream = torch.cuda.Stream()
    res = {"what": "like_timing", "rows": n, "calls": a.calls, "rounds": a.rounds}
    for storage in a.storage.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        for lo in range(0, n, 1 << 18):                   # in pieces: the f32 staging of a bf16 / i8 index stays small
            hi = min(n, lo + (1 << 18))
            E = unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda"))
            ix.add(E, group[lo:hi], slot[lo:hi])
            del E
        torch.cuda.empty_cache()
        with torch.cuda.stream(stream):
            q64 = ix.fetch(track, device_out=True)
        stream.synchronize()
        sc = torch.empty((64, n), dtype=torch.float32, device="cuda")

        def scores(_):
            _lib.check(_lib.lib().cc_index_scores(ix._h, _lib.ptr(q64), 64, _lib.ptr(sc), 1, C.c_void_p(stream.cuda_stream)))

        calls = {"A_rank_1": lambda qi: ix.rank_device(qi, 0, 100, with_total=False),
                 "B_like_1": lambda qi: ix.rank_like_device(track[:1], 0, 100, with_total=False),
                 "C_rank_64": lambda qi: ix.rank_device(q64, 0, 100, with_total=False),
                 "D_like_64_track": lambda qi: ix.rank_like_device(track, 0, 100, exclude="track", with_total=False),
                 "S_scores_64": scores,
                 "E_fetch_64": lambda qi: ix.fetch(track, device_out=True)}
        # what is timed is what the tests check: B answers as A does for the fetched row, D hides the track
        b = ix.rank_like(track[:1], 0, 100)
        a1 = ix.rank(ix.fetch(track[:1]), 0, 100)
        assert np.array_equal(b[0], a1[0]) and np.array_equal(b[1], a1[1]) and b[2][0] == a1[2][0]
        d = ix.rank_like(track, 0, 100, exclude="track")
        res.setdefault("answers", {})[storage] = {"B_total": int(b[2][0]), "D_total": int(d[2][0]), "D_path": ix.last_scores_path()}
        assert not set(d[0][0].tolist()) & set(track.tolist())
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
        res[storage] = {k: {"p50_ms": round(statistics.median(every[k]), 4), "round_p50_min_ms": round(min(per_round[k]), 4),
                            "round_p50_max_ms": round(max(per_round[k]), 4), "min_ms": round(min(every[k]), 4)} for k in calls}
        print(json.dumps({storage: res[storage]}), flush=True)
        ix.close()
        del ix, sc, q64
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
