"""What a day digest costs on the device (docs/measurement.md, "Day digest"):

    python tools/dev/measure_digest.py [--rows N] [--storage f32,bf16,i8] [--calls C] [--big-calls B] [--rounds R] [--warmup W] [--limit SECONDS] [--trace]

One world per storage of N x 768 crops (default 1 M) in 24 groups, filled on the device: every group has 500 objects of its own, a
crop is its object's centre with noise (cosine about 0.98 inside an object), groups and objects drawn at random per row, ts at random.
Timed with hipEvents on the stream the calls run on (a digest reads one number back inside, so the span of a call includes that
wait), results left on the device; R rounds that alternate the calls, per call the median over all rounds and the span of the round
medians:
  A    rank(0, 100) of one query under the group filter              the yardstick: a page of a search over the same folder
  D1   digest of ONE group (N / 24 rows, about 500 objects), same_at 0.9, a page of 100 by count, no totals
  D1t  D1 with the totals asked for
  D2   digest of the WHOLE index: the cap of 1024 leaders is reached within the first pieces, so every later piece meets 1024
       leaders - the worst case (B calls per round instead of C)
  H1   what D1 costs without the call: `fetch` the group's rows in pieces of 65535, then the float32 greedy walk in numpy on the
       host, piece by piece of 1024 rows with one matrix product per piece (run twice, the faster one counts; wall clock)
The script first checks the device form against the host form, and the host walk's answer against the device's.
--trace: no timing, only 5 calls of D1 and one of D2 per storage, for a kernel trace taken from outside.  One JSON line out."""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

DIM, GROUPS, OBJECTS = 768, 24, 500
SAME_AT = 0.9


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def host_walk(E, same_at, cap=1024, piece=1024):
    """The float32 greedy walk over rows E in order -> (leader positions, counts): per piece one product against the leaders so far
    and one against itself, then the sequential part over the piece."""
    t = np.float32(same_at)
    leaders, counts = [], []
    L = np.empty((cap, E.shape[1]), np.float32)
    for a in range(0, len(E), piece):
        P = E[a:a + piece]
        old = (P @ L[:len(leaders)].T >= t) if leaders else np.zeros((len(P), 1), bool)
        has = old.any(axis=1)
        first = old.argmax(axis=1)
        own = P @ P.T >= t
        claimed = has.copy()
        for j in range(len(P)):
            if has[j]:
                counts[first[j]] += 1
            elif not claimed[j] and len(leaders) < cap:
                hit = own[j] & ~claimed
                hit[:j + 1] = False
                claimed |= hit
                L[len(leaders)] = P[j]
                leaders.append(a + j)
                counts.append(1 + int(hit.sum()))
    return np.asarray(leaders), np.asarray(counts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--storage", default="f32,bf16,i8")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--big-calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=540)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    signal.alarm(a.limit)                                 # the default action of SIGALRM ends the process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from clearcam_amd.objects import EmbeddingIndex
    n = a.rows
    gen = torch.Generator(device="cuda"); gen.manual_seed(11)
    centres = unit(torch.randn((GROUPS * OBJECTS, DIM), generator=gen, device="cuda"))
    group = torch.randint(0, GROUPS, (n,), generator=gen, device="cuda")
    obj = torch.randint(0, OBJECTS, (n,), generator=gen, device="cuda")
    ts = torch.randint(0, 86400, (n,), generator=gen, device="cuda")
    group_h, ts_h = group.cpu().numpy().astype(np.int32), ts.cpu().numpy().astype(np.int32)
    q = unit(centres[:1] + 0.15 * unit(torch.randn((1, DIM), generator=gen, device="cuda")))
    allowed = np.zeros(GROUPS, np.uint8)
    allowed[3] = 1
    mine = np.flatnonzero(group_h == 3)
    stream = torch.cuda.Stream()
    res = {"what": "measure_digest", "rows": n, "group_rows": int(mine.size), "calls": a.calls, "big_calls": a.big_calls, "rounds": a.rounds, "same_at": SAME_AT}
    for storage in a.storage.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        for lo in range(0, n, 1 << 18):                   # in pieces: the f32 staging of a bf16 / i8 index stays small
            hi = min(n, lo + (1 << 18))
            E = unit(centres[group[lo:hi] * OBJECTS + obj[lo:hi]] + 0.15 * unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda")))
            ix.add(E, groups=group_h[lo:hi], ts=ts_h[lo:hi])
            del E
        torch.cuda.empty_cache()

        def host_way():
            E = np.concatenate([ix.fetch(mine[k:k + 65535]) for k in range(0, mine.size, 65535)])
            return host_walk(E, SAME_AT)

        calls = {"A_rank_100": (a.calls, lambda: ix.rank_device(q, 0, 100, allowed, tracks=False, with_total=False)),
                 "D1_digest_group": (a.calls, lambda: ix.digest_device(SAME_AT, 0, 100, allowed, with_total=False)),
                 "D1t_digest_group_totals": (a.calls, lambda: ix.digest_device(SAME_AT, 0, 100, allowed)),
                 "D2_digest_all_capped": (a.big_calls, lambda: ix.digest_device(SAME_AT, 0, 100, with_total=False))}
        # what is timed is what the tests check: the device form answers as the host form
        with torch.cuda.stream(stream):
            got = ix.digest_device(SAME_AT, 0, 100, allowed, owners=True)
            big = ix.digest_device(SAME_AT, 0, 100)
        stream.synchronize()
        want = ix.digest(SAME_AT, 0, 100, allowed, owners=True)
        assert all(np.array_equal(g.cpu().numpy() if hasattr(g, "cpu") else g, w) for g, w in zip(got, want))
        res.setdefault("answers", {})[storage] = {"group": [int(v) for v in want[4]], "all": [int(v) for v in big[4]], "largest": int(want[1][0])}
        if a.trace:
            with torch.cuda.stream(stream):
                for _ in range(5):
                    calls["D1_digest_group"][1]()
                calls["D2_digest_all_capped"][1]()
            stream.synchronize()
            ix.close()
            continue
        host_ms = []
        for _ in range(2):
            t0 = time.perf_counter()
            leaders, counts = host_way()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        by_first = ix.digest(SAME_AT, 0, 1024, allowed, by="first")
        k = int(by_first[4][0])
        # the float32 walk of the host may differ from the device's only where a pair lies within rounding of the threshold
        res["answers"][storage]["host_walk_agrees"] = bool(len(leaders) == k and np.array_equal(mine[leaders], by_first[0][:k]) and np.array_equal(counts, by_first[1][:k]))
        per_round = {k_: [] for k_ in calls}
        every = {k_: [] for k_ in calls}
        wall = {k_: [] for k_ in calls}
        with torch.cuda.stream(stream):
            for r in range(a.rounds):
                for name, (reps, fn) in calls.items():    # A, D1, D1t, D2, A, ...: drift hits all of them alike
                    for i in range(a.warmup if reps > 2 else 1):
                        fn()
                    stream.synchronize()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
                    t0 = time.perf_counter()
                    for e0, e1 in ev:
                        e0.record(stream)
                        fn()
                        e1.record(stream)
                    stream.synchronize()
                    wall[name].append((time.perf_counter() - t0) * 1e3 / reps)
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
                    per_round[name].append(statistics.median(ms))
                    every[name] += ms
        res[storage] = {k_: {"p50_ms": round(statistics.median(every[k_]), 4), "round_p50_min_ms": round(min(per_round[k_]), 4),
                             "round_p50_max_ms": round(max(per_round[k_]), 4), "min_ms": round(min(every[k_]), 4),
                             "wall_ms_per_call": round(statistics.median(wall[k_]), 4)} for k_ in calls}
        res[storage]["H1_fetch_and_host_walk"] = {"wall_ms": round(min(host_ms), 1), "runs_ms": [round(v, 1) for v in host_ms]}
        print(json.dumps({storage: res[storage]}), flush=True)
        ix.close()
        del ix
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
