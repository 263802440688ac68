"""What "seen before?" costs on the device (docs/measurement.md, "Seen before"):

    python tools/dev/measure_sightings.py [--rows N] [--storage f32,bf16,i8] [--calls C] [--big-calls B] [--rounds R] [--warmup W] [--limit SECONDS] [--no-host]

The world of tools/dev/measure_digest.py: per storage N x 768 crops (default 1 M) in 24 groups, filled on the device; every group has
500 objects of its own, a crop is its object's centre with noise (cosine about 0.98 inside an object), groups and objects drawn at
random per row.  Timed with hipEvents on the stream the calls run on, results left on the device, no totals asked for (so nothing
waits); R rounds that alternate the calls, per call the median over all rounds and the span of the round medians:
  A    rank(0, 100) of one query under a group filter                 the yardstick, and the scan rate the TB/s are held against
  B    digest of the WHOLE index with the cap of 1024 leaders reached  the same n x M products in 64 x 64 tiles, plus the walks
  S1   one group's leaders (about 500) against the other 23 groups, group counts asked for: ObjectFinder.seen_before's call
  S2   1024 objects (B's leaders) against everything, group counts asked for
  S3a  1 object against everything          S3b  64 objects against everything
  C    what S1 costs without the call: `fetch` the leaders and the other groups' rows in pieces of 65535 and one float32 matrix
       product per piece in numpy on the host (once; wall clock).  Its counts are compared with S1's.
Per leg: ms, the achieved TFLOP/s (2 n M dim) against the 157 of the f32 MFMA pipe, and the TB/s of stored rows against A's.
The bar: S2 costs no more than B in the same run, per storage.  Before timing the device form is checked against the host form.
One JSON line out per storage, and one for the whole run."""
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
PEAK_TF = 157.0
ROW_BYTES = {"f32": DIM * 4, "bf16": DIM * 2, "i8": DIM + DIM // 8}


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--storage", default="f32,bf16,i8")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--big-calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=540)
    ap.add_argument("--no-host", action="store_true")
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
    today = np.zeros(GROUPS, np.uint8)
    today[3] = 1
    history = (1 - today).astype(np.uint8)
    others = np.flatnonzero(group_h != 3)
    stream = torch.cuda.Stream()
    res = {"what": "measure_sightings", "rows": n, "history_rows": int(others.size), "calls": a.calls, "big_calls": a.big_calls, "rounds": a.rounds,
           "same_at": SAME_AT, "peak_tf": PEAK_TF}
    for storage in a.storage.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        for lo in range(0, n, 1 << 18):                   # in pieces: the f32 staging of a bf16 / i8 index stays small
            hi = min(n, lo + (1 << 18))
            E = unit(centres[group[lo:hi] * OBJECTS + obj[lo:hi]] + 0.15 * unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda")))
            ix.add(E, groups=group_h[lo:hi], ts=ts_h[lo:hi])
            del E
        torch.cuda.empty_cache()
        lead = ix.digest(SAME_AT, 0, 1024, today, by="first")
        lead = lead[0][:int(lead[4][0])].astype(np.int64)
        big = ix.digest(SAME_AT, 0, 1024, by="first")
        cap = big[0][:int(big[4][0])].astype(np.int64)
        assert len(cap) == 1024 and int(big[4][2]) > 0    # B is the capped digest
        legs = {"A_rank_100": (a.calls, 0, n, lambda: ix.rank_device(q, 0, 100, today, tracks=False, with_total=False)),
                "B_digest_all_capped": (a.big_calls, 1024, n, lambda: ix.digest_device(SAME_AT, 0, 100, with_total=False)),
                "S1_group_leaders_vs_history": (a.calls, len(lead), int(others.size), lambda: ix.sightings_device(lead, SAME_AT, history, group_counts=GROUPS, with_total=False)),
                "S2_1024_vs_all": (a.big_calls, 1024, n, lambda: ix.sightings_device(cap, SAME_AT, group_counts=GROUPS, with_total=False)),
                "S3a_1_vs_all": (a.calls, 1, n, lambda: ix.sightings_device(cap[:1], SAME_AT, with_total=False)),
                "S3b_64_vs_all": (a.calls, 64, n, lambda: ix.sightings_device(cap[:64], SAME_AT, with_total=False))}
        # what is timed is what the tests check: the device form answers as the host form
        answers = {}
        for name, rows, kw in (("S1", lead, dict(allowed=history, group_counts=GROUPS)), ("S2", cap, dict(group_counts=GROUPS)), ("S3b", cap[:64], {})):
            with torch.cuda.stream(stream):
                got = ix.sightings_device(rows, SAME_AT, **kw)
            stream.synchronize()
            want = ix.sightings(rows, SAME_AT, **kw)
            for g, w in zip(got[:4], want[:4]):
                assert (g is None and w is None) or g.cpu().numpy().tobytes() == w.tobytes(), (storage, name)
            assert got[4] == want[4]
            answers[name] = {"objects": len(rows), "competing": int(want[4]), "seen": int((want[0] > 0).sum()), "matches": int(want[0].sum())}
            if name == "S1":
                s1 = want
        res.setdefault("answers", {})[storage] = answers
        host = None
        if not a.no_host:                                 # C: the leaders and the history rows fetched, one product per piece
            t0 = time.perf_counter()
            L = ix.fetch(lead)
            counts = np.zeros(len(lead), np.int64)
            best = np.full(len(lead), -np.inf, np.float32)
            for k in range(0, others.size, 65535):
                S = L @ ix.fetch(others[k:k + 65535]).T
                counts += (S >= np.float32(SAME_AT)).sum(axis=1)
                best = np.maximum(best, S.max(axis=1))
            host = {"wall_ms": round((time.perf_counter() - t0) * 1e3, 1),
                    # numpy sums in another order: the counts may differ only where a pair lies within rounding of the threshold
                    "counts_agree": bool(np.array_equal(counts, s1[0])), "best_within_1e-5": bool(np.abs(best - s1[2]).max() <= 1e-5)}
        per_round = {k_: [] for k_ in legs}
        every = {k_: [] for k_ in legs}
        with torch.cuda.stream(stream):
            for r in range(a.rounds):
                for name, (reps, _, _, fn) in legs.items():   # A, B, S1, S2, S3a, S3b, A, ...: drift hits all of them alike
                    for i in range(a.warmup if reps > 2 else 1):
                        fn()
                    stream.synchronize()
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
                    for e0, e1 in ev:
                        e0.record(stream)
                        fn()
                        e1.record(stream)
                    stream.synchronize()
                    ms = [e0.elapsed_time(e1) for e0, e1 in ev]
                    per_round[name].append(statistics.median(ms))
                    every[name] += ms
        out = {}
        for name, (_, n_obj, m, _) in legs.items():
            p50 = statistics.median(every[name])
            out[name] = {"p50_ms": round(p50, 4), "round_p50_min_ms": round(min(per_round[name]), 4), "round_p50_max_ms": round(max(per_round[name]), 4),
                         "min_ms": round(min(every[name]), 4), "tb_per_s": round(m * ROW_BYTES[storage] / p50 / 1e9, 3)}
            if n_obj:
                out[name]["tflops"] = round(2.0 * n_obj * m * DIM / p50 / 1e9, 2)
                out[name]["of_peak"] = round(out[name]["tflops"] / PEAK_TF, 3)
        for name in out:
            out[name]["of_scan_rate"] = round(out[name]["tb_per_s"] / out["A_rank_100"]["tb_per_s"], 3)
        out["bar_S2_le_B"] = bool(out["S2_1024_vs_all"]["p50_ms"] <= out["B_digest_all_capped"]["p50_ms"])
        if host is not None:
            out["C_fetch_and_numpy"] = host
        res[storage] = out
        print(json.dumps({storage: out}), flush=True)
        ix.close()
        del ix
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
