"""What a page of distinct answers costs on the device (docs/measurement.md, "Distinct answers"):

    python tools/dev/measure_distinct.py [--rows N] [--storage f32,bf16,i8] [--calls C] [--rounds R] [--warmup W] [--limit SECONDS] [--trace]

One world per storage of N x 768 crops (default 1 M) filled on the device: N / 20 centres with about 20 crops each at cosine about
0.98 of one another (the same object again and again), no track ids, so that the head of a ranking is full of near-duplicates.  The
queries are centres with fresh noise.  Timed with hipEvents on the stream the calls run on, results left on the device; R rounds that
alternate the calls, C calls each after W warm-up calls, per call the median over all rounds and the span of the round medians:
  A   rank(0, 100), one query                                        the yardstick: a page as it is today
  B   rank(0, 1024), one query                                       the list a distinct page is cut from
  C   B, then distinct(same_at 0.9, 0, 100), no total                nothing waits on the host
  Ct  C with the total asked for                                     one wait for the stream
  B8  rank(0, 1024), eight queries
  D   B8, then distinct of the eight lists, no total
--trace: no timing, only 20 calls of C per storage, for a kernel trace taken from outside (squeeze_kernel, gram_kernel, walk_kernel).
One JSON line out."""
import argparse
import json
import os
import signal
import statistics
import sys

import numpy as np
import torch

DIM = 768
SAME_AT = 0.9


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
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    signal.alarm(a.limit)                                 # the default action of SIGALRM ends the process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from clearcam_amd.objects import EmbeddingIndex
    n = a.rows
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    n_centres = max(n // 20, 8)
    centres = unit(torch.randn((n_centres, DIM), generator=gen, device="cuda"))
    member = torch.randint(0, n_centres, (n,), generator=gen, device="cuda")
    q = unit(centres[:8] + 0.15 * unit(torch.randn((8, DIM), generator=gen, device="cuda")))
    stream = torch.cuda.Stream()
    res = {"what": "measure_distinct", "rows": n, "calls": a.calls, "rounds": a.rounds, "same_at": SAME_AT}
    for storage in a.storage.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        for lo in range(0, n, 1 << 18):                   # in pieces: the f32 staging of a bf16 / i8 index stays small
            hi = min(n, lo + (1 << 18))
            E = unit(centres[member[lo:hi]] + 0.15 * unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda")))
            ix.add(E, tracks=None)
            del E
        torch.cuda.empty_cache()

        def page(qs, with_total=False):
            idx, sc, _ = ix.rank_device(qs, 0, 1024, tracks=False, with_total=False)
            return ix.distinct_device(idx, sc, SAME_AT, 0, 100, with_total=with_total)

        calls = {"A_rank_100": lambda qi: ix.rank_device(qi, 0, 100, tracks=False, with_total=False),
                 "B_rank_1024": lambda qi: ix.rank_device(qi, 0, 1024, tracks=False, with_total=False),
                 "C_distinct_page": lambda qi: page(qi),
                 "Ct_distinct_page_total": lambda qi: page(qi, True),
                 "B8_rank_1024_q8": lambda qi: ix.rank_device(q, 0, 1024, tracks=False, with_total=False),
                 "D_distinct_page_q8": lambda qi: page(q)}
        # what is timed is what the tests check: the device form answers as the host form, and the page really is thinned
        with torch.cuda.stream(stream):
            got = page(q[:1], True)
            hi_, hs_, _ = ix.rank(q[:1].cpu().numpy(), 0, 1024, tracks=False)
            want = ix.distinct(hi_, hs_, SAME_AT, 0, 100)
        stream.synchronize()
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[2]) and got[3][0] == want[3][0]
        res.setdefault("answers", {})[storage] = {"kept_of_1024": int(want[3][0]), "dups_of_first": int(want[2][0, 0])}
        if a.trace:
            with torch.cuda.stream(stream):
                for i in range(20):
                    page(q[i % 8:i % 8 + 1])
            stream.synchronize()
            ix.close()
            continue
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
        del ix
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
