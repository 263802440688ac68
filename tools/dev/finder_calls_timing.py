"""What ObjectFinder's Python layer costs per call, with no GPU and no library: each of the ten questions over the recording stub index
of tests/test_finder_calls_host.py (docs/measurement.md, "One question path through ObjectFinder").

    python tools/dev/finder_calls_timing.py [--calls N] [--warmup W]

p50 of N calls (default 5000) per question after W warm-up calls, wall clock, in microseconds; under "min" the fastest call of each,
which a machine that changes its clock between calls leaves alone.  One JSON line out.  To compare two
commits, run it in alternating processes, one per tree."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_finder_calls_host as T  # noqa: E402

ONE_EACH = ("search tracks", "page", "timeline", "similar", "compound", "compound_timeline", "together", "together_timeline", "digest", "seen_before")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=200)
    a = ap.parse_args()
    cases = {c[0]: c for c in T.CASES}
    res = {"what": "finder_calls", "calls": a.calls, "min": {}}
    for name in ONE_EACH:
        _, world, hidden, question, args, kw = cases[name]
        f, events = T.finder(world, hidden)
        ask = getattr(f, question)
        us = []
        for i in range(a.warmup + a.calls):
            del events[:]
            t0 = time.perf_counter()
            ask(*args, **kw)
            us.append(1e6 * (time.perf_counter() - t0))
        res[question] = round(statistics.median(us[a.warmup:]), 2)
        res["min"][question] = round(min(us[a.warmup:]), 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
