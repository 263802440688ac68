"""What "together" costs on the device (docs/measurement.md, "Together"):

    python tools/dev/measure_near.py [--rows N] [--storage f32,bf16,i8] [--calls C] [--big-calls B] [--rounds R] [--warmup W] [--limit SECONDS] [--no-host]

The world of tools/dev/measure_sightings.py: per storage N x 768 crops (default 1 M) in 24 groups, filled on the device; every group has
500 objects of its own, a crop is its object's centre with noise, groups and objects drawn at random per row.  Every row has a ts: the
rows of a folder are spread over a day, each at a second of its own, so that within = 0 pairs nothing (two rows of one folder never
share a second) while within = 30 pairs a quarter of the rows with one of the 1 % of rows that pass B's cut (a ninth of them with one
of the best 4096).  No track slots.
Timed with hipEvents on the stream the calls run on, results left on the device, no totals asked for (so nothing waits); R rounds that
alternate the calls, per call the median over all rounds and the span of the round medians:
  A      rank(0, 100) of one query over all folders                      the yardstick: a page of `rank`
  N<P>   rank_near(a, b, within 30, 0, 100) with partners = P in 1024 / 4096 / 16384, cut_b at the 99th percentile of b's scores
  W<P>   the same with within = 0: nothing qualifies anywhere, every row walks the whole list (the worst case for that list; the cut
         leaves about 10 000 rows, so the list of the 16384 leg is that long)
  X      W16384 without the cut: the list is full, 1 M rows walk 16384 entries each - the worst case of the call
  B      digest of the WHOLE index with the cap of 1024 leaders reached  the most expensive call the index documents
  H      what N4096 costs without the call: two `rank` calls fetched whole (a: every row, b: the list) and the join in numpy, per folder
         one (rows, entries) matrix of |dt| <= within (once; wall clock).  Its first page is compared with N4096's.
Per leg: ms and the multiple of A.  The bar for the default `partners`: X costs no more than B in the same run, per storage.
Before timing the device form is checked against the host form.  One JSON line out per storage, and one for the whole run."""
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
DAY = 86400
WITHIN = 30
PARTNERS = (1024, 4096, 16384)


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def host_join(ix, qa, qb, cut_b, partners, within, group, ts, n):
    """Two rankings fetched whole and joined on the host -> (the first 100 rows of the joined ranking, value min, living rows)"""
    ia, sa, ta = ix.rank(qa, 0, n, tracks=False)
    ib, sb, tb = ix.rank(qb, 0, partners, min_score=cut_b, tracks=False)
    ib, sb = ib[0][ib[0] >= 0].astype(np.int64), sb[0][ib[0] >= 0]
    Sa = np.empty(n, np.float32)
    Sa[ia[0]] = sa[0]
    v = np.full(n, -np.inf, np.float32)
    for g in np.unique(group[ib]):                        # the entries of a folder stay in list order: the first qualifying one is the best
        at = group[ib] == g
        P, Sp = ib[at], sb[at]
        R = np.flatnonzero(group == g)
        near = np.abs(ts[P].astype(np.int64)[None, :] - ts[R].astype(np.int64)[:, None]) <= within
        near &= P[None, :] != R[:, None]
        hit = near.any(axis=1)
        v[R[hit]] = np.minimum(Sa[R[hit]], Sp[near.argmax(axis=1)[hit]])
    order = np.lexsort((np.arange(n), -v))[:100]
    return order[np.isfinite(v[order])], int(np.isfinite(v).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--storage", default="f32,bf16,i8")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--big-calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=840)
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
    group_h = group.cpu().numpy().astype(np.int32)
    rng = np.random.default_rng(11)
    ts_h = np.empty(n, np.int32)
    for g in range(GROUPS):                               # a folder's rows over its day, no second twice
        rows = np.flatnonzero(group_h == g)
        assert rows.size <= DAY, "more rows in a folder than seconds in its day"
        ts_h[rows] = rng.permutation(DAY)[:rows.size]
    qa = unit(centres[:1] + 0.15 * unit(torch.randn((1, DIM), generator=gen, device="cuda")))
    qb = unit(centres[OBJECTS + 7:OBJECTS + 8] + 0.15 * unit(torch.randn((1, DIM), generator=gen, device="cuda")))
    qa_h, qb_h = qa.cpu().numpy()[0], qb.cpu().numpy()[0]
    stream = torch.cuda.Stream()
    res = {"what": "measure_near", "rows": n, "calls": a.calls, "big_calls": a.big_calls, "rounds": a.rounds, "within": WITHIN, "same_at": SAME_AT}
    for storage in a.storage.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        for lo in range(0, n, 1 << 18):                   # in pieces: the f32 staging of a bf16 / i8 index stays small
            hi = min(n, lo + (1 << 18))
            E = unit(centres[group[lo:hi] * OBJECTS + obj[lo:hi]] + 0.15 * unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda")))
            ix.add(E, groups=group_h[lo:hi], ts=ts_h[lo:hi])
            del E
        torch.cuda.empty_cache()
        big = ix.digest(SAME_AT, 0, 1024, by="first")
        assert int(big[4][0]) == 1024 and int(big[4][2]) > 0   # B is the capped digest
        cut_b = float(np.quantile(ix.scores(qb_h)[0], 0.99))   # about 1 % of the rows pass
        ask = dict(a=qa, b=qb, start=0, count=100, cut_b=cut_b, tracks=False)
        legs = {"A_rank_100": (a.calls, lambda: ix.rank_device(qa, 0, 100, tracks=False, with_total=False))}
        for p in PARTNERS:
            legs[f"N{p}_within_{WITHIN}"] = (a.calls, lambda p=p: ix.rank_near_device(within=WITHIN, partners=p, with_total=False, **ask))
        for p in PARTNERS:
            legs[f"W{p}_within_0"] = (a.calls, lambda p=p: ix.rank_near_device(within=0, partners=p, with_total=False, **ask))
        legs["X16384_within_0_no_cut"] = (a.calls, lambda: ix.rank_near_device(within=0, partners=16384, with_total=False, **dict(ask, cut_b=None)))
        legs["B_digest_all_capped"] = (a.big_calls, lambda: ix.digest_device(SAME_AT, 0, 100, with_total=False))
        # what is timed is what the tests check: the device form answers as the host form
        answers = {}
        for p in PARTNERS:
            for within in (WITHIN, 0):
                with torch.cuda.stream(stream):
                    got = ix.rank_near_device(within=within, partners=p, **ask)
                stream.synchronize()
                want = ix.rank_near(qa_h, qb_h, within, 0, 100, partners=p, cut_b=cut_b, tracks=False)
                for i in (0, 1, 3, 4):
                    assert got[i].cpu().numpy().tobytes() == want[i].tobytes(), (storage, p, within)
                assert got[2][0] == want[2][0] and got[5] == want[5]
                answers[f"{p}_within_{within}"] = {"total": int(want[2][0]), "n_partners": int(want[5])}
                assert within or want[2][0] == 0           # within = 0: nothing pairs, every row walked the whole list
        want = ix.rank_near(qa_h, qb_h, 0, 0, 100, partners=16384, tracks=False)
        assert want[2][0] == 0 and want[5] == n              # X: every row is in B's ranking, the list is full, nothing pairs
        answers["16384_within_0_no_cut"] = {"total": int(want[2][0]), "n_partners": int(want[5])}
        res.setdefault("answers", {})[storage] = answers
        host = None
        if not a.no_host:                                 # H: two rankings fetched whole, the join in numpy
            t0 = time.perf_counter()
            first, living = host_join(ix, qa_h, qb_h, cut_b, 4096, WITHIN, group_h, ts_h, n)
            wall = time.perf_counter() - t0
            want = ix.rank_near(qa_h, qb_h, WITHIN, 0, 100, partners=4096, cut_b=cut_b, tracks=False)
            host = {"wall_ms": round(wall * 1e3, 1), "living": living, "total_agrees": bool(living == int(want[2][0])),
                    "first_page_agrees": bool(np.array_equal(first, want[0][0][want[0][0] >= 0]))}
        per_round = {k_: [] for k_ in legs}
        every = {k_: [] for k_ in legs}
        with torch.cuda.stream(stream):
            for r in range(a.rounds):
                for name, (reps, fn) in legs.items():     # A, N.., W.., B, A, ...: drift hits all of them alike
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
        out = {"cut_b": round(cut_b, 5)}
        for name in legs:
            p50 = statistics.median(every[name])
            out[name] = {"p50_ms": round(p50, 4), "round_p50_min_ms": round(min(per_round[name]), 4), "round_p50_max_ms": round(max(per_round[name]), 4),
                         "min_ms": round(min(every[name]), 4)}
        for name in legs:
            out[name]["of_rank"] = round(out[name]["p50_ms"] / out["A_rank_100"]["p50_ms"], 2)
        for p in PARTNERS:
            out[f"bar_W{p}_le_B"] = bool(out[f"W{p}_within_0"]["p50_ms"] <= out["B_digest_all_capped"]["p50_ms"])
        out["bar_X_le_B"] = bool(out["X16384_within_0_no_cut"]["p50_ms"] <= out["B_digest_all_capped"]["p50_ms"])
        if host is not None:
            out["H_two_ranks_and_numpy"] = host
        res[storage] = out
        print(json.dumps({storage: out}), flush=True)
        ix.close()
        del ix
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
