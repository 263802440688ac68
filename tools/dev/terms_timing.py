"""What a compound search costs on the device beside the calls it is made of (docs/measurement.md, "Compound search"):

    python tools/dev/terms_timing.py [--rows N] [--storage f32] [--calls C] [--rounds R] [--warmup W] [--limit SECONDS]

The world of tools/dev/like_timing.py for ONE storage per process: N x 768 crops (default 1 M) filled on the device, 50 k tracks of
about 20 crops, 5 % of the rows without a track id, 20 groups, one planted track of 64 crops in one group, a ts per row.  Timed with
hipEvents on the stream the calls run on, results left on the device and no total asked for, so a call waits for nothing on the
host; R rounds that alternate the calls, C calls each after W warm-up calls, per call the median over all rounds and the span of the
round medians:
  A  rank(0, 100), one query on the device                              the yardstick of a one-vector question
  D  rank_like(the 64 rows of the track, 0, 100, exclude=track)         the yardstick of a 64-row question
  F  rank_terms, one vector RANK term                                   A's launches
  G  rank_terms, the same 64 rows as RANK terms, MAX, track excluded,   D's launches (the same terms_fold_kernel), one more
     which asked for                                                    byte a row stored, and the gather of 100 entries
  H  rank_terms, a text RANK term, 8 stored REJECT rows, one REQUIRE    ten terms scored by scan passes (below the GEMM / MFMA thresholds), one fold
     vector
  I  timeline_terms of H, 24 bins                                       H's scoring and fold, the histogram in place of the selection
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


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--storage", default="f32")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240)
    a = ap.parse_args()
    signal.alarm(a.limit)                                 # the default action of SIGALRM ends the process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from clearcam_amd.objects import EmbeddingIndex
    n, storage = a.rows, a.storage
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    rng = np.random.default_rng(1)
    q = unit(torch.randn((8, DIM), generator=gen, device="cuda"))
    n_tracks = max(n // 20, 1)
    slot = rng.integers(0, n_tracks, n).astype(np.int32)
    slot[rng.random(n) < 0.05] = -1
    group = rng.integers(1, 21, n).astype(np.int32)
    ts = rng.integers(0, 86400, n).astype(np.int32)
    track = (1000 + (n - 2000) // 64 * np.arange(64)).astype(np.int64)   # the planted track: 64 crops of one folder, spread over the matrix
    slot[track], group[track] = n_tracks, 1
    stream = torch.cuda.Stream()
    ix = EmbeddingIndex(DIM, n, storage=storage)
    for lo in range(0, n, 1 << 18):                       # in pieces: the f32 staging of a bf16 / i8 index stays small
        hi = min(n, lo + (1 << 18))
        E = unit(torch.randn((hi - lo, DIM), generator=gen, device="cuda"))
        ix.add(E, group[lo:hi], slot[lo:hi], ts=ts[lo:hi])
        del E
    torch.cuda.empty_cache()
    # H: "this text, none of these eight crops, and it must look a little like that vector".  The cuts come from the scores themselves:
    # a REJECT row kills its nearest 0.1 % of the rows, the REQUIRE vector spares its upper half.
    rejected = track[::8]
    S = ix.scores(np.vstack([q[7:8].cpu().numpy(), ix.fetch(rejected)]))
    h_roles = ["rank", "require"] + ["reject"] * 8
    h_cuts = [None, float(np.median(S[0]))] + [float(np.quantile(S[1 + i], 0.999)) for i in range(8)]
    del S

    def h_vectors(qi):
        return torch.cat([qi, q[7:8]])

    h = dict(rows=rejected, roles=h_roles, cuts=h_cuts)
    calls = {"A_rank_1": lambda qi: ix.rank_device(qi, 0, 100, with_total=False),
             "D_like_64_track": lambda qi: ix.rank_like_device(track, 0, 100, exclude="track", with_total=False),
             "F_terms_1": lambda qi: ix.rank_terms_device(q=qi, start=0, count=100, with_total=False),
             "G_terms_64_track_which": lambda qi: ix.rank_terms_device(rows=track, start=0, count=100, exclude="track", which=True, with_total=False),
             "H_terms_text_8_reject_require": lambda qi: ix.rank_terms_device(q=h_vectors(qi), start=0, count=100, with_total=False, **h),
             "I_timeline_of_H": None}
    # what is timed is what the tests check: F answers as A does, G as D does, H hides the rejected crops
    a1, f1 = ix.rank(q[:1].cpu().numpy(), 0, 100), ix.rank_terms(q=q[:1].cpu().numpy(), start=0, count=100)
    assert all(np.array_equal(x, y) for x, y in zip(a1, f1))
    d1, g1 = ix.rank_like(track, 0, 100, exclude="track"), ix.rank_terms(rows=track, start=0, count=100, exclude="track", which=True)
    g_path = ix.last_scores_path()
    assert all(np.array_equal(x, y) for x, y in zip(d1, g1[:3])) and (g1[3] >= 0).all() and (g1[3] < 64).all()
    h1 = ix.rank_terms(q=h_vectors(q[:1]).cpu().numpy(), start=0, count=100, **h)
    h_path = ix.last_scores_path()
    i1 = ix.timeline_terms(0, 3600, 24, q=h_vectors(q[:1]).cpu().numpy(), **h)
    assert not set(h1[0][0].tolist()) & set(rejected.tolist()) and i1[1][0] == h1[2][0] and i1[0].sum() == h1[2][0]
    res = {"what": "terms_timing", "rows": n, "storage": storage, "calls": a.calls, "rounds": a.rounds,
           "answers": {"A_total": int(a1[2][0]), "D_total": int(d1[2][0]), "G_path": g_path, "H_total": int(h1[2][0]), "H_path": h_path}}
    # the timeline leaves its 24 counters on the device too: the library call itself, as EmbeddingIndex.timeline_terms is a host call
    import ctypes as C
    from clearcam_amd import _lib
    counts = torch.zeros((1, 24), dtype=torch.int32, device="cuda")
    _, ids, terms, comb, flags = ix._terms(np.zeros((2, DIM), np.float32), rejected, h_roles, None, h_cuts, "max", None, True)

    def timeline(qi):
        v = h_vectors(qi).contiguous()
        _lib.check(_lib.lib().cc_index_timeline_terms(ix._h, _lib.ptr(v), 2, ids.ctypes.data_as(C.POINTER(C.c_int64)), int(ids.size), terms, comb,
                                                      float("-inf"), flags, None, 0, None, 0, 3600, 24, _lib.ptr(counts), None, 1, C.c_void_p(stream.cuda_stream)))
        v.record_stream(stream)

    calls["I_timeline_of_H"] = timeline
    with torch.cuda.stream(stream):
        timeline(q[:1])
    stream.synchronize()
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), i1[0])
    per_round = {k: [] for k in calls}
    every = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for r in range(a.rounds):
            for name, fn in calls.items():                # A, D, F, ..., A, D, F, ...: drift hits all of them alike
                for i in range(a.warmup):
                    fn(q[i % 7:i % 7 + 1])
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
                for i, (e0, e1) in enumerate(ev):
                    e0.record(stream)
                    fn(q[i % 7:i % 7 + 1])
                    e1.record(stream)
                stream.synchronize()
                ms = [e0.elapsed_time(e1) for e0, e1 in ev]
                per_round[name].append(statistics.median(ms))
                every[name] += ms
    res["ms"] = {k: {"p50_ms": round(statistics.median(every[k]), 4), "round_p50_min_ms": round(min(per_round[k]), 4),
                     "round_p50_max_ms": round(max(per_round[k]), 4), "min_ms": round(min(every[k]), 4)} for k in calls}
    print(json.dumps(res), flush=True)
    ix.close()


if __name__ == "__main__":
    main()
