"""Scan cost and score error of the index's storage modes (docs/measurement.md): python tools/index_storage_measure.py [--rows N] [--calls C]

One process, N x 768 unit rows (default 1 M) filled on the device, the same rows stored as f32, bf16 and i8, one after the other:
  search(q, 100) for Q = 1, 8 and 64 and search_tracks(q, 10) for Q = 1 on the world of tools/search_measure.py (about N / 20
  tracks, 20 folders): p50 of C calls after W warm-up calls, wall clock with the answer on the host, three repetitions each so that
  the spread is visible;
  effective GB/s of the Q = 1 search from the real row bytes (the select is inside that time);
  max and rms of |score - score_f32| over 8 queries and the top-100 overlap with the f32 index.
For i8 also the pass-width sweep: search(q, 100) with Q = 8 and 64 at cc_dev_set("index_i8_pass") = 1 .. 8 (what compute_scores'
default was chosen from) and the batch sweep: search(q, 100) for Q = 8 .. 256 with cc_dev_set("index_i8_mfma") at 0 (scan passes only)
and at 1 (the MFMA kernel of index_i8_mfma.hip), three repetitions each, from which compute_scores' threshold was chosen; bf16 rows
get the same Q column for comparison.  One JSON line per storage."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearcam_amd import _lib
from clearcam_amd.objects import EmbeddingIndex

DIM = 768
BATCHES = (8, 16, 24, 32, 48, 64, 128, 256)
ROW_BYTES = {"f32": DIM * 4, "bf16": DIM * 2, "i8": DIM + DIM // 8}


def unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def p50(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--storages", default="f32,bf16,i8")
    a = ap.parse_args()
    n = a.rows
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    q0 = unit(torch.randn(DIM, generator=gen, device="cuda"))
    queries = unit(q0 + 0.2 * torch.randn((64, DIM), generator=gen, device="cuda") / DIM ** 0.5).cpu().numpy()
    E = unit(torch.randn((n, DIM), generator=gen, device="cuda"))
    more = unit(q0 + 0.2 * torch.randn((BATCHES[-1] - 64, DIM), generator=gen, device="cuda") / DIM ** 0.5).cpu().numpy()
    queries = np.concatenate([queries, more])                      # the first 64 are those of the earlier columns
    rng = np.random.default_rng(1)
    slots = rng.integers(0, max(n // 20, 1), n).astype(np.int32)
    groups = rng.integers(0, 20, n).astype(np.int32)
    ref_scores = ref_top = None
    for storage in a.storages.split(","):
        ix = EmbeddingIndex(DIM, n, storage=storage)
        ix.add(E, groups, slots)
        torch.cuda.synchronize()
        res = {"what": "index_storage_measure", "storage": storage, "rows": n, "dim": DIM, "row_bytes": ROW_BYTES[storage], "calls": a.calls}
        for Q in (1, 8, 64):
            res[f"search_k100_q{Q}_p50_ms"] = [round(p50(lambda: ix.search(queries[:Q], 100), a.calls, a.warmup), 4) for _ in range(a.reps)]
        res["search_tracks_k10_q1_p50_ms"] = [round(p50(lambda: ix.search_tracks(queries[:1], 10), a.calls, a.warmup), 4) for _ in range(a.reps)]
        res["search_q1_effective_GBps"] = [round(n * ROW_BYTES[storage] / (ms * 1e-3) / 1e9, 1) for ms in res["search_k100_q1_p50_ms"]]
        sc = ix.scores(queries[:8])
        top = ix.search(queries[:8], 100)[0]
        if storage == "f32":
            ref_scores, ref_top = sc, top
        elif ref_scores is not None:
            err = np.abs(sc.astype(np.float64) - ref_scores)
            res["score_err_max"] = float(err.max())
            res["score_err_rms"] = float(np.sqrt((err ** 2).mean()))
            res["top100_overlap_min_mean"] = [min(len(set(x) & set(y)) for x, y in zip(top, ref_top)),
                                              float(np.mean([len(set(x) & set(y)) for x, y in zip(top, ref_top)]))]
        def batch_column():
            return {f"q{Q}": [round(p50(lambda: ix.search(queries[:Q], 100), a.calls, a.warmup), 4) for _ in range(a.reps)] for Q in BATCHES}

        if storage == "bf16":
            res["batch_sweep_p50_ms"] = batch_column()
        if storage == "i8":
            res["batch_sweep_p50_ms"] = {}
            for key, name in ((0, "scan"), (1, "mfma")):
                _lib.check(_lib.lib().cc_dev_set(b"index_i8_mfma", key))
                res["batch_sweep_p50_ms"][name] = batch_column()
                assert ix.last_scores_path() == (2 if key else 0)
            _lib.check(_lib.lib().cc_dev_set(b"index_i8_mfma", -1))
            sweep = {}
            _lib.check(_lib.lib().cc_dev_set(b"index_i8_mfma", 0))      # the pass width is a property of the scan passes
            for w in range(1, 9):
                _lib.check(_lib.lib().cc_dev_set(b"index_i8_pass", w))
                sweep[str(w)] = {f"q{Q}": round(p50(lambda: ix.search(queries[:Q], 100), a.calls, a.warmup), 4) for Q in (8, 64)}
            _lib.check(_lib.lib().cc_dev_set(b"index_i8_pass", -1))
            _lib.check(_lib.lib().cc_dev_set(b"index_i8_mfma", -1))
            res["pass_width_sweep_p50_ms"] = sweep
        print(json.dumps(res), flush=True)
        ix.close()
        del ix
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
