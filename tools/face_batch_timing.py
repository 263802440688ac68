"""Per-crop against batched face path (docs/measurement.md, "Faces for a batch of crops"):

    timeout 600 python tools/face_batch_timing.py [--counts 32,256] [--dtypes f32,bf16] [--warmup 3] [--reps 20]

The thirteen crops of tests/test_gpu_face_batch.py (eight show a face to the synthetic detector) tiled to each count, models built
from the seeded synthetic weights.  Two ways from crops to (n,512) embeddings, both wall time around synchronous calls:
  per crop   [img_to_face(c) for c in crops], then adaface.embed_batch of the faces found   (four host<->device round trips, a
             host border copy and a batch-1 BlazeFace graph per crop)
  batched    embed_faces(crops)                                                              (one upload, two device passes)
--warmup runs of each first (plans and graphs are built there), then the median of --reps.  One JSON line per result; figures
per crop."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearcam_amd.objects import ObjectFinder
from clearcam_amd.weights import synthetic_adaface_state_dict, synthetic_blazeface_state_dict

SHAPES = [(720, 960), (1280, 900), (500, 500), (640, 640), (1280, 1280), (1280, 960), (300, 200), (96, 128), (64, 64), (2, 2),
          (400, 1300), (1081, 607), (900, 1280)]


def per_crop(f, crops):
    faces = [f.img_to_face(c) for c in crops]
    valid = np.array([x is not None for x in faces])
    emb = np.zeros((len(crops), 512), np.float32)
    if valid.any():
        emb[valid] = f.adaface.embed_batch(np.stack([x for x in faces if x is not None]))
    return emb, valid


def timed(fn, warmup, reps):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms), max(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="32,256")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(20)
    base = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SHAPES]
    for dtype in a.dtypes.split(","):
        f = ObjectFinder()
        f.init_face(blazeface_kwargs=dict(state_dict=synthetic_blazeface_state_dict(555), dtype=dtype),
                    adaface_kwargs=dict(state_dict=synthetic_adaface_state_dict(777), dtype=dtype))
        for n in [int(c) for c in a.counts.split(",")]:
            crops = [base[i % len(base)] for i in range(n)]
            p50a, lo_a, hi_a, (emb_a, valid_a) = timed(lambda: per_crop(f, crops), a.warmup, a.reps)
            p50b, lo_b, hi_b, (emb_b, valid_b) = timed(lambda: f.embed_faces(crops), a.warmup, a.reps)
            same = bool(np.array_equal(valid_a, valid_b))
            print(json.dumps(dict(dtype=dtype, crops=n, faces=int(valid_b.sum()), warmup=a.warmup, reps=a.reps,
                                  per_crop_path_ms_per_crop=p50a / n, batched_ms_per_crop=p50b / n, speedup=p50a / p50b,
                                  per_crop_path_p50_min_max_ms=[p50a, lo_a, hi_a], batched_p50_min_max_ms=[p50b, lo_b, hi_b],
                                  same_faces_found=same,
                                  max_embedding_diff=float(np.abs(emb_a - emb_b).max()) if same else None)), flush=True)
        f.turn_off_face()


if __name__ == "__main__":
    main()
