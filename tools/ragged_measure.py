"""Measurements of the ragged batch (docs/measurement.md): python tools/ragged_measure.py entry|site|stem|stem_uniform"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearcam_amd.streams import MixedCameraBank, MixedStreamPipeline, StreamPipeline, make_cameras, parse_mix
from clearcam_amd.weights import synthetic_yolov9_state_dict
from clearcam_amd.yolov9 import YOLOv9

MIX = "1080x1920:32,720x1280:16,2160x3840:8,480x640:8"


def model():
    return YOLOv9("c", 640, state_dict=synthetic_yolov9_state_dict("c", 1234), dtype="f16h")


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def entry():
    m = model()
    B, H, W = 64, 1080, 1920
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, 300, 6), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(out)
    offs = np.arange(B, dtype=np.int64) * (H * W * 3)
    hs, ws = np.full(B, H, np.int32), np.full(B, W, np.int32)
    flat = frames.view(-1)
    uni = lambda: m.detect_batch_device(frames, out)
    rag = lambda: m.detect_ragged_device(flat, offs, hs, ws, out2)
    for _ in range(3):
        uni(); rag()
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "ragged entry != uniform entry"
    u, r = [], []
    for _ in range(7):
        u.append(timed(uni, 10)); r.append(timed(rag, 10))
    print(json.dumps({"what": "entry", "B": B, "uniform_ms": u, "ragged_ms": r, "uniform_median": statistics.median(u), "ragged_median": statistics.median(r),
                      "uniform_spread_pct": 100 * (max(u) - min(u)) / statistics.median(u), "ragged_spread_pct": 100 * (max(r) - min(r)) / statistics.median(r)}))


def site():
    sizes = parse_mix(MIX)
    m = model()
    ticks, reps = 20, 3
    res = {"what": "site", "mix": MIX, "mixed_fps": [], "per_size_fps": []}
    # new: one pipeline, one upload and two ragged batches per tick
    pipe = MixedStreamPipeline(m, sizes, depth=2)
    cams = MixedCameraBank(sizes, ring=3)
    for _ in range(reps):
        res["mixed_fps"].append(pipe.run(cams, ticks, warmup=2)["frames_per_sec"])
    res["mixed_h2d_GBps"] = pipe.run(cams, ticks, warmup=1)["h2d_GBps"]
    pipe.close()
    del pipe, cams
    # what the parent needs: one uniform pipeline per source size on the same handle, all running at the same time.  A handle takes
    # one submitting thread, so the pipelines are driven round robin from this thread, each with `depth` ticks in flight.
    by = {}
    for hw in sizes:
        by[hw] = by.get(hw, 0) + 1
    pipes = [(StreamPipeline(m, n, hw, depth=2, in_flight=False), make_cameras(n, hw[0], hw[1], ring=3)) for hw, n in by.items()]

    def run(n_ticks):
        for p, _ in pipes:
            p.latency, p.track_s, p.n_dets = [], 0.0, 0
        t0 = time.perf_counter()
        for i in range(n_ticks + 2):
            for p, c in pipes:
                if p.submitted - p.collected == p.depth or i >= n_ticks:
                    if p.collected < p.submitted:
                        p.collect()
                if i < n_ticks:
                    p.submit(c.read_all())
        for p, _ in pipes:
            while p.collected < p.submitted:
                p.collect()
        return n_ticks * len(sizes) / (time.perf_counter() - t0)
    run(3)
    for _ in range(reps):
        res["per_size_fps"].append(run(ticks))
    res["mixed_median"] = statistics.median(res["mixed_fps"]); res["per_size_median"] = statistics.median(res["per_size_fps"])
    print(json.dumps(res))


def stem(uniform):
    """A few replays of the 56-frame 384x640-class batch of the mix (or 56 x 1080p through the uniform entry) for the kernel trace."""
    m = model()
    sizes = [hw for hw in parse_mix(MIX) if m.network_shape(*hw) == (384, 640)]
    if uniform:
        sizes = [(1080, 1920)] * len(sizes)
    B = len(sizes)
    nbytes = [h * w * 3 for h, w in sizes]
    offs = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    flat = torch.randint(0, 256, (int(sum(nbytes)),), dtype=torch.uint8, device="cuda")
    out = torch.empty((B, 300, 6), dtype=torch.float32, device="cuda")
    hs, ws = np.asarray([h for h, _ in sizes], np.int32), np.asarray([w for _, w in sizes], np.int32)
    for _ in range(6):
        if uniform:
            m.detect_batch_device(flat.view(B, 1080, 1920, 3), out)
        else:
            m.detect_ragged_device(flat, offs, hs, ws, out)
    torch.cuda.synchronize()
    if not uniform:                                   # share of stem blocks that stage / read directly: the kernel's own per-tile test
        from oracle.yolov9_oracle import interp_axis_tables, letterbox_geometry
        SCR = 256 * 72 * 2
        staged = direct = 0
        per = {}
        for h, w in sorted(set(sizes)):
            nh, nw, py, px = letterbox_geometry(h, w, 640)
            xlo, xhi, _ = interp_axis_tables(w, nw); ylo, yhi, _ = interp_axis_tables(h, nh)
            s = d = 0
            for ty in range(12):
                for tx in range(20):
                    Y0, X0 = 32 * ty - 1, 32 * tx - 1
                    yy0, yy1 = max(Y0 - py, 0), min(Y0 + 32 - py, nh - 1)
                    xx0, xx1 = max(X0 - px, 0), min(X0 + 32 - px, nw - 1)
                    if yy0 > yy1 or xx0 > xx1:
                        d += 1; continue
                    nrows = yhi[yy1] - ylo[yy0] + 1; rowbytes = (xhi[xx1] - xlo[xx0] + 1) * 3
                    if nrows * ((rowbytes + 6) // 4) * 4 <= SCR: s += 1
                    else: d += 1
            n = sizes.count((h, w))
            per[f"{h}x{w}"] = {"frames": n, "staged_blocks_per_frame": s, "direct_blocks_per_frame": d}
            staged += s * n; direct += d * n
        print(json.dumps({"what": "stem_blocks", "B": B, "staged": staged, "direct": direct, "staged_share": staged / (staged + direct), "per_size": per}))


if __name__ == "__main__":
    {"entry": entry, "site": site, "stem": lambda: stem(False), "stem_uniform": lambda: stem(True)}[sys.argv[1]]()
