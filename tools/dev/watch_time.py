"""dev tool: what the alerts cost at ingest (docs/measurement.md, "Alerts at ingest").

For (B, A) = (255, 16), (255, 256), (255, 2048), (1, 16) with the batch's embeddings resident on the device:
  match     WatchList.match -> host pairs: host clock around the call, which ends in a stream synchronise; median / p10 / p90
  enqueue   WatchList.match(device_out=True), N calls back to back between two device events: device time per call, nothing waited for
  host      what the same answer costs without the device path: download the (B, 768) embeddings, numpy product, the walk on the host
and, unless --skip-clip, the ViT-L/14 image tower on a 255-crop batch (bf16, synthetic weights) in the same run, so that the share of
the batch the alerts cost can be read off.  Kernel split: put the script behind `rocprofv3 --kernel-trace --stats --` with --skip-clip."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from clearcam_amd.objects import WatchList  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--skip-clip", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
CAMS = 16


def unit(rng, n):
    x = rng.standard_normal((n, 768)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def host_walk(S, thr, alert_group, crop_group):
    """The reference's walk over a score matrix, one vector operation per crop."""
    live = np.ones(S.shape[1], bool)
    out = []
    for b in range(S.shape[0]):
        w = (S[b] > thr) & (alert_group == crop_group[b]) & live
        if w.any():
            a = int(np.argmax(w))
            live[a] = False
            out.append((b, a, float(S[b, a])))
    return out


def pct(v):
    v = np.sort(np.asarray(v)) * 1e3
    return f"{np.median(v):8.3f} ms (p10 {v[len(v) // 10]:.3f}, p90 {v[len(v) * 9 // 10]:.3f})"


w = WatchList(768)
for B, A in ((255, 16), (255, 256), (255, 2048), (1, 16)):
    rng = np.random.default_rng(B * 10000 + A)
    E, D = unit(rng, B), unit(rng, A)
    alert_group = rng.integers(0, CAMS, A).astype(np.int32)
    crop_group = rng.integers(0, CAMS, B).astype(np.int32)
    thr = np.zeros(A, np.float32)                          # unit-normal rows: half of the pairs of a camera pass
    w.set(D, thr, alert_group)
    emb = torch.as_tensor(E).to(dev)
    torch.cuda.synchronize()
    for _ in range(10):
        alert, score = w.match(emb, crop_group)
        w.match(emb, crop_group, device_out=True)
    torch.cuda.synchronize()
    t_match = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        alert, score = w.match(emb, crop_group)
        t_match.append(time.perf_counter() - t0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.calls):
        w.match(emb, crop_group, device_out=True)
    e1.record()
    t_enq = (time.perf_counter() - t0) / args.calls
    torch.cuda.synchronize()
    t_dev = e0.elapsed_time(e1) / args.calls
    t_host = []
    for _ in range(max(100, args.calls // 2)):
        t0 = time.perf_counter()
        Eh = emb.cpu().numpy()
        ref = host_walk(Eh @ D.T, thr, alert_group, crop_group)
        t_host.append(time.perf_counter() - t0)
    fired = int((alert >= 0).sum())
    same = [b for b, _, _ in ref] == np.flatnonzero(alert >= 0).tolist() and [a for _, a, _ in ref] == alert[alert >= 0].tolist()
    print(f"B {B:3d} A {A:4d} ({fired} fired, host walk agrees: {same}): match {pct(t_match)} | device_out: {t_dev:.4f} ms device per call, {t_enq * 1e3:.4f} ms host per enqueue"
          f" | host path {pct(t_host)}", flush=True)
w.close()

if not args.skip_clip:
    from clearcam_amd.arch import CLIP_L14
    from clearcam_amd.objects import OpenCLIP
    from clearcam_amd.weights import synthetic_clip_state_dict
    m = OpenCLIP(state_dict=synthetic_clip_state_dict(CLIP_L14, 4321), arch=CLIP_L14, dtype="bf16", device=0)
    x = torch.rand(255, 3, 224, 224, device=dev) * 2 - 1
    out = torch.empty(255, 768, device=dev)
    for _ in range(2):
        m.precompute_embedding_device(x, out)
    torch.cuda.synchronize()
    ts = []
    for _ in range(6):
        t0 = time.perf_counter()
        m.precompute_embedding_device(x, out)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print(f"CLIP ViT-L/14 image tower, B 255 bf16: {np.median(ts) * 1e3:.2f} ms a batch ({255 / np.median(ts):.0f} images/s)", flush=True)
