"""Cost of removing rows from a large resident index (docs/measurement.md, "Removing rows"):

    python tools/index_remove_measure.py [--rows N] [--reps R] [--storages f32,bf16] [--sweep 8192,16384,...] [--only-remove]

N x 768 rows (default 1 M) generated on the device, 16 cameras x 50 days of groups in the order live appends produce (days one
after the other, the cameras interleaved inside a day), 50 k tracks.  Three removals, each on a freshly filled index:
  i    the oldest day of every camera   (2 %, the head of the matrix)        remove_groups
  ii   one whole camera                 (6.25 %, scattered)                  remove_groups
  iii  half of the rows at random       (50 %)                               remove (a host mask)
Per removal: median of R wall times around the synchronous call, and the survivors' bytes read + written per second.  The index is
rebuilt between repetitions, so each is the first removal of its handle and allocates the handle's scratch (the bounce slab: 96 MB).
Yardsticks in the same process:
  A    hipMemcpy device-to-device of the surviving bytes (the same read + write traffic; what growth does)
  B    what exists without removal: a new EmbeddingIndex + add() of the survivors, from device memory and from a host array
The host side (`_RowTable.remove`, a Python pass over the paths) is timed separately, once per removal.
--sweep times ii and iii at several slab sizes (cc_dev_set("index_slab_rows")); --only-remove runs the removals alone (the form to
put behind `rocprofv3 --kernel-trace --stats --`).  One JSON line per result."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clearcam_amd import _lib
from clearcam_amd.objects import EmbeddingIndex, _RowTable

DIM, CAMS, DAYS = 768, 16, 50


def say(**kw):
    print(json.dumps(kw), flush=True)


def world(n):
    rng = np.random.default_rng(3)
    day = (np.arange(n) * DAYS // n).astype(np.int32)                  # time order
    cam = rng.integers(0, CAMS, n).astype(np.int32)                    # the cameras of one day interleave
    group = 1 + cam * DAYS + day
    slot = rng.integers(0, max(n // 20, 1), n).astype(np.int32)
    drops = {"i oldest day of every camera": ("groups", day == 0), "ii one camera": ("groups", cam == 3),
             "iii random half": ("rows", rng.random(n) < 0.5)}
    return cam, day, group, slot, drops


def group_table(group, mask):
    t = np.zeros(int(group.max()) + 1, np.uint8)
    t[np.unique(group[mask])] = 1
    return t


def filled(E, group, slot, storage):
    ix = EmbeddingIndex(DIM, E.shape[0], storage=storage)
    ix.add(E, group, slot)
    return ix


def remove(ix, kind, mask, table):
    t0 = time.perf_counter()
    n = ix.remove_groups(table) if kind == "groups" else ix.remove(mask)
    return 1e3 * (time.perf_counter() - t0), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--storages", default="f32,bf16")
    ap.add_argument("--sweep", default="")
    ap.add_argument("--only-remove", action="store_true")
    a = ap.parse_args()
    n = a.rows
    L = _lib.lib()
    gen = torch.Generator(device="cuda"); gen.manual_seed(9)
    E = torch.randn((n, DIM), generator=gen, device="cuda")
    E /= E.norm(dim=-1, keepdim=True)
    cam, day, group, slot, drops = world(n)
    q = E[:2].cpu().numpy()
    for storage in a.storages.split(","):
        rb = DIM * (4 if storage == "f32" else 2)
        for name, (kind, mask) in drops.items():
            table = group_table(group, mask) if kind == "groups" else None
            live = int(n - mask.sum())
            ms = []
            for _ in range(a.reps):
                ix = filled(E, group, slot, storage)
                t, removed = remove(ix, kind, mask, table)
                assert removed == n - live and len(ix) == live
                ms.append(t)
                ix.close()
            med = statistics.median(ms)
            say(what="remove", storage=storage, removal=name, rows=n, removed=n - live, p50_ms=med, min_ms=min(ms), max_ms=max(ms),
                survivor_bytes_rw_per_s=2 * live * rb / (med * 1e-3))
            if a.only_remove:
                continue
            # A: the surviving bytes copied device to device
            src = torch.empty(live * rb, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src)
            cp = []
            for _ in range(a.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = L.hipMemcpy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), C.c_size_t(live * rb), 3)
                torch.cuda.synchronize()
                cp.append(1e3 * (time.perf_counter() - t0))
                assert rc == 0
            del src, dst
            a_ms = statistics.median(cp[1:])
            say(what="yardstick A: hipMemcpy D2D of the survivors", storage=storage, removal=name, p50_ms=a_ms,
                bytes_rw_per_s=2 * live * rb / (a_ms * 1e-3), remove_over_A=med / a_ms)
            # B: a new index from the survivors (gathered beforehand: the caller is taken to have them ready)
            keep = np.flatnonzero(~mask)
            Es = E[torch.as_tensor(keep, device="cuda")]
            gs, ss = group[keep], slot[keep]
            bd = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ix2 = filled(Es, gs, ss, storage)
                bd.append(1e3 * (time.perf_counter() - t0))
                ix2.close()
            b_dev = statistics.median(bd)
            Eh = Es.cpu().numpy()
            del Es
            t0 = time.perf_counter()
            ix2 = filled(Eh, gs, ss, storage)
            b_host = 1e3 * (time.perf_counter() - t0)
            # and the removal's answers are those of the rebuilt index
            ix = filled(E, group, slot, storage)
            remove(ix, kind, mask, table)
            same = all(np.array_equal(x, y) for x, y in zip(ix.search_tracks(q, 100), ix2.search_tracks(q, 100)))
            ix.close(); ix2.close()
            del Eh
            say(what="yardstick B: new index + add of the survivors", storage=storage, removal=name, from_device_p50_ms=b_dev,
                from_host_ms=b_host, B_device_over_remove=b_dev / med, B_host_over_remove=b_host / med, same_answers=same)
        torch.cuda.empty_cache()
    if a.sweep and not a.only_remove:
        for T in [int(t) for t in a.sweep.split(",")]:
            _lib.check(L.cc_dev_set(b"index_slab_rows", T))
            for storage in a.storages.split(","):
                for name, (kind, mask) in list(drops.items())[1:]:
                    table = group_table(group, mask) if kind == "groups" else None
                    ms = []
                    for _ in range(3):
                        ix = filled(E, group, slot, storage)
                        ms.append(remove(ix, kind, mask, table)[0])
                        ix.close()
                    say(what="slab sweep", slab_rows=T, storage=storage, removal=name, p50_ms=statistics.median(ms), min_ms=min(ms))
        _lib.check(L.cc_dev_set(b"index_slab_rows", -1))
    if not a.only_remove:
        paths = [f"data/cameras/cam{c}/objects/2026-{1 + d // 28:02d}-{1 + d % 28:02d}/{1700000000 + i}.0_{t}_2.jpg"
                 for i, (c, d, t) in enumerate(zip(cam.tolist(), day.tolist(), slot.tolist()))]
        for name, (kind, mask) in drops.items():
            t = _RowTable()
            t0 = time.perf_counter()
            t.extend(paths)
            built = time.perf_counter() - t0
            t0 = time.perf_counter()
            t.remove(mask)
            say(what="host: _RowTable.remove", removal=name, rows=n, seconds=time.perf_counter() - t0, build_seconds=built)


if __name__ == "__main__":
    main()
