"""Every conv of the shipped detector plan, recomputed in float64 from the GPU's own inputs (tests/restart_check.py).

The per-kernel tests force one variant at reduced shapes and the end-to-end 16-bit bars are statistical; neither sees a kernel that is
wrong in one tile of one frame.  Here the plan runs as bench.py runs it - YOLOv9-C, dtype "f16h", B = 64, 640 x 640, the conditioned
checkpoint with un-rounded weights - once as shipped and once with the parity taps on (CLEARCAM_TAP_BLOCKS / _CSP / _STEM keep every
block's tensors alive, which changes the arena layout); the two runs must agree bit for bit on the decoded rows and P3-P5, which ties the
tapped run to the shipped computation, buffer sharing included.  Frames 0, 31 and 63 of every tap are then restarted launch by launch:
every element of a single conv launch must be one of the two f16 values around the float64 result, with the rates and midpoint distances
of f32 accumulation noise (restart_check.check).  Units no tap splits - the fused hidden-32 RepNCSP (csp_tile_kernel), SPPELAN and the
DDetect tail - are restarted whole with their intermediate roundings emulated and held to relaxed bars.  Plan B is the reference's
batch-1 call (a 1080 x 1920 frame letterboxed to 384 x 640: the few-tile and small-pixel-tile kernels); plan C (bf16, B = 64, one plane
everywhere) runs under CLEARCAM_TEST_FULL=1.

Measured on the MI355X (plan A: 3 frames x 100 launches, plan B: 84; f16h), worst launch of each kind; the bars (BARS) are ~3x these:
  single launch, own inputs   differ 0.105 % of a tensor, 0.59 % of a 16x16x32 cell, p99 midpoint distance 0.0009 ulp, max 0.501 ulp
                              (every element one of the two f16 values around y64; typical differing share 0.03-0.1 %)
  bottleneck cv1              from the RECOMPUTED `a` (the GPU's was overwritten in place): 1.47 %, cell 3.1 %, within 0.76 ulp
  a + cv2(t), in place        residual = the recomputed `a`: 0.098 %, cell 0.39 %, within 2.2 ulps
  chained units               fused RepNCSP (csp_tile_kernel) / SPPELAN: 3.6 %, cell 14.5 %, within 1.5 ulps
  DDetect tail                anchors over the threshold in both: boxes within 0.0134 px, scores within 3.6e-5, same classes
"""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import restart_check as rc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = {"CLEARCAM_TAP_BLOCKS": "1", "CLEARCAM_TAP_CSP": "1", "CLEARCAM_TAP_STEM": "1"}
NAMES = (["input", "stem", "b1", "p3", "p4", "p5", "decoded"] + [f"b{i}" for i in (2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 19)]
         + [f"cat{i}" for i in range(8)] + [f"csp{i}_{s}" for i in range(16) for s in ("ab", "t", "u")])

# bars by kind of check: R, R_cell (per 16x16x32 cell), D (p99 midpoint distance, ulps; None: not held), ulps (None: strict bar 1)
BARS = {"single": dict(R=rc.BARS["R"], R_cell=rc.BARS["R_cell"], D=rc.BARS["D"], ulps=None),
        "from_a": dict(R=4.5e-2, R_cell=0.1, D=None, ulps=2.0),
        "residual": dict(R=3e-3, R_cell=1.5e-2, D=None, ulps=6.0),
        "chained": dict(R=0.11, R_cell=0.45, D=None, ulps=4.5)}
BOX_PX, SCORE = 0.04, 1e-4                                 # DDetect tail: 16x below the end-to-end 0.64 px bar

_RUN = r"""
import hashlib, sys, numpy as np
from clearcam_amd.weights import conditioned_yolov9_state_dict
from clearcam_amd.yolov9 import YOLOv9
dtype, B, H, W, res, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), sys.argv[6]
frames, names = [int(v) for v in sys.argv[7].split(",") if v], [n for n in sys.argv[8].split(",") if n]
fr = np.random.default_rng(1).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
m = YOLOv9("c", res, state_dict=conditioned_yolov9_state_dict("c", 1234, exact=False), dtype=dtype, device=0)
m.detect_batch(fr)
d = {}
for n in ("decoded", "p3", "p4", "p5"):                  # every frame, eight at a time
    h = hashlib.sha256()
    for b0 in range(0, B, 8):
        h.update(m.get_tensor(n, (b0, min(8, B - b0))).tobytes())
    d["digest_" + n] = np.frombuffer(h.digest(), np.uint8)
keep = np.float16 if dtype.startswith("f16") else np.float32          # f16 storage: lossless
for f in frames:
    for n in names:
        try:
            v = m.get_tensor(n, (f, 1))
        except Exception:                                 # a tap this plan does not have (fused RepNCSP: no _ab / _t)
            continue
        d[f"{n}@{f}"] = v if n == "decoded" else v.astype(keep)
np.savez(out, **d)
"""


def run_plan(path, dtype, B, H, W, res, frames, tapped, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT, **(TAPS if tapped else {}))
    for k in TAPS:
        if not tapped:
            env.pop(k, None)
    subprocess.run([sys.executable, "-c", _RUN, dtype, str(B), str(H), str(W), str(res), str(path), ",".join(map(str, frames)),
                    ",".join(NAMES if tapped else [])], check=True, env=env, timeout=timeout)
    return dict(np.load(path))


def restart_frame(d, f, sd, sdt, split_fn):
    """Every conv launch of frame f of a YOLOv9-C plan against its float64 restart: [(name, kind, stats)] + the DDetect tail's numbers."""
    has = lambda n: f"{n}@{f}" in d                                                                  # noqa: E731
    T = lambda n: torch.from_numpy(d[f"{n}@{f}"].astype(np.float64)).permute(0, 3, 1, 2)           # noqa: E731
    rnd = lambda y: rc.round_storage(y, sdt)                                                         # noqa: E731
    wc, out = {}, []

    def ref(x, prefixes, stride=1, groups=1, act=True, res=None):
        if tuple(prefixes) not in wc:
            ws = [torch.from_numpy(np.asarray(sd[p + ".weight"], np.float32)) for p in prefixes]
            we = rc.effective_weights(ws, sdt, split_fn(prefixes[0], ws[0].shape[-1]))
            wc[tuple(prefixes)] = (torch.cat(we), torch.cat([torch.from_numpy(np.asarray(sd[p + ".bias"], np.float64)) for p in prefixes]))
        w, b = wc[tuple(prefixes)]
        return rc.conv64(x, w, b, stride, groups, act, res)

    def chk(name, kind, gpu, y64):
        ulps = BARS[kind]["ulps"]
        out.append((name, kind, rc.check(gpu, y64, sdt, name, R_cell=BARS[kind]["R_cell"], ulps=ulps, enforce=False)))

    P = "model.list."
    stem = T("stem")
    chk(P + "0 (letterbox + stem)", "single", stem, ref(T("input"), [P + "0.conv"], stride=2))
    b = {n: T(f"b{n}") for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 19)}
    b[15], b[18], b[21] = T("p3"), T("p4"), T("p5")
    chk(P + "1", "single", b[1], ref(stem, [P + "1.conv"], stride=2))
    up = lambda t: t.repeat_interleave(2, 2).repeat_interleave(2, 3)                                # noqa: E731
    ins = {2: b[1], 4: b[3], 6: b[5], 8: b[7], 12: torch.cat((up(b[9]), b[6]), 1), 15: torch.cat((up(b[12]), b[4]), 1),
           18: torch.cat((b[16], b[12]), 1), 21: torch.cat((b[19], b[9]), 1)}
    for ci, n in enumerate((2, 4, 6, 8, 12, 15, 18, 21)):                                          # RepNCSPELAN4
        p, cat = f"{P}{n}", T(f"cat{ci}")
        h = cat.shape[1] // 8
        chk(p + ".cv1", "single", cat[:, :4 * h], ref(ins[n], [p + ".cv1.conv"]))
        for k in (0, 1):
            c, br = 2 * ci + k, f"{p}.cv{2 + k}"
            r = br + ".list.0"
            q = r + ".m.list.0"
            u = T(f"csp{c}_u")
            ab64 = ref(cat[:, (2 + 2 * k) * h:(4 + 2 * k) * h], [r + ".cv1.conv", r + ".cv2.conv"])
            if has(f"csp{c}_ab"):
                ab, t = T(f"csp{c}_ab"), T(f"csp{c}_t")
                a0 = rnd(ab64[:, :h])                     # the GPU's a was overwritten in place by the residual update: recomputed
                chk(r + ".cv2 (b half of cv1|cv2)", "single", ab[:, h:], ab64[:, h:])
                chk(q + ".cv1", "from_a", t, ref(a0, [q + ".cv1.conv"]))
                chk(q + ".cv2 (+ a, in place)", "residual", ab[:, :h], ref(t, [q + ".cv2.conv"], res=a0))
                chk(r + ".cv3", "single", u, ref(ab, [r + ".cv3.conv"]))
            else:                                         # fused RepNCSP: the four launches as one unit
                a = rnd(ab64)
                t = rnd(ref(a[:, :h], [q + ".cv1.conv"]))
                a1 = rnd(ref(t, [q + ".cv2.conv"], res=a[:, :h]))
                chk(r + " (fused RepNCSP)", "chained", u, ref(torch.cat((a1, a[:, h:]), 1), [r + ".cv3.conv"]))
            chk(br + ".list.1", "single", cat[:, (4 + 2 * k) * h:(6 + 2 * k) * h], ref(u, [br + ".list.1.conv"]))
        chk(p + ".cv4", "single", b[n], ref(cat, [p + ".cv4.conv"]))
    for n, src in ((3, 2), (5, 4), (7, 6), (16, 15), (19, 18)):                                     # ADown
        p, x = f"{P}{n}", b[src]
        C = x.shape[1] // 2
        avg = rnd(F.avg_pool2d(x, 2, 1, 0, False, True))                                            # rounded once; max-pool is exact
        chk(p + ".cv1", "single", b[n][:, :C], ref(avg[:, :C], [p + ".cv1.conv"], stride=2))
        chk(p + ".cv2", "single", b[n][:, C:], ref(F.max_pool2d(avg[:, C:], 3, 2, 1), [p + ".cv2.conv"]))
    ys = [rnd(ref(b[8], [P + "9.cv1.conv"]))]                                                      # SPPELAN
    for _ in range(3):
        ys.append(F.max_pool2d(ys[-1], 5, 1, 2))
    chk(P + "9 (SPPELAN)", "chained", b[9], ref(torch.cat(ys, 1), [P + "9.cv5.conv"]))
    H = P + "22."                                                                                   # DDetect, intermediates rounded
    raws = []
    for l, feat in enumerate((b[15], b[18], b[21])):
        hb, hc = f"{H}cv2.list.{l}.list.", f"{H}cv3.list.{l}.list."
        x0 = rnd(ref(rnd(ref(feat, [hb + "0.conv"])), [hb + "1.conv"], groups=4))
        c1 = rnd(ref(rnd(ref(feat, [hc + "0.conv"])), [hc + "1.conv"]))
        raws.append(torch.cat((ref(x0, [hb + "2"], groups=4, act=False), ref(c1, [hc + "2"], act=False)), 1))
    from oracle.yolov9_oracle import YOLOv9Oracle, decoded_rows
    dfl = SimpleNamespace(head=H, sd={H + "dfl.conv.weight": torch.from_numpy(np.asarray(sd[H + "dfl.conv.weight"], np.float64))})
    want = decoded_rows(YOLOv9Oracle.decode(dfl, raws))[0]
    got = d[f"decoded@{f}"][0]
    both = (want[:, 4] > 0) & (got[:, 4] > 0)
    tail = {"anchors_over": int(both.sum()), "only_one_over": int(((want[:, 4] > 0) != (got[:, 4] > 0)).sum()),
            "box_px": float(np.abs(want[both, :4] - got[both, :4]).max()) if both.any() else 0.0,
            "score": float(np.abs(want[both, 4] - got[both, 4]).max()) if both.any() else 0.0,
            "cls_differ": int((want[both, 5] != got[both, 5]).sum())}
    return out, tail


def hold(results, tails, label):
    """Print every launch's numbers, then hold them to BARS (all failures listed at once)."""
    bad = []
    for name, kind, st in results:
        print(f"{label} {kind:8s} {rc.fmt(name, st)}")
        bar = BARS[kind]
        near = st["not_faithful"] == 0 if bar["ulps"] is None else (st["nonfinite"] == 0 and st["max_ulp"] <= bar["ulps"])
        if not (near and st["differ"] <= bar["R"] and st["cell_excess"] <= 0 and (bar["D"] is None or st["p99_boundary"] <= bar["D"])):
            bad.append((name, kind, st))
    for f, t in tails:
        print(f"{label} DDetect tail frame {f}: {t}")
        if not (t["box_px"] <= BOX_PX and t["score"] <= SCORE and t["anchors_over"] > 0 and t["cls_differ"] <= max(2, t["anchors_over"] // 500)):
            bad.append(("DDetect tail", f, t))
    assert sum(t["anchors_over"] for _, t in tails) > 100, tails    # the tail check has anchors to look at
    assert not bad, bad


def _plan(tmp_path, dtype, B, H, W, frames, split_fn, sdt, label):
    from clearcam_amd.weights import conditioned_yolov9_state_dict
    shipped = run_plan(tmp_path / f"{label}_shipped.npz", dtype, B, H, W, 640, [], tapped=False)
    tapped = run_plan(tmp_path / f"{label}_tapped.npz", dtype, B, H, W, 640, frames, tapped=True)
    for n in ("decoded", "p3", "p4", "p5"):                # the taps change the arena layout, not one bit of the result
        assert np.array_equal(shipped["digest_" + n], tapped["digest_" + n]), (label, n)
    sd = conditioned_yolov9_state_dict("c", 1234, exact=False)
    results, tails = [], []
    with torch.no_grad():
        for f in frames:
            r, t = restart_frame(tapped, f, sd, sdt, split_fn)
            results += [(f"frame {f} {n}", k, s) for n, k, s in r]
            tails.append((f, t))
    n_single = len({n for n, k, _ in r if k != "chained"})
    print(f"{label}: {n_single} single conv launches + {len(r) - n_single} chained units checked per frame, frames {frames}")
    hold(results, tails, label)
    return n_single


def test_get_tensor_frames(sd_t):
    """cc_yolo_get_tensor_frames: a frame range of a tap is bit for bit that slice of the whole tap; ranges outside [0, B) are refused."""
    from clearcam_amd import _lib
    from clearcam_amd.yolov9 import YOLOv9
    m = YOLOv9("t", 320, state_dict=sd_t, dtype="f16", device=0)
    m.detect_batch(np.random.default_rng(2).integers(0, 256, (5, 240, 320, 3), dtype=np.uint8))
    for n in ("input", "p3", "p5", "decoded"):
        whole = m.get_tensor(n)
        assert whole.shape[0] == 5
        for b0, nb in ((0, 1), (2, 3), (4, 1), (0, 5)):
            part = m.get_tensor(n, (b0, nb))
            assert part.shape == (nb,) + whole.shape[1:] and np.array_equal(part, whole[b0:b0 + nb]), (n, b0, nb)
    for bad in ((-1, 1), (5, 1), (3, 3), (0, 0), (1, -1)):
        with pytest.raises(_lib.CCError):
            m.get_tensor("p3", bad)
    m.close()


# (label, dtype, B, H, W, frames restarted, storage type): A = bench.py's configuration (640 x 640 noise frames of seed 1); B = the
# reference's call, one 1080 x 1920 frame letterboxed to 384 x 640 (few-tile / small-pixel-tile kernels); C = bf16 at B = 64, one
# controlled-rounded plane everywhere (the bf16 instantiations of every kernel), under CLEARCAM_TEST_FULL=1
PLANS = [("A", "f16h", 64, 640, 640, [0, 31, 63], "f16"), ("B", "f16h", 1, 1080, 1920, [0], "f16")]
if os.environ.get("CLEARCAM_TEST_FULL"):
    PLANS.append(("C", "bf16", 64, 640, 640, [0, 63], "bf16"))


@pytest.mark.parametrize("plan", PLANS, ids=[p[0] for p in PLANS])
def test_plan_restart(tmp_path, plan):
    label, dtype, B, H, W, frames, sdt = plan
    split_fn = (lambda name, k: rc.f16h_split(name, k)) if dtype == "f16h" else (lambda name, k: False)
    n = _plan(tmp_path, dtype, B, H, W, frames, split_fn, sdt, label)
    if label == "A":
        assert n == 100                                     # every conv launch of the bench plan outside the chained units
