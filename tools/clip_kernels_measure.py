"""err / bar of the CLIP tower's non-GEMM kernels, one launch per case (docs/measurement.md): python tools/clip_kernels_measure.py [--out FILE]

Runs every case of tests/test_gpu_clip_kernels.py through the same cc_dev_* launches, past the bar too, and prints per kernel and
storage type the largest err / bar with its case, beside the CPU emulation's err / bar for the SAME case (tests/clip_kernel_cases.py).
For the peaked f16 attention case also: the distance of the GPU's output to the emulation that keeps rounded weights below 2^-14 and to
the one that flushes them.  One JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clip_kernel_cases as ck          # noqa: E402
import test_gpu_clip_kernels as tk      # noqa: E402


def emu_ratio_attn(c):
    r = ck.attn_ref(c)
    return ck.worst(np.abs(ck.attn_emulate(c) - r.out), ck.attn_bar(c, r))[0]


def emu_ratio_ln(c):
    y, br = ck.ln_ref(c)
    return ck.worst(np.abs(ck.ln_emulate(c) - y), ck.ln_bar(br, y, ck.U[c.dt] if c.out16 else 0.0))[0]


def emu_ratio_asm(c):
    y, br = ck.asm_ref(c)
    return ck.worst(np.abs(ck.asm_emulate(c) - y), ck.ln_bar(br, y))[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    tk.STRICT = False
    t0 = time.perf_counter()
    rows, over = {}, []

    def note(kernel, dt, name, ratio, emu):
        if ratio > 1.0:
            over.append((name, ratio))
        if ratio >= rows.get((kernel, dt), (-1.0,))[0]:
            rows[(kernel, dt)] = (ratio, name, emu)

    for c in tk.ATTN:
        ratio, _ = tk.attention_ratio(c)
        note("attn_simple_kernel" if c.dt == "f32" else "attn_mfma_kernel", c.dt, c.name, ratio, lambda c=c: emu_ratio_attn(c))
    for c in tk.LN:
        form = "vector" if c.vec else "scalar"
        note(f"layernorm_kernel ({form}, {'f32' if not c.out16 else '16-bit'} out)", c.dt, c.name, tk.layernorm_ratio(c), lambda c=c: emu_ratio_ln(c))
    for c in tk.ASM:
        note("assemble_ln_kernel", c.dt, c.name, tk.assemble_ratio(c), lambda c=c: emu_ratio_asm(c))
    for D in ck.L2_D:
        for eps in ck.L2_EPS:
            x = ck.l2_input(D, eps)
            y = ck.l2_ref(x, eps)
            note("l2norm_kernel", "f32", f"l2norm-D{D}-eps{eps:g}", tk.l2norm_ratio(D, eps),
                 lambda x=x, y=y, eps=eps: ck.worst(np.abs(ck.l2_emulate(x, eps) - y), ck.l2_bar(y))[0])
    doc = {"seconds": round(time.perf_counter() - t0, 2), "over_the_bar": over,
           "table": [{"kernel": k, "dtype": dt, "gpu_err_over_bar": round(r, 4), "case": name, "cpu_emulation_err_over_bar": round(emu(), 4)}
                     for (k, dt), (r, name, emu) in sorted(rows.items())]}
    peaked = next(c for c in tk.ATTN if c.dt == "f16" and c.tag == "peaked")
    _, got = tk.attention_ratio(peaked)
    keep, flush = ck.attn_emulate(peaked), ck.attn_emulate(peaked, flush16=True)
    doc["peaked_f16"] = {"max_abs_to_keeping_emulation": float(np.abs(got - keep).max()), "max_abs_to_flushing_emulation": float(np.abs(got - flush).max()),
                         "max_abs_between_emulations": float(np.abs(keep - flush).max()),
                         "elements_nearer_keeping": int((np.abs(got - keep) < np.abs(got - flush)).sum()),
                         "elements_nearer_flushing": int((np.abs(got - flush) < np.abs(got - keep)).sum())}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
