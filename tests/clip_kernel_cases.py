"""Inputs, float64 references, bars, float32 emulations and mutants of tests/test_gpu_clip_kernels.py, held on the CPU by
tests/test_clip_kernel_cases_host.py (helper module; not a conftest).  NumPy / PyTorch-CPU only: neither the oracle nor the library is
imported here.

The kernels are the CLIP tower's non-GEMM ones (clearcam_amd/csrc/clip_kernels.hip): attn_mfma_kernel (f16 / bf16), attn_simple_kernel
(f32), layernorm_kernel (vector and scalar form), assemble_ln_kernel, patchify_kernel, embed_kernel, l2norm_kernel.  Inputs are drawn in
float64, rounded to the storage type, and THOSE values go to the float64 reference.  Seeds come from the case name through zlib.crc32.

Bars (u = unit roundoff of the storage type, eps = 2^-24, every other quantity from the float64 reference; none is read off a kernel):
  attention, 16-bit   |got - ref| <= 1.02 u (A + |ref|) + 2^-20 A + S      p = softmax weights, ref = p v, A = p |v|,
                      S = sum of p_j |v_j| over visible keys whose un-normalised weight exp(s - max) is below 2^-14 (f16 only)
  attention, f32      |got - ref| <= eps (L + 128 T + 32) (A + |ref|)       T = max_j sum_d |q_d k_jd| scale of the row
  LayerNorm, assemble bar_j = 8 eps (|w_j| rstd (mean_i |x_i| + |x_j - mu|) + |y_j|)   (+ u |y_j| when the output is 16-bit)
  l2norm              8 eps |y|
  patchify, embed     bit-exact
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

EPS = 2.0 ** -24
U = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DTI = {"f32": 0, "f16": 1, "bf16": 2}
LOG2E_F32 = np.float32(1.4426950408889634)


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


def to_storage(a: np.ndarray, dt: str) -> torch.Tensor:
    """float64 / float32 values -> the storage type, round-to-nearest-even (torch's .to)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_DT[dt])


def f64(t: torch.Tensor) -> np.ndarray:
    return t.double().numpy()


# =====================================================================================================================================
# attention
# =====================================================================================================================================
ATTN_L16 = (1, 16, 17, 50, 64, 65, 77, 80, 81, 96, 97, 129, 144, 208, 256, 257, 272, 273, 288)
ATTN_L32 = (1, 3, 4, 5, 77, 257, 288)
Q_PLANT = 4.0            # the reserved dimensions (62, 63) of every q in the planted family
BOOST = 4.0              # score a planted key gains: its k[63] = BOOST / (scale * Q_PLANT)


@dataclass(frozen=True)
class AttnCase:
    dt: str
    L: int
    causal: int
    family: str              # "uniform" | "planted"
    B: int = 2
    H: int = 3
    scale: float = 0.125
    q_gain: float = 1.0      # 4 = the peaked case
    copy_batch: bool = False
    tag: str = ""

    @property
    def name(self) -> str:
        return f"attn-{self.dt}-L{self.L}-{'causal' if self.causal else 'full'}-{self.family}" + (f"-{self.tag}" if self.tag else "")

    @property
    def D(self) -> int:
        return 64 * self.H


def attn_cases(dt: str) -> List[AttnCase]:
    out = [AttnCase(dt, L, causal, fam) for L in (ATTN_L32 if dt == "f32" else ATTN_L16) for causal in (0, 1) for fam in ("uniform", "planted")]
    if dt != "f32":
        out += [AttnCase(dt, 77, 1, "uniform", scale=0.09, tag="scale009"),
                AttnCase(dt, 65, 0, "uniform", H=1, tag="H1"),
                AttnCase(dt, 17, 1, "planted", B=1, H=16, tag="H16"),
                AttnCase(dt, 257, 0, "uniform", q_gain=4.0, tag="peaked"),
                AttnCase(dt, 129, 1, "uniform", copy_batch=True, tag="copy")]
    return out


def planted_keys(L: int) -> List[int]:
    """Keys that must not be lost: 0, L-1, the first key of the last fragment, 15 and 16."""
    return sorted(k for k in {0, L - 1, 16 * ((L + 15) // 16 - 1), 15, 16} if 0 <= k < L)


def split_ranges(L: int) -> Optional[List[Tuple[int, int]]]:
    """attn_mfma_kernel's split last tile: the key range [lo, hi) each of the four waves takes, or None where the tile is not split."""
    tiles = (L + 15) // 16
    if tiles % 4 != 1 or tiles == 1:
        return None
    nb = (6 if L <= 96 else 18) // 2
    bq, br = divmod(nb, 4)
    out = []
    for w in range(4):
        b0 = w * bq + min(w, br)
        out.append((32 * b0, 32 * (b0 + bq + (1 if w < br else 0))))
    return out


@functools.lru_cache(maxsize=None)
def attn_inputs(c: AttnCase) -> torch.Tensor:
    """(B*L, 3*D) [q | k | v] in the storage type."""
    rng = np.random.default_rng(seed_of(c.name))
    B, L, H = c.B, c.L, c.H
    q = rng.normal(0, 0.8, (B, L, H, 64)) * c.q_gain
    k = rng.normal(0, 1.0, (B, L, H, 64))
    v = 3.0 * rng.normal(0, 1.0, (B, L, H, 64)) + 1.0
    if c.family == "planted":
        # two reserved dimensions, constant in every q: 63 is zero in ordinary keys and set in planted ones (score + BOOST); 62 is the same
        # negative value in EVERY key (all real scores - BOOST: nothing changes among real keys, but a padding key admitted with zero K,
        # score 0, then weighs as much as a planted key)
        q[..., 62:] = Q_PLANT
        k[..., 63] = 0.0
        k[..., 62] = -BOOST / (c.scale * Q_PLANT)
        qa, ka = q[..., :62], k[..., :62]
        if c.causal:      # every diagonal key: k_j's ordinary part is made orthogonal to q_j, then q_j . k_j is raised by BOOST / scale
            ka -= (ka * qa).sum(-1, keepdims=True) / (qa * qa).sum(-1, keepdims=True) * qa
            ka += (BOOST / c.scale) * qa / (qa * qa).sum(-1, keepdims=True)
        for i, j in enumerate(planted_keys(L)):
            if c.causal:
                ka[:, j] -= (BOOST / c.scale) * qa[:, j] / (qa[:, j] * qa[:, j]).sum(-1, keepdims=True)   # its boost comes through dim 63
            ka[:, j] *= 0.1
            k[:, j, :, 63] = BOOST / (c.scale * Q_PLANT)
            d = np.arange(64)
            for h in range(H):
                v[:, j, h] = (4.0 + i) * np.where((d >> ((i + h) % 6)) & 1, -1.0, 1.0)
    if c.copy_batch:
        q[1], k[1], v[1] = q[0], k[0], v[0]
    x = np.stack((q, k, v), 2).reshape(B * L, 3 * H * 64)
    return to_storage(x, c.dt)


ATTN_MUTANTS = ("drop_last", "pad_key", "drop_16", "no_diagonal", "admit_next", "exp_base", "v_next_head", "batch1_reads_0", "split_no_rescale")


def mutant_applies(c: AttnCase, m: str) -> bool:
    return {"drop_last": c.L > 1, "pad_key": c.L % 16 != 0, "drop_16": c.L >= 18, "no_diagonal": bool(c.causal) and c.L > 1,
            "admit_next": bool(c.causal) and c.L > 1, "exp_base": c.L > 1, "v_next_head": c.H > 1, "batch1_reads_0": c.B > 1 and not c.copy_batch,
            "split_no_rescale": c.dt != "f32" and split_ranges(c.L) is not None}[m]


def _qkv64(c: AttnCase):
    x = f64(attn_inputs(c)).reshape(c.B, c.L, 3, c.H, 64)
    return tuple(np.ascontiguousarray(x[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))      # each (B,H,L,64)


def _visible(L: int, causal: int, shift: int = 0) -> np.ndarray:
    i, j = np.arange(L)[:, None], np.arange(L)[None, :]
    return (j <= i + shift) if causal else np.ones((L, L), bool)


@dataclass
class AttnRef:
    out: np.ndarray        # (B*L, D) float64
    A: np.ndarray          # p . |v|
    S: np.ndarray          # mass of visible keys whose un-normalised weight is below 2^-14, times |v|
    T: np.ndarray          # (B*L, D) max_j sum_d |q_d k_jd| scale of the row, broadcast over the head's 64 outputs
    p: np.ndarray          # (B,H,L,L) softmax weights
    e_min: float           # the smallest un-normalised weight of a visible key


def _rows(x: np.ndarray) -> np.ndarray:
    """(B,H,L,64) -> (B*L, H*64)"""
    B, H, L, _ = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * L, H * 64)


def attn_ref(c: AttnCase, mutant: Optional[str] = None) -> AttnRef:
    """softmax(q k^T scale [+ causal mask]) v per head in float64; `mutant` = one of ATTN_MUTANTS applied to the model."""
    q, k, v = _qkv64(c)
    L = c.L
    if mutant == "batch1_reads_0":
        q, k, v = q.copy(), k.copy(), v.copy()
        q[1], k[1], v[1] = q[0], k[0], v[0]
    if mutant == "v_next_head":
        v = np.roll(v, -1, axis=1)
    vis = _visible(L, c.causal, 1 if mutant == "admit_next" else 0)
    if mutant == "no_diagonal":
        vis = vis & ~np.eye(L, dtype=bool)
        vis[0, 0] = True
    if mutant == "drop_last":
        vis = vis.copy(); vis[:, L - 1] = False                  # L > 1: every row keeps key 0
    if mutant == "drop_16":
        vis = vis.copy(); vis[:, 16] = False
    s = np.einsum("bhid,bhjd->bhij", q, k) * c.scale
    if mutant == "exp_base":
        s = s * np.log2(np.e)
    T = (np.einsum("bhid,bhjd->bhij", np.abs(q), np.abs(k)) * c.scale).max(-1) if c.dt == "f32" else np.zeros(q.shape[:3])   # (B,H,L): the f32 bar's
    if mutant == "pad_key":                                                                      # key L: zero K (score 0) and zero V
        s = np.concatenate((s, np.zeros(s.shape[:3] + (1,))), -1)
        vis = np.concatenate((vis, np.ones((L, 1), bool)), -1)
        v = np.concatenate((v, np.zeros(v.shape[:2] + (1, 64))), 2)
    sm = np.where(vis, s, -np.inf)
    e = np.exp(sm - sm.max(-1, keepdims=True))
    if mutant == "split_no_rescale":
        q0 = ((L + 15) // 16 - 1) * 16
        for lo, hi in split_ranges(L):
            part = sm[:, :, q0:, lo:hi]
            if part.shape[-1] == 0:
                continue
            m = part.max(-1, keepdims=True)
            e[:, :, q0:, lo:hi] = np.where(np.isfinite(m), np.exp(part - np.where(np.isfinite(m), m, 0.0)), 0.0)
    p = e / e.sum(-1, keepdims=True)
    av = np.abs(v)
    tiny = np.where(vis & (e < 2.0 ** -14), p, 0.0)
    return AttnRef(_rows(p @ v), _rows(p @ av), _rows(tiny @ av), _rows(np.repeat(T[..., None], 64, -1)), p, float(e[..., vis].min()))


def attn_bar(c: AttnCase, r: AttnRef) -> np.ndarray:
    if c.dt == "f32":
        return EPS * (c.L + 128.0 * r.T + 32.0) * (r.A + np.abs(r.out))
    return 1.02 * U[c.dt] * (r.A + np.abs(r.out)) + 2.0 ** -20 * r.A + (r.S if c.dt == "f16" else 0.0)


def attn_emulate(c: AttnCase, flush16: bool = False) -> np.ndarray:
    """The kernel's arithmetic restated on the CPU -> (B*L, D) in float64 (values of the storage type).
    16-bit (attn_mfma_kernel): float32 raw scores, maximum on the raw scores, e = exp2(fma(s, scale log2 e, -max scale log2 e)) in
    float32, the row sum over the unrounded e, e rounded to the storage type before P V, float32 accumulation, one multiply by 1 / sum,
    the output rounded once; the split last tile as four partial (max, sum, P V) merged with exp2 factors.
    f32 (attn_simple_kernel): float32 scores times scale, expf(s - max), p = e / sum, float32 accumulation.
    flush16: rounded weights below the storage type's smallest normal number (2^-14 for f16) count as zero in P V."""
    t = TORCH_DT[c.dt]
    x = attn_inputs(c).float().reshape(c.B, c.L, 3, c.H, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))
    vis = torch.from_numpy(_visible(c.L, c.causal))
    s = q @ k.transpose(-1, -2)
    ninf = torch.tensor(float("-inf"))
    if c.dt == "f32":
        s = torch.where(vis, s * np.float32(c.scale), ninf)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        o = (e / e.sum(-1, keepdim=True)) @ v
        return _rows(o.double().numpy())
    cc = np.float32(c.scale) * LOG2E_F32

    def part(sv, vv):           # sv (B,H,n,keys) masked raw scores -> local max (raw), row sum, P V; an all-masked range gives (-inf, 0, 0)
        m = sv.amax(-1, keepdim=True)
        mc = torch.where(torch.isinf(m), torch.zeros(()), m * cc)
        e = torch.exp2((sv.double() * float(cc) - mc.double()).float())
        er = e.to(t).float()
        if flush16:
            er = torch.where(er < torch.finfo(t).smallest_normal, torch.zeros(()), er)
        return m, e.sum(-1, keepdim=True), er @ vv

    sm = torch.where(vis, s, ninf)
    m, l, o = part(sm, v)
    out = (o * (1.0 / l)).to(t)
    rng = split_ranges(c.L)
    if rng is not None:
        q0 = ((c.L + 15) // 16 - 1) * 16
        parts = [part(sm[:, :, q0:, lo:hi], v[:, :, lo:hi]) for lo, hi in rng if lo < c.L]
        mm = torch.stack([p_[0] for p_ in parts]).amax(0)
        acc, ll = torch.zeros_like(parts[0][2]), torch.zeros_like(parts[0][1])
        for mw, lw, ow in parts:
            fac = torch.where(torch.isinf(mw), torch.zeros(()), torch.exp2((mw - mm) * cc))
            ll = ll + lw * fac
            acc = acc + ow * fac
        out[:, :, q0:] = (acc * (1.0 / ll)).to(t)
    return _rows(out.double().numpy())


# =====================================================================================================================================
# LayerNorm / assemble_ln
# =====================================================================================================================================
ROW_KINDS = ("plain", "offset50", "spike", "tight", "const")


def make_row(rng, kind: str, D: int) -> np.ndarray:
    x = rng.normal(0, 1, D)
    if kind == "offset50":
        x += 50.0
    elif kind == "spike":
        x[(7 * D) // 11] *= 300.0
    elif kind == "tight":
        x = 3.0 + 0.01 * x                     # variance 1e-4: eps = 1e-5 matters
    elif kind == "const":
        x[:] = 2.5                             # every partial sum exact in float32: the output is beta
    return x.astype(np.float32)


@dataclass(frozen=True)
class LnCase:
    dt: str
    out_f32: int
    D: int
    rows: int
    offset: int = 0                            # floats from the 16-byte aligned start of the input buffer to row 0
    stride: int = -1                           # -1: D
    index: Optional[Tuple[int, ...]] = None
    nrows_buf: int = -1                        # rows (of `stride` floats) the input buffer holds; -1: rows
    tag: str = ""

    @property
    def name(self) -> str:
        return f"ln-{self.dt}-{'f32out' if self.out_f32 else 'stout'}-D{self.D}-r{self.rows}" + (f"-{self.tag}" if self.tag else "")

    @property
    def row_stride(self) -> int:
        return self.D if self.stride < 0 else self.stride

    @property
    def vec(self) -> bool:
        """launch_layernorm's choice, for buffers whose base is 16-byte aligned"""
        return self.D % 4 == 0 and self.row_stride % 4 == 0 and self.offset % 4 == 0

    @property
    def out16(self) -> bool:
        return not self.out_f32 and self.dt != "f32"

    def starts(self, ignore_index=False, stride=None) -> List[int]:
        st = self.row_stride if stride is None else stride
        return [self.offset + (self.index[r] if self.index and not ignore_index else r) * st for r in range(self.rows)]


def ln_cases(dt: str) -> List[LnCase]:
    out = []
    for o32 in (0, 1):
        for D in (64, 100, 192, 768, 1024, 130, 1023):
            for rows in (1, 5):
                out.append(LnCase(dt, o32, D, rows))
        out.append(LnCase(dt, o32, 768, 5, offset=1, tag="off1"))
        out.append(LnCase(dt, o32, 768, 5, stride=769, tag="stride769"))
        out.append(LnCase(dt, o32, 192, 2, index=(0 * 7 + 4, 1 * 7 + 6), nrows_buf=14, tag="gather"))      # rows b*L + eot, L = 7
        out.append(LnCase(dt, o32, 192, 2, stride=7 * 192, nrows_buf=2, tag="clspool"))                   # the class token of each image
    return out


@functools.lru_cache(maxsize=None)
def ln_inputs(c: LnCase) -> Dict[str, np.ndarray]:
    """buf: the whole float32 input buffer (finite everywhere; `read` marks what the kernel may read), w, b."""
    rng = np.random.default_rng(seed_of(c.name))
    nrows = c.rows if c.nrows_buf < 0 else c.nrows_buf
    n = c.offset + (nrows - 1) * c.row_stride + max(c.D, c.row_stride if c.tag == "clspool" else 0)
    buf = rng.normal(0, 1, n).astype(np.float32)
    read = np.zeros(n, bool)
    for r, s in enumerate(c.starts()):
        buf[s:s + c.D] = make_row(rng, ROW_KINDS[(r + c.D) % 5], c.D)
        read[s:s + c.D] = True
    return {"buf": buf, "read": read, "w": rng.normal(1, 0.3, c.D).astype(np.float32), "b": rng.normal(0, 0.5, c.D).astype(np.float32)}


def ln_math(x: np.ndarray, w: np.ndarray, b: np.ndarray, eps=1e-5, ddof=0):
    """float64 LayerNorm of the rows of x -> (y, bracket) with bracket_j = |w_j| rstd (mean_i |x_i| + |x_j - mu|) + |y_j|."""
    x, w, b = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    D = x.shape[-1]
    mu = x.sum(-1, keepdims=True) / D
    d = x - mu
    rstd = 1.0 / np.sqrt((d * d).sum(-1, keepdims=True) / (D - ddof) + eps)
    y = d * rstd * w + b
    return y, np.abs(w) * rstd * (np.abs(x).mean(-1, keepdims=True) + np.abs(d)) + np.abs(y)


LN_MUTANTS = ("eps_1e-6", "var_d_minus_1", "no_beta", "index_ignored", "stride_is_d")


def ln_mutant_applies(c: LnCase, m: str) -> bool:
    return {"index_ignored": c.index is not None, "stride_is_d": c.row_stride != c.D and c.rows > 1}.get(m, True)


def ln_ref(c: LnCase, mutant: Optional[str] = None):
    i = ln_inputs(c)
    st = c.starts(ignore_index=mutant == "index_ignored", stride=c.D if mutant == "stride_is_d" else None)
    x = np.stack([i["buf"][s:s + c.D] for s in st])
    return ln_math(x, i["w"], np.zeros_like(i["b"]) if mutant == "no_beta" else i["b"], 1e-6 if mutant == "eps_1e-6" else 1e-5,
                   1 if mutant == "var_d_minus_1" else 0)


def ln_bar(bracket: np.ndarray, y: np.ndarray, u16: float = 0.0) -> np.ndarray:
    return 8.0 * EPS * bracket + u16 * np.abs(y)


def _wave_sum(v: np.ndarray) -> np.ndarray:
    """the xor butterfly 32, 16, .. 1 over the last axis (64 lanes), float32"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def ln_emulate_f32(x: np.ndarray, w: np.ndarray, b: np.ndarray, vec: bool) -> np.ndarray:
    """layernorm_kernel's float32 arithmetic in its own summation order.  x (rows, D) float32.  Scalar form: lane l sums elements l + 64 i,
    i = 0..15, in turn; vector form: lane l owns elements 4 (l + 64 i) .. + 3 and adds (x + y) + (z + w) per group; both end in the
    xor butterfly.  The squared deviations are summed in register order."""
    assert x.dtype == np.float32 and w.dtype == np.float32 and b.dtype == np.float32
    R, D = x.shape
    pad = np.zeros((R, 1024), np.float32); pad[:, :D] = x
    live = np.zeros(1024, bool); live[:D] = True
    if vec:
        g = pad.reshape(R, 4, 64, 4)                                                    # [i][lane][k]
        s = np.zeros((R, 64), np.float32)
        for i in range(4):
            s = s + ((g[:, i, :, 0] + g[:, i, :, 1]) + (g[:, i, :, 2] + g[:, i, :, 3]))
        regs = [(g[:, i, :, k_], live.reshape(4, 64, 4)[i, :, k_]) for i in range(4) for k_ in range(4)]
    else:
        g = pad.reshape(R, 16, 64)
        s = np.zeros((R, 64), np.float32)
        for i in range(16):
            s = s + g[:, i]
        regs = [(g[:, i], live.reshape(16, 64)[i]) for i in range(16)]
    Df = np.float32(D)
    mean = (_wave_sum(s) / Df)[:, None]
    qq = np.zeros((R, 64), np.float32)
    for v, lv in regs:
        d = np.where(lv, v - mean, np.float32(0))
        qq = qq + d * d
    rstd = (np.float32(1) / np.sqrt(_wave_sum(qq) / Df + np.float32(1e-5)))[:, None]
    return (x - mean) * rstd * w + b


def ln_emulate(c: LnCase) -> np.ndarray:
    i = ln_inputs(c)
    x = np.stack([i["buf"][s:s + c.D] for s in c.starts()])
    y = ln_emulate_f32(x, i["w"], i["b"], c.vec)
    return f64(to_storage(y, c.dt)) if c.out16 else y.astype(np.float64)


@dataclass(frozen=True)
class AsmCase:
    dt: str
    D: int
    B: int = 2
    L: int = 5

    @property
    def name(self) -> str:
        return f"assemble-{self.dt}-D{self.D}"


def asm_cases(dt: str) -> List[AsmCase]:
    return [AsmCase(dt, D) for D in (64, 100, 192, 1024)]


@functools.lru_cache(maxsize=None)
def asm_inputs(c: AsmCase):
    rng = np.random.default_rng(seed_of(c.name))
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)      # noqa: E731
    return {"patches": to_storage(rng.normal(0, 1, (c.B * (c.L - 1), c.D)), c.dt), "cls": f(c.D), "pos": 0.5 * f(c.L, c.D),
            "w": rng.normal(1, 0.3, c.D).astype(np.float32), "b": 0.5 * f(c.D)}


ASM_MUTANTS = ("patch_row_t", "no_class_token")


def _asm_tokens(c: AsmCase, dtype, mutant=None) -> np.ndarray:
    """cat(class token, patches) + positional -> (B*L, D) in `dtype` (one rounding per sum when float32)"""
    i = asm_inputs(c)
    p = (i["patches"].float().numpy() if dtype == np.float32 else f64(i["patches"])).reshape(c.B, c.L - 1, c.D)
    x = np.empty((c.B, c.L, c.D), dtype)
    for t in range(c.L):
        if t == 0:
            x[:, 0] = p[:, 0] if mutant == "no_class_token" else i["cls"].astype(dtype)
        else:
            x[:, t] = p[:, t % (c.L - 1) if mutant == "patch_row_t" else t - 1]
    return (x + i["pos"].astype(dtype)).reshape(c.B * c.L, c.D)


def asm_ref(c: AsmCase, mutant: Optional[str] = None):
    i = asm_inputs(c)
    return ln_math(_asm_tokens(c, np.float64, mutant), i["w"], i["b"])


def asm_emulate(c: AsmCase) -> np.ndarray:
    i = asm_inputs(c)
    return ln_emulate_f32(_asm_tokens(c, np.float32), i["w"], i["b"], False).astype(np.float64)


# =====================================================================================================================================
# patchify, embed, l2norm
# =====================================================================================================================================
PATCH_SHAPES = ((28, 14, 640), (8, 4, 64))      # (S, patch, Kpad)


@functools.lru_cache(maxsize=None)
def patch_input(S: int, B: int = 2) -> np.ndarray:
    """(B,3,S,S) float32 pixels: N(0,1) and, sprinkled in, exact ties of both 16-bit roundings (1 + 2^-11, 1 + 3 2^-11, 1 + 2^-8, ..)."""
    rng = np.random.default_rng(seed_of(f"patchify-S{S}"))
    x = rng.normal(0, 1, (B, 3, S, S)).astype(np.float32)
    ties = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(2 + 2.0 ** -7), 0.0, -0.0], np.float32)
    flat = x.reshape(-1)
    flat[rng.choice(flat.size, 64, replace=False)] = np.tile(ties, 8)
    return x


def patchify_ref(x: np.ndarray, patch: int, Kpad: int, dt: str) -> torch.Tensor:
    """(B*g*g, Kpad) in the storage type: k = c p p + kh p + kw, columns past 3 p p zero."""
    B, _, S, _ = x.shape
    g = S // patch
    t = x.reshape(B, 3, g, patch, g, patch).transpose(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * patch * patch)
    out = np.zeros((B * g * g, Kpad), np.float32)
    out[:, :3 * patch * patch] = t
    return torch.from_numpy(out).to(TORCH_DT[dt])


EMBED_D = (64, 192)
EMBED_VOCAB, EMBED_B, EMBED_L = 50, 2, 7
EMBED_TOKENS = np.array([[0, 49, 7, 7, 23, 49, 0], [49, 1, 48, 23, 23, 0, 31]], np.int32)


@functools.lru_cache(maxsize=None)
def embed_inputs(D: int):
    rng = np.random.default_rng(seed_of(f"embed-D{D}"))
    return rng.normal(0, 1, (EMBED_VOCAB, D)).astype(np.float32), rng.normal(0, 1, (EMBED_L, D)).astype(np.float32)


def embed_ref(D: int) -> np.ndarray:
    table, pos = embed_inputs(D)
    return (table[EMBED_TOKENS] + pos[None]).reshape(EMBED_B * EMBED_L, D)            # float32 + float32: the kernel's one rounding


L2_D = (1, 64, 100, 512, 768)
L2_EPS = (1e-8, 0.0)


@functools.lru_cache(maxsize=None)
def l2_input(D: int, eps: float) -> np.ndarray:
    """5 rows: N(0,1); norm ~ 1e-3 sqrt(D) (where eps = 1e-8 shows); x 1000; all zero (eps > 0 only, else another plain row); one-hot."""
    rng = np.random.default_rng(seed_of(f"l2norm-D{D}-eps{eps:g}"))
    x = rng.normal(0, 1, (5, D)).astype(np.float32)
    x[1] *= np.float32(1e-3)
    x[2] *= np.float32(1000.0)
    if eps > 0:
        x[3] = 0.0
    x[4] = 0.0
    x[4, D // 3] = -3.0
    return x


def l2_ref(x: np.ndarray, eps: float, mutant: Optional[str] = None) -> np.ndarray:
    x = x.astype(np.float64)
    n2 = (x * x).sum(-1, keepdims=True)
    return x / (np.sqrt(n2 + np.float32(eps).astype(np.float64)) if mutant == "eps_under_root" else np.sqrt(n2) + np.float32(eps).astype(np.float64))


def l2_bar(y: np.ndarray) -> np.ndarray:
    return 8.0 * EPS * np.abs(y)


def l2_emulate(x: np.ndarray, eps: float) -> np.ndarray:
    """l2norm_kernel in float32: lane l sums x_j^2 over j = l, l + 64, .. in turn, the xor butterfly, sqrt, + eps, one division per element."""
    R, D = x.shape
    n = (D + 63) // 64
    pad = np.zeros((R, n * 64), np.float32); pad[:, :D] = x
    g = pad.reshape(R, n, 64)
    s = np.zeros((R, 64), np.float32)
    for i in range(n):
        s = s + g[:, i] * g[:, i]
    nrm = np.sqrt(_wave_sum(s)) + np.float32(eps)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x / nrm[:, None]).astype(np.float64)


def worst(err: np.ndarray, bar: np.ndarray):
    """(largest err / bar, its flat index); 0 / 0 counts as 0, err > 0 over bar = 0 as inf."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bar)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r.reshape(-1)[i]), i
