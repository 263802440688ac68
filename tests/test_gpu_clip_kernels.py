"""The CLIP tower's non-GEMM kernels, ONE launch each through the cc_dev_* entries of dev_clip.hip, against the float64 references and
derived bars of tests/clip_kernel_cases.py (whose conditions tests/test_clip_kernel_cases_host.py holds on the CPU): attn_mfma_kernel at
every dispatch branch of launch_attn_t, attn_simple_kernel, layernorm_kernel in both forms, assemble_ln_kernel, patchify_kernel,
embed_kernel, l2norm_kernel.

Every buffer a kernel touches lives inside a larger NaN-filled tensor (>= 64 elements in front, a whole extra row behind): a stray read
shows as NaN in the result, a stray write in the guards, which must be bit-unchanged after the launch.  Every element that should be
written must be finite and within its bar; failures name the case, the index and err / bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_kernel_cases as ck
from clearcam_amd import _lib

pytestmark = pytest.mark.gpu
NAN = float("nan")
FRONT = 64
STRICT = True            # tools/clip_kernels_measure.py clears it to collect err / bar of every case, past the bar too
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


class Guarded:
    """`n` elements of `dtype` on the device between NaN guards: FRONT elements in front, max(FRONT, row) behind."""

    def __init__(self, n, dtype, row, data=None):
        self.lo, self.hi = FRONT, FRONT + n
        self.big = torch.full((FRONT + n + max(FRONT, row),), NAN, dtype=dtype, device="cuda")
        self.view = self.big[self.lo:self.hi]
        if data is not None:
            self.view.copy_(data.reshape(-1).to("cuda"))
        self.before = self.big.view(BITS[dtype]).clone()

    def guards_intact(self):
        now = self.big.view(BITS[self.big.dtype])
        return bool(torch.equal(now[:self.lo], self.before[:self.lo]) and torch.equal(now[self.hi:], self.before[self.hi:]))

    def untouched(self):
        return bool(torch.equal(self.big.view(BITS[self.big.dtype]), self.before))


def _in(t: torch.Tensor, row: int) -> Guarded:
    return Guarded(t.numel(), t.dtype, row, t)


def _np_in(a: np.ndarray, row: int) -> Guarded:
    return _in(torch.from_numpy(np.ascontiguousarray(a)), row)


def _judge(name, got: np.ndarray, ref: np.ndarray, bar: np.ndarray):
    """-> err / bar of the worst element; fails with the case name, the index and the ratio."""
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = np.flatnonzero(~np.isfinite(got).reshape(-1))
    assert bad.size == 0, f"{name}: {bad.size} non-finite outputs, first at flat index {bad[0]}"
    ratio, i = ck.worst(np.abs(got - ref), np.broadcast_to(bar, ref.shape))
    assert ratio <= 1.0 or not STRICT, f"{name}: index {np.unravel_index(i, ref.shape)}: err/bar = {ratio:.3f} (got {got.reshape(-1)[i]!r}, ref {ref.reshape(-1)[i]!r})"
    return ratio


# ---- attention --------------------------------------------------------------------------------------------------------------------------
def launch_attention(c: ck.AttnCase, L=None):
    """One cc_dev_attention launch -> (status, output Guarded, input Guarded)."""
    x = ck.attn_inputs(c)
    gin = _in(x, 3 * c.D)
    gout = Guarded(c.B * c.L * c.D, x.dtype, c.D)
    torch.cuda.synchronize()
    rc = _lib.lib().cc_dev_attention(ck.DTI[c.dt], _lib.ptr(gin.view), c.B, c.L if L is None else L, c.H, c.causal, C.c_float(c.scale), _lib.ptr(gout.view), None)
    return rc, gout, gin


def attention_ratio(c: ck.AttnCase):
    rc, gout, gin = launch_attention(c)
    _lib.check(rc)
    assert gout.guards_intact() and gin.untouched(), f"{c.name}: a guard or the input was written"
    got = gout.view.double().cpu().numpy().reshape(c.B * c.L, c.D)
    r = ck.attn_ref(c)
    return _judge(c.name, got, r.out, ck.attn_bar(c, r)), got


ATTN = [c for dt in ("f16", "bf16", "f32") for c in ck.attn_cases(dt)]


@pytest.mark.parametrize("c", ATTN, ids=[c.name for c in ATTN])
def test_attention_against_float64(c):
    _, got = attention_ratio(c)
    if c.copy_batch:                                          # batch 1 is a copy of batch 0: the two outputs are the same bits
        g = got.reshape(c.B, c.L * c.D)
        assert np.array_equal(g[0], g[1]), c.name


def test_attention_refusals():
    c = ck.AttnCase("f16", 288, 0, "uniform")
    for L in (289, 0, -1):
        rc, gout, _ = launch_attention(c, L=L)
        assert rc != 0 and gout.untouched(), L
    Lb = _lib.lib()
    x, out = _in(ck.attn_inputs(c), 3 * c.D), Guarded(c.B * c.L * c.D, torch.float16, c.D)
    args = lambda **k: [k.get("dt", 1), k.get("x", _lib.ptr(x.view)), k.get("B", c.B), c.L, k.get("H", c.H), 0, C.c_float(k.get("scale", 0.125)),   # noqa: E731
                        k.get("out", _lib.ptr(out.view)), None]
    for bad in (dict(dt=3), dict(dt=-1), dict(x=None), dict(out=None), dict(B=0), dict(H=0), dict(scale=0.0), dict(scale=-0.125),
                dict(x=C.c_void_p(x.view.data_ptr() + 2)), dict(out=C.c_void_p(out.view.data_ptr() + 2))):
        assert Lb.cc_dev_attention(*args(**bad)) != 0, bad
        assert out.untouched(), bad


# ---- LayerNorm --------------------------------------------------------------------------------------------------------------------------
def layernorm_ratio(c: ck.LnCase):
    i = ck.ln_inputs(c)
    buf = np.where(i["read"], i["buf"], np.float32(NAN)).astype(np.float32)      # what the kernel must not read is NaN
    gin = _np_in(buf, c.row_stride)
    gw, gb = _np_in(i["w"], c.D), _np_in(i["b"], c.D)
    odt = torch.float32 if (c.out_f32 or c.dt == "f32") else ck.TORCH_DT[c.dt]
    gout = Guarded(c.rows * c.D, odt, c.D)
    # the index addresses rows of `row_stride` floats from row 0 of the buffer, `offset` floats into it
    idx = torch.tensor(c.index, dtype=torch.int32, device="cuda") if c.index else None
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_layernorm(ck.DTI[c.dt], C.c_void_p(gin.view.data_ptr() + 4 * c.offset), c.row_stride, _lib.ptr(idx), _lib.ptr(gw.view),
                                           _lib.ptr(gb.view), _lib.ptr(gout.view), c.out_f32, c.rows, c.D, None))
    assert gout.guards_intact() and gin.untouched() and gw.untouched() and gb.untouched(), f"{c.name}: a guard or an input was written"
    y, br = ck.ln_ref(c)
    return _judge(c.name, gout.view.double().cpu().numpy().reshape(c.rows, c.D), y, ck.ln_bar(br, y, ck.U[c.dt] if c.out16 else 0.0))


LN = [c for dt in ("f32", "f16", "bf16") for c in ck.ln_cases(dt)]


@pytest.mark.parametrize("c", LN, ids=[c.name for c in LN])
def test_layernorm_against_float64(c):
    layernorm_ratio(c)


def assemble_ratio(c: ck.AsmCase):
    i = ck.asm_inputs(c)
    gp = _in(i["patches"], c.D)
    g = {k: _np_in(i[k], c.D) for k in ("cls", "pos", "w", "b")}
    gout = Guarded(c.B * c.L * c.D, torch.float32, c.D)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_assemble_ln(ck.DTI[c.dt], _lib.ptr(gp.view), _lib.ptr(g["cls"].view), _lib.ptr(g["pos"].view), _lib.ptr(g["w"].view),
                                             _lib.ptr(g["b"].view), _lib.ptr(gout.view), c.B, c.L, c.D, None))
    assert gout.guards_intact() and gp.untouched() and all(x.untouched() for x in g.values()), f"{c.name}: a guard or an input was written"
    y, br = ck.asm_ref(c)
    return _judge(c.name, gout.view.double().cpu().numpy().reshape(c.B * c.L, c.D), y, ck.ln_bar(br, y))


ASM = [c for dt in ("f32", "f16", "bf16") for c in ck.asm_cases(dt)]


@pytest.mark.parametrize("c", ASM, ids=[c.name for c in ASM])
def test_assemble_ln_against_float64(c):
    assemble_ratio(c)


def test_layernorm_and_assemble_refuse_wide_rows():
    L = _lib.lib()
    x, w, out = _np_in(np.ones(2 * 1025, np.float32), 1025), _np_in(np.ones(1025, np.float32), 1025), Guarded(2 * 1025, torch.float32, 1025)
    ln = lambda **k: L.cc_dev_layernorm(k.get("dt", 0), k.get("x", _lib.ptr(x.view)), k.get("D", 1024), None, _lib.ptr(w.view), _lib.ptr(w.view),   # noqa: E731
                                        k.get("out", _lib.ptr(out.view)), 1, k.get("rows", 2), k.get("D", 1024), None)
    for bad in (dict(D=1025), dict(D=0), dict(rows=0), dict(dt=3), dict(x=None), dict(out=None)):
        assert ln(**bad) != 0, bad
        assert out.untouched(), bad
    p = _np_in(np.ones(2 * 1025, np.float32), 1025)
    asm = lambda **k: L.cc_dev_assemble_ln(k.get("dt", 0), k.get("p", _lib.ptr(p.view)), _lib.ptr(w.view), _lib.ptr(x.view), _lib.ptr(w.view), _lib.ptr(w.view),   # noqa: E731
                                           _lib.ptr(out.view), k.get("B", 1), 2, k.get("D", 1024), None)
    for bad in (dict(D=1025), dict(D=0), dict(B=0), dict(dt=7), dict(p=None)):
        assert asm(**bad) != 0, bad
        assert out.untouched(), bad


# ---- patchify, embed, l2norm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("shape", ck.PATCH_SHAPES, ids=lambda s: "S%d-p%d-K%d" % s)
def test_patchify_bit_exact(shape, dt):
    S, patch, Kpad = shape
    x = ck.patch_input(S)
    B, g = x.shape[0], S // patch
    gin = _np_in(x, S)
    gout = Guarded(B * g * g * Kpad, ck.TORCH_DT[dt], Kpad)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_patchify(ck.DTI[dt], _lib.ptr(gin.view), _lib.ptr(gout.view), B, S, patch, Kpad, None))
    assert gout.guards_intact() and gin.untouched()
    ref = ck.patchify_ref(x, patch, Kpad, dt)
    bits = BITS[ref.dtype]
    got = gout.view.cpu().reshape(ref.shape)
    diff = (got.view(bits) != ref.view(bits)).nonzero()
    assert diff.numel() == 0, f"patchify {shape} {dt}: {len(diff)} elements differ, first at {diff[0].tolist()}"
    assert not got[:, 3 * patch * patch:].view(bits).any()                       # the pad columns: +0, bit for bit


def test_patchify_refusals():
    L = _lib.lib()
    x, out = _np_in(ck.patch_input(8), 8), Guarded(2 * 4 * 64, torch.float32, 64)
    call = lambda dt=0, xp=_lib.ptr(x.view), B=2, S=8, patch=4, Kpad=64: L.cc_dev_patchify(dt, xp, _lib.ptr(out.view), B, S, patch, Kpad, None)   # noqa: E731
    for bad in (dict(patch=3), dict(Kpad=47), dict(B=0), dict(S=0), dict(patch=0), dict(dt=3), dict(xp=None)):
        assert call(**bad) != 0, bad
        assert out.untouched(), bad


def _embed(D, tokens):
    table, pos = ck.embed_inputs(D)
    gt, gp = _np_in(table, D), _np_in(pos, D)
    gout = Guarded(ck.EMBED_B * ck.EMBED_L * D, torch.float32, D)
    tok = np.ascontiguousarray(tokens, np.int32)
    torch.cuda.synchronize()
    rc = _lib.lib().cc_dev_embed(_lib.ptr(tok), ck.EMBED_VOCAB, _lib.ptr(gt.view), _lib.ptr(gp.view), _lib.ptr(gout.view), ck.EMBED_B, ck.EMBED_L, D, None)
    assert gt.untouched() and gp.untouched()
    return rc, gout


@pytest.mark.parametrize("D", ck.EMBED_D)
def test_embed_bit_exact_and_token_range(D):
    rc, gout = _embed(D, ck.EMBED_TOKENS)
    _lib.check(rc)
    assert gout.guards_intact()
    got, ref = gout.view.cpu().numpy().reshape(-1, D), ck.embed_ref(D)
    diff = np.argwhere(got.view(np.int32) != ref.view(np.int32))
    assert diff.size == 0, f"embed D={D}: {len(diff)} elements differ, first at {diff[0].tolist()}"
    for bad in (ck.EMBED_VOCAB, -1):                                              # checked on the host: an error, and no launch
        tok = ck.EMBED_TOKENS.copy()
        tok[1, 3] = bad
        rc, gout = _embed(D, tok)
        assert rc != 0 and gout.untouched(), bad


def l2norm_ratio(D, eps):
    x = ck.l2_input(D, eps)
    g = _np_in(x, D)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cc_dev_l2norm(_lib.ptr(g.view), x.shape[0], D, C.c_float(eps), None))
    assert g.guards_intact()
    y = ck.l2_ref(x, eps)
    got = g.view.double().cpu().numpy().reshape(x.shape)
    if eps > 0:
        assert not got[3].any(), f"l2norm D={D}: the all-zero row did not stay zero"
    return _judge(f"l2norm-D{D}-eps{eps:g}", got, y, ck.l2_bar(y))


@pytest.mark.parametrize("eps", ck.L2_EPS)
@pytest.mark.parametrize("D", ck.L2_D)
def test_l2norm_against_float64(D, eps):
    l2norm_ratio(D, eps)


def test_l2norm_refusals():
    L = _lib.lib()
    g = _np_in(np.ones((2, 8), np.float32), 8)
    for args in ((None, 2, 8, 0.0), (_lib.ptr(g.view), 0, 8, 0.0), (_lib.ptr(g.view), 2, 0, 0.0), (_lib.ptr(g.view), 2, 8, -1.0)):
        assert L.cc_dev_l2norm(args[0], args[1], args[2], C.c_float(args[3]), None) != 0, args
        assert g.untouched()
