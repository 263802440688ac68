"""CPU checks of tests/clip_kernel_cases.py - everything tests/test_gpu_clip_kernels.py relies on, held before anything runs on a GPU:
1. each float64 reference agrees to 1e-12 with an independent torch-float64 statement of the same operation;
2. the float32 / storage-type emulation of each kernel's arithmetic stays within its bar on every case (attention, LayerNorm: below 0.8);
3. every mutant of the float64 model exceeds the bar at least fourfold at some element, in at least one case of each input family it
   applies to and for each storage type - the cases are strong enough to see it;
4. the planted keys hold their mass, and no weight of the uniform family is below f16's normal range."""
import numpy as np
import pytest
import torch

import clip_kernel_cases as ck

DT16 = ("f16", "bf16")
DTS = ("f32", "f16", "bf16")


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- 1. references ---------------------------------------------------------------------------------------------------------------------
def _attn_torch(c):
    x = ck.attn_inputs(c).double().reshape(c.B, c.L, 3, c.H, 64)
    out = torch.empty(c.B, c.L, c.H, 64, dtype=torch.float64)
    mask = torch.full((c.L, c.L), float("-inf"), dtype=torch.float64).triu(1) if c.causal else torch.zeros(c.L, c.L, dtype=torch.float64)
    for b in range(c.B):
        for h in range(c.H):
            q, k, v = x[b, :, 0, h], x[b, :, 1, h], x[b, :, 2, h]
            out[b, :, h] = torch.softmax(q @ k.T * c.scale + mask, -1) @ v
    return out.reshape(c.B * c.L, c.D).numpy()


@pytest.mark.parametrize("dt", DTS)
def test_attention_reference_agrees_with_torch(dt):
    for c in ck.attn_cases(dt):
        if c.L in (1, 17, 77, 257, 288) or c.tag:
            assert _rel(ck.attn_ref(c).out, _attn_torch(c)) <= 1e-12, c.name


def test_layernorm_and_assemble_references_agree_with_torch():
    for c in ck.ln_cases("f32"):
        i = ck.ln_inputs(c)
        x = torch.from_numpy(np.stack([i["buf"][s:s + c.D] for s in c.starts()])).double()
        ref = torch.nn.functional.layer_norm(x, (c.D,), torch.from_numpy(i["w"]).double(), torch.from_numpy(i["b"]).double(), 1e-5).numpy()
        assert _rel(ck.ln_ref(c)[0], ref) <= 1e-12, c.name
    for dt in DTS:
        for c in ck.asm_cases(dt):
            i = ck.asm_inputs(c)
            tok = torch.cat((torch.from_numpy(i["cls"]).double().expand(c.B, 1, c.D), i["patches"].double().reshape(c.B, c.L - 1, c.D)), 1)
            tok = tok + torch.from_numpy(i["pos"]).double()
            ref = torch.nn.functional.layer_norm(tok, (c.D,), torch.from_numpy(i["w"]).double(), torch.from_numpy(i["b"]).double(), 1e-5)
            assert _rel(ck.asm_ref(c)[0], ref.reshape(c.B * c.L, c.D).numpy()) <= 1e-12, c.name


def test_patchify_embed_l2norm_references_agree_with_torch():
    for S, patch, Kpad in ck.PATCH_SHAPES:
        x = ck.patch_input(S)
        unf = torch.nn.functional.unfold(torch.from_numpy(x), patch, stride=patch).transpose(1, 2).reshape(-1, 3 * patch * patch)   # (B*g*g, c p p)
        for dt in DTS:
            ref = ck.patchify_ref(x, patch, Kpad, dt)
            assert torch.equal(ref[:, :3 * patch * patch].float(), unf.to(ck.TORCH_DT[dt]).float()) and not ref[:, 3 * patch * patch:].any(), (S, dt)
        ties = ck.patchify_ref(x, patch, Kpad, "f16").float() != ck.patchify_ref(x, patch, Kpad, "f32")
        assert ties.any()
    for D in ck.EMBED_D:
        table, pos = ck.embed_inputs(D)
        ref = torch.nn.functional.embedding(torch.from_numpy(ck.EMBED_TOKENS).long(), torch.from_numpy(table)) + torch.from_numpy(pos)
        assert np.array_equal(ck.embed_ref(D), ref.reshape(-1, D).numpy())
        assert {0, ck.EMBED_VOCAB - 1} <= set(ck.EMBED_TOKENS.ravel().tolist()) and len(set(ck.EMBED_TOKENS.ravel().tolist())) < ck.EMBED_TOKENS.size
    for D in ck.L2_D:
        for eps in ck.L2_EPS:
            x = ck.l2_input(D, eps)
            t = torch.from_numpy(x).double()
            ref = t / (torch.linalg.vector_norm(t, dim=-1, keepdim=True) + float(np.float32(eps)))
            assert np.allclose(ck.l2_ref(x, eps), ref.numpy(), rtol=1e-12, atol=0), (D, eps)
            zero_rows = (~x.any(-1)).sum()
            assert zero_rows == (1 if eps > 0 else 0)
            if eps > 0:
                assert not ck.l2_ref(x, eps)[3].any()


# ---- 2. emulations within the bars -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_attention_emulation_within_bar(dt):
    top = (0.0, "")
    for c in ck.attn_cases(dt):
        r = ck.attn_ref(c)
        ratio, i = ck.worst(np.abs(ck.attn_emulate(c) - r.out), ck.attn_bar(c, r))
        top = max(top, (ratio, c.name))
        assert ratio < 0.8, (c.name, i, ratio)
    print(f"attention {dt}: emulation reaches {top[0]:.3f} of the bar ({top[1]})")


@pytest.mark.parametrize("dt", DTS)
def test_layernorm_emulation_within_bar(dt):
    top = (0.0, "")
    forms = set()
    for c in ck.ln_cases(dt):
        y, br = ck.ln_ref(c)
        ratio, i = ck.worst(np.abs(ck.ln_emulate(c) - y), ck.ln_bar(br, y, ck.U[dt] if c.out16 else 0.0))
        top = max(top, (ratio, c.name))
        forms.add((c.vec, c.tag))
        if c.out16:     # the rounding to the storage type alone reaches u |y| just above a power of two: the rounded value is held to the whole
            # bar, the float32 value in front of the rounding to 0.8 of the float32 term
            assert ratio <= 1.0, (c.name, i, ratio)
            i_ = ck.ln_inputs(c)
            y32 = ck.ln_emulate_f32(np.stack([i_["buf"][s:s + c.D] for s in c.starts()]), i_["w"], i_["b"], c.vec)
            ratio, i = ck.worst(np.abs(y32 - y), ck.ln_bar(br, y))
        assert ratio < 0.8, (c.name, i, ratio)
    assert {(True, ""), (False, ""), (False, "off1"), (False, "stride769"), (True, "gather"), (True, "clspool")} <= forms
    print(f"layernorm {dt}: emulation reaches {top[0]:.3f} of the bar ({top[1]})")
    for c in ck.asm_cases(dt):
        y, br = ck.asm_ref(c)
        ratio, i = ck.worst(np.abs(ck.asm_emulate(c) - y), ck.ln_bar(br, y))
        assert ratio < 0.8, (c.name, i, ratio)


def test_layernorm_constant_row_gives_beta():
    for c in ck.ln_cases("f32"):
        i = ck.ln_inputs(c)
        y = ck.ln_ref(c)[0]
        for r in range(c.rows):
            if ck.ROW_KINDS[(r + c.D) % 5] == "const":
                assert np.array_equal(y[r], i["b"].astype(np.float64)), c.name


def test_l2norm_emulation_within_bar():
    for D in ck.L2_D:
        for eps in ck.L2_EPS:
            x = ck.l2_input(D, eps)
            y = ck.l2_ref(x, eps)
            ratio, i = ck.worst(np.abs(ck.l2_emulate(x, eps) - y), ck.l2_bar(y))
            assert ratio <= 1.0, (D, eps, i, ratio)


EDGE_MUTANTS = ("drop_last", "drop_16", "no_diagonal", "admit_next", "pad_key")


# ---- 3. mutants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_attention_mutants_exceed_the_bar(dt):
    """For each mutant and each family it applies to: the largest err / bar over the cases of that family is >= 4.  Sharper in the planted
    family: at EVERY length, dropping the last key, key 16 or the diagonal, or admitting the padding key or the key after the diagonal,
    exceeds the bar fourfold - the late-row and padding-edge errors a cosine over a whole tower cannot see."""
    best = {}
    for c in ck.attn_cases(dt):
        if c.tag:
            continue
        r = ck.attn_ref(c)
        bar = ck.attn_bar(c, r)
        for m in ck.ATTN_MUTANTS:
            if ck.mutant_applies(c, m):
                ratio, _ = ck.worst(np.abs(ck.attn_ref(c, m).out - r.out), bar)
                if c.family == "planted" and m in EDGE_MUTANTS:
                    assert ratio >= 4.0, (c.name, m, ratio)
                key = (m, c.family)
                best[key] = max(best.get(key, (0.0, "")), (ratio, c.name))
    expect = [m for m in ck.ATTN_MUTANTS if not (dt == "f32" and m == "split_no_rescale")]
    assert sorted({m for m, _ in best}) == sorted(expect)
    for (m, fam), (ratio, name) in sorted(best.items()):
        print(f"{dt} {m:18s} {fam:8s} {ratio:10.1f} x bar ({name})")
        assert ratio >= 4.0, (dt, m, fam, ratio, name)


@pytest.mark.parametrize("dt", DTS)
def test_layernorm_assemble_l2norm_mutants_exceed_the_bar(dt):
    for o32 in (0, 1):
        best = {}
        for c in ck.ln_cases(dt):
            if c.out_f32 != o32:
                continue
            y, br = ck.ln_ref(c)
            bar = ck.ln_bar(br, y, ck.U[dt] if c.out16 else 0.0)
            for m in ck.LN_MUTANTS:
                if ck.ln_mutant_applies(c, m):
                    best[m] = max(best.get(m, 0.0), ck.worst(np.abs(ck.ln_ref(c, m)[0] - y), bar)[0])
        assert sorted(best) == sorted(ck.LN_MUTANTS)
        for m, ratio in best.items():
            assert ratio >= 4.0, (dt, o32, m, ratio)
    for c in ck.asm_cases(dt):
        y, br = ck.asm_ref(c)
        for m in ck.ASM_MUTANTS:
            assert ck.worst(np.abs(ck.asm_ref(c, m)[0] - y), ck.ln_bar(br, y))[0] >= 4.0, (c.name, m)
    if dt == "f32":
        for D in ck.L2_D:
            x = ck.l2_input(D, 1e-8)
            y = ck.l2_ref(x, 1e-8)
            assert ck.worst(np.abs(ck.l2_ref(x, 1e-8, "eps_under_root") - y), ck.l2_bar(y))[0] >= 4.0, D


# ---- 4. what the input families promise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_attention_families_hold_their_conditions(dt):
    for c in ck.attn_cases(dt):
        r = ck.attn_ref(c)
        if c.tag == "peaked":
            assert r.e_min < 2.0 ** -14 and (r.S > 0).mean() > 0.5, c.name          # most weights underflow f16
            continue
        assert not r.S.any(), c.name
        if c.family == "uniform":
            assert r.e_min >= 2.0 ** -14, (c.name, np.log2(r.e_min))
        else:
            vis = ck._visible(c.L, c.causal)
            for j in ck.planted_keys(c.L):
                assert r.p[:, :, vis[:, j], j].min() >= 0.05, (c.name, j, r.p[:, :, vis[:, j], j].min())
            if c.causal:
                d = np.arange(c.L)
                assert r.p[:, :, d, d].min() >= 0.05, (c.name, "diagonal", r.p[:, :, d, d].min())
            x = ck.f64(ck.attn_inputs(c)).reshape(c.B, c.L, 3, c.H, 64)
            assert np.abs(x[:, ck.planted_keys(c.L), 2]).min() >= 4.0
        if c.copy_batch:
            x = ck.attn_inputs(c).reshape(c.B, c.L, -1)
            assert torch.equal(x[0], x[1])


def test_split_ranges_cover_every_key_once():
    for L in ck.ATTN_L16:
        rng = ck.split_ranges(L)
        assert (rng is not None) == (L in (65, 77, 80, 129, 144, 208, 257, 272)), L
        if rng:
            assert rng[0][0] == 0 and all(a[1] == b[0] for a, b in zip(rng, rng[1:])) and rng[-1][1] == (96 if L <= 96 else 288)
