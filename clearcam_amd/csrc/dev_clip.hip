// Development entries that run ONE launch of a CLIP tower kernel other than the GEMMs, outside any plan, on buffers the caller owns:
// cc_dev_attention (attn_mfma_kernel / attn_simple_kernel), cc_dev_layernorm, cc_dev_assemble_ln, cc_dev_patchify, cc_dev_embed and
// cc_dev_l2norm.  Each validates its arguments and launches nothing on bad input, makes exactly one call to the production launcher
// (clip_kernels.hip) and synchronises the stream.  Only cc_dev_embed allocates: the device copy of its host tokens, freed before it returns.
#include <cmath>
#include "kernels.h"
#include "../../include/clearcam_hip.h"

using namespace cc;

namespace {

void check_dtype(int dt) { CC_CHECK(dt == F32 || dt == F16 || dt == BF16, "dtype must be 0 (f32), 1 (f16) or 2 (bf16)"); }
bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

extern "C" {

int cc_dev_attention(int dtype, const void* qkv_dev, int B, int L, int H, int causal, float scale, void* ctx_dev, void* stream) {
  CC_API_BEGIN
  CC_CHECK(qkv_dev && ctx_dev, "null argument");
  check_dtype(dtype);
  CC_CHECK(B > 0 && H > 0 && B <= 65535 && H <= 65535, "bad shape");   // grid (1, H, B)
  CC_CHECK(L >= 1 && L <= 288, "attention: 1..288 tokens");
  CC_CHECK(scale > 0.f && scale < INFINITY, "attention: scale must be positive (the row maximum is taken on the raw scores)");
  // attn_mfma_kernel reads 16-byte chunks of q / k / v and stores 8-byte groups; attn_simple_kernel single elements
  CC_CHECK(dtype == F32 ? aligned(qkv_dev, 4) && aligned(ctx_dev, 4) : aligned(qkv_dev, 16) && aligned(ctx_dev, 8), "misaligned buffer");
  AttnP p{};
  p.qkv = qkv_dev; p.ctx = ctx_dev; p.B = B; p.L = L; p.H = H; p.D = 64 * H; p.causal = causal ? 1 : 0; p.scale = scale; p.abl = 0;
  launch_attention(dtype, p, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

int cc_dev_layernorm(int dtype, const float* in_dev, long long in_row_stride, const int32_t* row_index_dev, const float* w_dev, const float* b_dev,
                     void* out_dev, int out_f32, int rows, int D, void* stream) {
  CC_API_BEGIN
  CC_CHECK(in_dev && w_dev && b_dev && out_dev, "null argument");
  check_dtype(dtype);
  CC_CHECK(rows > 0 && D > 0 && in_row_stride >= 0, "bad shape");
  CC_CHECK(D <= 1024, "layernorm: D > 1024");
  CC_CHECK(aligned(in_dev, 4) && aligned(w_dev, 4) && aligned(b_dev, 4) && aligned(out_dev, out_f32 || dtype == F32 ? 4 : 2), "misaligned buffer");
  LnP p{};
  p.in = in_dev; p.in_row_stride = (long)in_row_stride; p.row_index = row_index_dev; p.w = w_dev; p.b = b_dev;
  p.out = out_dev; p.out_f32 = out_f32 ? 1 : 0; p.rows = rows; p.D = D;
  launch_layernorm(dtype, p, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

int cc_dev_assemble_ln(int dtype, const void* patches_dev, const float* cls_dev, const float* pos_dev, const float* w_dev, const float* b_dev,
                       float* out_dev, int B, int L, int D, void* stream) {
  CC_API_BEGIN
  CC_CHECK(patches_dev && cls_dev && pos_dev && w_dev && b_dev && out_dev, "null argument");
  check_dtype(dtype);
  CC_CHECK(B > 0 && L > 0 && D > 0 && (long)B * L < (1L << 28), "bad shape");
  CC_CHECK(D <= 1024, "assemble: D > 1024");
  AssembleP p{};
  p.patches = patches_dev; p.cls = cls_dev; p.pos = pos_dev; p.w = w_dev; p.b = b_dev; p.out = out_dev; p.B = B; p.L = L; p.D = D;
  launch_assemble_ln(dtype, p, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

int cc_dev_patchify(int dtype, const float* x_dev, void* out_dev, int B, int S, int patch, int Kpad, void* stream) {
  CC_API_BEGIN
  CC_CHECK(x_dev && out_dev, "null argument");
  check_dtype(dtype);
  CC_CHECK(B > 0 && S > 0 && patch > 0 && Kpad > 0, "bad shape");
  CC_CHECK(S % patch == 0, "patchify: the image side is not a multiple of the patch");
  CC_CHECK(patch <= 1024 && Kpad >= 3 * patch * patch, "patchify: Kpad < 3 * patch * patch");
  CC_CHECK((long)B * (S / patch) * (S / patch) * Kpad < (1L << 38), "patchify: more blocks than one launch holds");
  PatchP p{};
  p.x = x_dev; p.out = out_dev; p.B = B; p.S = S; p.patch = patch; p.Kpad = Kpad;
  launch_patchify(dtype, p, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

int cc_dev_embed(const int32_t* tokens, int vocab, const float* table_dev, const float* pos_dev, float* out_dev, int B, int L, int D, void* stream) {
  int* tok_dev = nullptr;
  try {
    CC_CHECK(tokens && table_dev && pos_dev && out_dev, "null argument");
    CC_CHECK(vocab > 0 && B > 0 && L > 0 && D > 0 && (long)B * L < (1L << 28), "bad shape");
    for (size_t i = 0; i < (size_t)B * L; ++i) CC_CHECK(tokens[i] >= 0 && tokens[i] < vocab, "token id out of range");
    CC_HIP(hipMalloc(reinterpret_cast<void**>(&tok_dev), (size_t)B * L * sizeof(int)));
    CC_HIP(hipMemcpyAsync(tok_dev, tokens, (size_t)B * L * sizeof(int), hipMemcpyHostToDevice, (hipStream_t)stream));
    launch_embed(EmbedP{tok_dev, table_dev, pos_dev, out_dev, B, L, D}, (hipStream_t)stream);
    CC_HIP(hipStreamSynchronize((hipStream_t)stream));
    hipFree(tok_dev);
    return 0;
  } catch (const cc::Error& e) { hipFree(tok_dev); cc::set_error(e.what()); return e.code; }
  catch (const std::exception& e) { hipFree(tok_dev); cc::set_error(e.what()); return -1; }
}

int cc_dev_l2norm(float* x_dev, int rows, int D, float eps, void* stream) {
  CC_API_BEGIN
  CC_CHECK(x_dev, "null argument");
  CC_CHECK(rows > 0 && D > 0 && eps >= 0.f && eps < INFINITY, "bad shape");
  launch_l2norm(NormP{x_dev, rows, D, eps}, (hipStream_t)stream);
  CC_HIP(hipStreamSynchronize((hipStream_t)stream));
  CC_API_END
}

}  // extern "C"
