// The frozen image tower in training mode (reference trainers/classification/vpt.py: VPT's shallow prompt `visual.VPT` and the deep prompts
// `visual.transformer.resblocks.{i}.VPT_shallow`; clip/model.py: VisionTransformer.forward with the prompt rows appended behind the patch
// rows): its training forward with a stash and its backward down to the prompt rows, which VPT's step (prompt_train.hip) puts between its
// loss head and its SGD step.  DESIGN.md "VPT fit" has the data flow, the stash and the rounding points.
//
// The blocks are the text training tower's (text_backward.hip: LayerNorm, GEMM, attention, QuickGELU as separate launches on the fp32
// residual stream; every Linear's backward is the forward's fp16 GEMM on a transposed copy of the weight) without a mask, and the
// attention backward is attention.hip's attention_backward_full_kernel (beyond 224 rows per image, option vision_train_long: its two-launch
// sibling attention_backward_long).  New here:
//   splice_reduce_kernel   the gradient of one block's prompt rows: the batch's rows added in ascending order, the rows zeroed behind
// Nothing below ln_pre is differentiated: patch rows, the class embedding and conv1 are frozen.
// No float atomics and no workgroup waits for another: the same inputs give the same bits.
#include <cmath>

#include "common.h"
#include "model.h"

namespace clipmi {
namespace {

constexpr int THREADS = 256;

// out[j, d] = sum_b g[(b L + first + j) D + d], b ascending; with `zero` the rows are cleared in g and g16 afterwards (the block below the
// splice never sees them: its output rows there were overwritten by the prompt)
__global__ __launch_bounds__(THREADS) void splice_reduce_kernel(float* __restrict__ g, half_t* __restrict__ g16, float* __restrict__ out, int B, int L, int D,
                                                                int first, int n_ctx, int zero) {
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= (int64_t)n_ctx * D) return;
  const int d = (int)(idx % D), j = (int)(idx / D);
  float s = 0.f;
  for (int64_t b = 0; b < B; ++b) {
    const int64_t at = (b * L + first + j) * D + d;
    s += g[at];
    if (zero) {
      g[at] = 0.f;
      g16[at] = (half_t)0.f;
    }
  }
  out[idx] = s;
}

}  // namespace

int launch_splice_reduce(float* g, half_t* g16, float* out, int B, int L, int D, int first, int n_ctx, int zero, hipStream_t s) {
  hipLaunchKernelGGL(splice_reduce_kernel, dim3((unsigned)(((int64_t)n_ctx * D + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, g, g16, out, B, L, D, first,
                     n_ctx, zero);
  return check_launch("splice_reduce_kernel");
}

namespace {

// The front end in front of ln_pre.  Patch rows that are whole 16-byte LDS slots (P in {8, 16, 32}) go through patch_embed.hip's im2col-free
// loader; every other patch size that divides the resolution (ViT-L/14: kpad 640 against K = 588) takes the inference pass's route
// (capi.hip, encode_image_pass): patchify into the [B G^2, kpad] fp16 matrix, then the dense GEMM whose epilogue adds the positional rows.
bool loader_serves(const clipmi_model* m, int B) {
  const int P = m->g.patch_size;
  return patch_embed_fits(B, m->g.image_resolution, P, m->g.vision_width) && m->kpad() == 3 * P * P;
}

// behind the text tower's workspace: the fp32 gradient stream, the front end's slot (the fp16 copy of an fp32 image batch for the loader,
// the im2col matrix for the patchify route, which reads the image itself), the prompts as fp16, slot 0's batch sum
struct VisionWs {
  TrainWs t;
  float* g;        // [M, D]
  void* img16;     // patch_embed_scratch_bytes(B, R, fp32), or col_bytes(B): [B G^2, kpad] fp16
  half_t* p16;     // [layers, n_ctx, D]
  float* dsum;     // [n_ctx, D]
  void* abl;       // attention_backward_long's statistics, beyond ABF_MAX_L rows per image only (shorter geometries keep their size)
  size_t abl_bytes;
  size_t bytes;
};
VisionWs carve_vision_ws(void* p, const clipmi_model* m, int B, int n_ctx) {
  const int D = m->g.vision_width, L = m->tokens0() + n_ctx;
  const int64_t M = (int64_t)B * L;
  VisionWs w;
  w.t = carve_ws(p, M, B, D, m->g.embed_dim);
  Carver c(p);
  c.off = w.t.bytes;
  w.g = c.take<float>((size_t)M * D * 4);
  w.img16 = c.take<char>(loader_serves(m, B) ? patch_embed_scratch_bytes(B, m->g.image_resolution, CLIPMI_F32) : m->col_bytes(B));
  w.p16 = c.take<half_t>((size_t)m->g.vision_layers * n_ctx * D * 2);
  w.dsum = c.take<float>((size_t)n_ctx * D * 4);
  w.abl_bytes = L > ABF_MAX_L ? attention_backward_long_bytes(B, L, D / 64) : 0;
  w.abl = w.abl_bytes ? c.take<char>(w.abl_bytes) : nullptr;
  w.bytes = c.off;
  return w;
}

// the text stash's layout over M = B L rows (idx: the class rows b L, and B zeros behind them), then the prompts rounded through fp16
struct VisionStash {
  Stash st;
  float* prompts;   // [layers, n_ctx, D] fp32
  size_t bytes;
};
VisionStash carve_vision_stash(void* p, const clipmi_model* m, int B, int n_ctx) {
  const int D = m->g.vision_width, L = m->tokens0() + n_ctx;
  VisionStash v;
  v.st = carve_stash(p, (int64_t)B * L, D, m->g.vision_layers);
  const size_t head = v.st.bytes(B);
  v.prompts = p ? reinterpret_cast<float*>(static_cast<char*>(p) + head) : nullptr;
  v.bytes = head + align256((size_t)m->g.vision_layers * n_ctx * D * 4);
  return v;
}

int check_vision_shape(const char* who, const clipmi_model* m, int B, int n_ctx) {
  CLIPMI_REQUIRE(m, CLIPMI_ERR_ARG, "%s: null model", who);
  CLIPMI_REQUIRE(B >= 0 && n_ctx >= 1, CLIPMI_ERR_SHAPE, "%s: B=%d n_ctx=%d", who, B, n_ctx);
  const int L = m->tokens0() + n_ctx;
  const int max_l = options().vision_train_long.load(std::memory_order_relaxed) != 0 ? ABL_MAX_L : ABF_MAX_L;   // DESIGN.md "Long attention backward"
  CLIPMI_REQUIRE(L <= max_l, CLIPMI_ERR_SHAPE, "%s: %d token rows per image (%d tokens + %d prompt rows; at most %d)", who, L, m->tokens0(), n_ctx, max_l);
  CLIPMI_REQUIRE((int64_t)B * L < (1ll << 31) / 4, CLIPMI_ERR_SHAPE, "%s: batch too large for one call", who);
  CLIPMI_REQUIRE(m->g.vision_width % 64 == 0 && m->g.embed_dim % 64 == 0, CLIPMI_ERR_SHAPE, "%s: vision width %d / embed dim %d", who, m->g.vision_width,
                 m->g.embed_dim);
  // what launch_patchify and the patch GEMM ask of the geometry (kpad is a multiple of the GEMM's K-step by construction)
  CLIPMI_REQUIRE(m->g.patch_size > 0 && m->g.image_resolution > 0 && m->g.image_resolution % m->g.patch_size == 0, CLIPMI_ERR_SHAPE,
                 "%s: resolution %d is not a multiple of the patch size %d", who, m->g.image_resolution, m->g.patch_size);
  return CLIPMI_OK;
}

}  // namespace

int check_vision_train_call(const char* who, const clipmi_model* m, int B, int n_ctx, int depth, const void* ws, size_t ws_bytes, const void* stash,
                            size_t stash_bytes) {
  if (int rc = check_vision_shape(who, m, B, n_ctx)) return rc;
  CLIPMI_REQUIRE(m->has_vision, CLIPMI_ERR_STATE, "%s: vision weights not bound (clipmi_set_vision_weights)", who);
  CLIPMI_REQUIRE(depth >= 1 && depth <= m->g.vision_layers, CLIPMI_ERR_SHAPE, "%s: depth=%d for %d layers", who, depth, m->g.vision_layers);
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(ws && stash, CLIPMI_ERR_ARG, "%s: null workspace or stash", who);
  CLIPMI_REQUIRE((uintptr_t)ws % 256 == 0 && (uintptr_t)stash % 256 == 0, CLIPMI_ERR_ARG, "%s: workspace and stash must be 256-byte aligned", who);
  const size_t need_ws = carve_vision_ws(nullptr, m, B, n_ctx).bytes, need_st = carve_vision_stash(nullptr, m, B, n_ctx).bytes;
  CLIPMI_REQUIRE(ws_bytes >= need_ws, CLIPMI_ERR_WORKSPACE, "%s: workspace too small: %zu < %zu", who, ws_bytes, need_ws);
  CLIPMI_REQUIRE(stash_bytes >= need_st, CLIPMI_ERR_WORKSPACE, "%s: stash too small: %zu < %zu", who, stash_bytes, need_st);
  return CLIPMI_OK;
}

int check_vision_dgrad(const char* who, const clipmi_model* m, const clipmi_vision_dgrad* wt) {
  CLIPMI_REQUIRE(wt && wt->proj && wt->blocks, CLIPMI_ERR_ARG, "%s: null transposed weights", who);
  CLIPMI_REQUIRE((uintptr_t)wt->proj % 16 == 0, CLIPMI_ERR_ARG, "%s: transposed weights must be 16-byte aligned", who);
  for (int i = 0; i < m->g.vision_layers; ++i) {
    const void* p[] = {wt->blocks[i].w_qkv_t, wt->blocks[i].w_out_t, wt->blocks[i].w_fc_t, wt->blocks[i].w_proj_t};
    for (const void* q : p) CLIPMI_REQUIRE(q && (uintptr_t)q % 16 == 0, CLIPMI_ERR_ARG, "%s: block %d: null or unaligned transposed weight", who, i);
  }
  return CLIPMI_OK;
}

int run_vision_train_forward(clipmi_model* m, const void* image, int image_dtype, int B, const float* prompts, int n_ctx, int depth, float* out,
                             void* workspace, void* stash_p, hipStream_t s) {
  const clipmi_geometry& g = m->g;
  const int L0 = m->tokens0(), L = L0 + n_ctx, D = g.vision_width, E = g.embed_dim, H = D / 64, layers = g.vision_layers;
  const int64_t M = (int64_t)B * L, per = (int64_t)n_ctx * D;
  const VisionWs vw = carve_vision_ws(workspace, m, B, n_ctx);
  const VisionStash vs = carve_vision_stash(stash_p, m, B, n_ctx);
  const TrainWs& w = vw.t;
  const Stash& st = vs.st;
  int rc;
  // the fp32 masters rounded through fp16: the reference's .half()
  if ((rc = launch_cast_f32(prompts, vw.p16, CLIPMI_F16, depth * per, s))) return rc;
  if ((rc = launch_cast_f16(vw.p16, vs.prompts, CLIPMI_F32, depth * per, s))) return rc;
  float* x0 = w.dy;   // [M, D] embeddings before ln_pre
  const bool loader = loader_serves(m, B);
  if (loader) {
    if ((rc = launch_patch_embed(image, image_dtype, vw.img16, (const half_t*)m->vw.conv_w, m->kpad(), nullptr, x0, CLIPMI_F32, B, g.image_resolution,
                                 g.patch_size, D, L, s)))
      return rc;
  } else {
    half_t* col = static_cast<half_t*>(vw.img16);   // [B G^2, kpad], the columns behind 3 P^2 zero
    if ((rc = launch_patchify(image, image_dtype, col, B, g.image_resolution, g.patch_size, m->kpad(), s))) return rc;
    GemmArgs a{};
    a.A = col; a.lda = m->kpad(); a.W = (const half_t*)m->vw.conv_w; a.ldw = m->kpad(); a.out = x0; a.ldo = D; a.out_dtype = CLIPMI_F32;
    a.M = B * (L0 - 1); a.N = D; a.K = m->kpad(); a.epilogue = EPI_PATCH_POS;
    a.pos = m->vw.positional_embedding; a.patches = L0 - 1; a.tokens = L;   // this epilogue adds pos[1 + p] itself: ln_pre's pass must not
    if ((rc = launch_gemm(a, s))) return rc;
  }
  if ((rc = launch_embed_ln(x0, CLIPMI_F32, loader ? 1 : 0, m->vw.class_embedding, m->vw.positional_embedding, vs.prompts, m->vw.ln_pre_g, m->vw.ln_pre_b,
                            st.x(0), nullptr, nullptr, B, L, L0, D, 1e-5f, s)))
    return rc;
  if (hipMemsetAsync(st.idx() + B, 0, (size_t)B * 4, s) != hipSuccess) return check_launch("hipMemsetAsync");
  if ((rc = launch_eot_rows(st.idx() + B, st.idx(), B, L, s))) return rc;   // the class rows b L
  for (int i = 0; i < layers; ++i) {
    const clipmi_block_weights& b = m->vblocks[i];
    float *x_in = st.x(2 * i), *x_mid = st.x(2 * i + 1), *x_out = st.x(2 * i + 2);
    if (i > 0 && i < depth && (rc = launch_overwrite_tokens(x_in, vs.prompts + i * per, B, L, D, L0, n_ctx, s))) return rc;
    if ((rc = launch_layernorm(x_in, CLIPMI_F32, D, nullptr, b.ln1_g, b.ln1_b, w.xn, CLIPMI_F16, D, (int)M, D, 1e-5f, s))) return rc;
    if ((rc = tower_gemm(w.xn, D, b.w_qkv, D, b.b_qkv, nullptr, st.qkv(i), 3 * D, CLIPMI_F16, M, 3 * D, D, CLIPMI_EPI_BIAS, s))) return rc;
    if ((rc = launch_attention(st.qkv(i), w.att, B, L, H, 0, s))) return rc;
    if ((rc = tower_gemm(w.att, D, b.w_out, D, b.b_out, x_in, x_mid, D, CLIPMI_F32, M, D, D, CLIPMI_EPI_BIAS_RESIDUAL, s))) return rc;
    if ((rc = launch_layernorm(x_mid, CLIPMI_F32, D, nullptr, b.ln2_g, b.ln2_b, w.xn, CLIPMI_F16, D, (int)M, D, 1e-5f, s))) return rc;
    if ((rc = tower_gemm(w.xn, D, b.w_fc, D, b.b_fc, nullptr, st.h(i), 4 * D, CLIPMI_F16, M, 4 * D, D, CLIPMI_EPI_BIAS, s))) return rc;
    if ((rc = launch_quickgelu_forward(st.h(i), w.hid, M * 4 * D, s))) return rc;
    if ((rc = tower_gemm(w.hid, 4 * D, b.w_proj, 4 * D, b.b_proj, x_mid, x_out, D, CLIPMI_F32, M, D, 4 * D, CLIPMI_EPI_BIAS_RESIDUAL, s))) return rc;
  }
  if ((rc = launch_layernorm(st.x(2 * layers), CLIPMI_F32, D, st.idx(), m->vw.ln_post_g, m->vw.ln_post_b, w.rows16, CLIPMI_F16, D, B, D, 1e-5f, s))) return rc;
  return tower_gemm(w.rows16, D, m->vw.proj_t, D, nullptr, nullptr, out, E, CLIPMI_F32, B, E, D, CLIPMI_EPI_NONE, s);
}

int run_vision_backward(clipmi_model* m, const clipmi_vision_dgrad* wt, const float* d_out, int B, int n_ctx, int depth, float* d_prompts,
                        void* workspace, const void* stash_p, unsigned long long* stats, hipStream_t s) {
  const clipmi_geometry& gm = m->g;
  const int L0 = m->tokens0(), L = L0 + n_ctx, D = gm.vision_width, E = gm.embed_dim, H = D / 64, layers = gm.vision_layers;
  const int64_t M = (int64_t)B * L, per = (int64_t)n_ctx * D;
  const VisionWs vw = carve_vision_ws(workspace, m, B, n_ctx);
  const VisionStash vs = carve_vision_stash(const_cast<void*>(stash_p), m, B, n_ctx);
  const TrainWs& w = vw.t;
  const Stash& st = vs.st;
  float* g = vw.g;
  half_t* g16 = w.xn;
  int rc;
  // tail: d_out proj^T, ln_post's backward on the class rows, scattered into the zeroed stream
  if ((rc = launch_cast_f32(d_out, w.dfeat16, CLIPMI_F16, (int64_t)B * E, s))) return rc;
  if ((rc = launch_operand_stats(w.dfeat16, (int64_t)B * E, stats, s))) return rc;
  if ((rc = tower_gemm(w.dfeat16, E, wt->proj, E, nullptr, nullptr, w.dxf, D, CLIPMI_F32, B, D, E, CLIPMI_EPI_NONE, s))) return rc;
  if (hipMemsetAsync(g, 0, (size_t)M * D * 4, s) != hipSuccess || hipMemsetAsync(g16, 0, (size_t)M * D * 2, s) != hipSuccess) return check_launch("hipMemsetAsync");
  if ((rc = launch_ln_backward(st.x(2 * layers), D, st.idx(), m->vw.ln_post_g, w.dxf, CLIPMI_F32, g, g16, B, D, 1e-5f, s))) return rc;
  for (int i = layers - 1; i >= 0; --i) {
    const clipmi_block_weights& b = m->vblocks[i];
    const clipmi_block_dgrad& t = wt->blocks[i];
    if ((rc = launch_operand_stats(g16, M * D, stats, s))) return rc;
    if ((rc = tower_gemm(g16, D, t.w_proj_t, D, nullptr, nullptr, w.hid, 4 * D, CLIPMI_F16, M, 4 * D, D, CLIPMI_EPI_NONE, s))) return rc;       // d_a = g W_proj
    if ((rc = launch_quickgelu_backward(st.h(i), w.hid, w.hid, M * 4 * D, s))) return rc;
    if ((rc = launch_operand_stats(w.hid, M * 4 * D, stats, s))) return rc;
    if ((rc = tower_gemm(w.hid, 4 * D, t.w_fc_t, 4 * D, nullptr, nullptr, w.dy, D, CLIPMI_F32, M, D, 4 * D, CLIPMI_EPI_NONE, s))) return rc;    // . W_fc
    if ((rc = launch_ln_backward(st.x(2 * i + 1), D, nullptr, b.ln2_g, w.dy, CLIPMI_F32, g, g16, M, D, 1e-5f, s))) return rc;
    if ((rc = launch_operand_stats(g16, M * D, stats, s))) return rc;
    if ((rc = tower_gemm(g16, D, t.w_out_t, D, nullptr, nullptr, w.att, D, CLIPMI_F16, M, D, D, CLIPMI_EPI_NONE, s))) return rc;                // g W_out
    if (L <= ABF_MAX_L) {
      if ((rc = launch_attention_backward_full(st.qkv(i), w.att, w.qkv, B, L, H, s))) return rc;
    } else if ((rc = launch_attention_backward_long(st.qkv(i), w.att, w.qkv, vw.abl, vw.abl_bytes, B, L, H, s))) {
      return rc;
    }
    if ((rc = launch_operand_stats(w.qkv, M * 3 * D, stats, s))) return rc;
    if ((rc = tower_gemm(w.qkv, 3 * D, t.w_qkv_t, 3 * D, nullptr, nullptr, w.dy, D, CLIPMI_F32, M, D, 3 * D, CLIPMI_EPI_NONE, s))) return rc;   // dqkv W_qkv
    if ((rc = launch_ln_backward(st.x(2 * i), D, nullptr, b.ln1_g, w.dy, CLIPMI_F32, g, g16, M, D, 1e-5f, s))) return rc;
    // block i's prompt rows were written here: their gradient leaves the stream
    if (i >= 1 && i < depth && (rc = launch_splice_reduce(g, g16, d_prompts + i * per, B, L, D, L0, n_ctx, 1, s))) return rc;
  }
  // slot 0 through ln_pre: every image's pre-LN row is the prompt itself and the backward is linear in dy -- sum over the batch first
  if ((rc = launch_splice_reduce(g, g16, vw.dsum, B, L, D, L0, n_ctx, 0, s))) return rc;
  if (hipMemsetAsync(d_prompts, 0, (size_t)per * 4, s) != hipSuccess) return check_launch("hipMemsetAsync");
  return launch_ln_backward(vs.prompts, D, nullptr, m->vw.ln_pre_g, vw.dsum, CLIPMI_F32, d_prompts, nullptr, n_ctx, D, 1e-5f, s);
}

}  // namespace clipmi

using namespace clipmi;

extern "C" {

int clipmi_vision_train_bytes(const clipmi_model* m, int B, int n_ctx, size_t* workspace_bytes, size_t* stash_bytes) {
  if (workspace_bytes) *workspace_bytes = 0;
  if (stash_bytes) *stash_bytes = 0;
  if (int rc = check_vision_shape("vision_train_bytes", m, B, n_ctx)) return rc;
  if (workspace_bytes) *workspace_bytes = carve_vision_ws(nullptr, m, B, n_ctx).bytes;
  if (stash_bytes) *stash_bytes = carve_vision_stash(nullptr, m, B, n_ctx).bytes;
  return CLIPMI_OK;
}

int clipmi_vision_encoder_train(clipmi_model* m, const void* image, int image_dtype, int B, const float* prompts, int n_ctx, int depth, float* out,
                                void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, unsigned flags, clipmi_stream_t stream) {
  CLIPMI_REQUIRE(!(flags & ~(CLIPMI_CALL_STREAM_F32 | CLIPMI_CALL_STREAM_F16)), CLIPMI_ERR_ARG, "vision_encoder_train: bad flags 0x%x", flags);
  CLIPMI_REQUIRE(!(flags & CLIPMI_CALL_STREAM_F16), CLIPMI_ERR_STATE, "vision_encoder_train: the training forward runs the fp32 residual stream only");
  if (int rc = check_vision_train_call("vision_encoder_train", m, B, n_ctx, depth, workspace, workspace_bytes, stash, stash_bytes)) return rc;
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(image && prompts && out, CLIPMI_ERR_ARG, "vision_encoder_train: null pointer");
  CLIPMI_REQUIRE(image_dtype == CLIPMI_F16 || image_dtype == CLIPMI_F32, CLIPMI_ERR_ARG, "vision_encoder_train: image dtype %d", image_dtype);
  return run_vision_train_forward(m, image, image_dtype, B, prompts, n_ctx, depth, out, workspace, stash, (hipStream_t)stream);
}

int clipmi_vision_encoder_backward(clipmi_model* m, const clipmi_vision_dgrad* wt, const float* d_out, int B, int n_ctx, int depth, float* d_prompts,
                                   void* workspace, size_t workspace_bytes, const void* stash, size_t stash_bytes, unsigned long long* operand_stats,
                                   clipmi_stream_t stream) {
  if (int rc = check_vision_train_call("vision_encoder_backward", m, B, n_ctx, depth, workspace, workspace_bytes, stash, stash_bytes)) return rc;
  if (B == 0) return CLIPMI_OK;
  if (int rc = check_vision_dgrad("vision_encoder_backward", m, wt)) return rc;
  CLIPMI_REQUIRE(d_out && d_prompts, CLIPMI_ERR_ARG, "vision_encoder_backward: null pointer");
  CLIPMI_REQUIRE((uintptr_t)d_prompts % 16 == 0, CLIPMI_ERR_ARG, "vision_encoder_backward: d_prompts must be 16-byte aligned");
  return run_vision_backward(m, wt, d_out, B, n_ctx, depth, d_prompts, workspace, stash, operand_stats, (hipStream_t)stream);
}

}  // extern "C"
