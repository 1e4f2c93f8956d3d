/*
 * clipmi.h -- C ABI of libclipmi.so: the MI355X (gfx950) CLIP inference-and-calibration hot path.
 *
 * The reference (ml-stat-Sustech/CLIP_Calibration) is pure Python and has no FFI of its own; its "operator
 * API" for this path is the attribute surface of the object returned by clip.build_model (reference
 * clip/model.py:656-699) plus DistanseAwareCalibration.predict and the ECE metric.  Each entry point below
 * names the reference interface it replaces.  Conventions:
 *
 *   - every pointer is a DEVICE pointer owned by the caller (torch-ROCm tensors in the Python host code)
 *     unless the parameter is documented as "host";
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 *     never synchronises the device; nothing is allocated or freed inside a launch call (graph-capture safe);
 *   - weights are BORROWED: the handle stores the pointers given to clipmi_set_*_weights, the caller keeps the
 *     tensors alive and re-binds after moving them;
 *   - the return value is CLIPMI_OK (0) or a negative error code; nothing throws across the boundary;
 *     clipmi_last_error() returns a thread-local detail string for the most recent failure;
 *   - activations are token-major ("NLD"): row (n*L + l) of a [N*L, D] matrix.
 *
 * dtype codes: CLIPMI_F16 = IEEE half, CLIPMI_F32 = float.  All GEMMs run on v_mfma_f32_16x16x32_f16 with fp32
 * accumulation; LayerNorm, softmax, residual stream, L2 norms and the final logits are fp32.
 */
#ifndef CLIPMI_H
#define CLIPMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLIPMI_ABI_VERSION 16

typedef void* clipmi_stream_t; /* hipStream_t */

enum {
  CLIPMI_OK = 0,
  CLIPMI_ERR_ARG = -1,         /* null pointer / bad enum */
  CLIPMI_ERR_SHAPE = -2,       /* shape the kernels do not support (see each call) */
  CLIPMI_ERR_HIP = -3,         /* a HIP runtime call failed (launch error, no device) */
  CLIPMI_ERR_WORKSPACE = -4,   /* workspace too small */
  CLIPMI_ERR_STATE = -5        /* weights not bound */
};

enum { CLIPMI_F16 = 0, CLIPMI_F32 = 1 };

enum {
  CLIPMI_EPI_NONE = 0,          /* out = acc */
  CLIPMI_EPI_BIAS = 1,          /* out = acc + bias[n] */
  CLIPMI_EPI_BIAS_QUICKGELU = 2,/* t = acc + bias[n]; out = t * sigmoid(1.702 t)   (clip/model.py:162-164) */
  CLIPMI_EPI_BIAS_RESIDUAL = 3, /* out = residual[m,n] + acc + bias[n]             (clip/model.py:186-187) */
  CLIPMI_EPI_BIAS_RELU = 4,     /* out = max(acc + bias[n], 0): conv + folded BatchNorm + ReLU (clip/model.py:45-46,139) */
  CLIPMI_EPI_BIAS_RESIDUAL16_RELU = 5 /* out = max(acc + bias[n] + residual16[m,n], 0): the tail of a Bottleneck
                                         (clip/model.py:48-55); `residual` points at fp16 [M,N] (ld = ldo), fp16 out only */
};

int clipmi_abi_version(void);
const char* clipmi_strerror(int code);
const char* clipmi_last_error(void);

/* Runtime switches, process-wide.  The reference has none (its knobs are yacs config keys read by Dassl); these select
 * between parity-tested implementations of the same operator and exist for tests, A/B measurements and the DEFAULT precision
 * policy.  Each option also has an environment spelling that is read ONCE, at the first launch; after that only
 * clipmi_set_option changes it (no launch path calls getenv, and no launch path writes an option).  Unknown names return
 * CLIPMI_ERR_ARG.
 *   gemm_variant     (CLIPMI_GEMM_VARIANT)    -1 = default dispatch; 0 (128 x 128 tiles), 1 (256 x 256, 16 waves), 10 / 'a' (320 x 256
 *                                             ping-pong), 13 / 's' (persistent, streamed fp16 epilogue), 16 / 'r' (persistent row ranges,
 *                                             streamed residual epilogue) force one kernel family where the shape allows it (test aid)
 *   gemm_band        (CLIPMI_GEMM_BAND)       0 = default; n-tiles per traversal band
 *   gemm_stream      (CLIPMI_GEMM_STREAM)     1 (default) = ping-pong persistent kernel with streamed epilogue for multi-round fp16-out
 *                                             GEMMs, K >= 512 (in-proj / c_fc); 0 = one tile per workgroup (same bits with the bias epilogue)
 *   gemm_rstream     (CLIPMI_GEMM_RSTREAM)    1 (default) = persistent row-range kernel with streamed residual epilogue for the fp16-stream
 *                                             residual GEMMs with K <= 1536 (out-proj); 0 = one 320 x 256 tile per workgroup.  The row-range
 *                                             kernel adds the residual inside its K loop: both round the same fp32 sum once, in another order
 *   gemm_split_rows  (CLIPMI_GEMM_SPLIT_ROWS) 1 (default) = where the ragged last row of 256-row tiles (M % 256 <= 128 rows) would open a round of
 *                                             its own in the persistent kernel (ViT-L/14@336 at 64 images: c_fc 9.06 rounds), those rows go to
 *                                             the tile kernels as a second launch; 0 = one launch
 *   attn_loader      (CLIPMI_ATTN_LOADER)     2 (default) = 193..200-token non-causal attention runs the kernel whose operands all arrive
 *                                             by LDS-DMA from a dedicated loader wave and whose output rows are stored non-temporal;
 *                                             1 = the same with plain stores; 0 = the persistent kernel (all three: same bits)
 *   attn_ring        (CLIPMI_ATTN_RING)       1 (default) = non-causal attention over more than 224 tokens (ViT-L/14: 257, 577) runs the ring kernel
 *                                             (persistent workgroups, loader wave, 128-key blocks through a three-slot LDS ring); 0 = the round-1
 *                                             streaming kernel (also taken for a causal mask of that length)
 *   attn_small       (CLIPMI_ATTN_SMALL)      1 (default) = attention over at most 32 tokens (the text tower after dead-row elimination) gives every
 *                                             (sequence, head) item to ONE wave, no workgroup barrier; 0 = the persistent kernel (same bits)
 *   tail_unfused     (CLIPMI_TAIL_UNFUSED)    1 = clipmi_logits / clipmi_fused_tail as separate launches instead of the fused tail kernel
 *   vision_pass      (CLIPMI_VISION_PASS)     stream elements (token rows x width) of one pass of clipmi_encode_image, default 50432 * 768
 *                                             (256 images of ViT-B/16, 128 of ViT-L/14, 64 of ViT-L/14@336): a batch of one and a half
 *                                             passes or more runs as consecutive passes on the same stream and workspace -- each pass is an ordinary
 *                                             call on its images: features equal to the one-pass result up to the library's usual batch
 *                                             dependence (tile and kernel choice follow the row count: <= 2e-4 on normalised features),
 *                                             +8..10 % images/s at 512-1024 images of ViT-B/16; 0 = never split
 *   vision_train_long (CLIPMI_VISION_TRAIN_LONG)  0 (default) = the image tower's training path (clipmi_vision_train_bytes, clipmi_vision_encoder_train /
 *                                             _backward, the VPT / MaPLe / PromptSRC one-call steps, clipmi_vision_val_chunk) takes at most 224 token
 *                                             rows per image; 1 = up to 640 (the lengths of ViT-L/14 and ViT-L/14@336; the patch sizes stay 8, 16, 32): beyond 224 rows the attention backward is
 *                                             clipmi_attention_backward_long and the workspace holds its statistics; at most 224 rows the same
 *                                             kernels, sizes and bits either way.  Opt-in until measured
 * and the process-wide DEFAULTS of the three per-model settings (clipmi_model_set_option overrides them per handle):
 *   cls_only_last_block (CLIPMI_CLS_ONLY_LAST_BLOCK)  1 (default since round 6) = the image tower's LAST block computes what the class row
 *                    needs and nothing else -- K | V of every token, Q / attention / out-proj / ln_2 / c_fc / c_proj of the class rows, the only
 *                    rows ln_post reads (clip/model.py:419) -- as GEMMs with M = batch and row stride L * D and a one-query attention kernel;
 *                    same per-element arithmetic, features equal to the every-row computation to ~1e-6 in cosine, 7 % fewer flops per image of
 *                    ViT-B/16; 0 = every block computes every token row (what bench.py's headline `value` times)
 *   ln_fold          (CLIPMI_LN_FOLD)         1 = ln_1 / ln_2 inside the GEMM epilogues (default), 0 = LayerNorm kernels
 *   residual_f16     (CLIPMI_RESIDUAL_F16)    0 = fp32 residual stream, 1 = fp16 on both towers, 2 = image tower only
 *                                             (default; env 'v'), 3 = text tower only (env 't') */
int clipmi_set_option(const char* name, int value);
int clipmi_get_option(const char* name, int* value);

/* ------------------------------------------------------------------------------------------------------
 * Operator level (stateless).  These are the kernels; the tower drivers below are sequences of them.
 * ---------------------------------------------------------------------------------------------------- */

/* nn.Linear / in_proj / out_proj / c_fc / c_proj / `x @ proj` (clip/model.py:174-176,183,422,611):
 * out[M,N] = epilogue(A[M,K] @ W[N,K]^T).  A, W fp16 row-major with leading dimensions lda, ldw (elements);
 * bias fp32[N] or NULL; residual fp32 [M,N] (fp16 for BIAS_RESIDUAL16_RELU; ld = ldo) or NULL; out fp16 or fp32 (out_dtype), ld = ldo.
 * Requires K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0; M, N otherwise arbitrary. */
int clipmi_gemm_f16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                    const void* residual, void* out, int64_t ldo, int out_dtype,
                    int M, int N, int K, int epilogue, clipmi_stream_t stream);

/* The residual GEMM of a block on the fp16 residual stream (out-proj / c_proj, clip/model.py:186-187: `x = x + f(x)` on fp16 tensors):
 * x16[m,n] = fp16(x16[m,n] + A[m,:] . W[n,:] + bias[n]) IN PLACE (one rounding of the fp32 sum), plus the LayerNorm-fold row
 * partials the next GEMM consumes: stats[(t * M + m) * 2 + {0,1}] = (sum, sum of squares) over the 256 columns of column tile t of
 * the ROUNDED row m; *parts (host int) receives the number of column tiles of the kernel that ran: (N + 255) / 256, or (N + 127) / 128
 * (partials are then per 128 columns) where the 128 x 128 tile kernel runs -- small problems, or gemm_variant = 0 forced -- and that
 * count is at most 8; at most 8 either way.  A fp16 [M,K]
 * (lda), W fp16 [N,K] (ldw), bias fp32 [N], x16 fp16 [M,N] (ldx), stats fp32 [8 * M * 2] (room for the largest count).  K % 64 == 0, N % 8 == 0, ldx % 8 == 0, 16-byte aligned. */
int clipmi_gemm_residual_f16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* x16, int64_t ldx,
                             float* stats, int* parts, int M, int N, int K, clipmi_stream_t stream);

/* The residual GEMM of a block on the fp32 residual stream with the LayerNorm-fold outputs (the text tower's out-proj / c_proj):
 * x[m,n] += A[m,:] . W[n,:] + bias[n] IN PLACE (fp32), x16[m,n] = fp16(x[m,n]) and the row partials of the fp32 row:
 * stats[(t * M + m) * 2 + {0,1}] = (sum, sum of squares) over column tile t; *parts as for clipmi_gemm_residual_f16.  x fp32 and x16 fp16
 * [M,N], both with leading dimension ldx; stats fp32 [8 * M * 2].  K % 64 == 0, N % 8 == 0, ldx % 8 == 0, 16-byte aligned. */
int clipmi_gemm_residual_fold(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, float* x, int64_t ldx, void* x16,
                              float* stats, int* parts, int M, int N, int K, clipmi_stream_t stream);

/* A LayerNorm-folded consumer GEMM (in-proj / c_fc with ln_1 / ln_2 folded in, csrc/gemm.hip "LayerNorm folded into the GEMMs"):
 * out[m,n] = epi(rstd[m] * (A[m,:] . W_f[n,:]) - rstd[m] mean[m] g[n] + c[n]), epilogue CLIPMI_EPI_BIAS or CLIPMI_EPI_BIAS_QUICKGELU,
 * mean / rstd (eps inside the square root) from the `parts` producer partials of row m over ln_dim columns:
 * stats[(p * ln_plane + m * ln_row_stride) * 2 + {0,1}], p < parts (ln_plane 0 = M).  W_f = fp16(gamma W), g = row sums of W_f,
 * c = W beta + b (clip_calibration_amd.ops.fold_layernorm_linear).  ln_rows: optional fp32 [M][2] scratch that lets the streamed kernel
 * take more than 4 partials (else NULL).  A fp16 (lda), W_f fp16 (ldw), out fp16 / fp32 (out_dtype, ldo); g, c fp32 [N]; 1 <= parts <= 8,
 * ln_row_stride >= 1; K % 64 == 0, N % 4 == 0, 16-byte aligned operands, 8-byte aligned stats / ln_rows. */
int clipmi_gemm_ln_fold(const void* A, int64_t lda, const void* W_f, int64_t ldw, const float* c, const float* g, const float* stats, int parts,
                        int64_t ln_plane, int ln_row_stride, int ln_dim, float eps, float* ln_rows, void* out, int64_t ldo, int out_dtype,
                        int M, int N, int K, int epilogue, clipmi_stream_t stream);

/* LayerNorm subclass with fp32 statistics (clip/model.py:153-159): y[r,:] = (x[row(r),:] - mean) * rsqrt(var+eps)
 * * gamma + beta.  row(r) = gather_idx ? gather_idx[r] : r, addressed with in_stride (elements).  D % 4 == 0,
 * D <= 4096. */
int clipmi_layernorm(const void* x, int x_dtype, int64_t in_stride, const int32_t* gather_idx,
                     const float* gamma, const float* beta, void* y, int y_dtype, int64_t out_stride,
                     int rows, int D, float eps, clipmi_stream_t stream);

/* nn.MultiheadAttention core after the packed in-projection (clip/model.py:181-183; SURVEY a-5a):
 * qkv fp16 [N*L, 3*D] (q | k | v, head h at columns h*64..h*64+63 of each third), out fp16 [N*L, D] =
 * merge_heads(softmax(q k^T / 8 + mask) v).  head_dim is 64 (D == 64*H).  causal != 0 applies the text
 * tower's mask (clip/model.py:585-591).  qkv 16-byte aligned, out 8-byte aligned; N == 0 is OK (nothing is read or written). */
int clipmi_attention(const void* qkv, void* out, int N, int L, int H, int causal, clipmi_stream_t stream);

/* The same attention for ONE query per sequence, token 0 (the class token of the image tower's last block, whose other rows never reach
 * ln_post: clip/model.py:419), never masked: qkv fp16 [N*L, 3*64*H] packed q | k | v as above; out fp16 [N*L, 64*H], of which only row n*L
 * of every sequence n is written -- every other row is left as it was.  fp32 scores, probabilities and accumulation, one fp16 rounding of
 * the output.  Both pointers 16-byte aligned; N == 0 is OK (nothing is read or written). */
int clipmi_attention_cls(const void* qkv, void* out, int N, int L, int H, clipmi_stream_t stream);

/* image.type(dtype) + the im2col half of conv1 (clip/model.py:598,395-397): image [B,3,R,R] (fp32 or fp16,
 * NCHW) -> col fp16 [B*(R/P)^2, Kpad], column c*P*P + ky*P + kx, zero padded up to Kpad (a multiple of 64). */
int clipmi_patchify(const void* image, int image_dtype, void* col, int B, int R, int P, int Kpad,
                    clipmi_stream_t stream);

/* image.type(dtype) + conv1 + reshape / permute + positional embedding of the PATCH rows as a GEMM whose loader reads the image itself
 * (clip/model.py:598,395-397,401; conv1 has stride = kernel = P, so its im2col matrix is an address map of the NCHW image):
 *   x0[b * tokens + 1 + p, :] = sum_k pixel(b, p, k) * conv_w[:, k] + pos[1 + p, :]        p = py * (R/P) + px,  k = c*P*P + ky*P + kx
 * image [B,3,R,R] fp32 or fp16; an fp32 image is first cast to fp16 into `scratch` (clipmi_patch_embed_scratch_bytes bytes, 16-byte aligned;
 * NULL for an fp16 image); conv_w fp16 [D, ldw] = conv1.weight.reshape(D, 3*P*P) (ldw >= 3*P*P); pos fp32 [1 + (R/P)^2, D] or NULL (the bare conv
 * output: clipmi_embed_ln then adds pos -- what clipmi_encode_image does, the positional rows cost this GEMM's epilogue 13 us); x0 fp16 or fp32
 * (x0_dtype) [B * tokens, D]: only the patch rows are written -- row 0 (class token) and rows beyond 1 + (R/P)^2 (prompt tokens) of every
 * sequence are left to clipmi_embed_ln.  fp16 operands, fp32 accumulation, pos added in fp32, one rounding.  Requires P in {8, 16, 32},
 * R % P == 0, D % 8 == 0, an fp16 image batch below 2 GB; 16-byte aligned pointers.  CLIPMI_ERR_SHAPE otherwise (clipmi_encode_image then
 * takes clipmi_patchify + clipmi_gemm_f16: ViT-L/14). */
size_t clipmi_patch_embed_scratch_bytes(int B, int R, int image_dtype);
int clipmi_patch_embed(const void* image, int image_dtype, void* scratch, const void* conv_w, int64_t ldw, const float* pos, void* x0,
                       int x0_dtype, int B, int R, int P, int D, int tokens, clipmi_stream_t stream);

/* cat(class_embedding) + positional embedding of the class row + ln_pre over every token row (clip/model.py:398-402,413; MaPLe's shallow
 * prompt rows, :459-460), one wave per row:  row (b, l) = l == 0 ? cls + pos[0] : l < tokens0 ? x0[b * L + l] (+ pos[l] if add_pos) : shallow[l - tokens0];
 * out = LayerNorm(row) with fp32 statistics.  x0 fp16 / fp32 [B * L, D] as clipmi_patch_embed left it; cls fp32 [D]; pos fp32 [tokens0, D];
 * shallow fp32 [L - tokens0, D] or NULL when L == tokens0; y fp32 [B * L, D] or NULL; y16 fp16 [B * L, D] + stats fp32 [B * L * 2]
 * ((sum, sum of squares) of each output row: the LayerNorm-fold partial the first in-projection consumes) or both NULL. */
int clipmi_embed_ln(const void* x0, int x0_dtype, int add_pos, const float* cls, const float* pos, const float* shallow,
                    const float* gamma, const float* beta, float* y, void* y16, float* stats, int B, int L, int tokens0, int D, float eps,
                    clipmi_stream_t stream);

/* Row L2 normalisation  f / ||f||  (zsclip.py:99; coop.py:212-213): in (fp16|fp32) [rows,E] -> out fp32. */
int clipmi_l2_normalize(const void* in, int in_dtype, float* out, int rows, int E, clipmi_stream_t stream);

/* The same with a choice of output type: out fp32 or fp16 [rows,E] (out_dtype).  fp16 is the exchange format of the
 * multi-GPU path: the fp32 quotient rounded once (what the reference's fp16 GPU path holds after zsclip.py:99). */
int clipmi_l2_normalize_to(const void* in, int in_dtype, void* out, int out_dtype, int rows, int E, clipmi_stream_t stream);

/* Fused  logits = (scale * img_n) @ txt_n^T  (zsclip.py:100-101, coop.py:215-217, tempscaling.py:53-56)
 * + DistanseAwareCalibration.predict (distanse_aware_calibration.py:49-58: logits[i,:] *= conf[argmax_i])
 * + softmax top-1 (vl_calibrator.py:91, vl_evaluator.py:68,83): conf[i] = max_c softmax(logits[i,:]),
 * pred[i] = argmax.  img_n [B,E], txt_n [C,E] fp32, ALREADY L2-normalised.  dac_conf fp32[C] or NULL.
 * logits fp32 [B,C] (required), conf fp32[B], pred int32[B] (either may be NULL).  E % 16 == 0. */
int clipmi_logits(const float* img_n, const float* txt_n, float scale, const float* dac_conf,
                  float* logits, float* conf, int32_t* pred, int B, int C, int E, clipmi_stream_t stream);

/* The tail of the path as ONE launch (the fused normalise + matmul + DAC-temperature kernel):
 *   img_n = img / ||img||                      zsclip.py:99, coop.py:212-213            (normalize != 0; else img is used as given)
 *   logits = scale * img_n @ txt_n^T           zsclip.py:100-101, coop.py:215-217, tempscaling.py:53-56
 *   pred = argmax_c; logits[i,:] *= dac[pred]  distanse_aware_calibration.py:49-58      (dac_conf != NULL)
 *   conf = max_c softmax(logits[i,:])          vl_calibrator.py:91, vl_evaluator.py:68,83
 *   ECE bins += (1, conf, pred == label)       tools/metrics.py:90-130                  (bins != NULL; layout of clipmi_ece_accumulate)
 * img fp32 or fp16 [B,E] (img_dtype; un-normalised tower output when normalize != 0, e.g. the fp16 embeddings gathered from
 * all ranks when normalize == 0), txt_n fp32 [C,E] L2-normalised; logits fp32 [B,C] required;
 * img_n_out fp32 [B,E] (the normalised image features of the reference's 3-tuple; NULL to skip; only with normalize), conf fp32 [B],
 * pred int32 [B], labels int64 [B] + bins float64 [3*(n_bins+1)]: each may be NULL.  Results are bit-identical to
 * clipmi_l2_normalize + clipmi_logits + clipmi_ece_accumulate (the ECE sums of confidences up to the order of their atomics).  E % 64 == 0 and E <= 2048 run fused; other shapes, and option
 * tail_unfused = 1, run the separate launches (which need img_n_out or fp32 normalised input, and conf + pred when bins are given).
 * workspace: clipmi_fused_tail_workspace_bytes(B, C) bytes of device memory whose first 64 KiB (ticket counters, one int32 per 16- or
 * 32-row block) are ZERO before the first launch; every launch leaves them zero again.  The rest holds one 16-byte partial (max, argmax,
 * sum of exponentials) per (row, 64-column block), written and consumed inside a launch: no initialisation.  One workspace serves ONE
 * launch at a time (launches on one stream are fine; concurrent launches on different streams need a workspace each).  Re-zero the counters
 * after a launch that failed.  Features must be finite with |x| <= 65504 (L2-normalised ones are <= 1): the products run on the
 * fp16 matrix cores with every fp32 operand split into fp16 hi + lo halves, ~1e-6 absolute on logits of scale 100. */
size_t clipmi_fused_tail_workspace_bytes(int B, int C);
int clipmi_fused_tail(const void* img, int img_dtype, int normalize, const float* txt_n, float scale, const float* dac_conf, float* logits,
                      float* img_n_out, float* conf, int32_t* pred, const int64_t* labels, double* bins, int n_bins,
                      void* workspace, size_t workspace_bytes, int B, int C, int E, clipmi_stream_t stream);

/* The row pass of clipmi_logits alone, on logits that already exist -- DistanseAwareCalibration.predict
 * (distanse_aware_calibration.py:49-58) + softmax top-1: pred = argmax_c logits[i,:]; if dac_conf != NULL the row is
 * multiplied in place by dac_conf[pred]; conf[i] = max_c softmax(row).  conf / pred may be NULL. */
int clipmi_calibrate_rows(float* logits, const float* dac_conf, float* conf, int32_t* pred, int B, int C,
                          clipmi_stream_t stream);

/* VLCalibration.predict on its DAC / plain branches (trainers/calibration/vl_calibrator.py:83-109): probs[i,:] =
 * softmax(logits[i,:] * (dac_conf ? dac_conf[argmax_i] : 1)), the full probability matrix the reference hands to
 * VLClassification.evaluate (vl_evaluator.py:59).  logits fp32 [B,C] are NOT modified; probs fp32 [B,C] (required, may
 * alias logits); conf / pred as above, may be NULL. */
int clipmi_softmax_rows(const float* logits, const float* dac_conf, float* probs, float* conf, int32_t* pred,
                        int B, int C, clipmi_stream_t stream);

/* ModifiedResNet image tower (clip/model.py:10-150) -- SURVEY f-4.  Activations NHWC fp16; a 1x1 convolution is
 * clipmi_gemm_f16 on the [B*H*W, C] rows with the folded BatchNorm as bias (CLIPMI_EPI_BIAS_RELU / _RESIDUAL16_RELU).
 *  clipmi_im2col3x3_nchw   stem conv1 (clip/model.py:106, stride 2, pad 1) from the NCHW image (fp32|fp16):
 *                          col fp16 [B*Ho*Wo, Kpad], column c*9 + ky*3 + kx, zero padded (Kpad % 64 == 0); col 16-byte aligned
 *  clipmi_im2col3x3_nhwc   every other 3x3 convolution (stride 1, pad 1; clip/model.py:20,108,110):
 *                          col[(b,y,x), (ky*3+kx)*C + c] = x[b, y+ky-1, x+kx-1, c]; C % 8 == 0, Kpad % 64 == 0, x and col
 *                          16-byte aligned (CLIPMI_ERR_ARG otherwise: both are moved 16 bytes at a time)
 *  clipmi_avgpool_nhwc     nn.AvgPool2d(k) (clip/model.py:23,33,112): x [B,H,W,C] -> y [B,H/k,W/k,C]
 *  clipmi_attnpool_tokens  AttentionPool2d token build (clip/model.py:69-71): tokens fp16 [B, HW+1, C] = [mean | x] + pos (fp32 [HW+1, C])
 *  clipmi_attnpool         its attention with the mean token as the only query (clip/model.py:72-90): q fp16 [B,C] (projected,
 *                          biased), kv fp16 [B*T, 2C] (k | v projected, biased), head_dim 64 -> out fp16 [B, C] (before c_proj)
 *  clipmi_conv3x3_nhwc     Bottleneck.conv2 + bn2 (+ ReLU) as an IMPLICIT GEMM (no im2col matrix): x fp16 [B,H,W,C], w fp16
 *                          [Cout, 9*C] tap-major ((ky*3+kx)*C + c, BatchNorm folded), bias fp32 [Cout] -> out fp16 [B,H,W,Cout];
 *                          stride 1, pad 1, C % 64 == 0, Cout % 8 == 0 */
int clipmi_conv3x3_nhwc(const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int C, int Cout,
                        int relu, clipmi_stream_t stream);
int clipmi_im2col3x3_nchw(const void* image, int image_dtype, void* col, int B, int Cin, int H, int W, int stride, int Kpad,
                          clipmi_stream_t stream);
int clipmi_im2col3x3_nhwc(const void* x, void* col, int B, int H, int W, int C, int Kpad, clipmi_stream_t stream);
int clipmi_avgpool_nhwc(const void* x, void* y, int B, int H, int W, int C, int k, clipmi_stream_t stream);
int clipmi_attnpool_tokens(const void* x, const float* pos, void* tokens, int B, int HW, int C, clipmi_stream_t stream);
int clipmi_attnpool(const void* q, const void* kv, void* out, int B, int T, int heads, clipmi_stream_t stream);

/* CLIP-Adapter's feature blend (trainers/classification/clip_adapter.py:138-172): out[b,:] = ratio * relu(W2 relu(W1 f[b,:]))
 * + (1 - ratio) * f[b,:]; feats [B,E] (un-normalised image features), w1 [H,E], w2 [E,H], no biases; all fp32. */
int clipmi_adapter_blend(const float* feats, const float* w1, const float* w2, float ratio, float* out, int B, int E,
                         int H, clipmi_stream_t stream);

/* TaskRes' classifier (trainers/classification/taskres.py:105-106): out = a + alpha * b over n fp32 elements
 * (a = base text features, b = learned residual).  out may alias a. */
int clipmi_scale_add(const float* a, const float* b, float alpha, float* out, long long n, clipmi_stream_t stream);

/* ProDA's classifier (trainers/classification/proda.py:316-333): out[g,:] = mean over the P prompts of class g of the
 * (already L2-normalised) text features in [(g*P + p), :].  fp32; the mean is NOT re-normalised, as in the reference. */
int clipmi_group_mean(const float* in, float* out, int G, int P, int E, clipmi_stream_t stream);

/* CoCoOp (trainers/classification/cocoop.py:154-199) -- SURVEY f-4: instance-conditioned prompts.  All fp32 unless noted.
 *  clipmi_cocoop_ctx       PromptLearner.forward's meta-net and shift (:154-161): ctx_shifted[b,t,:] = ctx[t,:] +
 *                          W2 relu(W1 img_n[b] + b1) + b2.  img_n [B,E] (L2-normalised image features), w1 [H,E], b1 [H],
 *                          w2 [D,H], b2 [D], ctx [n_ctx,D] -> ctx_shifted [B,n_ctx,D].
 *  clipmi_cocoop_prompts   construct_prompts for `n_images` images x C classes (:163-171): prompts[(b,c),l,:] =
 *                          ctx_shifted[b,l-1,:] for 1 <= l <= n_ctx, else base[c,l,:] (base = token embedding of the
 *                          "X X .. X name." prompts, [C,L,D] fp16|fp32).  prompts fp16 [n_images*C, L, D], the input of
 *                          clipmi_text_encoder.  D % 8 == 0.
 *  clipmi_logits_per_image the loop body of CustomCLIP.forward (:193-199): logits[b,c] = scale * <img_n[b],
 *                          txt[b,c,:] / ||txt[b,c,:]||>, txt [B,C,E] UN-normalised text-encoder outputs; then the same
 *                          DAC / softmax top-1 row pass as clipmi_logits.  txt_n_last [C,E] (may be NULL) receives the
 *                          normalised text features of the last image -- what the reference's 3-tuple carries. */
int clipmi_cocoop_ctx(const float* img_n, const float* w1, const float* b1, const float* w2, const float* b2,
                      const float* ctx, float* ctx_shifted, int B, int E, int H, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_cocoop_prompts(const void* base, int base_dtype, const float* ctx_shifted, void* prompts, int n_images,
                          int C, int L, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_logits_per_image(const float* img_n, const float* txt, float scale, const float* dac_conf, float* logits,
                            float* conf, int32_t* pred, float* txt_n_last, int B, int C, int E, clipmi_stream_t stream);

/* Device-side accumulation of the ECE statistics (tools/metrics.py:90-130) -- SURVEY f-1.  bins: float64
 * [3*(n_bins+1)] = per-bin (count, sum_conf, sum_correct), bin n_bins collects conf == 1.0 (the digitize
 * quirk).  Accumulates over calls; zero it with hipMemsetAsync.  The final reduction to a scalar is host
 * code (clip_calibration_amd.metrics.ece_from_bins). */
int clipmi_ece_accumulate(const float* conf, const int32_t* pred, const int64_t* labels, int n,
                          double* bins, int n_bins, clipmi_stream_t stream);

/* get_knn_dists / get_val_image_knn_dists (trainers/calibration/proximity.py:19-70) -- SURVEY f-2: for every query row
 * the K smallest L2 distances ||refs[j] - queries[i]||_2, ascending, out fp32 [Nq, K].  queries [Nq,E], refs [Nr,E]
 * fp32; E % 64 == 0; 1 <= K <= min(16, Nr).  (The "val image" variant asks for K+1 against itself and drops column 0.) */
int clipmi_knn_dists(const float* queries, const float* refs, float* out, int Nq, int Nr, int E, int K,
                     clipmi_stream_t stream);

/* The nearest rows WITH their indices (interpret_prompts/interpret_prompt.py:66-76: torch.cdist + argsort of the whole matrix, for
 * the nearest vocabulary words of a learned context): for every query row the K rows of refs at the smallest L2 distance, ascending
 * in the total order (distance, index) -- ties go to the lower index.  queries [Nq, E], refs [Nr, E] fp32; out_dist fp32 [Nq, K] (the
 * distance, not its square); out_idx int32 [Nq, K].  Distances are fp32 in difference form, sum_e (q_e - r_e)^2 with e ascending: a
 * pair's distance does not depend on Nq or on `splits`.  A NaN distance counts as +inf: such rows come last, by index.
 * The grid is (blocks of 16 queries) x (`splits` slices of the 64-row reference tiles); every workgroup writes its slice's K best
 * pairs per query to the workspace (slices with fewer than K rows, or none, pad with (+inf, INT32_MAX)) and a second launch on the
 * same stream merges them: the outputs are bit-identical for every `splits` >= 1.  splits = 0: the library chooses
 * (clipmi_nearest_rows_splits: eight workgroups per CU, what the chip holds at once, where there are tiles for it; never more slices
 * than tiles).
 * 1 <= K <= min(32, Nr); E % 64 == 0; pointers 16-byte aligned; Nq == 0: CLIPMI_OK, nothing is launched.  Shapes are checked before
 * pointers (CLIPMI_ERR_SHAPE, then CLIPMI_ERR_ARG, then CLIPMI_ERR_WORKSPACE), and all of it before anything touches a device. */
int clipmi_nearest_rows(const float* queries, const float* refs, float* out_dist, int32_t* out_idx, int Nq, int Nr, int E, int K,
                        int splits, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
size_t clipmi_nearest_rows_workspace(int Nq, int Nr, int K, int splits);   /* bytes; 0 on bad arguments */
int clipmi_nearest_rows_splits(int Nq, int Nr);                            /* the slice count that splits = 0 picks */

/* ProCal, the proximity-informed density-ratio calibrator (trainers/calibration/density_ratio_calibration.py:28-117, used by
 * vl_calibrator.py:112-121 on base_calibration_mode "scaling_based" with procal_flag).  The fit stays on the host (float64); the
 * device evaluates, per test row with confidence c and proximity p,
 *   c* = T / max(T + ratio * F, 1e-10),  S(c, p) = norm_S * sum_{s in S} exp(-((c - s_c) / h_c)^2 / 2 - ((p - s_p) / h_p)^2 / 2)
 * for the sets T (correct val samples) and F (incorrect), norm_S = 1 / (|S| h_c h_p 2 pi): statsmodels' KDEMultivariate.pdf with a
 * Gaussian product kernel.  The model describes the fitted sets as the kernels take them: point i of set k (k = 0: T, 1: F) is
 * (points_k[2 i], points_k[2 i + 1]) = (s_c * scale[k][0], s_p * scale[k][1]) with scale = sqrt(log2(e) / 2) / h, so that a pair term
 * is exp2(-(du^2 + dv^2)) of the equally scaled query.  Host struct; the point arrays are device fp64, 16-byte aligned, n_true and
 * n_false >= 2, every scale and norm finite and > 0, ratio finite and >= 0. */
typedef struct clipmi_procal_model {
  const double* points_true;
  const double* points_false;
  int32_t n_true, n_false;
  double scale[2][2];
  double norm[2];
  double ratio;
} clipmi_procal_model;

/* c*[i] for given confidences and proximities (fp32 [n] each; cstar fp32 [n]).  n == 0: CLIPMI_OK.  One launch. */
int clipmi_procal_kde(const clipmi_procal_model* model, const float* conf, const float* proximity, float* cstar, int n,
                      clipmi_stream_t stream);

/* VLCalibration.predict with ProCal (vl_calibrator.py:83-109) plus the evaluator's top-1 of the result (vl_evaluator.py:68, 83), in
 * one launch and without host synchronisation.  Per row of logits fp32 [n, C] (not modified):
 *   y = logits * (dac_conf ? dac_conf[argmax logits] : 1), probs = softmax(y), i1 = argmax (lowest index on ties), c* from
 *   (probs[i1], proximity[i]); out[i1] = c*, out[j] = probs[j] * (1 - c*) / S for j != i1, S = sum_{j != i1} probs[j], evaluated as
 *   exp(y_j - y_i2) / sum_{j != i1} exp(y_j - y_i2) so that it never underflows; a row whose other probabilities are all exactly zero
 *   (C == 1, or every other y is -inf) keeps them at 0 (the reference divides 0 by 0 there).
 * Outputs: pred[i] = argmax out (int32, lowest index on ties) and conf[i] = out[pred[i]] (fp32, required); probs fp32 [n, C] the whole
 * calibrated matrix and cstar fp32 [n], both optional (NULL).  proximity fp32 [n].  n == 0: CLIPMI_OK. */
int clipmi_procal_rows(const clipmi_procal_model* model, const float* logits, const float* dac_conf, const float* proximity,
                       float* probs, float* conf, int32_t* pred, float* cstar, int n, int C, clipmi_stream_t stream);

/* Multi-class isotonic calibration and Bin-Mean-Shift (trainers/calibration/multi_isotonic_regression.py,
 * multi_proximity_isotonic.py:130-247; vl_calibrator.py:121-147 on base_calibration_mode "bin_based" with base_bin_calibrator_name
 * "multi_isotonic_regression").  Per row: p = softmax(DAC(logits)) in clipmi_softmax_rows' lane-strided form, x = exp(p) / sum_j exp(p_j)
 * in fp32 (a second softmax, of the probabilities), out = g(x) + 1e-9 x with g the fitted isotonic function: linear interpolation
 * through the thresholds, clipped outside them.  Rows are not renormalised.  from_probs != 0: the input rows already hold p (the
 * reference's numpy interface takes probabilities); the first softmax is skipped and a DAC factor is refused.
 * These exports are additive: the ABI version does not change with them. */
#define CLIPMI_ISOTONIC_MAX_TABLES 8

/* Host only: check thresholds (finite, X strictly ascending inside a table) and pack them as the kernel reads them.  x, y: the
 * n_tables tables one after the other, counts[t] >= 1 thresholds each; packed receives 3 * sum(counts) fp64: per table X | Y | slope
 * (slope[i] = (Y[i+1] - Y[i]) / (X[i+1] - X[i]) as numpy.interp forms it, 0 for the last).  Upload `packed` as it is. */
int clipmi_isotonic_pack(const double* x, const double* y, const int32_t* counts, int n_tables, double* packed);

/* Host struct.  table: device fp64, the output of clipmi_isotonic_pack, 8-byte aligned; table t owns thresholds offset[t] ..
 * offset[t+1] (offset[0] = 0, every table >= 1 threshold).  A row's table is the number of edges[e] <= proximity (e < n_tables - 1;
 * np.searchsorted(bin_edges[1:-1], proximity, side="right")); the edges are finite and ascending. */
typedef struct clipmi_isotonic_model {
  const double* table;
  int32_t n_tables;
  int32_t offset[CLIPMI_ISOTONIC_MAX_TABLES + 1];
  double edges[CLIPMI_ISOTONIC_MAX_TABLES - 1];
} clipmi_isotonic_model;

/* One launch, no host synchronisation.  logits fp32 [n, C] (not modified), dac_conf fp32 [C] or NULL, proximity fp32 [n] (required
 * when n_tables > 1, else optional and ignored).  Outputs: pred[i] = argmax of the calibrated row (int32, lowest index among equal
 * maxima), conf[i] the value there (both required); probs fp32 [n, C] the calibrated rows and xs fp32 [n, C] the x values, both
 * optional (NULL).  n == 0: CLIPMI_OK. */
int clipmi_isotonic_rows(const clipmi_isotonic_model* model, const float* logits, const float* dac_conf, const float* proximity,
                         int from_probs, float* probs, float* xs, float* conf, int32_t* pred, int n, int C, clipmi_stream_t stream);

/* The fit's two device passes.  An isotonic fit to 0/1 targets is determined by the positive keys (x at the label) and per-gap
 * statistics of the zeros; the host pools the resulting <= 2 m + 1 weighted points per bin in float64.
 * clipmi_isotonic_keys: keys[i] = x[i, labels[i]] (NaN when the label is outside [0, C)).  labels int64 [n], keys fp32 [n].
 * clipmi_isotonic_gap_stats: keys fp32 (device) holds, bin after bin, each bin's sorted distinct positive keys; key_offset int32
 * [n_bins + 1] (HOST): bin b owns keys[key_offset[b] .. key_offset[b+1]), m_b >= 1 of them.  bin int32 [n] (device) the bin of
 * each row, NULL when n_bins == 1.  stats int32 [3][total] (device), total = 3 * key_offset[n_bins] + n_bins: plane 0 counts, plane 1
 * the smallest and plane 2 the largest fp32 bit pattern seen; bin b's slots start at 3 * key_offset[b] + b:
 *   slot g (0 <= g <= m_b): the zeros strictly between key g-1 and key g (count, min, max);  slot m_b + 1 + k: the zeros equal to
 *   key k (count);  slot 2 m_b + 1 + k: the positives equal to key k (count).
 * status int32 [1] (device): 0, or bits 1 (a positive x is not among the keys), 2 (an x outside (0, 1]: non-finite input),
 * 4 (a bin index outside [0, n_bins)).  Both are initialised by the call.  n * C < 2^31. */
int clipmi_isotonic_keys(const float* logits, const int64_t* labels, float* keys, int n, int C, int from_probs, clipmi_stream_t stream);
int clipmi_isotonic_gap_stats(const float* logits, const int64_t* labels, const int32_t* bin, const float* keys,
                              const int32_t* key_offset, int n_bins, int32_t* stats, int32_t* status, int n, int C, int from_probs,
                              clipmi_stream_t stream);

/* TempScaling's fit of its one parameter (trainers/calibration/tempscaling.py:146-169: F.cross_entropy(exp(logit_scale) * cosine
 * logits, label), torch.optim.SGD on the scalar) from cosine logits computed ONCE: the base model is frozen and the val loader is
 * sequential, so every epoch of the reference's loop sees the same matrix.  cosine fp32 [n, C] with row stride ld >= C (elements),
 * labels int64 [n], C >= 2.  With theta = logit_scale, s = exp(theta), p = softmax(s * cosine[i, :]):
 *   loss_i = logsumexp_j(s c_ij) - s c_iy,   d loss_i / d theta = s (sum_j p_ij c_ij - c_iy),
 * the row maximum subtracted before the exponential, fp32 throughout; a batch's loss and gradient are the means over its rows, summed
 * in float64 in a fixed order (no atomics): the same inputs give the same bits.  A label outside [0, C) or a sample index outside
 * [0, n) is never dereferenced; it makes the batch's loss and gradient NaN.  Two short launches per batch; workspace (device, 8-byte
 * aligned) of clipmi_tempscale_workspace_bytes(rows of the widest batch) bytes.  These exports are additive: the ABI version does not
 * change with them.
 *
 * clipmi_tempscale_batch: one batch at the theta held in device memory (theta fp32 [1]): out fp32 [2] (device) = {mean loss, mean
 * d loss / d theta} over the samples order[0 .. rows) (int32, device), or 0 .. rows-1 when order is NULL.
 *
 * clipmi_tempscale_fit: the whole run, epochs * ceil(n / batch) steps (floor with drop_last), enqueued on `stream` without a host
 * synchronisation; step k of epoch e takes the samples order[e * n + k * batch ..] (order int32 [epochs, n], device; NULL = 0 .. n-1
 * in every epoch, the reference's sequential loader), the last batch of an epoch may be short.  state (device, four 32-bit words):
 * {theta fp32, momentum buffer fp32, steps taken int32, loss of the last batch fp32}; the caller sets {init, 0, 0, 0} for a fresh
 * fit, and every kernel reads theta from there.  Each step applies torch.optim.SGD's rule in fp32 with lr[step] (lr fp32 [steps],
 * device, filled once by the host):
 *   g += weight_decay * theta;  buf = g on the state's first step, else momentum * buf + (1 - dampening) * g;
 *   g = nesterov ? g + momentum * buf : buf  (momentum != 0 only);  theta -= lr * g.
 * losses fp32 [steps] (device) receives every step's batch loss, or NULL.  epochs == 0: CLIPMI_OK, nothing is launched.
 * CLIPMI_ERR_ARG: a null pointer, epochs < 0, momentum or dampening outside [0, 1), a negative or non-finite weight decay, nesterov
 * with zero momentum or non-zero dampening.  CLIPMI_ERR_SHAPE: n < 1, C < 2, batch < 1, rows < 1, ld < C. */
size_t clipmi_tempscale_workspace_bytes(int rows);
int clipmi_tempscale_batch(const float* cosine, int64_t ld, const int64_t* labels, const int32_t* order, int rows, int n, int C,
                           const float* theta, float* out, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
int clipmi_tempscale_fit(const float* cosine, int64_t ld, const int64_t* labels, const int32_t* order, int n, int C, int batch, int epochs,
                         int drop_last, const float* lr, float momentum, float dampening, float weight_decay, int nesterov, float* state,
                         float* losses, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* Parameterized temperature scaling (PTS; Tomani, Cremers, Buettner, ECCV 2022; the reference's CALIBRATION.SCALING.MODE
 * 'ParameterizedTempScaling' with its P_TS block, for which it ships no trainer): a small MLP on the K largest logits of a row gives
 * that row's temperature.  For a row z of C logits, fp32 throughout:
 *   f = the K largest values of z, descending;  h_0 = f;  h_l = relu(W_l h_(l-1) + b_l) for l = 1 .. n_layers, each n_nodes wide;
 *   t = w_out . h_last + b_out;  T = clamp(|t|, 1e-12, 1e12);  calibrated logits z / T;  p = softmax(z / T);
 *   loss = (1 / C) sum_c (p_c - [c == y])^2, and a batch's loss is the mean over its rows.
 * The gradient is torch autograd's on logits / t.abs().clamp(1e-12, 1e12): abs has derivative 0 at 0, clamp passes the gradient on the
 * closed interval, relu has derivative 0 at 0.  params fp32 [P] = [W_1 | b_1 | ... | W_n | b_n | w_out | b_out], every W row-major
 * [out, in] (nn.Linear's layout), P = clipmi_pts_param_count(n_layers, n_nodes, K) (0 outside the limits).  Limits: 0 <= n_layers <= 4,
 * 1 <= n_nodes <= 32, 1 <= K <= 32, C >= K, C >= 2.  logits fp32 [N, C] with row stride ld >= C (elements), labels int64 [N].  One wave
 * per row; a batch's sums are formed in float64 in a fixed order, without atomics: the same inputs give the same bits.  These exports
 * are additive: the ABI version does not change with them.
 *
 * clipmi_pts_topk: out fp32 [N, K] = the K largest values of every row, descending (the values torch.sort(descending=True) puts first).
 * -inf is an ordinary value; a row that holds a NaN gives K NaNs.
 *
 * clipmi_pts_apply: out[i, c] = logits[i, c] / T_i (IEEE division) in one launch, out with row stride ld_out >= C; out may be logits
 * itself.  temperature fp32 [N] receives T, or NULL.
 *
 * clipmi_pts_eval: one batch at params, nothing updated: batch_out fp32 [1 + P] (device) = {mean loss, the mean gradient of every
 * parameter} over the samples order[0 .. rows) (int32, device), or first .. first + rows - 1 when order is NULL.  features fp32 [N, K]
 * is clipmi_pts_topk's output for logits.  workspace (device) of rows * (2 + 2 n_layers n_nodes) floats.
 *
 * clipmi_pts_fit: the whole run, epochs * ceil(N / batch) steps (floor with drop_last), enqueued on `stream` without a host
 * synchronisation: the features once, then two launches per step.  Step k of epoch e takes the samples order[e * N + k * batch ..]
 * (order int32 [epochs, N], device; NULL = 0 .. N-1 in every epoch); the last batch of an epoch may be short.  state (device) fp32
 * words [3 P + 2] = {params P | buffer P | buffer P | steps taken int32 | loss of the last batch}: SGD's momentum buffer is the first
 * buffer, Adam's exp_avg and exp_avg_sq are the two; the caller sets {init, 0 ...} for a fresh fit and may hand a returned state back
 * to continue.  optimizer 0: torch.optim.SGD's rule as clipmi_tempscale_fit states it (the buffer is initialised on the state's first
 * step); 1: torch.optim.Adam's (no amsgrad) with the bias corrections of step `steps taken + 1`, formed in float64.  Each step uses
 * lr[step] (fp32 [steps], device).  losses fp32 [steps] (device) receives every step's batch loss, or NULL.  workspace (device) of
 * N * K + min(batch, N) * (2 + 2 n_layers n_nodes) floats.  A label outside [0, C) or a sample index outside [0, N) is never
 * dereferenced; it makes the step's loss and the parameters NaN.  epochs == 0: CLIPMI_OK, nothing is launched.
 * CLIPMI_ERR_ARG: a null pointer, epochs < 0, an unknown optimizer, its hyper-parameters outside torch's ranges.  CLIPMI_ERR_SHAPE: the
 * limits above, ld < C, rows < 1, batch < 1, N < 0 (N < 1 for the fit; topk and apply accept N == 0).  CLIPMI_ERR_WORKSPACE: too small. */
int clipmi_pts_param_count(int n_layers, int n_nodes, int K);
int clipmi_pts_topk(const float* logits, int64_t ld, int N, int C, int K, float* out, clipmi_stream_t stream);
int clipmi_pts_apply(const float* logits, int64_t ld, int N, int C, const float* params, int n_layers, int n_nodes, int K, float* out,
                     int64_t ld_out, float* temperature, clipmi_stream_t stream);
int clipmi_pts_eval(const float* features, const float* logits, int64_t ld, const int64_t* labels, const int32_t* order, int first, int rows,
                    int N, int C, const float* params, int n_layers, int n_nodes, int K, float* batch_out, float* workspace,
                    size_t workspace_floats, clipmi_stream_t stream);
int clipmi_pts_fit(const float* logits, int64_t ld, const int64_t* labels, const int32_t* order, int N, int C, int n_layers, int n_nodes, int K,
                   int batch, int epochs, int drop_last, const float* lr, int optimizer, float momentum, float dampening, float weight_decay,
                   int nesterov, double beta1, double beta2, double eps, float* state, float* losses, float* workspace, size_t workspace_floats,
                   clipmi_stream_t stream);

/* CLIP-Adapter's bottleneck trained on the device (trainers/classification/clip_adapter.py:138-187: both towers frozen, the text
 * features constant under the shipped config): forward, backward and torch.optim.SGD's step on the two bias-free matrices, all fp32
 * with fp32 master weights.  feats fp32 [n, E] raw (un-normalised) image features with row stride ld >= E (elements), labels int64
 * [n], text fp32 [C, E] L2-normalised, w1 [H, E], w2 [E, H] and their momentum buffers m1, m2 of the same shapes (may be NULL when
 * momentum == 0), ratio as clipmi_adapter_blend takes it, scale = exp(logit_scale).  Per batch of B rows:
 *   h = relu(f W1^T);  a = relu(h W2^T);  g = ratio a + (1 - ratio) f;  u = g / |g|;  z = scale u T^T;  loss = mean CE(z, y)
 *   dz = (softmax(z) - onehot(y)) / B;  du = scale dz T;  dg = (du - u (u . du)) / |g|;  da = ratio dg [a > 0];  dW2 = da^T h;
 *   dh = (da W2) [h > 0];  dW1 = dh^T f;   then on every element of W2 and W1, with the step's rate *lr (device):
 *   g += weight_decay * w;  buf = g on a first step, else momentum * buf + (1 - dampening) * g;
 *   g = nesterov ? g + momentum * buf : buf  (momentum != 0 only);  w -= lr * g.
 * Two launches per step: one workgroup per sample (forward, loss, backward down to da and dh), then one thread per weight element
 * (the gradient summed over the batch rows in row order, the update in place; the row losses averaged in float64).  Fixed summation
 * orders, no atomics: the same inputs give the same bits.  A label outside [0, C) or a sample index outside [0, n) is never
 * dereferenced; it makes the step's loss and the weights NaN.  workspace (device, 8-byte aligned) of
 * clipmi_adapter_train_workspace_bytes(rows of the widest batch, E, H, C) bytes (0 for shapes the calls refuse outright).  These
 * exports are additive: the ABI version does not change with them.
 *
 * clipmi_adapter_train_step: one step on the batch feats[0 .. rows) -- for callers that run the image tower on every step.  first_step
 * != 0 initialises the momentum buffers from this step's gradient (torch's first step); loss fp32 [1] (device) or NULL.
 *
 * clipmi_adapter_fit: the whole run from a cached feature matrix, epochs * ceil(n / batch) steps (floor with drop_last), enqueued on
 * `stream` without a host synchronisation; step k of epoch e takes the samples order[e * n + k * batch ..] (order int32 [epochs, n],
 * device; NULL = 0 .. n-1 in every epoch), the last batch of an epoch may be short.  lr fp32 [steps] (device), one rate per step;
 * first_step applies to the run's first step; losses fp32 [steps] (device) receives every step's batch loss, or NULL.  epochs == 0:
 * CLIPMI_OK, nothing is launched.
 * CLIPMI_ERR_ARG: a null or misaligned pointer, epochs < 0, momentum or dampening outside [0, 1), a negative or non-finite weight
 * decay, nesterov with zero momentum or non-zero dampening, a non-finite ratio or scale.  CLIPMI_ERR_SHAPE: n or rows < 1, C < 2,
 * E < 1, H < 1, batch < 1, ld < E, or 4 E + 2 H beyond
 * the 64 KiB of LDS a sample's workgroup holds (4 E + 2 H + 1056 floats: E = 512, H = 128 need 13 KiB; H may exceed E).
 * CLIPMI_ERR_WORKSPACE: a workspace that is too small. */
size_t clipmi_adapter_train_workspace_bytes(int rows, int E, int H, int C);
int clipmi_adapter_train_step(const float* feats, int64_t ld, const int64_t* labels, const float* text, float* w1, float* w2, float* m1,
                              float* m2, int rows, int E, int H, int C, float ratio, float scale, const float* lr, int first_step,
                              float momentum, float dampening, float weight_decay, int nesterov, float* loss, void* workspace,
                              size_t workspace_bytes, clipmi_stream_t stream);
int clipmi_adapter_fit(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* text, float* w1, float* w2,
                       float* m1, float* m2, int n, int E, int H, int C, int batch, int epochs, int drop_last, float ratio, float scale,
                       const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses,
                       void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* TaskRes' text residuals trained on the device (trainers/classification/taskres.py:96-210: both towers and logit_scale frozen, the
 * base text features computed once): forward, backward and the optimiser's step on the residual matrix, all fp32 with fp32 master
 * values.  feats fp32 [n, E] raw (un-normalised) image features with row stride ld >= E (elements), labels int64 [n], base fp32
 * [C, E] the base text features (not normalised), residuals fp32 [C, E] updated in place, scale = exp(logit_scale).  Per batch of B:
 *   x_b = f_b / |f_b|;  t_c = base_c + alpha r_c;  n_c = |t_c|;  u_c = t_c / n_c;  z = scale X U^T;  loss = mean CE(z, y)
 *   dz = (softmax(z) - onehot(y)) / B;  du_c = scale sum_b dz[b, c] x_b;  dr_c = alpha (du_c - u_c (u_c . du_c)) / n_c
 * then on every element of r, with the step's rate *lr (device), the rule `optimizer` selects:
 *   optimizer == 0    torch.optim.SGD: the rule of clipmi_adapter_train_step; state1 is the momentum buffer (may be NULL when
 *                      momentum == 0), state2 is not used; a step with steps_done == 0 initialises the buffer from its gradient.
 *   optimizer == 1    torch.optim.Adam without amsgrad, step number t = steps_done + 1: g += weight_decay * r;
 *                      m += (g - m) (1 - beta1);  v = beta2 v + ((1 - beta2) g) g;
 *                      r -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps);  state1 = m, state2 = v, both [C, E] and zero
 *                      before the first step; the two bias corrections are formed in double on the host.  momentum, dampening and
 *                      nesterov are not looked at.
 * Three launches per step: z in 64 x 64 tiles (the tiles sum the squares of the rows they stream and divide the raw dot by both
 * norms), one workgroup per sample (row loss, dz), dU in 64 x 64 tiles with the projection and the optimiser's rule in the epilogue
 * (u_c . du_c is taken as sum_b dz[b, c] z[b, c]; the row losses averaged in float64).  Every product is one fmaf chain in depth
 * order, no atomics: the same inputs give the same bits.  A label outside [0, C) or a sample index outside [0, n) is never
 * dereferenced; it makes the step's loss and the residuals NaN.  workspace (device, 8-byte aligned) of
 * clipmi_taskres_train_workspace_bytes(rows of the widest batch, E, C) bytes (0 for shapes the calls refuse outright).  These
 * exports are additive: the ABI version does not change with them.
 *
 * clipmi_taskres_train_step: one step on the batch feats[0 .. rows) -- for callers that run the image tower on every step; loss fp32
 * [1] (device) or NULL.
 *
 * clipmi_taskres_fit: the whole run from a cached feature matrix, epochs * ceil(n / batch) steps (floor with drop_last), enqueued on
 * `stream` without a host synchronisation; batches, order, lr and losses as clipmi_adapter_fit takes them; steps_done counts the steps
 * taken before the run's first.  epochs == 0: CLIPMI_OK, nothing is launched.
 * CLIPMI_ERR_ARG: a null or misaligned pointer, an unknown optimizer, steps_done < 0, epochs < 0, a negative or non-finite weight decay
 * or eps, momentum, dampening or a beta outside [0, 1), nesterov with zero momentum or non-zero dampening, a non-finite alpha or scale.
 * CLIPMI_ERR_SHAPE: n or rows < 1, C < 2, E < 1, batch < 1, ld < E, or C or the rows of a batch above 4 194 240 (65 535 tiles of 64).
 * CLIPMI_ERR_WORKSPACE: a workspace that is too small. */
size_t clipmi_taskres_train_workspace_bytes(int rows, int E, int C);
int clipmi_taskres_train_step(const float* feats, int64_t ld, const int64_t* labels, const float* base, float* residuals, float* state1,
                              float* state2, int rows, int E, int C, float alpha, float scale, const float* lr, int optimizer,
                              int64_t steps_done, float weight_decay, float momentum, float dampening, int nesterov, double beta1, double beta2,
                              double eps, float* loss, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
int clipmi_taskres_fit(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* base, float* residuals,
                       float* state1, float* state2, int n, int E, int C, int batch, int epochs, int drop_last, float alpha, float scale,
                       const float* lr, int optimizer, int64_t steps_done, float weight_decay, float momentum, float dampening, int nesterov,
                       double beta1, double beta2, double eps, float* losses, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* Per-epoch validation inside the two one-call fits above (reference base_learner.py:41-47; DESIGN.md "Fit monitor").  Additive exports:
 * the ABI version stays.
 *
 * clipmi_adapter_val_logits: logits[i, c] = scale * normalise(ratio relu(relu(f_i W1^T) W2^T) + (1 - ratio) f_i) . text_c for the
 * validation features feats fp32 [n_val, E] with row stride ld >= E, fp32 [n_val, C] out (row stride C).  One workgroup per row runs the
 * device function the training step's first launch runs (csrc/adapter_train.hip, adapter_forward_row): the same operations in the same
 * order with the same rounding points, so these are the logits a training step on those rows would see.
 * clipmi_taskres_val_logits: logits[i, c] = scale * normalise(f_i) . normalise(base_c + alpha residuals_c), by the training step's own
 * first launch (taskres_logits_kernel) on the validation rows; a tile normalises its 64 classifier rows once for its 64 validation rows.
 * Both: plain fp32 vector code, no atomics, a fixed summation order (the same inputs give the same bytes), every output element has one
 * owner, nothing is read outside [n_val, ld] or written outside [n_val, C], no workspace.  A non-finite feature row gives a row of NaN
 * and touches no other row.  CLIPMI_ERR_ARG: a null pointer, an fp32 array not 4-byte aligned, logits not 16-byte aligned (as
 * clipmi_val_score takes them), a non-finite ratio / alpha / scale; CLIPMI_ERR_SHAPE: n_val < 1, C < 2, E < 1, H < 1, ld < E, the
 * adapter's LDS limit, TaskRes' 4 194 240 rows or classes.
 *
 * clipmi_adapter_fit_monitored / clipmi_taskres_fit_monitored: clipmi_adapter_fit / clipmi_taskres_fit -- the same body, the same
 * launches for the steps, the same fitted bits -- which behind the last step of every epoch e also enqueue: the validation logits of the
 * weights as they are into monitor_workspace, clipmi_val_score's two launches into record e of `records` (epochs records of
 * 16 + 16 (n_bins + 1) bytes each, 8-byte aligned) and, when best_block and best_params are given (both or neither), clipmi_best_select's
 * two launches under `criterion` (0 accuracy, 1 nll).  Nothing waits, nothing is read back.  The selected block is n_floats = 2 E H
 * floats at w1 for the adapter, which then requires w2 == w1 + H E (one master block [w1 | w2]), and the C E residuals for TaskRes;
 * either 16-byte aligned, as best_params is.  The optimiser's state is not selected.  val_feats fp32 [n_val, E] with row stride val_ld
 * >= E, val_labels int64 [n_val] (a label outside [0, C) counts as wrong with a NaN nll).  monitor_workspace (256-byte aligned):
 * clipmi_*_fit_monitored_workspace_bytes(n_val, C, n_bins) = 4 n_val C for the logits, rounded up to 256, plus clipmi_val_score's and
 * clipmi_best_select's; 0 for arguments the call refuses.  Every check precedes the first launch.  Beyond the unmonitored call's:
 * CLIPMI_ERR_ARG: a null or misaligned pointer, n_bins outside 1..64, a criterion other than 0 or 1, a best block without a best slot
 * or the reverse, a best slot with split or misaligned parameters; CLIPMI_ERR_SHAPE: n_val < 1, val_ld < E; CLIPMI_ERR_WORKSPACE. */
int clipmi_adapter_val_logits(const float* feats, int64_t ld, const float* text, const float* w1, const float* w2, int n_val, int E, int H, int C,
                              float ratio, float scale, float* logits, clipmi_stream_t stream);
int clipmi_taskres_val_logits(const float* feats, int64_t ld, const float* base, const float* residuals, int n_val, int E, int C, float alpha,
                              float scale, float* logits, clipmi_stream_t stream);
size_t clipmi_adapter_fit_monitored_workspace_bytes(int n_val, int C, int n_bins);
int clipmi_adapter_fit_monitored(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* text, float* w1, float* w2,
                                 float* m1, float* m2, int n, int E, int H, int C, int batch, int epochs, int drop_last, float ratio, float scale,
                                 const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses,
                                 void* workspace, size_t workspace_bytes, const float* val_feats, int64_t val_ld, const int64_t* val_labels,
                                 int n_val, int n_bins, void* records, int criterion, void* best_block, float* best_params,
                                 void* monitor_workspace, size_t monitor_workspace_bytes, clipmi_stream_t stream);
size_t clipmi_taskres_fit_monitored_workspace_bytes(int n_val, int C, int n_bins);
int clipmi_taskres_fit_monitored(const float* feats, int64_t ld, const int64_t* labels, const int32_t* order, const float* base, float* residuals,
                                 float* state1, float* state2, int n, int E, int C, int batch, int epochs, int drop_last, float alpha, float scale,
                                 const float* lr, int optimizer, int64_t steps_done, float weight_decay, float momentum, float dampening,
                                 int nesterov, double beta1, double beta2, double eps, float* losses, void* workspace, size_t workspace_bytes,
                                 const float* val_feats, int64_t val_ld, const int64_t* val_labels, int n_val, int n_bins, void* records,
                                 int criterion, void* best_block, float* best_params, void* monitor_workspace, size_t monitor_workspace_bytes,
                                 clipmi_stream_t stream);

/* The sample-level metrics of the evaluator on the device (vl_evaluator.py:77-82 macro-F1; tools/metrics.py:132-178 PIECE, :212-236
 * AdaptiveECE) -- SURVEY f-1.  Three small kernels; the host turns their outputs into the scalars (clip_calibration_amd.metrics:
 * quantile_edges_from_order_stats, gap_from_groups, macro_f1_from_counts).  These exports are additive: the ABI version does not
 * change with them.
 *
 * clipmi_order_stats: exact order statistics without a sort.  x fp32 [n] (device, not modified); ranks int32 [k] (HOST), 0-based,
 * non-decreasing, each in [0, n), 1 <= k <= CLIPMI_ORDER_STATS_MAX_RANKS.  out fp32 [k] (device): out[j] == np.sort(x)[ranks[j]] --
 * every NaN sorts behind +inf, as in numpy, and comes back as a NaN; -0.0 sorts before +0.0.  nan_count int32 [1] (device): the
 * number of NaNs in x.  A most-significant-digit radix select on the order-preserving integer image of the floats: four 8-bit passes,
 * each one histogram launch (per distinct prefix among the targets, 256 digit counts: LDS partials, then integer global atomics) and
 * one one-workgroup launch that narrows every target's prefix and residual rank; nine enqueues, no host synchronisation, integer
 * counts only -- the same input gives the same bits.  workspace (device, 16-byte aligned) of clipmi_order_stats_workspace_bytes(n, k)
 * bytes (0 for arguments the call would refuse); the call initialises it.
 * CLIPMI_ERR_ARG: a null pointer, a rank outside [0, n) or below its predecessor.  CLIPMI_ERR_SHAPE: n < 1, k < 1,
 * k > CLIPMI_ORDER_STATS_MAX_RANKS.  CLIPMI_ERR_WORKSPACE: a workspace that is too small. */
#define CLIPMI_ORDER_STATS_MAX_RANKS 64
size_t clipmi_order_stats_workspace_bytes(int n, int k);
int clipmi_order_stats(const float* x, int n, const int32_t* ranks, int k, float* out, int32_t* nan_count, void* workspace,
                       size_t workspace_bytes, clipmi_stream_t stream);

/* clipmi_group_gap_accumulate: per sample i, key_bin = the number of key_edges <= key[i] and conf_bin = the number of conf_edges <=
 * conf[i] (np.searchsorted(edges, v, side="right"): compared in float64, a NaN value lands behind the last edge);
 * group = key_bin * (n_conf_edges + 1) + conf_bin;  groups float64 [3][G] (device), G = (n_key_edges + 1) * (n_conf_edges + 1) <=
 * CLIPMI_GROUP_GAP_MAX_GROUPS (what the LDS partials hold): plane 0 += 1, plane 1 += conf[i], plane 2 += (labels[i] == pred[i]).
 * Accumulates over calls; the caller zeroes it.  conf, key fp32 [n], pred int32 [n], labels int64 [n]; both edge lists float64
 * (device), ascending, NULL when their count is 0; key may be NULL when n_key_edges == 0.  n == 0: CLIPMI_OK.  One launch.
 * AdaptiveECE: key = conf with the inner quantile edges and no conf_edges.  PIECE: key = proximity with its inner quantile edges,
 * conf_edges = np.linspace(0, 1, n_bins + 1)[1:-1] uploaded as the host computed them. */
#define CLIPMI_GROUP_GAP_MAX_GROUPS 1024
int clipmi_group_gap_accumulate(const float* conf, const int32_t* pred, const int64_t* labels, const float* key,
                                const double* key_edges, int n_key_edges, const double* conf_edges, int n_conf_edges, double* groups,
                                int n, clipmi_stream_t stream);

/* clipmi_class_counts: counts int64 [3 * C + 1] (device): counts[c] += samples with pred == labels == c (true positives),
 * counts[C + c] += samples predicted c, counts[2 C + c] += samples labelled c; a sample whose label or prediction lies outside
 * [0, C) adds to counts[3 C] and to nothing else.  Accumulates over calls; the caller zeroes it.  pred int32 [n], labels int64 [n].
 * Integer atomics (LDS partials per workgroup while 3 C + 1 counters fit, global atomics alone beyond).  n == 0: CLIPMI_OK. */
int clipmi_class_counts(const int32_t* pred, const int64_t* labels, int n, int C, int64_t* counts, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Multi-GPU exchange: one process per GPU, the image batch sharded over the ranks, weights and text
 * features replicated and resident; per step ONE all-gather of the per-GPU L2-normalised image embeddings (fp16 [B/G,E])
 * before the shared logits kernel.  Replaces the reference's nn.DataParallel wrapping, which re-broadcasts the weights on
 * every call (trainers/classification/coop.py:266-272, trainers/calibration/tempscaling.py:117-120).  RCCL (librccl,
 * opened on first use) over xGMI; gather, not reduce, so results do not depend on the rank count.
 *   clipmi_comm_unique_id  rank 0: fills id_out (host, CLIPMI_COMM_ID_BYTES) -- hand it to every rank out of band
 *   clipmi_comm_create     every rank, collectively, AFTER selecting its GPU (hipSetDevice / torch.cuda.set_device)
 *   clipmi_comm_ranks      what the communicator itself reports (world size, this rank)
 *   clipmi_allgather       out[r*bytes .. (r+1)*bytes) = rank r's `in`, on every rank; asynchronous on `stream`
 * ---------------------------------------------------------------------------------------------------- */
#define CLIPMI_COMM_ID_BYTES 128
typedef struct clipmi_comm clipmi_comm;
int clipmi_comm_unique_id(void* id_out);
int clipmi_comm_create(const void* id, int world, int rank, clipmi_comm** out);
int clipmi_comm_destroy(clipmi_comm* comm);
int clipmi_comm_ranks(const clipmi_comm* comm, int* world, int* rank);
int clipmi_allgather(clipmi_comm* comm, const void* in, void* out, size_t bytes_per_rank, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Model level.  One handle per CLIP model per GPU.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct clipmi_model clipmi_model;

typedef struct clipmi_geometry {
  int32_t embed_dim;        /* E */
  int32_t image_resolution; /* R */
  int32_t patch_size;       /* P */
  int32_t vision_width;     /* Dv (multiple of 64) */
  int32_t vision_layers;
  int32_t context_length;   /* 77 */
  int32_t vocab_size;
  int32_t text_width;       /* Dt */
  int32_t text_layers;
  int32_t text_heads;       /* Dt / 64 */
} clipmi_geometry;

/* ResidualAttentionBlock parameters (clip/model.py:167-188).  GEMM weights fp16 [out,in] row-major exactly as in
 * the checkpoint; biases and LayerNorm parameters fp32. */
typedef struct clipmi_block_weights {
  const float* ln1_g; const float* ln1_b;
  const void* w_qkv;  const float* b_qkv;   /* attn.in_proj_weight [3D,D], in_proj_bias [3D] */
  const void* w_out;  const float* b_out;   /* attn.out_proj [D,D] */
  const float* ln2_g; const float* ln2_b;
  const void* w_fc;   const float* b_fc;    /* mlp.c_fc [4D,D] */
  const void* w_proj; const float* b_proj;  /* mlp.c_proj [D,4D] */
  /* Optional LayerNorm-folded operands (all six or none; NULL = run ln_1 / ln_2 as separate kernels):
   *   w_*_f = fp16(gamma * W) row-wise over the input dim, g_*[n] = sum_k float(w_*_f[n,k]),
   *   c_*[n] = sum_k beta[k] * W[n,k] + b[n];  LN(x) W^T + b = rstd*(x w_f^T) - rstd*mean*g + c. */
  const void* w_qkv_f; const float* g_qkv; const float* c_qkv;   /* ln_1 folded into attn.in_proj */
  const void* w_fc_f;  const float* g_fc;  const float* c_fc;    /* ln_2 folded into mlp.c_fc */
} clipmi_block_weights;

typedef struct clipmi_vision_weights {
  const void* conv_w;                /* visual.conv1.weight as fp16 [Dv, Kpad], Kpad = roundup(3*P*P, 64), zero padded */
  const float* class_embedding;      /* [Dv] */
  const float* positional_embedding; /* [(R/P)^2 + 1, Dv] */
  const float* ln_pre_g; const float* ln_pre_b;
  const float* ln_post_g; const float* ln_post_b;
  const void* proj_t;                /* visual.proj^T as fp16 [E, Dv] */
  const clipmi_block_weights* blocks;/* host array [vision_layers] (copied by the call) */
} clipmi_vision_weights;

typedef struct clipmi_text_weights {
  const float* token_embedding;      /* [vocab, Dt] fp32 */
  const float* positional_embedding; /* [context_length, Dt] */
  const float* ln_final_g; const float* ln_final_b;
  const void* proj_t;                /* text_projection^T as fp16 [E, Dt] */
  const clipmi_block_weights* blocks;/* host array [text_layers] (copied by the call) */
} clipmi_text_weights;

/* MaPLe prompt injection (clip/model.py:287-331,447-478; maple.py:170-187).  `shallow` (vision only) is
 * appended after the positional embedding; deep[i] overwrites, before block i+1, the LAST n_ctx tokens (vision)
 * or tokens 1..n_ctx (text).  fp32, already rounded through fp16 by the caller (the reference's .half()). */
typedef struct clipmi_prompt_hook {
  int32_t n_ctx;
  int32_t n_deep;
  const float* shallow;  /* [n_ctx, D] or NULL */
  const float* deep;     /* [n_deep, n_ctx, D] or NULL */
} clipmi_prompt_hook;

int clipmi_create(const clipmi_geometry* geom, clipmi_model** out);
int clipmi_destroy(clipmi_model* m);

/* Per-model settings.  The reference chooses precision per model (cfg.TRAINER.<X>.PREC, trainers/classification/coop.py:243-245) and
 * builds a second CLIP inside the same process (trainers/classification/base_learner.py:262-272), so these live on the handle:
 * names "residual_f16" (0..3, see clipmi_set_option), "ln_fold" (0 / 1), "cls_only_last_block" (0 / 1); value -1 (the initial
 * state) follows the process-wide option of the same name.  clipmi_model_get_option returns the EFFECTIVE value.
 * Threading contract: calls on DIFFERENT handles may run concurrently from different threads and streams (each call touches only
 * its handle, its workspace and its stream); calls on one handle, and clipmi_model_set_option on it, are serialised by the caller. */
int clipmi_model_set_option(clipmi_model* m, const char* name, int value);
int clipmi_model_get_option(const clipmi_model* m, const char* name, int* value);

/* Per-call flags of the tower calls (last argument before the stream): 0, or ONE of the two stream-precision overrides for THIS
 * call only (no state is changed): CoCoOp's per-image text passes run the fp16 stream while the same handle's zero-shot features
 * keep the fp32 stream.  CLIPMI_CALL_STREAM_F16 needs the LayerNorm-folded operands (else CLIPMI_ERR_STATE). */
#define CLIPMI_CALL_DEFAULT 0u
#define CLIPMI_CALL_STREAM_F32 1u /* residual stream in fp32 (+ fp16 operand shadow) */
#define CLIPMI_CALL_STREAM_F16 2u /* residual stream in fp16: the reference's own GPU precision (clip/model.py:186-187) */
int clipmi_set_vision_weights(clipmi_model* m, const clipmi_vision_weights* w);
int clipmi_set_text_weights(clipmi_model* m, const clipmi_text_weights* w);

/* Bytes of scratch the caller must pass to the tower calls for `batch` images / `n_prompts` prompts.  clipmi_encode_image works a large
 * batch in passes (option vision_pass): the vision figure is that of the largest pass, under the option's value at the time of the call to
 * clipmi_encode_image -- size the workspace after any clipmi_set_option("vision_pass", ...).  The text figure is for a call with the
 * same `seq_rows` (below; 0 = the whole context). */
size_t clipmi_vision_workspace_bytes(const clipmi_model* m, int batch, int n_ctx);
size_t clipmi_text_workspace_bytes(const clipmi_model* m, int n_prompts, int seq_rows);

/* CLIP.encode_image / VisionTransformer.forward (clip/model.py:597-598,394-424; MaPLe :447-478 when hook != NULL):
 * image [B,3,R,R] (fp32|fp16) -> out fp32 [B,E] (un-normalised, as the reference returns).  Batches of one and a half passes or more
 * (option vision_pass) run as consecutive passes on `stream`, each an ordinary call on its images (an image's features depend on its batch only through the
 * tile and kernel choice, which follows the row count: <= 2e-4 on normalised features, as between any two batch sizes). */
int clipmi_encode_image(clipmi_model* m, const void* image, int image_dtype, int batch,
                        const clipmi_prompt_hook* hook, float* out, void* workspace, size_t workspace_bytes,
                        unsigned flags, clipmi_stream_t stream);

/* `clip_model.transformer(x)` as the trainers' TextEncoder uses it (coop.py:58-60, maple.py:64-66): the causal
 * blocks only.  x fp16|fp32 [C, L, Dt] token-major in, y same dtype/shape out (x == y allowed when seq_rows covers the context).
 * seq_rows (see clipmi_text_encoder below; 0 = every row): an OPT-IN of the caller, who alone knows where its prompts end -- the blocks return
 * every row, so by default they run every row.  With 0 < seq_rows < L only the first seq_rows token rows of every sequence are read and
 * computed; y receives them in place and ZEROS in the rows behind (Python: `clip_model.transformer.live_rows = ...`, INTEGRATION.md Level 1). */
int clipmi_text_blocks(clipmi_model* m, const void* x, void* y, int dtype, int n_prompts, int seq_rows,
                       const clipmi_prompt_hook* hook, void* workspace, size_t workspace_bytes,
                       unsigned flags, clipmi_stream_t stream);

/* TextEncoder.forward (coop.py:56-67, maple.py:60-74): prompts (fp16|fp32) [C,L,Dt] WITHOUT positional embedding,
 * eot int32[C] = tokenized_prompts.argmax(-1)  ->  out fp32 [C,E] = ln_final(blocks(prompts + pos))[eot] @ text_projection.
 *
 * seq_rows -- dead-row elimination.  The text blocks mask causally (clip/model.py:585-591: token l attends to tokens <= l only) and the
 * one row that leaves the tower is the EOT row (clip/model.py:611, coop.py:65), so no token behind the LAST prompt's EOT can influence any
 * output.  With 0 < seq_rows < L the tower embeds, runs and reads only the first `seq_rows` token positions of every prompt (the inputs keep
 * their [C,L,..] layout; rows >= seq_rows are never read): identical features, L / seq_rows times fewer rows through every GEMM
 * ("X X X X a photo of a <name>." ends at token ~22 of 77).  The CALLER guarantees max(eot) < seq_rows -- it holds the tokenised prompts on the
 * host side and computes the bound once, without a per-call device sync -- and 1 + hook->n_ctx <= seq_rows; an EOT index outside is clamped
 * to seq_rows - 1 as it is to L - 1 today, and a negative one to 0: eot[c] is read as clamp(eot[c], 0, rows - 1) with rows the token rows that are
 * computed, so the feature is finite and is that of the clamped row (tests/test_gpu_text_ops.py).  A VIOLATION IS NOT DETECTED: with a bound that is too small the call returns CLIPMI_OK and the
 * features of token row seq_rows - 1 for every prompt whose EOT lies behind it (the EOT indices live on the device; checking them would cost the
 * sync this argument exists to avoid).  Callers that cannot vouch for the bound pass 0.  seq_rows <= 0 or >= L: the whole context. */
int clipmi_text_encoder(clipmi_model* m, const void* prompts, int dtype, const int32_t* eot, int n_prompts, int seq_rows,
                        const clipmi_prompt_hook* hook, float* out, void* workspace, size_t workspace_bytes,
                        unsigned flags, clipmi_stream_t stream);

/* CLIP.encode_text (clip/model.py:600-613): ids int64 [C,L] -> out fp32 [C,E]; EOT row = argmax(ids), computed on device.
 * seq_rows as above (the argmax always scans all L ids). */
int clipmi_encode_text(clipmi_model* m, const int64_t* ids, int n_prompts, int seq_rows, float* out, void* workspace,
                       size_t workspace_bytes, unsigned flags, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * CoOp's context trained on the device (trainers/classification/coop.py:70-144, 192-222, 282-309): the gradient of the text features
 * with respect to the text tower's INPUT EMBEDDINGS with the tower frozen, CoOp's cross-entropy head and torch.optim.SGD's step on the
 * context vectors (csrc/text_backward.hip, csrc/prompt_train.hip, DESIGN.md "CoOp fit").  No weight gradient exists: every Linear's backward is dX = dY W,
 * clipmi_gemm_f16 on a transposed copy of the weight that the caller packs once.  The whole backward carries grad_scale * gradient
 * (a power of two: fp16 operands flush small values); only clipmi_coop_head and clipmi_ctx_step know the factor.
 * These exports are additive: the ABI version does not change with them.
 * ---------------------------------------------------------------------------------------------------- */

/* Operator level.
 * clipmi_layernorm_backward: per row r, with xs = x[row(r)] (fp32, row stride x_stride elements), row(r) = row_idx ? row_idx[r] : r:
 *   mean / rstd recomputed in fp32 (eps inside the square root);  xhat = (xs - mean) rstd;  t = dy[r, :] * gamma;
 *   dX = rstd (t - mean(t) - xhat mean(t xhat));   g[row(r), :] += dX (fp32, row stride D);   g16[row(r), :] = fp16(g[row(r), :]).
 *   dy fp32 or fp16 [rows, D] dense (dy_dtype); g16 may be NULL.  One launch does the residual add and the fp16 operand copy of the
 *   next GEMM.  D % 4 == 0, D <= 4096, x_stride % 4 == 0; 16-byte aligned x, gamma, g, 8-byte aligned dy, g16.  rows == 0: CLIPMI_OK.
 * clipmi_quickgelu_backward: d_h = d_a (s + 1.702 h s (1 - s)), s = sigmoid(1.702 h), from the saved fp16 pre-activation h; fp32
 *   arithmetic, fp16 in and out, n elements; d_h may alias d_a.
 * clipmi_attention_backward: the backward of clipmi_attention with the causal mask, head dim 64, 1 <= L <= 80 token rows per sequence.
 *   qkv fp16 [N*L, 3*64*H] as clipmi_attention takes it, d_out fp16 [N*L, 64*H] the gradient of its output, dqkv fp16 [N*L, 3*64*H] the
 *   gradient in qkv's layout.  One workgroup per (sequence, head) holds Q, K, V and dO in LDS, recomputes S = Q K^T / 8 and the causal
 *   softmax P in fp32, then dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dP o P)), dQ = dS K / 8, dK = dS^T Q / 8 on the fp16 matrix
 *   cores with P and dS rounded to fp16; no atomics, the same inputs give the same bits.  16-byte aligned pointers. */
int clipmi_layernorm_backward(const float* x, int64_t x_stride, const int32_t* row_idx, const float* gamma, const void* dy, int dy_dtype,
                              float* g, void* g16, int rows, int D, float eps, clipmi_stream_t stream);
int clipmi_quickgelu_backward(const void* h, const void* d_a, void* d_h, int64_t n, clipmi_stream_t stream);
int clipmi_attention_backward(const void* qkv, const void* d_out, void* dqkv, int N, int L, int H, clipmi_stream_t stream);
/* clipmi_attention_backward_full: the same backward WITHOUT a mask for 1 <= L <= 224 token rows per sequence, the lengths of the image
 *   towers at 224 px with their prompt rows (the lengths clipmi_attention serves with one key block); layouts, rounding points and
 *   refusals as above (L > 224: CLIPMI_ERR_SHAPE).  One workgroup per (sequence, head) holds Q, K, V and dO in LDS; P and dS are
 *   never stored: a query-owned phase forms the row statistics (maximum, 1 / sum, rowsum(dP o P)) and dQ, a key-owned phase recomputes
 *   S and dP per pair of query tiles and accumulates dK and dV in registers.  No atomics, the same inputs give the same bits. */
int clipmi_attention_backward_full(const void* qkv, const void* d_out, void* dqkv, int N, int L, int H, clipmi_stream_t stream);
/* clipmi_attention_backward_long: the same backward without a mask for 1 <= L <= 640 token rows per sequence: ViT-L/14's 257 and 577
 *   tokens with any prompt rows; short lengths are accepted too.  Operands, layouts and rounding points as clipmi_attention_backward_full
 *   (fp16 operands; S, softmax, rowsum(dP o P) and dS in fp32; P and dS rounded to fp16 as matrix-core operands; fp32 accumulation; fp16
 *   outputs).  Nothing of size L x L and no whole item is ever resident.  Two launches of four-wave workgroups over (sequence, head, block
 *   of 64 rows) with the other side streaming through LDS in blocks of 64 rows: a query-owned launch forms each row's statistics (the
 *   running maximum, rescaled sums, then 1 / sum and rowsum(dP o P)) into `workspace` and dQ in a second sweep over the keys; a key-owned
 *   launch recomputes P and dS from the statistics and accumulates dK and dV in registers.  A workgroup owns every row it writes and there
 *   are no float atomics: the same inputs give the same bits (not the sibling's: the softmax sums are taken in another order).
 *   workspace: clipmi_attention_backward_long_bytes(N, L, H) = 12 N H L bytes (three fp32 per sequence, head and query row), 16-byte aligned;
 *   the size query returns 0 for a shape the call refuses and for N == 0.
 *   CLIPMI_ERR_SHAPE: L > 640, L < 1, H < 1, N < 0, N H, N L or the workgroup count beyond 31 bits.  CLIPMI_ERR_ARG: a null pointer, a
 *   pointer that is not 16-byte aligned, workspace_bytes below the size query.  N == 0: CLIPMI_OK, pointers may be NULL. */
size_t clipmi_attention_backward_long_bytes(int N, int L, int H);
int clipmi_attention_backward_long(const void* qkv, const void* d_out, void* dqkv, void* workspace, size_t workspace_bytes, int N, int L, int H,
                                   clipmi_stream_t stream);

/* CoOp's loss head (coop.py:205-222 + F.cross_entropy): feats fp32 [B, E] raw image features with row stride ld >= E, labels int64 [B],
 * text fp32 [C, E] raw text features, scale = exp(logit_scale):
 *   x_b = f_b / |f_b|;  u_c = t_c / |t_c|;  z = scale X U^T;  loss = mean_b CE(z_b, y_b);  dz = grad_scale (softmax(z) - onehot(y)) / B
 *   du_c = scale sum_b dz[b, c] x_b;  d_text[c, :] = (du_c - u_c (u_c . du_c)) / |t_c|
 * all fp32, fixed summation orders, the batch loss the float64 mean of the row losses.  loss fp32 [1] or NULL; d_text fp32 [C, E]
 * (= grad_scale * d loss / d text); d_text16 fp16 [C, E], the same rounded, or NULL.  A label outside [0, C) is never used as an address:
 * it makes the loss and the gradient NaN.  workspace (8-byte aligned): clipmi_coop_head_workspace_bytes(B, E, C) bytes.  Four launches.
 * CLIPMI_ERR_SHAPE: B < 1, C < 2, E < 1, ld < E.  CLIPMI_ERR_ARG: a null pointer, a non-finite scale or grad_scale. */
size_t clipmi_coop_head_workspace_bytes(int B, int E, int C);
int clipmi_coop_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                     float grad_scale, float* loss, float* d_text, void* d_text16, void* workspace, size_t workspace_bytes,
                     clipmi_stream_t stream);

/* The context's gradient and torch.optim.SGD's step.  d_embed fp32 [C * L, D]: grad_scale * d loss / d (input embedding row), L rows per
 * prompt.  grad[j, :] = (sum_c d_embed[c * L + 1 + j, :]) / grad_scale for j < n_ctx, the classes added in ascending order (generic
 * context, ctx [n_ctx, D]); with per_class != 0 there is no sum and ctx is [C, n_ctx, D].  Then torch.optim.SGD's rule (the steps of
 * clipmi_adapter_train_step, each add(other, alpha) as ONE fused multiply-add, which is how torch's GPU kernels round it: the step equals
 * torch.optim.SGD on the GPU bit for bit) on every element of ctx with the rate *lr (device); buf: the momentum buffer (NULL when momentum == 0); first_step != 0 initialises
 * it from this gradient.  grad_out (ctx's shape, may be NULL) receives the gradient before weight decay.  ctx == NULL: only grad_out is
 * written (no step; lr may be NULL).  1 + n_ctx <= L.  One launch, no atomics. */
int clipmi_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class,
                    float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                    clipmi_stream_t stream);

/* The transposed weight copies of the frozen text tower, packed once by the caller: fp16, contiguous, 16-byte aligned.  w_*_t is the
 * transpose of the clipmi_block_weights member of the same name ([in, out] row-major); proj is text_projection itself, fp16 [Dt, E]. */
typedef struct clipmi_block_dgrad {
  const void* w_qkv_t;   /* [D, 3D] */
  const void* w_out_t;   /* [D, D]  */
  const void* w_fc_t;    /* [D, 4D] */
  const void* w_proj_t;  /* [4D, D] */
} clipmi_block_dgrad;
typedef struct clipmi_text_dgrad {
  const void* proj;                  /* [Dt, E] */
  const clipmi_block_dgrad* blocks;  /* host array [text_layers] */
} clipmi_text_dgrad;

/* Bytes of the workspace and of the stash the three calls below need for n_prompts prompts of seq_rows live token rows (0 = the whole
 * context).  Either pointer may be NULL.  Both are 0 for arguments the calls refuse. */
int clipmi_text_train_bytes(const clipmi_model* m, int n_prompts, int seq_rows, size_t* workspace_bytes, size_t* stash_bytes);

/* clipmi_text_encoder with everything its backward needs kept in `stash`.  prompts (fp16 | fp32) [C, context_length, Dt] without the
 * positional embedding; ctx fp32 (NULL = none): the context vectors that replace token rows 1 .. n_ctx of every prompt, [n_ctx, Dt], or
 * [C, n_ctx, Dt] with ctx_per_class != 0, taken in fp32 as they are.  The blocks run LayerNorm, GEMM and attention as separate launches
 * on the fp32 residual stream (the unfolded path of clipmi_text_encoder), and c_fc keeps its fp16 pre-activation: QuickGELU is an
 * element-wise launch on that rounded value.  Per block the stash keeps the fp32 input rows, the fp32 rows before ln_2, the fp16 qkv
 * and the fp16 c_fc pre-activation (22 Dt bytes per token row and layer), plus the last block's output rows (the input of ln_final)
 * and the gathered EOT row indices.  seq_rows as clipmi_text_encoder takes it.  A hook with deep prompts: CLIPMI_ERR_ARG;
 * CLIPMI_CALL_STREAM_F16: CLIPMI_ERR_STATE.  workspace and stash 256-byte aligned.
 *
 * Byte layout of the stash, with M = C * L token rows (L = the live rows), layers = text_layers and align256(n) = n rounded up to a
 * multiple of 256; every slab is row-major over the M rows and starts where the one before it ends:
 *   2 * layers + 1 fp32 slabs [M, Dt] of align256(M * Dt * 4) bytes each, in the order x_in(0), x_mid(0), x_in(1), x_mid(1), ...,
 *       x_in(layers - 1), x_mid(layers - 1), the input of ln_final -- x_in(i): the input rows of block i (x_in(0): prompts with the
 *       context in place plus the positional embedding), x_mid(i): its rows before ln_2; x_in(i + 1) is the output of block i;
 *   layers fp16 slabs [M, 3 Dt] of align256(M * Dt * 6) bytes each: qkv(0), ..., qkv(layers - 1), the in-projection's output with its bias;
 *   layers fp16 slabs [M, 4 Dt] of align256(M * Dt * 8) bytes each: c_fc's pre-activation with its bias, block 0 first;
 *   C int32: the EOT row indices c * L + eot[c], eot clamped into [0, L - 1] (the stash reserves align256(C * 8) bytes for them).
 * clipmi_text_train_bytes reports the sum.  The backward only reads the stash. */
int clipmi_text_encoder_train(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int ctx_per_class,
                              const int32_t* eot, int n_prompts, int seq_rows, const clipmi_prompt_hook* hook, float* out,
                              void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, unsigned flags,
                              clipmi_stream_t stream);

/* The backward of the call above from the stash it left: d_out fp32 [C, E] (the gradient of `out`, e.g. clipmi_coop_head's d_text) ->
 * d_embed fp32 [C * L, Dt], the gradient of the input embedding rows (L = the live rows), overwritten.  Tail: d_out text_projection^T,
 * ln_final's backward on the EOT rows scattered into the zeroed stream; then per block, last to first: c_proj's dgrad, QuickGELU's
 * backward, c_fc's dgrad, ln_2's backward, out-proj's dgrad, the attention backward, in-proj's dgrad, ln_1's backward.  GEMM operands
 * fp16, accumulation and the gradient stream fp32.  operand_stats (device, NULL or 4 x uint64, zeroed by the caller): over every fp16
 * dgrad-GEMM operand element of the call {elements, exact zeros, fp16 subnormals, the largest magnitude's fp16 bits} -- the measurement
 * behind grad_scale's default (profiles/coopfit_parity.txt); it costs one launch per operand.  The counts are added into the four
 * words and the magnitude is kept as a maximum; +0 and -0 both count as zeros, 0x0400 (2^-14) is the smallest pattern that is not a
 * subnormal, infinity reads 0x7c00, and a NaN operand element makes the largest-magnitude statistic read 0x7fff. */
int clipmi_text_encoder_backward(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int n_prompts, int seq_rows,
                                 float* d_embed, void* workspace, size_t workspace_bytes, const void* stash, size_t stash_bytes,
                                 unsigned long long* operand_stats, clipmi_stream_t stream);

/* One training step of CoOp as ONE call: clipmi_text_encoder_train, clipmi_coop_head, clipmi_text_encoder_backward and clipmi_ctx_step
 * enqueued in this order on `stream` -- the same launches, the same bits.  ctx is the fp32 master, updated in place.  workspace of
 * clipmi_coop_train_step_bytes(...) bytes (256-byte aligned), stash as clipmi_text_train_bytes reports it. */
size_t clipmi_coop_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B);
int clipmi_coop_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                           int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld,
                           const int64_t* labels, int B, float scale, float grad_scale, const float* lr, int first_step, float momentum,
                           float dampening, float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace,
                           size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * VPT's visual prompts trained on the device (trainers/classification/vpt.py; clip/model.py VisionTransformer with prompt rows): the
 * gradient of the image features with respect to the prompt rows `visual.VPT` and `visual.transformer.resblocks.{i}.VPT_shallow`
 * with the image tower frozen, the image-side cross-entropy head and torch.optim.SGD's step on the prompts (csrc/vision_backward.hip,
 * csrc/prompt_train.hip, DESIGN.md "VPT fit").  The blocks' backward is the text tower's without a mask (clipmi_attention_backward_full).
 * The whole backward carries grad_scale * gradient; only clipmi_vpt_head and clipmi_vpt_step know the factor.
 * These exports are additive: the ABI version does not change with them.
 * ---------------------------------------------------------------------------------------------------- */

/* The transposed weight copies of the frozen image tower, packed once by the caller like clipmi_text_dgrad: proj is visual.proj itself,
 * fp16 [Dv, E]; blocks a host array [vision_layers]. */
typedef struct clipmi_vision_dgrad {
  const void* proj;                  /* [Dv, E] */
  const clipmi_block_dgrad* blocks;  /* host array [vision_layers] */
} clipmi_vision_dgrad;

/* Bytes of the workspace and of the stash the calls below need for B images with n_ctx prompt rows each.  Either pointer may be NULL.
 * Both are 0 for arguments the calls refuse (tokens + n_ctx > 224: CLIPMI_ERR_SHAPE). */
int clipmi_vision_train_bytes(const clipmi_model* m, int B, int n_ctx, size_t* workspace_bytes, size_t* stash_bytes);

/* clipmi_encode_image with VPT's prompts and everything its backward needs kept in `stash`.  image [B, 3, R, R] fp16 | fp32; prompts fp32
 * [depth, n_ctx, Dv], the masters: slot 0 is visual.VPT, whose rows are appended behind the patch rows after the positional embedding and
 * pass through ln_pre; slot i (1 <= i < depth) overwrites the LAST n_ctx token rows of every image before block i.  The values the
 * forward reads are the masters rounded through fp16 (the reference's .half()).  L = tokens + n_ctx rows per image.  The blocks run
 * LayerNorm, GEMM, attention (no mask) as separate launches on the fp32 residual stream, c_fc keeps its fp16 pre-activation and
 * QuickGELU is an element-wise launch on that rounded value; then ln_post on the class rows and the projection: out fp32 [B, E].
 * Requires a patch size that divides the resolution, Dv % 64 == 0, E % 64 == 0, L <= 224 (640 with the option vision_train_long;
 * CLIPMI_ERR_SHAPE), 1 <= depth <= vision_layers.  Patches of 8, 16 and 32 pixels go through clipmi_patch_embed's loader and
 * clipmi_embed_ln; any other patch size (ViT-L/14) through clipmi_patchify into the workspace, the dense GEMM whose epilogue adds the
 * positional rows, and clipmi_embed_ln without the positional add, as in clipmi_encode_image (the workspace then holds the im2col
 * matrix, B * grid^2 * kpad * 2 bytes, where it holds the fp16 copy of an fp32 image batch otherwise: clipmi_vision_train_bytes).
 * CLIPMI_CALL_STREAM_F16: CLIPMI_ERR_STATE.  workspace and stash 256-byte aligned.
 *
 * Byte layout of the stash: clipmi_text_encoder_train's with M = B * L token rows, Dt = Dv and layers = vision_layers --
 *   2 * layers + 1 fp32 slabs [M, Dv] of align256(M * Dv * 4) bytes: x_in(0), x_mid(0), ..., x_in(layers - 1), x_mid(layers - 1), the input
 *       of ln_post; x_in(0) is ln_pre's output, x_in(i) the output of block i - 1 with block i's prompt rows in place;
 *   layers fp16 slabs [M, 3 Dv] of align256(M * Dv * 6) bytes: qkv(i);  layers fp16 slabs [M, 4 Dv] of align256(M * Dv * 8) bytes: c_fc's
 *       pre-activation;
 *   B int32: the class row indices b * L (align256(B * 8) bytes reserved; the B words behind them are zero);
 * and behind it the rounded prompts fp32 [depth, n_ctx, Dv] (align256(layers * n_ctx * Dv * 4) bytes reserved).  The backward only reads
 * the stash. */
int clipmi_vision_encoder_train(clipmi_model* m, const void* image, int image_dtype, int B, const float* prompts, int n_ctx, int depth,
                                float* out, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, unsigned flags,
                                clipmi_stream_t stream);

/* The backward of the call above from the stash it left: d_out fp32 [B, E] -> d_prompts fp32 [depth, n_ctx, Dv] = the gradient of the
 * prompts (the rounding passes it straight through), overwritten.  Tail: d_out proj^T, ln_post's backward on the class rows scattered into
 * the zeroed stream; per block, last to first, clipmi_text_encoder_backward's sequence with clipmi_attention_backward_full; after block
 * i's ln_1 backward (1 <= i < depth) d_prompts[i][j] = sum_b g[b * L + tokens + j] (b ascending) and those rows of the stream are zeroed;
 * after block 0 the batch sum of the prompt rows goes through ln_pre's backward on n_ctx rows (LayerNorm's backward is linear in dy and
 * every image's pre-LN row is the prompt).  Nothing below ln_pre is differentiated.  operand_stats as clipmi_text_encoder_backward's. */
int clipmi_vision_encoder_backward(clipmi_model* m, const clipmi_vision_dgrad* wt, const float* d_out, int B, int n_ctx, int depth,
                                   float* d_prompts, void* workspace, size_t workspace_bytes, const void* stash, size_t stash_bytes,
                                   unsigned long long* operand_stats, clipmi_stream_t stream);

/* VPT's loss head: clipmi_coop_head with the gradient on the image side.  feats fp32 [B, E] (row stride ld), text fp32 [C, E]:
 *   x_b = f_b / |f_b|;  u_c = t_c / |t_c|;  z = scale X U^T;  loss = mean_b CE(z_b, y_b);  dz = grad_scale (softmax(z) - onehot(y)) / B
 *   dx_b = scale sum_c dz[b, c] u_c (c ascending);  d_feats[b, :] = (dx_b - x_b (x_b . dx_b)) / |f_b|
 * loss fp32 [1] or NULL, the float64 mean of the row losses; d_feats fp32 [B, E] dense.  A label outside [0, C) is never used as an
 * address: it makes the loss and that row's gradient NaN.  workspace (8-byte aligned) of clipmi_vpt_head_workspace_bytes bytes.  Four
 * launches.  Refusals as clipmi_coop_head's. */
size_t clipmi_vpt_head_workspace_bytes(int B, int E, int C);
int clipmi_vpt_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                    float grad_scale, float* loss, float* d_feats, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* torch.optim.SGD's step on the [depth, n_ctx, D] master block, one launch: grad = d_prompts / grad_scale, then clipmi_ctx_step's rule on
 * every element (the same arguments; equal to torch.optim.SGD on the GPU bit for bit).  grad_out (the block's shape, may be NULL)
 * receives the gradient before weight decay.  prompts == NULL: only grad_out is written. */
int clipmi_vpt_step(const float* d_prompts, float* prompts, float* buf, float* grad_out, int depth, int n_ctx, int D, float grad_scale,
                    const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                    clipmi_stream_t stream);

/* One training step of VPT as ONE call: clipmi_vision_encoder_train, clipmi_vpt_head, clipmi_vision_encoder_backward and clipmi_vpt_step
 * enqueued in this order on `stream` -- the same launches, the same bits.  prompts is the fp32 master, updated in place.  workspace of
 * clipmi_vpt_train_step_bytes(m, B, n_ctx, C) bytes (256-byte aligned), stash as clipmi_vision_train_bytes reports it. */
size_t clipmi_vpt_train_step_bytes(const clipmi_model* m, int B, int n_ctx, int C);
int clipmi_vpt_train_step(clipmi_model* m, const clipmi_vision_dgrad* wt, const void* image, int image_dtype, int B, float* prompts, float* buf,
                          int n_ctx, int depth, const float* text, int C, const int64_t* labels, float scale, float grad_scale,
                          const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* loss,
                          float* grad_out, void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes,
                          clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * MaPLe's multi-modal prompts trained on the device (trainers/classification/maple.py:77-216; clip/model.py:259-331): the loss reaches the
 * learned parameters through BOTH frozen towers.  The text tower's training forward and backward with deep prompts, the coupling
 * functions (Linear Dt -> Dv) that make the image tower's prompt rows, a joint loss head and torch.optim.SGD's step over one fp32 master
 * block (csrc/text_backward.hip, csrc/maple_train.hip, csrc/prompt_train.hip, DESIGN.md "MaPLe fit").  The master block, d = the depth:
 *   [ ctx [n_ctx, Dt] | compound_prompts_text [d - 1, n_ctx, Dt] | proj.weight [Dv, Dt] | proj.bias [Dv] |
 *     compound_prompt_projections.weight [d - 1, Dv, Dt] | compound_prompt_projections.bias [d - 1, Dv] ]
 * Both backwards carry grad_scale * gradient; only clipmi_maple_head and clipmi_maple_step know the factor.
 * These exports are additive: the ABI version does not change with them.
 * ---------------------------------------------------------------------------------------------------- */

/* clipmi_text_encoder_train with MaPLe's deep text prompts: deep fp32 [n_deep, n_ctx, Dt] (NULL with n_deep == 0).  Before block i
 * (1 <= i <= n_deep) the rows 1 .. n_ctx of every prompt in the stash slab x_in(i) are overwritten with deep[i - 1] rounded through fp16
 * (the reference's .half(); no positional embedding) -- in place, so the stash holds what block i read; workspace and stash sizes are
 * clipmi_text_train_bytes's.  n_deep == 0: the plain call, bit for bit.  1 + n_deep > text_layers or 1 + n_ctx > the live rows:
 * CLIPMI_ERR_SHAPE, nothing written. */
int clipmi_text_encoder_train_deep(clipmi_model* m, const void* prompts, int dtype, const float* ctx, int n_ctx, int ctx_per_class,
                                   const int32_t* eot, int n_prompts, int seq_rows, const float* deep, int n_deep, float* out,
                                   void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, unsigned flags,
                                   clipmi_stream_t stream);

/* Its backward: clipmi_text_encoder_backward, and after block i's ln_1 backward (1 <= i <= n_deep) d_deep[i - 1][j] = sum_c g[c L + 1 + j]
 * (c ascending) with those rows of the gradient stream zeroed behind the sum (block i - 1's outputs there were discarded).  d_deep fp32
 * [n_deep, n_ctx, Dt], overwritten; ctx's gradient comes from d_embed rows 1 .. n_ctx as clipmi_ctx_step forms it.  No float atomics. */
int clipmi_text_encoder_backward_deep(clipmi_model* m, const clipmi_text_dgrad* wt, const float* d_out, int n_prompts, int seq_rows,
                                      int n_ctx, int n_deep, float* d_embed, float* d_deep, void* workspace, size_t workspace_bytes,
                                      const void* stash, size_t stash_bytes, unsigned long long* operand_stats, clipmi_stream_t stream);

/* Floats of the master block (0 for arguments the calls refuse). */
size_t clipmi_maple_block_floats(int n_ctx, int depth, int Dt, int Dv);

/* The coupling functions, one launch: vis fp32 [depth, n_ctx, Dv], the prompt block clipmi_vision_encoder_train takes (slot 0 is
 * shared_ctx).  vis[0] = h(ctx) h(proj.weight)^T + h(proj.bias), h = rounding through fp16 (proj is a half Linear); vis[i] = t_i W_i^T + b_i
 * in fp32 for i >= 1.  fp32 accumulation: 64 interleaved chains over k ascending, then a fixed tree. */
int clipmi_maple_couple(const float* block, int n_ctx, int depth, int Dt, int Dv, float* vis, clipmi_stream_t stream);

/* The joint head: clipmi_coop_head's d_text [C, E] (and its fp16 copy d_text16, may be NULL) and clipmi_vpt_head's d_feats [B, E] and
 * loss from ONE logits matrix -- norms, logits and softmax once, then both heads' gradient kernels: each output equals its own head's
 * bit for bit.  workspace as clipmi_coop_head's.  Five launches. */
size_t clipmi_maple_head_workspace_bytes(int B, int E, int C);
int clipmi_maple_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                      float grad_scale, float* loss, float* d_feats, float* d_text, void* d_text16, void* workspace,
                      size_t workspace_bytes, clipmi_stream_t stream);

/* The coupling functions' backward and torch.optim.SGD's step on every element of the master block, two launches whatever the depth.
 * d_embed fp32 [C * L, Dt] and d_deep fp32 [depth - 1, n_ctx, Dt] from clipmi_text_encoder_backward_deep, d_vis fp32 [depth, n_ctx, Dv]
 * from clipmi_vision_encoder_backward.  First launch: the text-side prompts' gradient d_t_i = (text tower's) + d_vis[i] W_i into the
 * workspace, beside a copy of the prompts.  Second launch, one thread per element: dW_i[v, k] = sum_j d_vis[i][j][v] t_i[j][k] and
 * db_i[v] = sum_j d_vis[i][j][v] formed in registers from that copy (slot 0 multiplies h(ctx) and h(proj.weight)); every gradient times
 * 1 / grad_scale, then clipmi_ctx_step's rule (equal to torch.optim.SGD on the GPU bit for bit given grad_out).  grad_out (the block's
 * shape, may be NULL) receives the gradient before weight decay.  apply == 0: only grad_out is written.  workspace (256-byte aligned) of
 * clipmi_maple_step_workspace_bytes bytes. */
size_t clipmi_maple_step_workspace_bytes(int n_ctx, int depth, int Dt);
int clipmi_maple_step(const float* d_embed, const float* d_deep, const float* d_vis, float* block, float* buf, float* grad_out, int apply,
                      int C, int L, int n_ctx, int depth, int Dt, int Dv, float grad_scale, const float* lr, int first_step,
                      float momentum, float dampening, float weight_decay, int nesterov, void* workspace, size_t workspace_bytes,
                      clipmi_stream_t stream);

/* One training step of MaPLe as ONE call: clipmi_maple_couple, clipmi_text_encoder_train_deep, clipmi_vision_encoder_train,
 * clipmi_maple_head, clipmi_text_encoder_backward_deep, clipmi_vision_encoder_backward and clipmi_maple_step enqueued in this order on
 * `stream` -- the same launches, the same bits.  block is the fp32 master, updated in place.  workspace of
 * clipmi_maple_train_step_bytes(...) bytes (256-byte aligned); the stashes as clipmi_text_train_bytes / clipmi_vision_train_bytes report. */
size_t clipmi_maple_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int n_ctx, int depth);
int clipmi_maple_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype,
                            const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B,
                            const int64_t* labels, float* block, float* buf, int n_ctx, int depth, float scale, float grad_scale,
                            const float* lr, int first_step, float momentum, float dampening, float weight_decay, int nesterov,
                            float* loss, float* grad_out, void* workspace, size_t workspace_bytes, void* text_stash,
                            size_t text_stash_bytes, void* vision_stash, size_t vision_stash_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * PromptSRC's and IVLP's independent prompts trained on the device (trainers/classification/promptsrc.py:73-317; clip/model.py:191-256):
 * MaPLe's two training towers without the coupling functions -- the text prompts (ctx and the blocks' VPT_shallow) and the image prompts
 * (visual.VPT and the image blocks' VPT_shallow) are parameters of their own -- and a head of four terms against a frozen teacher: the
 * cross-entropy, two L1 distances (text features to the teacher's text features, image features to the frozen plain tower's) and the KL
 * divergence of the prompted logits from the teacher's (csrc/promptsrc_train.hip, csrc/prompt_train.hip, DESIGN.md "PromptSRC fit").
 * The master block, dt / dv = the text / image prompt depth:
 *   [ ctx [nt, Dt] | text deep [dt - 1, nt, Dt] | visual.VPT and image deep [dv, nv, Dv] ]
 * Its text part is the [ctx; deep] pair of clipmi_text_encoder_train_deep, its image part the block of clipmi_vision_encoder_train.
 * IVLP is the same path with the three weights 0.  These exports are additive: the ABI version does not change with them.
 * ---------------------------------------------------------------------------------------------------- */

/* The head.  feats fp32 [B, E] (row stride ld) the prompted image features, zs_feats fp32 [B, E] (dense) the frozen plain tower's,
 * text fp32 [C, E] the prompted text features, teacher fp32 [C, E] the frozen text features; all four are normalised here:
 *   x_b = f_b / |f_b|;  y_b = zs_b / |zs_b|;  u_c = t_c / |t_c|;  o_c = teacher_c / |teacher_c|;  z = scale X U^T;  zz = scale Y O^T
 *   p = softmax(z_b);  q = softmax(zz_b)
 *   loss = mean_b CE(z_b, label_b) + w_text mean_{c,e} |u - o| + w_image mean_{b,e} |x - y| + w_logit sum_{b,c} q (log q - log p) / (B C)
 *   dz = grad_scale ((p - onehot) / B + w_logit (p - q) / (B C))
 * d_text [C, E] (and its fp16 copy d_text16, may be NULL) and d_feats [B, E] are clipmi_maple_head's on that dz, plus the images of
 * grad_scale w_text sign(u - o) / (C E) and grad_scale w_image sign(x - y) / (B E) under the two normalisation backwards; sign(0) = 0 and
 * an addend of exactly 0 is not added.  losses fp32 [5] = {total, CE, text L1, image L1, logit KL}: each the float64 mean of fp32 row
 * sums in a fixed order, each unweighted but the total.  A term whose weight is 0 is SKIPPED, not multiplied in: its loss reads 0, its
 * operand is not read beyond the pointer check, and with all three weights 0 d_text, d_feats and losses[0] are clipmi_maple_head's bit
 * for bit.  w_text, w_image, w_logit: finite, >= 0.  A label outside [0, C) is never used as an address: it makes the cross-entropy,
 * the total, that row of d_feats and -- du_c sums over the images -- every entry of d_text NaN; the two L1 terms and the logit KL keep
 * the bits of the same call with good labels.  A zero row of teacher or zs_feats has no direction: with a non-zero weight that reads it, that
 * row's terms, and through the means the losses they enter, are NaN (as clipmi_prompt_head documents for KgCoOp's teacher).
 * workspace (8-byte aligned) of clipmi_promptsrc_head_workspace_bytes bytes.  Six launches with all weights 0, nine with none 0 (two norm, two logits, the softmax, the two gradient kernels, the L1 kernel, the losses).
 * No float atomics: the same inputs give the same bits.  Every refusal comes ahead of the first launch. */
size_t clipmi_promptsrc_head_workspace_bytes(int B, int E, int C);
int clipmi_promptsrc_head(const float* feats, int64_t ld, const float* zs_feats, const float* text, const float* teacher, const int64_t* labels,
                          int B, int E, int C, float scale, float grad_scale, float w_text, float w_image, float w_logit, float* losses,
                          float* d_feats, float* d_text, void* d_text16, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* Floats of the master block (0 for arguments the calls refuse). */
size_t clipmi_promptsrc_block_floats(int nt, int dt, int Dt, int nv, int dv, int Dv);

/* torch.optim.SGD's step on every element of the master block, one launch.  d_embed fp32 [C * L, Dt] and d_deep fp32 [dt - 1, nt, Dt]
 * (NULL with dt == 1) from clipmi_text_encoder_backward_deep, d_vis fp32 [dv, nv, Dv] from clipmi_vision_encoder_backward.  ctx's gradient
 * is d_embed's rows 1 .. nt summed over the classes in ascending order, as clipmi_ctx_step sums them; every gradient times 1 / grad_scale,
 * then clipmi_ctx_step's rule.  The ctx part equals clipmi_ctx_step and the image part clipmi_vpt_step on the same inputs bit for bit.
 * grad_out (the block's shape, may be NULL) receives the gradient before weight decay.  apply == 0: only grad_out is written. */
int clipmi_promptsrc_step(const float* d_embed, const float* d_deep, const float* d_vis, float* block, float* buf, float* grad_out, int apply,
                          int C, int L, int nt, int dt, int Dt, int nv, int dv, int Dv, float grad_scale, const float* lr, int first_step,
                          float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream);

/* Gaussian-weighted prompt aggregation, one launch over n floats: gpa = first ? weight * block : fmaf(weight, block, gpa). */
int clipmi_gpa_accumulate(const float* block, float* gpa, int64_t n, float weight, int first, clipmi_stream_t stream);

/* One training step as ONE call: clipmi_encode_image (no hook, CLIPMI_CALL_STREAM_F32, on this handle: no second copy of the weights),
 * clipmi_text_encoder_train_deep, clipmi_vision_encoder_train, clipmi_promptsrc_head, clipmi_text_encoder_backward_deep,
 * clipmi_vision_encoder_backward and clipmi_promptsrc_step enqueued in this order on `stream` -- the same launches, the same bits.  The
 * frozen forward runs the fp32 residual stream, as the training forward does; it keeps its fused kernels, which apply QuickGELU to c_fc's
 * fp32 accumulator where the training forward rounds the pre-activation to fp16 first: a model whose image prompts change nothing gives
 * x = y up to that rounding point, not bit for bit.  teacher fp32 [C, E]; block is the fp32 master, updated in place; losses fp32 [5].
 * workspace of clipmi_promptsrc_train_step_bytes(...) bytes (256-byte aligned; the frozen forward shares the image tower's part); the
 * stashes as clipmi_text_train_bytes / clipmi_vision_train_bytes (with nv) report.  Every refusal comes ahead of the first launch. */
size_t clipmi_promptsrc_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int nt, int dt, int nv);
int clipmi_promptsrc_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype,
                                const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B,
                                const int64_t* labels, const float* teacher, float* block, float* buf, int nt, int dt, int nv, int dv,
                                float scale, float grad_scale, float w_text, float w_image, float w_logit, const float* lr, int first_step,
                                float momentum, float dampening, float weight_decay, int nesterov, float* losses, float* grad_out,
                                void* workspace, size_t workspace_bytes, void* text_stash, size_t text_stash_bytes, void* vision_stash,
                                size_t vision_stash_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * KgCoOp's and ProGrad's context trained on the device (trainers/classification/kgcoop.py:246-269, prograd.py:291-304, 371-409): CoOp's
 * forward and backward with another loss head and, for ProGrad, a projection between the backward and the optimiser (DESIGN.md
 * "KgCoOp / ProGrad fit").  `mode` is a plain integer: 0 CoOp, 1 KgCoOp, 2 ProGrad.  `teacher` fp32 [C, E]: the frozen zero-shot text
 * features; the head normalises its rows itself (normalised rows pass unchanged up to rounding).  Additive exports: the ABI version stays.
 * ---------------------------------------------------------------------------------------------------- */

/* The loss head of the three methods.  Arguments as clipmi_coop_head's, and: losses fp32 [3] (required), d_text_kl fp32 [C, E] (ProGrad).
 *   mode 0: clipmi_coop_head; losses[0] = the loss.
 *   mode 1: loss = CE + w (1 - mean_c u_c . o_c), o_c = teacher_c / |teacher_c|; losses = [total, CE, 1 - mean_c u_c . o_c], the mean
 *           over the classes in float64 in a fixed order.  d_text = CoOp's d_text + (-grad_scale w / C) (o_c - u_c (u_c . o_c)) / |t_c|:
 *           with w = 0 CoOp's d_text bit for bit.  w finite, >= 0.  The reference's eps = 1e-7 guards unit vectors and is left out: a
 *           zero teacher row makes that class's loss and gradient NaN.  Five launches.
 *   mode 2: z_tea = scale X O^T;  losses = [xe, kl, not written], xe = mean_b CE(z_b, y_b),
 *           kl = mean_b sum_c -softmax(z_tea / T)[b, c] log_softmax(z / T)[b, c] T^2;
 *           dz_xe = grad_scale (softmax(z) - onehot(y)) / B -> d_text;  dz_kl = grad_scale T (softmax(z / T) - softmax(z_tea / T)) / B
 *           -> d_text_kl, both through CoOp's projection.  T finite, > 0.  The labels reach xe only.  Six launches.
 * d_text16 (may be NULL): d_text rounded to fp16.  A label outside [0, C) makes the cross-entropy and its gradient NaN and is never used
 * as an address.  No float atomics, fixed summation orders: the same input gives the same bits.  workspace (8-byte aligned):
 * clipmi_prompt_head_workspace_bytes(B, E, C, mode) bytes (0 for a bad argument).
 * CLIPMI_ERR_ARG: a bad mode, a null pointer, a non-finite scale or grad_scale, w or T outside its range. */
size_t clipmi_prompt_head_workspace_bytes(int B, int E, int C, int mode);
int clipmi_prompt_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                       float grad_scale, int mode, const float* teacher, float w, float T, float* losses, float* d_text, void* d_text16,
                       float* d_text_kl, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* ProGrad's projection and torch.optim.SGD's step (prograd.py:371-409).  d_embed_xe, d_embed_kl fp32 [C * L, D]: the two outputs of
 * clipmi_text_encoder_backward for clipmi_prompt_head's d_text and d_text_kl.  a and b, the context's two gradients, are formed as
 * clipmi_ctx_step forms its gradient; a.a, b.b and a.b are accumulated in float64 over a partition that depends on the context's size
 * alone.  If a.b < 0, both norms are non-zero and the three sums are finite, the gradient is g = a - lambda (a.b / b.b) b (the scalar in
 * float64, the element in fp32), otherwise g = a -- the reference's `dot(a / |a|, b / |b|) < 0`, which is false for a zero or NaN norm.
 * Then clipmi_ctx_step's SGD rule on ctx.  Optional outputs (device, may be NULL): grad_out (ctx's shape) the gradient applied,
 * projected int [1], dots float64 [3] = {a.a, b.b, a.b}.  ctx == NULL: only the outputs are written (lr may be NULL).  workspace
 * (256-byte aligned): clipmi_prograd_step_workspace_bytes(C, D, n_ctx, per_class) bytes.  Two launches, no atomics. */
size_t clipmi_prograd_step_workspace_bytes(int C, int D, int n_ctx, int per_class);
int clipmi_prograd_step(const float* d_embed_xe, const float* d_embed_kl, float* ctx, float* buf, float* grad_out, int* projected,
                        double* dots, int C, int L, int D, int n_ctx, int per_class, float grad_scale, float lambda, const float* lr,
                        int first_step, float momentum, float dampening, float weight_decay, int nesterov, void* workspace,
                        size_t workspace_bytes, clipmi_stream_t stream);

/* The class-sharded fit of CoOp, KgCoOp and ProGrad (DESIGN.md "Class-sharded CoOp fit"): G ranks, rank r owning the contiguous classes
 * the balanced split gives it (the first C mod G ranks one class more, C >= G), two all-gathers per step.  Everything below is fp32 with
 * fixed summation orders and no atomics; with G = 1 each chain is the unsharded entry point's, bit for bit.
 *
 * Compaction: gathered fp32 [G, P, E], P = ceil(C / G), block r holding rank r's rows first and padding behind them that is never read;
 * out fp32 [C, E], row c the row of the rank that owns class c.  One launch. */
int clipmi_shard_compact(const float* gathered, float* out, int C, int G, int64_t E, clipmi_stream_t stream);

/* A rank's partial context gradient (generic context): partial fp32 [n_ctx, D], partial[j, :] = sum_c d_embed[c * L + 1 + j, :] over the
 * C classes of d_embed fp32 [C * L, D] -- the rank's own -- in ascending order, unscaled.  1 + n_ctx <= L.  One launch. */
int clipmi_ctx_partial(const float* d_embed, float* partial, int C, int L, int D, int n_ctx, clipmi_stream_t stream);

/* The gathered partials' sum and the step: partials fp32, rank r's [n_ctx, D] at partials + r * rank_stride (elements, >= n_ctx * D);
 * grad = (partial_0 + partial_1 + .. + partial_{G-1}) / grad_scale, added in rank order, then clipmi_ctx_step's SGD rule on ctx
 * [n_ctx, D] with the same optional outputs and NULL conventions.  Every rank that is given the same partials writes the same bits,
 * whatever order the bytes arrived in.  One launch. */
int clipmi_ctx_step_gathered(const float* partials, int G, int64_t rank_stride, float* ctx, float* buf, float* grad_out, int D, int n_ctx,
                             float grad_scale, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                             int nesterov, clipmi_stream_t stream);

/* ProGrad under the sharding, in two calls with at most one all-gather between them.  The first forms a and b (kept in the workspace) and
 * this rank's float64 dots {a.a, b.b, a.b} into dots_rank [3], over the partition clipmi_prograd_step uses.  per_class == 0 (generic
 * context): src_a, src_b are the gathered partials of the two losses as clipmi_ctx_step_gathered takes them, a and b their rank-ordered
 * sums over 1 / grad_scale, n_ctx * D elements, the same on every rank (nothing more to gather: the second call takes G = 1).
 * per_class != 0: src_a, src_b are the rank's own two d_embed fp32 [C * L, D], a and b its own C * n_ctx * D elements; G and rank_stride
 * are not read, and dots_rank is what the ranks gather.  The second call adds dots_ranks float64 [G, 3] in rank order, decides as
 * clipmi_prograd_step decides and steps the `total` elements of ctx that the first call's a and b cover, with clipmi_prograd_step's
 * optional outputs.  workspace (256-byte aligned, the same for both calls): clipmi_shard_prograd_workspace_bytes(total) bytes (0 for a
 * total outside the range).  Two launches and one launch. */
size_t clipmi_shard_prograd_workspace_bytes(int64_t total);
int clipmi_shard_prograd_dots(const float* src_a, const float* src_b, int G, int64_t rank_stride, int C, int L, int D, int n_ctx,
                              int per_class, float grad_scale, double* dots_rank, void* workspace, size_t workspace_bytes,
                              clipmi_stream_t stream);
int clipmi_shard_prograd_apply(const double* dots_ranks, int G, float lambda, float* ctx, float* buf, float* grad_out, int* projected,
                               double* dots, int64_t total, const float* lr, int first_step, float momentum, float dampening,
                               float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* The batch-sharded fits through the image tower (VPT, MaPLe, PromptSRC / IVLP; DESIGN.md "Batch-sharded image-tower fits"): every rank
 * runs the step over its own B / G images and sends one block [scale * gradient | losses]; one all-gather leaves rank r's block at
 * gathered + r * stride (floats; stride >= total, and the floats of a row behind `total` are never read).
 *
 * The rank-ordered mean: out[i] = (((p_0[i] + p_1[i]) + p_2[i]) + ..) * inv with inv = (float)(1.0 / world), all in fp32, no atomics:
 * the same bits on every rank and on every run; an inf or a NaN of any rank stays one; with world == 1 the output is the input bit for
 * bit.  16-byte loads and stores where the row bases, the stride and the output allow, single floats elsewhere.  Refused before any
 * launch: a null or misaligned (4 bytes) pointer, world < 1, total outside [1, 2^39), stride < total, out overlapping the gathered
 * blocks.  One launch. */
int clipmi_block_rank_mean(const float* gathered, int world, size_t stride, size_t total, float* out, clipmi_stream_t stream);

/* The same mean, divided by grad_scale, and torch.optim.SGD's rule on params fp32 [total] in place (clipmi_ctx_step's optional outputs
 * and NULL conventions: params NULL forms grad_out alone, buf may be NULL without a momentum): the static SGD route's step.  With
 * world == 1 the bits are those of the fit's own step entry applied to the same scale * gradient.  params, buf and grad_out must not
 * overlap the gathered blocks.  One launch. */
int clipmi_block_step_gathered(const float* gathered, int world, size_t stride, size_t total, float grad_scale, float* params, float* buf,
                               float* grad_out, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                               int nesterov, clipmi_stream_t stream);

/* One training step of CoOp, KgCoOp or ProGrad as ONE call: clipmi_text_encoder_train, clipmi_prompt_head, clipmi_text_encoder_backward
 * (twice for ProGrad, one after the other: they share the tower's workspace and read the same stash) and clipmi_ctx_step or
 * clipmi_prograd_step, enqueued in this order on `stream` -- the same launches, the same bits as the calls one by one.  losses fp32 [3]
 * as clipmi_prompt_head writes them; projected and dots as clipmi_prograd_step's (ProGrad; may be NULL). */
size_t clipmi_prompt_train_step_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx, int ctx_per_class);
int clipmi_prompt_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf, int n_ctx,
                             int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld,
                             const int64_t* labels, int B, float scale, float grad_scale, int mode, const float* teacher, float w, float T,
                             float lambda, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                             int nesterov, float* losses, float* grad_out, int* projected, double* dots, void* workspace,
                             size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * A dynamic loss scale for the fits that step through clipmi_ctx_step (CoOp, KgCoOp): torch.cuda.amp.GradScaler's rule on the device
 * (reference trainers/classification/coop.py:286-291; csrc/grad_scaler.hip, DESIGN.md "Dynamic loss scale").  The backward carries
 * scale * gradient with the scale read from a device block, a step whose gradient holds an inf or a NaN changes neither the context nor the
 * momentum buffer, and the scale backs off and grows again; nothing is read back to the host.  Additive exports: the ABI version stays.
 *
 * The scaler's state: 20 bytes on the device, 4-byte aligned, owned by the caller, who writes {init_scale, 0, 0, 0, 0} into it before the
 * first step (on the stream or before it) and may read it after a synchronisation.  Only the calls below write it.
 * ---------------------------------------------------------------------------------------------------- */
typedef struct clipmi_scaler_state {
  float scale;            /* the backward of the next step carries scale * gradient */
  int32_t growth_tracker; /* clean steps in a row since the scale last changed, < growth_interval */
  int32_t skipped_steps;  /* steps that found an inf or a NaN and were not applied */
  int32_t applied_steps;  /* steps whose SGD update was applied */
  int32_t found_inf;      /* 1 when the last step was skipped, else 0 */
} clipmi_scaler_state;

/* x[r, c] *= state->scale over a dense fp32 [rows, cols] matrix: clipmi_prompt_head run at grad_scale = 1 followed by this launch gives
 * scale * d_text.  For a power-of-two scale the product is exact, so the result equals the head run at grad_scale = scale bit for bit --
 * unless an fp32 intermediate of the head at grad_scale = 1 is a subnormal (or overflows at grad_scale = scale), where the two round
 * differently.  One launch. */
int clipmi_grad_scale_rows(float* x, int rows, int cols, const clipmi_scaler_state* state, clipmi_stream_t stream);

/* clipmi_ctx_step under the scaler's rule.  d_embed, ctx ([n_ctx, D], or [C, n_ctx, D] with per_class != 0), buf, grad_out, lr (device) and
 * the SGD rule as clipmi_ctx_step's, with four differences:
 *   grad_scale is state->scale, read on the device;
 *   found = any element of the gradient (a context row's sum over the classes, divided by the scale) is an inf or a NaN -- every element is
 *     looked at, rows outside 1 .. n_ctx are not (torch._amp_foreach_non_finite_check_and_unscale_);
 *   ctx and buf are written only when found is clear; grad_out (may be NULL) receives the unscaled gradient either way;
 *   the momentum buffer is initialised from the gradient of the first APPLIED step (state->applied_steps == 0), not of the first call, as
 *     torch.optim.SGD does when GradScaler.step skips the first steps: there is no first_step argument.
 * Then torch._amp_update_scale_ on the block: found: scale *= backoff_factor, growth_tracker = 0, skipped_steps += 1; otherwise
 * applied_steps += 1 and growth_tracker += 1, and when it reaches growth_interval the scale is multiplied by growth_factor (unless the
 * product is not finite) and the tracker starts again.  found_inf = found.  ctx, lr and state are required.  Three launches: the gradient
 * with one integer flag per workgroup, one workgroup that decides and updates the block, the step; no atomics, no workgroup reads what another
 * of the same launch writes, the same inputs give the same bits.  With found clear ctx, buf and grad_out equal clipmi_ctx_step's at
 * grad_scale = scale and first_step = (applied_steps == 0) bit for bit.  workspace (256-byte aligned):
 * clipmi_ctx_step_scaled_workspace_bytes(C, D, n_ctx, per_class) bytes, 0 for arguments the call refuses.  Every check precedes the first
 * launch.  CLIPMI_ERR_ARG: a null pointer, a factor that is not finite or not positive, growth_interval < 1, SGD's own refusals;
 * CLIPMI_ERR_SHAPE: C < 1, D < 1, n_ctx < 1, 1 + n_ctx > L. */
size_t clipmi_ctx_step_scaled_workspace_bytes(int C, int D, int n_ctx, int per_class);
int clipmi_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, int C, int L, int D, int n_ctx, int per_class,
                           clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr,
                           float momentum, float dampening, float weight_decay, int nesterov, void* workspace, size_t workspace_bytes,
                           clipmi_stream_t stream);

/* One training step of CoOp or KgCoOp under the scaler as ONE call: clipmi_text_encoder_train, clipmi_prompt_head at grad_scale = 1,
 * clipmi_grad_scale_rows on its d_text, clipmi_text_encoder_backward and clipmi_ctx_step_scaled, enqueued in this order on `stream` --
 * the same launches, the same bits as the calls one by one.  Arguments as clipmi_prompt_train_step's; mode 2 (ProGrad): CLIPMI_ERR_ARG
 * (the reference's own amp branch hands GradScaler.scale a tuple there).  The scalar, shape and pointer checks of every stage precede
 * the first launch.  workspace of clipmi_prompt_train_step_scaled_bytes(...) bytes (256-byte aligned; 0 for arguments the call refuses). */
size_t clipmi_prompt_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx,
                                             int ctx_per_class);
int clipmi_prompt_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf,
                                    int n_ctx, int ctx_per_class, const int32_t* eot, int n_prompts, int seq_rows, const float* feats,
                                    int64_t ld, const int64_t* labels, int B, float scale, clipmi_scaler_state* state, float growth_factor,
                                    float backoff_factor, int growth_interval, int mode, const float* teacher, float w, const float* lr,
                                    float momentum, float dampening, float weight_decay, int nesterov, float* losses, float* grad_out,
                                    void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * The class token at the front or in the middle of a CoOp, KgCoOp or ProGrad prompt (reference trainers/classification/coop.py:128-192,
 * kgcoop.py:172-230, prograd.py:150-210; csrc/prompt_position.hip, DESIGN.md "CoOp fit").  `position` is a plain int with ProDA's codes
 * (0 front, 1 middle, 2 end) and the row rule is clipmi_proda_embed's: with nl the class's name length and h = n_ctx / 2, context vector j
 * sits on row 1 + j (end), 1 + nl + j (front), or 1 + j for j < h and 1 + nl + j otherwise (middle); the name tokens take the rows left
 * free in [1, 1 + n_ctx + nl), in order; every other row, SOS included, is the base prompt's.  name_lens int32 [C] lives on the device; a
 * name length is read clamped to [0, L - 2 - n_ctx] and is never used as an unchecked address.  Additive exports: the ABI version stays.
 *
 * clipmi_prompt_place: base [C, Lc, D] (dtype: CLIPMI_F16 or CLIPMI_F32), the token embeddings of "X .. X name.", and ctx fp32 [n_ctx, D]
 *   (or [C, n_ctx, D] with per_class != 0) -> prompts fp32 [C, Lc, D], rows [0, L) of each written (L <= Lc the live rows; the positional
 *   embedding is the tower's to add).  A context row is copied from the fp32 master unchanged, a base row is widened, which is exact.
 *   One launch, 16-byte loads and stores: 16-byte aligned pointers, D a multiple of 4.  The tower then runs on the result:
 *   clipmi_text_encoder_train(m, prompts, CLIPMI_F32, NULL, 0, 0, eot, C, seq_rows, ...) with the token ids' own EOT indices, which do
 *   not change with the position.
 * clipmi_prompt_unplace: the inverse on the gradient stream.  d_embed fp32 [C L, D] as the backward wrote it -> out fp32
 *   [C (1 + n_ctx), D]: row 1 + j of class c is the row of prompt c that holds context vector j, row 0 is zeros.  clipmi_ctx_step,
 *   clipmi_ctx_step_scaled and clipmi_prograd_step then run on `out` unchanged with L = 1 + n_ctx.  One launch, plain copies, no atomics.
 * Both: CLIPMI_ERR_ARG for a null pointer or a position outside {0, 1, 2}; CLIPMI_ERR_SHAPE for C < 1, n_ctx < 1, 2 + n_ctx > L, L > Lc
 *   or D % 4 != 0.
 *
 * clipmi_prompt_train_step_placed, clipmi_prompt_train_step_scaled_placed: clipmi_prompt_train_step and clipmi_prompt_train_step_scaled
 *   with clipmi_prompt_place in front of the tower's forward (which then takes ctx = NULL) and clipmi_prompt_unplace (twice for ProGrad,
 *   behind the second backward) in front of the step, enqueued in this order on `stream` -- the same launches, the same bits as the calls
 *   one by one.  Arguments as those steps' plus position and name_lens; prompts is the base.  Every argument check is made before the first
 *   launch.  workspace of the `_bytes` function's size (256-byte aligned; 0 for arguments the call refuses).
 * ---------------------------------------------------------------------------------------------------- */
int clipmi_prompt_place(const void* base, int dtype, const float* ctx, int per_class, int position, const int32_t* name_lens, float* prompts,
                        int C, int L, int Lc, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_prompt_unplace(const float* d_embed, int position, const int32_t* name_lens, float* out, int C, int L, int D, int n_ctx,
                          clipmi_stream_t stream);
size_t clipmi_prompt_train_step_placed_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx,
                                             int ctx_per_class);
int clipmi_prompt_train_step_placed(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx, float* buf,
                                    int n_ctx, int ctx_per_class, int position, const int32_t* name_lens, const int32_t* eot, int n_prompts,
                                    int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale,
                                    float grad_scale, int mode, const float* teacher, float w, float T, float lambda, const float* lr,
                                    int first_step, float momentum, float dampening, float weight_decay, int nesterov, float* losses,
                                    float* grad_out, int* projected, double* dots, void* workspace, size_t workspace_bytes, void* stash,
                                    size_t stash_bytes, clipmi_stream_t stream);
size_t clipmi_prompt_train_step_scaled_placed_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int mode, int n_ctx,
                                                    int ctx_per_class);
int clipmi_prompt_train_step_scaled_placed(clipmi_model* m, const clipmi_text_dgrad* wt, const void* prompts, int dtype, float* ctx,
                                           float* buf, int n_ctx, int ctx_per_class, int position, const int32_t* name_lens,
                                           const int32_t* eot, int n_prompts, int seq_rows, const float* feats, int64_t ld,
                                           const int64_t* labels, int B, float scale, clipmi_scaler_state* state, float growth_factor,
                                           float backoff_factor, int growth_interval, int mode, const float* teacher, float w,
                                           const float* lr, float momentum, float dampening, float weight_decay, int nesterov,
                                           float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* stash,
                                           size_t stash_bytes, clipmi_stream_t stream);

/* The scaler's rule for the fits whose parameters are ONE fp32 master block stepped element by element (CoCoOp, VPT, MaPLe, PromptSRC and
 * IVLP; DESIGN.md "Dynamic loss scale for the block fits").  grad fp32 [total] is scale * the gradient of the block: what the fit's own
 * gradient-forming launches leave at grad_scale = 1 once the head's outputs have been multiplied by the block's scale
 * (clipmi_grad_scale_rows).  Three launches:
 *   one thread per element, workgroups of 256: g = grad[i] * (1 / state->scale) into the workspace and into grad_out (may be NULL; may be
 *     grad itself), and one integer flag per workgroup, set when any g of the workgroup is an inf or a NaN;
 *   clipmi_ctx_step_scaled's second launch: one workgroup ORs the flags, writes the decision and updates the state block by its rule;
 *   clipmi_ctx_step_scaled's third launch: clipmi_ctx_step's SGD rule on params and buf with the unscaled gradient, only on a clean step.
 * A skipped step writes neither params nor buf; the momentum buffer starts from the gradient of the first APPLIED step; there is no
 * first_step argument.  No atomics, no workgroup reads what another of the same launch writes, the same inputs give the same bits.  With
 * the flags clear params, buf and grad_out equal a static step at grad_scale = scale and first_step = (applied_steps == 0) bit for bit.
 * workspace (256-byte aligned): clipmi_block_step_scaled_workspace_bytes(total) bytes, 0 for a total the call refuses.  Every check
 * precedes the first launch.  CLIPMI_ERR_ARG: a null pointer (grad, params, lr, state, the workspace; buf with a momentum), a pointer that
 * is not 4-byte aligned, a factor that is not finite or not positive, growth_interval < 1, SGD's own refusals; CLIPMI_ERR_SHAPE: total < 1
 * or total >= 2^39; CLIPMI_ERR_WORKSPACE. */
size_t clipmi_block_step_scaled_workspace_bytes(int64_t total);
int clipmi_block_step_scaled(const float* grad, float* params, float* buf, float* grad_out, int64_t total, clipmi_scaler_state* state,
                             float growth_factor, float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening,
                             float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* torch.optim.Adam's and torch.optim.AdamW's step (no amsgrad) on ONE fp32 master block, for the prompt fits: their own launches form the
 * block's gradient without applying it (apply = 0 / grad_out) and one of these two calls applies it (csrc/optim_step.hip, DESIGN.md "Adam
 * steps for the prompt fits").  Additive exports: the ABI version stays.
 *   grad [total]        grad_scale * gradient (clipmi_block_step_adam) or state->scale * gradient (the _scaled call); g = grad * (1 / scale)
 *   params, exp_avg, exp_avg_sq [total]   the master block and Adam's two moments (zero before the first step), updated in place
 *   grad_out [total]    optional (NULL): receives g; may be grad itself
 *   lr                  the step's rate, fp32 [1] on the device
 *   bias_table          float64 [table_len, 2] on the device, 8-byte aligned: row t - 1 holds 1 - beta1^t and sqrt(1 - beta2^t) as the host
 *                       forms them in double for Adam's step number t = 1 .. table_len; the kernels index it and call no pow
 *   decoupled           0: Adam (g += weight_decay w, then the rule); != 0: AdamW (w *= 1 - lr weight_decay, then the rule without weight decay)
 * clipmi_block_step_adam is ONE launch, one thread per element, at the caller's step number t (1 on the first step).
 * clipmi_block_step_adam_scaled is three launches: clipmi_block_step_scaled's first two (unscale and flag; decide and update the state
 * block) and the rule on a clean step alone, at t = state->applied_steps as the second launch has just left it (this step counted).  A
 * skipped step writes none of params, exp_avg, exp_avg_sq and does not advance t; the caller keeps table_len >= the steps it has enqueued
 * (an upper bound of the applied ones; a t behind the table writes nothing).  With the flags clear the scaled call's bits are the static
 * call's at grad_scale = scale and t = applied_steps.  No atomics, integer flags, the same inputs give the same bits.  workspace (256-byte
 * aligned): clipmi_block_step_adam_scaled_workspace_bytes(total) bytes, 0 for a total the call refuses.  Every check precedes the first
 * launch.  CLIPMI_ERR_ARG: a null pointer (grad, params, exp_avg, exp_avg_sq, lr, bias_table; state and the workspace), a pointer that is
 * not aligned, table_len < 1, t < 1, t > table_len, a beta outside [0, 1), eps not finite or <= 0, weight_decay negative or not finite,
 * grad_scale not finite or <= 0, the scaler's own refusals; CLIPMI_ERR_SHAPE: total < 1 or total >= 2^39; CLIPMI_ERR_WORKSPACE. */
int clipmi_block_step_adam(const float* grad, float* params, float* exp_avg, float* exp_avg_sq, float* grad_out, int64_t total, float grad_scale,
                           const float* lr, int64_t t, const double* bias_table, int64_t table_len, double beta1, double beta2, double eps,
                           float weight_decay, int decoupled, clipmi_stream_t stream);
size_t clipmi_block_step_adam_scaled_workspace_bytes(int64_t total);
int clipmi_block_step_adam_scaled(const float* grad, float* params, float* exp_avg, float* exp_avg_sq, float* grad_out, int64_t total,
                                  clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr,
                                  const double* bias_table, int64_t table_len, double beta1, double beta2, double eps, float weight_decay,
                                  int decoupled, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* The four one-call steps under the scaler.  Each is its static call with `state` and the scaler's three arguments in grad_scale's place
 * and without first_step (the state block knows the first applied step), and enqueues, in order: the static call's launches up to the
 * head, the head at grad_scale = 1, clipmi_grad_scale_rows on every fp32 gradient the head hands to a backward (d_text for CoCoOp; d_feats
 * for VPT; d_text and d_feats for MaPLe and PromptSRC -- before anything rounds them to fp16), the backward(s), the fit's gradient
 * formation at grad_scale = 1 without applying (clipmi_cocoop_reduce; VPT's d_prompts as they are; clipmi_maple_step and
 * clipmi_promptsrc_step with apply = 0) and clipmi_block_step_scaled on the block.  grad_out (may be NULL) receives the unscaled gradient.
 * The same launches, the same bits as the calls one by one; with a scale that never changes, the static call's bits at that scale.  The
 * scaler's and the optimiser's refusals precede the first launch.  workspace: the static call's, then (MaPLe, PromptSRC) the block of
 * scale * gradient, then clipmi_block_step_scaled's -- the matching _scaled_bytes function, 0 for arguments the call refuses (VPT's and
 * PromptSRC's take the image prompt depth as well: the block's size depends on it). */
size_t clipmi_cocoop_train_step_scaled_bytes(const clipmi_model* m, int C, int seq_rows, int B, int H, int n_ctx);
int clipmi_cocoop_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, int dtype, float* params, float* buf,
                                    int n_ctx, int H, const int32_t* cls_eot, int C, int seq_rows, const float* feats, int64_t ld,
                                    const int64_t* labels, int B, float scale, clipmi_scaler_state* state, float growth_factor,
                                    float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening,
                                    float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes,
                                    void* stash, size_t stash_bytes, clipmi_stream_t stream);
size_t clipmi_vpt_train_step_scaled_bytes(const clipmi_model* m, int B, int n_ctx, int depth, int C);
int clipmi_vpt_train_step_scaled(clipmi_model* m, const clipmi_vision_dgrad* wt, const void* image, int image_dtype, int B, float* prompts,
                                 float* buf, int n_ctx, int depth, const float* text, int C, const int64_t* labels, float scale,
                                 clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr,
                                 float momentum, float dampening, float weight_decay, int nesterov, float* loss, float* grad_out,
                                 void* workspace, size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream);
size_t clipmi_maple_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int n_ctx, int depth);
int clipmi_maple_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts, int dtype,
                                   const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B,
                                   const int64_t* labels, float* block, float* buf, int n_ctx, int depth, float scale,
                                   clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval, const float* lr,
                                   float momentum, float dampening, float weight_decay, int nesterov, float* loss, float* grad_out,
                                   void* workspace, size_t workspace_bytes, void* text_stash, size_t text_stash_bytes, void* vision_stash,
                                   size_t vision_stash_bytes, clipmi_stream_t stream);
size_t clipmi_promptsrc_train_step_scaled_bytes(const clipmi_model* m, int n_prompts, int seq_rows, int B, int nt, int dt, int nv, int dv);
int clipmi_promptsrc_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const clipmi_vision_dgrad* wv, const void* prompts,
                                       int dtype, const int32_t* eot, int n_prompts, int seq_rows, const void* image, int image_dtype, int B,
                                       const int64_t* labels, const float* teacher, float* block, float* buf, int nt, int dt, int nv, int dv,
                                       float scale, clipmi_scaler_state* state, float growth_factor, float backoff_factor, int growth_interval,
                                       float w_text, float w_image, float w_logit, const float* lr, float momentum, float dampening,
                                       float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace,
                                       size_t workspace_bytes, void* text_stash, size_t text_stash_bytes, void* vision_stash,
                                       size_t vision_stash_bytes, clipmi_stream_t stream);

/* ProDA's collection of contexts trained on the same frozen-tower backward (reference trainers/classification/proda.py:146-228, 258-304;
 * csrc/proda_train.hip, DESIGN.md "ProDA fit").  ctx fp32 [P, n_ctx, D] is the master of all P contexts; pos int32 [P] gives each one's
 * class-token position (0 front, 1 middle, 2 end); a step uses the Pb contexts sel int32 [Pb] names, the caller having put them into
 * the reference's end | middle | front order; name_lens int32 [C] is every class's name length in tokens.  sel, pos and name_lens live
 * on the device.  N = C Pb + P prompts go through the tower: prompt c Pb + q is class c with context sel[q], prompt C Pb + p the
 * no-class prompt [SOS | ctx_p | '.' EOT] of context p.  These exports are additive: the ABI version does not change with them.
 *
 * clipmi_proda_embed: the N prompts as fp32 embeddings [N, Lc, D] (rows [0, L) of each written, L <= Lc the live rows; the positional
 *   embedding is the tower's to add) and their EOT indices int32 [N] (cls_eot[c], int32 [C] on the device, for every prompt of class c,
 *   whatever its position and name length -- the reference takes it from the token ids; n_ctx + 2 for a no-class prompt).  base
 *   [C, Lc, D] and nc_base [1, Lc, D] (dtype: CLIPMI_F16 or CLIPMI_F32) are the token embeddings of "X .. X name ." and of "X .. X .".
 *   With nl the name length and h = n_ctx / 2, context vector j sits on row 1 + j (end), 1 + nl + j (front), or 1 + j for j < h and
 *   1 + nl + j otherwise (middle); the name tokens take the rows left free in [1, 1 + n_ctx + nl); every other row is the base's.  A
 *   context row is copied from the fp32 master unchanged.  A name length is read clamped to [0, L - 3 - n_ctx] and a selection outside
 *   [0, P) poisons its prompts with NaN: neither is used as an address.  One launch.  16-byte aligned pointers, D a multiple of 4.
 *   The tower then runs on it unchanged: clipmi_text_encoder_train(m, prompts, CLIPMI_F32, NULL, 0, 0, eot, N, seq_rows, ...).
 *
 * clipmi_proda_head: text fp32 [N, E] the tower's raw features.  x_b = unit(feats_b), u_{c,q} = unit(text_{c Pb + q}), m_c = mean_q u_{c,q},
 *   v = u - m, s = scale, n_p = unit(text_{C Pb + p}):
 *     z[b,c] = s x_b . m_c + 0.5 s^2 / (Pb + 1) sum_q sum_e x_be^2 (v_{y_b,q,e} - v_{c,q,e})^2;   upper = CE(z, y);
 *     m = mean_{p != q} |n_p . n_q| over all P contexts;   losses fp32 [3] = {upper + alpha m, upper, m}
 *   (upper the float64 mean of the fp32 row losses, m a float64 mean in a fixed order, the total in fp32).  d_text fp32 [N, E] =
 *   grad_scale d total / d text, ready for clipmi_text_encoder_backward.  The [E, C, C] covariance of the reference is never formed.
 *   A label outside [0, C) makes upper, the total and the class rows of d_text NaN and is never used as an address.  alpha finite, >= 0;
 *   alpha == 0 leaves exact zeros in the no-class rows of d_text.  Seven launches, no float atomics, fixed summation orders.  workspace
 *   (8-byte aligned): clipmi_proda_head_workspace_bytes(B, E, C, Pb, P) bytes (0 for a bad argument).
 *
 * clipmi_proda_ctx_step: d_embed fp32 [N L, D] as the backward wrote it.  The gradient of ctx[p, j, :] is, if p == sel[q], the sum over
 *   c = 0 .. C-1 (ascending) of the row of prompt c Pb + q that holds context vector j, plus -- always, and last -- row 1 + j of the
 *   no-class prompt C Pb + p; times 1 / grad_scale.  Then clipmi_ctx_step's SGD rule with the same arguments; grad_out (ctx's shape, may
 *   be NULL) receives the gradient; ctx == NULL: only grad_out is written.  One launch, no atomics.
 *
 * clipmi_proda_train_step: the three above around clipmi_text_encoder_train and clipmi_text_encoder_backward as ONE call on `stream`
 *   -- the same launches, the same bits as the calls one by one.  workspace of clipmi_proda_train_step_bytes(...) bytes (256-byte
 *   aligned), stash as clipmi_text_train_bytes(m, C Pb + P, seq_rows, ...) reports it.  At most 80 live rows (the backward's limit).
 *   Every argument check of the five stages is made before the first launch: a refused call enqueues nothing.
 *
 * clipmi_proda_ctx_step_scaled: clipmi_proda_ctx_step under the scaler's rule (DESIGN.md "Dynamic loss scale for ProDA"), with `state` and
 *   the scaler's three arguments in grad_scale's place, no first_step and a workspace.  Three launches, in clipmi_ctx_step_scaled's shape:
 *     one thread per element of ctx, workgroups of 256: clipmi_proda_ctx_step's sum in its order (c ascending where p == sel[q], the
 *       no-class row last) times 1 / state->scale, read on the device, into the workspace and into grad_out (may be NULL), and one integer
 *       flag per workgroup, set when any element the workgroup produced is an inf or a NaN.  Every context takes part: of one outside the
 *       selection the no-class row is looked at.  A row of d_embed that holds no context vector is not read;
 *     clipmi_ctx_step_scaled's second launch: one workgroup ORs the flags, writes the decision and updates the state block by its rule;
 *     clipmi_ctx_step_scaled's third launch: the SGD rule on ctx and buf over all P n_ctx D elements, only on a clean step; the momentum
 *       buffer starts from the first APPLIED step (state->applied_steps == 0).
 *   No atomics, no workgroup reads what another of the same launch writes, the same inputs give the same bits.  With the flags clear ctx,
 *   buf and grad_out equal clipmi_proda_ctx_step's at grad_scale = scale and first_step = (applied_steps == 0) bit for bit.  A selection
 *   outside [0, P) and a name length are read as there and are never an address.  ctx, lr, state and the workspace are required.
 *   workspace (256-byte aligned): clipmi_proda_ctx_step_scaled_workspace_bytes(P, D, n_ctx) bytes, 0 for arguments the call refuses.
 *   Every check precedes the first launch.  CLIPMI_ERR_ARG: a null pointer, a factor that is not finite or not positive,
 *   growth_interval < 1, SGD's own refusals; CLIPMI_ERR_SHAPE: clipmi_proda_ctx_step's; CLIPMI_ERR_WORKSPACE.
 *
 * clipmi_proda_train_step_scaled: one step under the scaler as ONE call: clipmi_proda_embed, clipmi_text_encoder_train, clipmi_proda_head
 *   at grad_scale = 1, clipmi_grad_scale_rows on its d_text (before anything rounds it to fp16), clipmi_text_encoder_backward and
 *   clipmi_proda_ctx_step_scaled, enqueued in this order on `stream` -- the same launches, the same bits as the calls one by one; with a
 *   scale that never changes, clipmi_proda_train_step's bits at that scale.  Arguments as clipmi_proda_train_step's.  Every stage's checks
 *   precede the first launch.  workspace of clipmi_proda_train_step_scaled_bytes(...) bytes (256-byte aligned; 0 for arguments the call
 *   refuses): clipmi_proda_train_step's, then the scaled step's. */
int clipmi_proda_embed(const void* base, const void* nc_base, int dtype, const float* ctx, const int32_t* sel, const int32_t* pos,
                       const int32_t* name_lens, const int32_t* cls_eot, float* prompts, int32_t* eot, int C, int Pb, int P, int L, int Lc, int D, int n_ctx,
                       clipmi_stream_t stream);
size_t clipmi_proda_head_workspace_bytes(int B, int E, int C, int Pb, int P);
int clipmi_proda_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, int Pb, int P,
                      float scale, float grad_scale, float alpha, float* losses, float* d_text, void* workspace, size_t workspace_bytes,
                      clipmi_stream_t stream);
int clipmi_proda_ctx_step(const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos,
                          const int32_t* name_lens, int C, int Pb, int P, int L, int D, int n_ctx, float grad_scale, const float* lr,
                          int first_step, float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream);
size_t clipmi_proda_train_step_bytes(const clipmi_model* m, int C, int Pb, int P, int seq_rows, int B);
int clipmi_proda_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, const void* nc_base, int dtype, float* ctx,
                            float* buf, int n_ctx, const int32_t* sel, const int32_t* pos, const int32_t* name_lens, const int32_t* cls_eot, int C, int Pb,
                            int P, int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B, float scale, float grad_scale,
                            float alpha, const float* lr, int first_step, float momentum, float dampening, float weight_decay,
                            int nesterov, float* losses, float* grad_out, void* workspace, size_t workspace_bytes, void* stash,
                            size_t stash_bytes, clipmi_stream_t stream);
size_t clipmi_proda_ctx_step_scaled_workspace_bytes(int P, int D, int n_ctx);
int clipmi_proda_ctx_step_scaled(const float* d_embed, float* ctx, float* buf, float* grad_out, const int32_t* sel, const int32_t* pos,
                                 const int32_t* name_lens, int C, int Pb, int P, int L, int D, int n_ctx, clipmi_scaler_state* state,
                                 float growth_factor, float backoff_factor, int growth_interval, const float* lr, float momentum, float dampening,
                                 float weight_decay, int nesterov, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
size_t clipmi_proda_train_step_scaled_bytes(const clipmi_model* m, int C, int Pb, int P, int seq_rows, int B, int n_ctx);
int clipmi_proda_train_step_scaled(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, const void* nc_base, int dtype, float* ctx,
                                   float* buf, int n_ctx, const int32_t* sel, const int32_t* pos, const int32_t* name_lens,
                                   const int32_t* cls_eot, int C, int Pb, int P, int seq_rows, const float* feats, int64_t ld,
                                   const int64_t* labels, int B, float scale, clipmi_scaler_state* state, float growth_factor,
                                   float backoff_factor, int growth_interval, float alpha, const float* lr, float momentum, float dampening,
                                   float weight_decay, int nesterov, float* losses, float* grad_out, void* workspace, size_t workspace_bytes,
                                   void* stash, size_t stash_bytes, clipmi_stream_t stream);

/* The class-sharded ProDA fit (DESIGN.md "Class-sharded ProDA fit"): G ranks, rank r owning the contiguous classes [c_lo, c_hi) of the
 * balanced split of C (the first C mod G ranks one more, C >= G) with all Pb prompts of each, and the no-class prompts of the contexts
 * [p_lo, p_hi) the same split of P gives it (P >= G): C_r Pb + P_r prompts, the class prompts first.  Two all-gathers per step.  fp32, fixed
 * summation orders, no atomics; with G = 1 every chain is clipmi_proda_ctx_step's (clipmi_proda_ctx_step_scaled's), bit for bit.  These
 * exports are additive: the ABI version does not change with them.
 *
 * clipmi_proda_embed_shard: clipmi_proda_embed for one rank.  base, name_lens and cls_eot start at the rank's first class and C is the
 *   number of its classes (>= 1); ctx [P, n_ctx, D], sel and pos are the whole collection's; the no-class prompts written are those of the
 *   contexts p0 .. p0 + Pn - 1.  prompts [C Pb + Pn, Lc, D], eot [C Pb + Pn].  With C the whole class set, p0 = 0 and Pn = P it is
 *   clipmi_proda_embed.
 * clipmi_proda_shard_compact: gathered fp32 [G, RB, E], RB = ceil(C / G) Pb + ceil(P / G), block r holding rank r's tower output as it lies
 *   -- C_r Pb class rows, then P_r no-class rows -- and padding behind them that is never read; out fp32 [C Pb + P, E] in the unsharded
 *   order clipmi_proda_head takes.  One launch.
 * clipmi_proda_ctx_partial: a rank's send block, fp32 [(Pb + Pn), n_ctx, D], from its own d_embed fp32 [(C Pb + Pn) L, D] (C, Pn, name_lens:
 *   the rank's own).  Slot q < Pb: for context vector j of context sel[q] the sum over the rank's classes c = 0 .. C-1 (ascending, from
 *   0) of the row of prompt c Pb + q that holds it (clipmi_proda_embed's row rule), unscaled; a selection outside [0, P) gives zeros and
 *   is never an index.  Slot Pb + i: row 1 + j of the rank's i-th no-class prompt, copied.  Ranks pad the block to (Pb + ceil(P / G))
 *   n_ctx D floats -- 4 (Pb + ceil(P / G)) n_ctx D bytes per rank and gather.  One launch; 16-byte accesses when D is a multiple of 4 and
 *   both pointers are 16-byte aligned, scalar ones otherwise.
 * clipmi_proda_ctx_step_gathered: the gathered send blocks, rank r's at gathered + r * rank_stride (elements, >= (Pb + ceil(P / G))
 *   n_ctx D).  The gradient of ctx[p, j, d]: if p == sel[q], the G class sums of slot q added in RANK order from 0; then -- always, and
 *   last -- the no-class row of the rank that owns p; times 1 / grad_scale.  Then clipmi_proda_ctx_step's SGD rule with the same optional
 *   outputs and NULL conventions.  The padding of a block is never read.  Every rank given the same blocks writes the same bits.  One
 *   launch, one thread per four elements when n_ctx D and rank_stride are multiples of 4 and every pointer is 16-byte aligned (a block of
 *   n_ctx D floats that is no multiple of 4 floats puts the streams on different 16-byte phases), per element otherwise.
 * clipmi_proda_ctx_reduce_gathered_scaled: the same sum under the scaler's rule, as clipmi_proda_ctx_step_scaled is
 *   clipmi_proda_ctx_step's: one thread per element, workgroups of 256, times 1 / state->scale into the workspace and grad_out with one
 *   integer flag per workgroup; clipmi_ctx_step_scaled's second and third launches follow unchanged.  Every rank reduces the same
 *   gathered bytes, so every rank takes the same decision and holds the same state block.  workspace (256-byte aligned):
 *   clipmi_proda_ctx_step_scaled_workspace_bytes(P, D, n_ctx) bytes.  Every check precedes the first launch. */
int clipmi_proda_embed_shard(const void* base, const void* nc_base, int dtype, const float* ctx, const int32_t* sel, const int32_t* pos,
                             const int32_t* name_lens, const int32_t* cls_eot, float* prompts, int32_t* eot, int C, int Pb, int P, int p0, int Pn,
                             int L, int Lc, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_proda_shard_compact(const float* gathered, float* out, int C, int Pb, int P, int G, int64_t E, clipmi_stream_t stream);
int clipmi_proda_ctx_partial(const float* d_embed, float* partial, const int32_t* sel, const int32_t* pos, const int32_t* name_lens, int C,
                             int Pb, int P, int Pn, int L, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_proda_ctx_step_gathered(const float* gathered, int G, int64_t rank_stride, float* ctx, float* buf, float* grad_out,
                                   const int32_t* sel, int Pb, int P, int D, int n_ctx, float grad_scale, const float* lr, int first_step,
                                   float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream);
int clipmi_proda_ctx_reduce_gathered_scaled(const float* gathered, int G, int64_t rank_stride, float* ctx, float* buf, float* grad_out,
                                            const int32_t* sel, int Pb, int P, int D, int n_ctx, clipmi_scaler_state* state,
                                            float growth_factor, float backoff_factor, int growth_interval, const float* lr, float momentum,
                                            float dampening, float weight_decay, int nesterov, void* workspace, size_t workspace_bytes,
                                            clipmi_stream_t stream);

/* CoCoOp's context and meta-net trained on the same frozen-tower backward (reference trainers/classification/cocoop.py:153-202, 259-278;
 * csrc/cocoop_train.hip, DESIGN.md "CoCoOp fit").  The five learned tensors live in ONE fp32 block of clipmi_cocoop_block_floats(n_ctx, D,
 * E, H) floats laid out as ctx [n_ctx, D] | W1 [H, E] | b1 [H] | W2 [D, H] | b2 [D] (D the text width, E the embedding width, H the
 * meta-net's hidden width, 1 <= H <= 4096; the reference uses E / 16, which is not required); the momentum block and the gradient block
 * have the same layout.  N = B C prompts go through the tower: prompt b C + c is image b with class c.  These exports are additive: the
 * ABI version does not change with them.
 *
 * clipmi_cocoop_meta: x_b = feats_b / |feats_b| (feats fp32 [B, E] with the row stride ld), hid_b = max(W1 x_b + b1, 0), pi_b = W2 hid_b
 *   + b2 -> x_n fp32 [B, E], hid fp32 [B, H], pi fp32 [B, D].  One workgroup per image, fixed-order sums.  One launch.
 * clipmi_cocoop_embed: the N prompts as fp32 embeddings [N, Lc, D] (rows [0, L) of each written, L <= Lc the live rows; the positional
 *   embedding is the tower's to add) and their EOT indices int32 [N] = cls_eot[c] (int32 [C] on the device).  Row 1 + j (j < n_ctx) is the
 *   single fp32 addition ctx[j] + pi[b]; every other row is base [C, Lc, D] (dtype: CLIPMI_F16 or CLIPMI_F32) widened.  One launch.
 *   16-byte aligned base, ctx, pi and prompts, D a multiple of 4, 1 + n_ctx <= L, B C Lc < 2^31.  The tower then runs on it unchanged:
 *   clipmi_text_encoder_train(m, prompts, CLIPMI_F32, NULL, 0, 0, eot, N, seq_rows, ...).
 * clipmi_cocoop_head: text fp32 [N, E] the tower's raw features, u_n = unit(text_n): z[b, c] = scale x_b . u_{b C + c};
 *   loss fp32 [1] = the float64 mean of the fp32 row losses CE(z[b, :], labels[b]) (row_losses fp32 [B], may be NULL, receives them);
 *   d_text fp32 [N, E] = grad_scale d loss / d text: with dz = grad_scale (softmax(z) - onehot) / B and v = scale dz[b, c] x_b,
 *   d_text_n = (v - u_n (u_n . v)) / |text_n| -- no sum over the images, every pair has its own text row.  A label outside [0, C) makes
 *   that image's row loss, its d_text rows and the batch loss NaN and is never used as an address; the other images' rows stay finite.
 *   Four launches, no float atomics.  workspace (8-byte aligned): clipmi_cocoop_head_workspace_bytes(B, C) bytes (0 for a bad argument).
 * clipmi_cocoop_reduce: d_embed fp32 [N L, D] as the backward wrote it -> the gradient block `grad`:
 *     dcs[b, j] = (1 / grad_scale) sum_c d_embed[(b C + c) L + 1 + j] (c ascending; the only place 1 / grad_scale is applied);
 *     dctx[j] = sum_b dcs[b, j];  dpi[b] = sum_j dcs[b, j];  db2 = sum_b dpi[b];  dW2[d, h] = sum_b dpi[b, d] hid[b, h];
 *     dhid[b, h] = [hid[b, h] > 0] sum_d W2[d, h] dpi[b, d];  db1 = sum_b dhid[b];  dW1[h, e] = sum_b dhid[b, h] x_n[b, e]
 *   (b and j ascending).  x_n, hid as clipmi_cocoop_meta wrote them, w2 fp32 [D, H].  No gradient with respect to x_n is formed: the
 *   image tower is frozen.  Four launches, no float atomics.  workspace: clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H) bytes.
 * clipmi_cocoop_step: torch.optim.SGD's rule as clipmi_ctx_step applies it, over every element of the parameter block `params` with the
 *   gradient block `grad` and the momentum block `buf` (required with a momentum): one set of hyper-parameters for the five tensors, weight
 *   decay on the biases too, as the reference's single optimiser has it.  lr fp32 [1] on the device.  One launch.
 * clipmi_cocoop_train_step: all of the above around clipmi_text_encoder_train and clipmi_text_encoder_backward as ONE call on `stream`
 *   -- the same launches, the same bits as the calls one by one.  workspace of clipmi_cocoop_train_step_bytes(m, C, seq_rows, B, H, n_ctx)
 *   bytes (256-byte aligned; 0 for arguments the call refuses), stash as clipmi_text_train_bytes(m, B C, seq_rows, ...) reports it.
 *   grad_out (may be NULL): the gradient block is formed there instead of in the workspace.  At most 80 live rows (the backward's
 *   limit).  Every argument check of the seven stages is made before the first launch: a refused call enqueues nothing. */
size_t clipmi_cocoop_block_floats(int n_ctx, int D, int E, int H);
int clipmi_cocoop_meta(const float* feats, int64_t ld, const float* w1, const float* b1, const float* w2, const float* b2, float* x_n, float* hid,
                       float* pi, int B, int E, int H, int D, clipmi_stream_t stream);
int clipmi_cocoop_embed(const void* base, int dtype, const float* ctx, const float* pi, const int32_t* cls_eot, float* prompts, int32_t* eot,
                        int B, int C, int L, int Lc, int D, int n_ctx, clipmi_stream_t stream);
size_t clipmi_cocoop_head_workspace_bytes(int B, int C);
int clipmi_cocoop_head(const float* feats, int64_t ld, const int64_t* labels, const float* text, int B, int E, int C, float scale,
                       float grad_scale, float* loss, float* row_losses, float* d_text, void* workspace, size_t workspace_bytes,
                       clipmi_stream_t stream);
size_t clipmi_cocoop_reduce_workspace_bytes(int B, int n_ctx, int D, int H);
int clipmi_cocoop_reduce(const float* d_embed, const float* x_n, const float* hid, const float* w2, float* grad, int B, int C, int L, int D,
                         int E, int H, int n_ctx, float grad_scale, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
int clipmi_cocoop_step(const float* grad, float* params, float* buf, int n_ctx, int D, int E, int H, const float* lr, int first_step,
                       float momentum, float dampening, float weight_decay, int nesterov, clipmi_stream_t stream);
size_t clipmi_cocoop_train_step_bytes(const clipmi_model* m, int C, int seq_rows, int B, int H, int n_ctx);
int clipmi_cocoop_train_step(clipmi_model* m, const clipmi_text_dgrad* wt, const void* base, int dtype, float* params, float* buf, int n_ctx,
                             int H, const int32_t* cls_eot, int C, int seq_rows, const float* feats, int64_t ld, const int64_t* labels, int B,
                             float scale, float grad_scale, const float* lr, int first_step, float momentum, float dampening,
                             float weight_decay, int nesterov, float* loss, float* grad_out, void* workspace, size_t workspace_bytes,
                             void* stash, size_t stash_bytes, clipmi_stream_t stream);

/* The class-sharded CoCoOp fit (DESIGN.md "Class-sharded CoCoOp fit"): G ranks, rank r owning the contiguous classes [lo, hi) of the
 * balanced split of C (the first C mod G ranks one more, C >= G), C_r = hi - lo of them.  Its tower runs over the B C_r prompts of its
 * classes, image-major: prompt b C_r + (c - lo) is image b with class c.  Two all-gathers per step; the meta-net, the head, the
 * meta-net's backward and the optimiser step run replicated.  fp32, fixed summation orders, no atomics; with G = 1 every chain is the
 * unsharded call's, bit for bit.  These exports are additive: the ABI version does not change with them.
 *
 * clipmi_cocoop_embed_classes: clipmi_cocoop_embed for the classes [lo, hi) of C (one class is enough): base [C, Lc, D] and cls_eot [C]
 *   are the whole class set's, prompts [B C_r, Lc, D] and eot [B C_r] the rank's.  The same kernel: the output is the slice [:, lo:hi] of
 *   clipmi_cocoop_embed's [B, C, Lc, D].  base + lo Lc D elements must be 16-byte aligned.
 * clipmi_cocoop_shard_compact: gathered fp32, rank r's block at gathered + r rank_stride (elements, >= B ceil(C / G) E) holding its tower's
 *   [B, C_r, E] as it lies and padding behind it that is never read; out fp32 [B, C, E], the unsharded order clipmi_cocoop_head takes.
 * clipmi_cocoop_shard_rows: out fp32 [B, C_r, E] = d_text[:, lo:hi] of d_text fp32 [B, C, E]: what the rank's backward is given.
 * clipmi_cocoop_dcs_partial: a rank's send block fp32 [B, n_ctx, D] from its own d_embed fp32 [B C L, D] (C: its own classes, >= 1):
 *   partial[b, j] = sum_c d_embed[(b C + c) L + 1 + j], c ascending from 0, unscaled.
 * clipmi_cocoop_reduce_gathered: clipmi_cocoop_reduce from the gathered partials, rank r's at partials + r rank_stride (elements, >= B n_ctx
 *   D): dcs[b, j] = (1 / grad_scale) (sum_r partial_r[b, j]), r ascending from 0 and the one multiplication last; then
 *   clipmi_cocoop_reduce's three further launches unchanged.  Every rank given the same blocks writes the same bits.  workspace:
 *   clipmi_cocoop_reduce_workspace_bytes(B, n_ctx, D, H) bytes.  Every check precedes the first launch.
 * The three copies and the two sums run one thread per four elements when the row length (E, D; B n_ctx D for the reduce) and rank_stride
 *   are multiples of 4 and the pointers are 16-byte aligned, one thread per element otherwise.  One launch each (four for the reduce). */
int clipmi_cocoop_embed_classes(const void* base, int dtype, const float* ctx, const float* pi, const int32_t* cls_eot, float* prompts,
                                int32_t* eot, int B, int C, int lo, int hi, int L, int Lc, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_cocoop_shard_compact(const float* gathered, float* out, int B, int C, int G, int E, int64_t rank_stride, clipmi_stream_t stream);
int clipmi_cocoop_shard_rows(const float* d_text, float* out, int B, int C, int lo, int hi, int E, clipmi_stream_t stream);
int clipmi_cocoop_dcs_partial(const float* d_embed, float* partial, int B, int C, int L, int D, int n_ctx, clipmi_stream_t stream);
int clipmi_cocoop_reduce_gathered(const float* partials, int G, int64_t rank_stride, const float* x_n, const float* hid, const float* w2,
                                  float* grad, int B, int D, int E, int H, int n_ctx, float grad_scale, void* workspace,
                                  size_t workspace_bytes, clipmi_stream_t stream);

/* Timing aid for bench.py (the per-kernel roofline of its JSON line): the five launches of the vision tower's residual
 * block 0 -- 0 in-proj, 1 attention, 2 out-proj + residual, 3 c_fc + QuickGELU, 4 c_proj + residual (clip/model.py:181-188)
 * -- issued exactly as clipmi_encode_image issues them (LayerNorm fold, fp16 stream, tile selection) on the operands the
 * workspace holds (call clipmi_encode_image on `batch` images first), each `iters` times back to back after one untimed launch,
 * the `iters` launches bracketed by ONE pair of hipEvents on `stream` (the GPU stays under load for the whole measurement).
 * ms_out: host float[5], mean milliseconds per launch.  only = -1 times all five, 0..4 just that one (the others report 0).
 * Synchronises the stream; overwrites the activations in the workspace (the residual steps accumulate `iters` + 1 times). */
int clipmi_profile_block(clipmi_model* m, int batch, int iters, int only, void* workspace, size_t workspace_bytes,
                         float* ms_out, clipmi_stream_t stream);

/* Timing aid for bench.py (`roofline.kernels[].us_in_tower`): ONE real pass of clipmi_encode_image on `batch` images (no prompt hook;
 * the batch must be a single pass of the tower, option vision_pass) with a hipEvent recorded on `stream` behind every launch, so that
 * each kernel is timed IN PLACE -- behind its real predecessor, on operands that predecessor has just written -- instead of back to
 * back with itself as clipmi_profile_block does.  us_out (host float[n_us]) receives the microseconds between consecutive events:
 *   [0 .. *n_pre_out)                       the embedding launches in front of the first block (today: patch embedding, ln_pre)
 *   [*n_pre_out + 5 * layer + step]         step 0 in-proj, 1 attention, 2 out-proj, 3 c_fc, 4 c_proj of each residual block
 *   the last two                            ln_post on the class rows, the final projection
 * (an interval holds the kernel and the launch gap in front of it, so the entries add up to the pass).  Returns the number of
 * entries written (> 0) or a negative error code; synchronises the stream; `out` receives the features as usual. */
int clipmi_encode_image_timed(clipmi_model* m, const void* image, int image_dtype, int batch, float* out, void* workspace,
                              size_t workspace_bytes, unsigned flags, float* us_out, int n_us, int* n_pre_out, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Image preprocessing: the reference's test transform (clip/clip.py:74-81 `_transform`, Dassl's test transform with
 * INPUT.INTERPOLATION "bicubic" / "bilinear") for a ragged batch of decoded uint8 RGB images, on the device.
 * ---------------------------------------------------------------------------------------------------- */

/* One input image inside the caller's uint8 pixel buffer: byte (y, x, c) is pixels[offset + y*stride_y + x*stride_x + c*stride_c],
 * c = 0, 1, 2 = R, G, B (HWC: stride_x = 3, stride_c = 1; CHW: stride_x = 1, stride_c = height * width; strided views likewise). */
typedef struct {
  int64_t offset;
  int32_t height, width;
  int64_t stride_y, stride_x, stride_c;
} clipmi_image_desc;

enum { CLIPMI_FILTER_BILINEAR = 2, CLIPMI_FILTER_BICUBIC = 3 };   /* Pillow's Image.BILINEAR / Image.BICUBIC */

/* Device workspace clipmi_preprocess needs for these images (host descriptors): the descriptor copy plus the tap tables of the
 * cropped outputs (2 * B * n_px * kmax int32, kmax = Pillow's largest kernel size over the batch).  0 when an argument is bad. */
size_t clipmi_preprocess_workspace_bytes(const clipmi_image_desc* images, int B, int n_px, int filter);

/* Resize(n_px, filter) on the shorter side + CenterCrop(n_px) + ToTensor + Normalize of B uint8 RGB images of any sizes:
 *   1. torchvision's resize size: the shorter side becomes n_px, the longer int(n_px * long / short) (identity if it already is n_px);
 *   2. Pillow's Image.resize for 8-bit images (libImaging/Resample.c), bit-exact: horizontal pass then vertical, uint8 intermediate,
 *      taps in double normalised by their sum, PRECISION_BITS = 22 fixed point, int32 accumulation from 1 << 21, >> 22, clamp to 0..255;
 *      only the n_px x n_px outputs CenterCrop keeps are computed (top = round((new_h - n_px) / 2), half to even; left likewise);
 *   3. out[b, c, y, x] = table[c * 256 + u] for the resized byte u: `table` (device, fp32 [3][256]) is ToTensor + Normalize evaluated on
 *      the host, ((float)u / 255 - mean[c]) / std[c] in fp32 (an identity table u -> (float)u returns the resized bytes); fp16 output
 *      rounds the table's value to nearest even (what `image.type(self.dtype)` does in encode_image).
 * pixels: device uint8 buffer of pixels_bytes bytes; images: HOST descriptors, every field checked against pixels_bytes before anything
 * is launched (1 <= B <= 65535, 1 <= height, width <= 32768, 1 <= n_px <= 4096: CLIPMI_ERR_SHAPE; bad filter or dtype, null pointers,
 * a byte outside the buffer: CLIPMI_ERR_ARG).  The descriptors are copied into the workspace on `stream` (hipMemcpyAsync: page-locked
 * descriptors must stay unchanged until the stream has passed the call; pageable ones are staged by the runtime); no synchronisation.
 * out: [B, 3, n_px, n_px] contiguous, out_dtype CLIPMI_F16 or CLIPMI_F32.  workspace: 256-byte aligned, at least
 * clipmi_preprocess_workspace_bytes(images, B, n_px, filter) bytes; one workspace serves one call in flight.  Two launches. */
int clipmi_preprocess(const void* pixels, int64_t pixels_bytes, const clipmi_image_desc* images, int B, int n_px, int filter,
                      const float* table, void* out, int out_dtype, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * The reference's train transform (every training config: INPUT.TRANSFORMS random_resized_crop, random_flip, normalize) on the
 * device, the random draws left to the host: one VIEW is one output image, a box of one input image stretched to n_px x n_px.
 * ---------------------------------------------------------------------------------------------------- */

/* One view: the box rows top .. top + height - 1, columns left .. left + width - 1 of images[image]; flip != 0 mirrors the OUTPUT
 * left to right.  Several views may name the same image. */
typedef struct {
  int32_t image;
  int32_t top, left, height, width;
  int32_t flip;
} clipmi_view_desc;

/* Device workspace clipmi_augment needs for these images and views (host descriptors): both descriptor copies plus the tap tables
 * (2 * V * n_px * kmax int32, kmax = Pillow's largest kernel size over the views' box sides).  0 when an argument is bad. */
size_t clipmi_augment_workspace_bytes(const clipmi_image_desc* images, int B, const clipmi_view_desc* views, int V, int n_px, int filter);

/* torchvision's PIL path of RandomResizedCrop + RandomHorizontalFlip + ToTensor + Normalize for V given views of B uint8 RGB images:
 *   1. img.crop(box).resize((n_px, n_px), filter): Pillow's 8-bit resampler as in clipmi_preprocess, bit-exact, but as a STRETCH of the
 *      box -- on each axis the coefficients are computed with in_size = the box's side and out_size = n_px, so no tap reaches past the
 *      box edge and no pixel outside the box is read; a pass whose in and out sizes are equal is skipped, as Pillow skips it;
 *   2. transpose(FLIP_LEFT_RIGHT) of the resized image when the view's flip is set;
 *   3. out[v, c, y, x] = table[c * 256 + u], the table of clipmi_preprocess.
 * images and views are HOST descriptors; every field is checked before anything is launched: the image checks of clipmi_preprocess,
 * 1 <= V <= 65535 (CLIPMI_ERR_SHAPE), box sides >= 1 (CLIPMI_ERR_SHAPE), view.image in [0, B) and the box inside its image
 * (CLIPMI_ERR_ARG).  Both descriptor arrays are copied into the workspace on `stream` under clipmi_preprocess's rule for page-locked
 * memory; no synchronisation.  out: [V, 3, n_px, n_px] contiguous, out_dtype CLIPMI_F16 or CLIPMI_F32.  workspace: 256-byte aligned,
 * at least clipmi_augment_workspace_bytes(...) bytes; one workspace serves one call in flight.  Two launches. */
int clipmi_augment(const void* pixels, int64_t pixels_bytes, const clipmi_image_desc* images, int B, const clipmi_view_desc* views, int V,
                   int n_px, int filter, const float* table, void* out, int out_dtype, void* workspace, size_t workspace_bytes,
                   clipmi_stream_t stream);

/* Ceiling probe for bench.py (`ceiling.mfma_only`; not on any product path): a register-only loop of v_mfma_f32_16x16x32_f16 -- no LDS, no
 * memory inside the loop -- on one workgroup of `waves` waves (1..8: two per SIMD, 256 registers each) per CU, every wave holding two register-resident sets of 4 + 4
 * operand fragments loaded once from `operands` (fp16 [16][waves * 64][8]: whatever distribution the caller wants the matrix pipe to
 * multiply, e.g. N(0, 0.25^2) like the tower's operands) and issuing iters x 32 MFMAs (one operand held for four instructions, as the GEMM
 * loops do).  2 * 2 * 64 * 64 * 32 flop per wave and iteration.  `sink` (fp32 [CUs * waves * 64]) keeps the results live; `clocks` (NULL or
 * 2 x uint64) receives workgroup 0's elapsed shader cycles and 100 MHz ticks.  *n_cus_out (host, may be NULL) = workgroups launched. */
int clipmi_probe_mfma_f16(const void* operands, float* sink, unsigned long long* clocks, int waves, int iters, int* n_cus_out,
                          clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Fit monitor: per-epoch validation and best-epoch selection on the device (reference base_learner.py:41-47, Dassl's after_epoch;
 * csrc/fit_monitor.hip, DESIGN.md "Fit monitor").  Nothing is read back to the host.  Additive exports: the ABI version stays.
 *
 * The epoch record, 8-byte aligned, 16 + 16 (n_bins + 1) bytes, written by clipmi_val_score alone:
 *   {int32 n, int32 correct, float64 nll_sum, bins[n_bins + 1] x {int32 count, int32 hits, float64 conf_sum}}
 * bin b holds the rows whose confidence falls into bin b of numpy.digitize(conf, numpy.linspace(0, 1, n_bins + 1)) - 1, so the last
 * one, bin n_bins, holds conf == 1.0 (and a NaN confidence, which sorts behind every edge).
 *
 * clipmi_val_score: logits fp32 [N, C] with the row stride ld (elements), labels int64 [N].  Per row, in fp32: the maximum and its
 * LOWEST index, sum = sum_c exp(z_c - max), nll = log(sum) - (z[label] - max), conf = 1 / sum (lse - z[label] and exp(max - lse) with the
 * maximum cancelled before the rounding).  A label outside [0, C) is never used as an address: the row counts as wrong and its nll is NaN.  A row that
 * holds a NaN counts as wrong, its nll and its confidence are NaN.  Launch 1: one wave per row, 64 rows per workgroup -- the partition
 * depends on N alone --, whose results are added in ascending row order (int32 counts, float64 sums) into one partial record per workgroup;
 * launch 2: one workgroup adds the partial records in ascending workgroup order into `record`.  No atomics: the same inputs give the same
 * bits.  workspace (256-byte aligned): clipmi_val_score_workspace_bytes(N, n_bins) bytes, 0 for arguments the call refuses.  Every check
 * precedes the first launch.  CLIPMI_ERR_ARG: a null pointer, logits not 16-byte aligned, labels or the record not 8-byte aligned, n_bins
 * outside 1..64; CLIPMI_ERR_SHAPE: N < 1, C < 1, ld < C; CLIPMI_ERR_WORKSPACE.
 *
 * The best block, 8-byte aligned, 24 bytes: {int32 best_epoch, int32 best_correct, float64 best_nll_sum, int32 epochs_seen, int32 pad}.
 * The caller writes {-1, -1, +inf, 0, 0} before the first call; only clipmi_best_select writes it afterwards.
 *
 * clipmi_best_select: criterion 0 (accuracy): better iff record.correct > best_correct, so the first epoch is taken unconditionally;
 * criterion 1 (nll): better iff record.nll_sum is finite and < best_nll_sum, so a non-finite epoch is never taken.  Strictly better only
 * (Dassl's `>`): on a tie the earlier epoch stays.  Launch 1 (one workgroup) decides, on "better" writes epoch, correct and nll_sum into
 * the block, counts epochs_seen and writes the decision word into the workspace; launch 2 copies params to best_params (n_floats fp32,
 * both 16-byte aligned, exactly n_floats floats are written) and returns at once when the word says "not better".  workspace (256-byte
 * aligned): clipmi_best_select_workspace_bytes(n_floats), 0 for n_floats < 1.  CLIPMI_ERR_ARG: a null pointer, an alignment, a criterion
 * other than 0 or 1, epoch < 0; CLIPMI_ERR_SHAPE: n_floats < 1; CLIPMI_ERR_WORKSPACE.
 *
 * The row-chunked score, for validation sets whose [N, C] logits never exist in one piece (the image-tower fits).  The row result, 16 bytes,
 * 16-byte aligned: {float conf, float nll, int32 hit, int32 bin} -- what clipmi_val_score's first launch holds per row before it adds.
 *
 * clipmi_val_score_rows: `rows` rows of logits fp32 [rows, C] with the row stride ld against labels int64 [rows], one wave per row, the
 * per-row code of clipmi_val_score (the same device function); row r's result goes to row_results[r] and nothing else is written.  For a
 * chunk that starts at row row0 of the set the caller passes row_results + 16 row0 (bytes) and labels + row0.  No workspace.
 * CLIPMI_ERR_ARG: a null pointer, logits or row_results not 16-byte aligned, labels not 8-byte aligned, n_bins outside 1..64;
 * CLIPMI_ERR_SHAPE: rows < 1, C < 1, ld < C.
 *
 * clipmi_val_score_finish: the N row results into `record` in clipmi_val_score's order of additions -- launch 1: one partial record per 64
 * rows, thread 0 the head and thread 1 + b bin b, each over the rows in ascending order (int32 counts, float64 sums); launch 2:
 * clipmi_val_score's own second launch.  The record is therefore byte for byte clipmi_val_score's on the concatenated logits, however the
 * rows were cut into chunks.  workspace (256-byte aligned): clipmi_val_score_finish_workspace_bytes(N, n_bins) =
 * clipmi_val_score_workspace_bytes(N, n_bins).  CLIPMI_ERR_ARG: a null pointer, row_results not 16-byte aligned, the record not 8-byte
 * aligned, the workspace not 256-byte aligned, n_bins outside 1..64; CLIPMI_ERR_SHAPE: N < 1; CLIPMI_ERR_WORKSPACE.
 *
 * clipmi_vision_val_chunk: one chunk of B validation images in one call -- clipmi_vision_encoder_train's body at the fp32 master `prompts`
 * (same stash; the tower's workspace is the head of `workspace`), clipmi_l2_normalize of the features, clipmi_logits against the already
 * normalised text features text_n fp32 [C, E] at `scale`, clipmi_val_score_rows into row_results (the caller's pointer for the chunk's
 * first row, as above) -- the same launches as the four calls, hence the same bits.  workspace (256-byte aligned):
 * clipmi_vision_val_chunk_bytes(m, B, n_ctx, C) = the tower's + 2 x align256(4 B E) + align256(4 B C); 0 for arguments the call refuses.
 * Every check precedes the first launch: clipmi_vision_encoder_train's, clipmi_val_score_rows', B >= 1, a finite scale.
 *
 * CoCoOp (every image has its own C prompts, so an [N_val, C] text matrix never exists) and ProDA (the classifier is the mean over ALL P
 * contexts) validate through the INFERENCE forward: the record is what clipmi_val_score gives on the trainers' forward logits.
 *
 * clipmi_cocoop_val_rows: the per-pair tail fused into the row score.  img_n fp32 [Bv, E] (unit image features), txt fp32 [Bv, C, E] (raw
 * text-encoder outputs, image-major).  One workgroup per image b: z[c] = scale * <img_n[b], txt[b, c] / |txt[b, c]|> by one wave per class
 * (clipmi_logits_per_image's device function, the same bits) into C fp32 values in LDS, then clipmi_val_score's per-row device function on
 * them against labels[b]; row_results[b] is written and nothing else -- the [Bv, C] logits never go to memory.  C <= 16384 (LDS).
 * CLIPMI_ERR_ARG: a null pointer, row_results not 16-byte aligned, labels not 8-byte aligned, n_bins outside 1..64, a non-finite scale;
 * CLIPMI_ERR_SHAPE: Bv < 1, E < 1, C outside 1..16384.
 *
 * clipmi_cocoop_val_chunk: one chunk of Bv validation images in one call, the launches of the inference forward (cocoop.py:186-199):
 * clipmi_cocoop_ctx (params: the fit's master block [ctx | W1 | b1 | W2 | b2]; img_n fp32 [Bv, E] contiguous, already normalised),
 * clipmi_cocoop_prompts (base [C, context_length, Dt] fp16 | fp32 -> fp16 prompts), clipmi_text_encoder over the Bv C prompts (eot int32
 * [Bv C]: the classes' EOT rows repeated per image; seq_rows and flags as that call takes them), clipmi_cocoop_val_rows into row_results
 * (the caller's pointer for the chunk's first row; labels: the chunk's).  clipmi_val_score_finish then builds the record.  workspace
 * (256-byte aligned): clipmi_cocoop_val_chunk_bytes(m, C, seq_rows, Bv, n_ctx) = the tower's + 4 Bv n_ctx Dt + 2 Bv C context_length Dt +
 * 4 Bv C E, each part rounded up to 256; 0 for arguments the call refuses.  Every check precedes the first launch.
 *
 * clipmi_proda_val_mean: text fp32 [G P, E] (raw text features, a class's P rows together) -> mean fp32 [G, E]: every row times the
 * reciprocal of its L2 norm (clipmi_l2_normalize's order and rounding), a class's P unit rows added in ascending row order from 0 and the
 * sum divided by P (clipmi_group_mean's) -- the bits of those two calls, without the normalised copy.  fp32, no atomics.  P <= 4096.
 *
 * clipmi_proda_val_logits: one validation in one call (proda.py:316-331, 304-313).  For classes c0, c0 + class_chunk, ...: the prompts of
 * ALL P contexts at their positions `pos` in the order `order` int32 [P] (end | middle | front, the inference mirror's), assembled in the
 * model's type `dtype` with the fp32 master ctx [P, n_ctx, Dt] rounded to it (clipmi_proda_embed's placement, one shared device function;
 * no selection, no no-class prompts), clipmi_text_encoder, clipmi_proda_val_mean into mean [C, E]; then clipmi_fused_tail of the raw
 * validation features val_feats fp32 [n_val, E] (contiguous, 16-byte aligned) against mean -- exp(logit_scale) x_n . mean_c, the mean not
 * renormalised -- into the head of monitor_workspace, fp32 [n_val, C]; then clipmi_val_score into record `epoch` of `records` and, with a best
 * block, clipmi_best_select of ctx (the arguments from val_labels on are clipmi_taskres_fit_monitored's).  monitor_workspace:
 * clipmi_proda_val_monitor_bytes(n_val, C, n_bins) = 4 n_val C rounded up to 256 + clipmi_val_score's + the decision word.  workspace:
 * clipmi_proda_val_logits_bytes(m, C, P, seq_rows, class_chunk, n_val); both sizers return 0 for arguments the call refuses.  The tower's
 * kernel choice follows the row count of a call (clipmi_encode_image's note): chunkings that keep the choice give the same bits.
 * ---------------------------------------------------------------------------------------------------- */
int clipmi_cocoop_val_rows(const float* img_n, const float* txt, float scale, const int64_t* labels, int Bv, int C, int E, int n_bins,
                           void* row_results, clipmi_stream_t stream);
size_t clipmi_cocoop_val_chunk_bytes(const clipmi_model* m, int C, int seq_rows, int Bv, int n_ctx);
int clipmi_cocoop_val_chunk(clipmi_model* m, const void* base, int dtype, const float* params, int n_ctx, int H, const int32_t* eot, int C,
                            int seq_rows, const float* img_n, int Bv, float scale, const int64_t* labels, int n_bins, void* row_results,
                            unsigned flags, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
int clipmi_proda_val_mean(const float* text, float* mean, int G, int P, int E, clipmi_stream_t stream);
size_t clipmi_proda_val_monitor_bytes(int n_val, int C, int n_bins);
size_t clipmi_proda_val_logits_bytes(const clipmi_model* m, int C, int P, int seq_rows, int class_chunk, int n_val);
int clipmi_proda_val_logits(clipmi_model* m, const void* base, int dtype, const float* ctx, const int32_t* order, const int32_t* pos,
                            const int32_t* name_lens, const int32_t* cls_eot, int C, int P, int n_ctx, int seq_rows, int class_chunk, float scale,
                            unsigned flags, int epoch, const float* val_feats, int64_t val_ld, const int64_t* val_labels, int n_val, int n_bins,
                            void* records, int criterion, void* best_block, float* best_params, void* monitor_workspace,
                            size_t monitor_workspace_bytes, void* workspace, size_t workspace_bytes, clipmi_stream_t stream);
int clipmi_val_score_rows(const float* logits, int64_t ld, const int64_t* labels, int rows, int C, int n_bins, void* row_results,
                          clipmi_stream_t stream);
size_t clipmi_val_score_finish_workspace_bytes(int N, int n_bins);
int clipmi_val_score_finish(const void* row_results, int N, int n_bins, void* record, void* workspace, size_t workspace_bytes,
                            clipmi_stream_t stream);
size_t clipmi_vision_val_chunk_bytes(const clipmi_model* m, int B, int n_ctx, int C);
int clipmi_vision_val_chunk(clipmi_model* m, const void* image, int image_dtype, int B, const float* prompts, int n_ctx, int depth,
                            const float* text_n, int C, float scale, const int64_t* labels, int n_bins, void* row_results, void* workspace,
                            size_t workspace_bytes, void* stash, size_t stash_bytes, clipmi_stream_t stream);
size_t clipmi_val_score_workspace_bytes(int N, int n_bins);
int clipmi_val_score(const float* logits, int64_t ld, const int64_t* labels, int N, int C, int n_bins, void* record, void* workspace,
                     size_t workspace_bytes, clipmi_stream_t stream);
size_t clipmi_best_select_workspace_bytes(int64_t n_floats);
int clipmi_best_select(const void* record, void* best_block, int criterion, int epoch, const float* params, float* best_params, int64_t n_floats,
                       void* workspace, size_t workspace_bytes, clipmi_stream_t stream);

/* ------------------------------------------------------------------------------------------------------
 * Row scores: proper scores of whole probability rows and the class-wise calibration error at test time (csrc/row_scores.hip, DESIGN.md
 * "Row scores"; the float64 restatement is clip_calibration_amd/metrics.py NLL / Brier / ClasswiseECE).  Nothing is read back to the host.
 * Additive exports: the ABI version stays.
 *
 * clipmi_row_scores: rows fp32 [N, C] with the row stride ld (elements), labels int64 [N].  from_probs = 0: the rows are logits and
 * p_c = exp(z_c - max) * (1 / sum), sum = sum_c exp(z_c - max), all in fp32, a lane of the row's wave adding its columns c = lane, lane + 64,
 * ... in ascending order before the xor butterfly (clipmi_val_score's order); from_probs = 1: p_c is the entry as given, the rows need not sum
 * to 1.  row_out fp32 [N, 2] = per row {nll, brier}: nll = log(sum) - (z[label] - max), or -log(max(p[label], FLT_MIN)); brier =
 * sum_c (p_c - [c == label])^2.  class_acc int64 [3][C][n_bins + 1] = count | conf_sum | hits is ADDED to: element (i, c) counts in bin
 * numpy.digitize(p_ic, numpy.linspace(0, 1, n_bins + 1)) - 1 of class c (clipmi_ece_accumulate's rule, one device function: the last bin,
 * n_bins, holds p == 1.0), adds round-to-nearest-even(clamp(p_ic, 0, 1) * 2^32) to conf_sum (32.32 fixed point) and, when c == label, 1 to
 * hits.  The caller zeroes the block once (clipmi_row_scores_acc_bytes(C, n_bins) = 24 C (n_bins + 1) bytes, 0 for arguments the call
 * refuses) and may then add any number of calls, in batches, in stream order: integer additions only (64-bit integer atomics), so the
 * block's bytes depend neither on the order of the atomics nor on how the rows were cut into calls, and the same inputs give the same bits.
 * For a chunk that starts at row row0 the caller passes row_out + 2 row0 and labels + row0.
 * Rows that cannot be scored follow clipmi_val_score's rule: a label outside [0, C) is never used as an address, the row's nll and brier are
 * NaN and it counts no hit (its probabilities are binned all the same); a row without a softmax -- it holds a NaN or a +inf or nothing but
 * -inf; with from_probs any non-finite entry -- has a NaN nll and brier, counts no hit, and each of its elements counts in bin n_bins (where
 * a NaN sorts) and adds nothing to conf_sum.  The inputs are not written.
 * N == 0 returns CLIPMI_OK without a launch.  Every check precedes the launch.  CLIPMI_ERR_SHAPE: N < 0, C < 1, ld < C, C (n_bins + 1) >=
 * 2^31; CLIPMI_ERR_ARG: n_bins outside 1..1024 (clipmi_ece_accumulate's limit), from_probs other than 0 or 1, a null pointer, rows not
 * 4-byte aligned, labels, row_out or class_acc not 8-byte aligned.
 *
 * clipmi_row_scores_finish: out float64 [4] (device) = {mean nll, mean brier, class-wise ECE, N} from the N row scores and the block:
 * class-wise ECE = (1 / C) sum_c sum_b (n_cb / N) |hits_cb / n_cb - conf_cb / n_cb| = sum_c sum_b |hits_cb - conf_cb| / (N C) over the
 * n_bins intervals, bin n_bins (p == 1.0) counted into the last one.  Launch 1: float64 partial sums, of the rows per 4096 rows (a thread
 * its 16 rows in ascending order, then a fixed halving tree) and of the classes' gaps per 256 classes; launch 2: one thread adds the
 * partials in ascending order.  The order depends on N and C alone: the four doubles are the same bits however the rows were chunked.
 * workspace (256-byte aligned): clipmi_row_scores_finish_workspace_bytes(N, C), 0 for arguments the call refuses.  CLIPMI_ERR_SHAPE: N < 1,
 * C < 1; CLIPMI_ERR_ARG: n_bins outside 1..1024, a null pointer, an alignment; CLIPMI_ERR_WORKSPACE.
 * ---------------------------------------------------------------------------------------------------- */
size_t clipmi_row_scores_acc_bytes(int C, int n_bins);
int clipmi_row_scores(const float* rows, int64_t ld, const int64_t* labels, int N, int C, int from_probs, int n_bins, float* row_out, void* class_acc,
                      clipmi_stream_t stream);
size_t clipmi_row_scores_finish_workspace_bytes(int N, int C);
int clipmi_row_scores_finish(const float* row_out, int N, const void* class_acc, int C, int n_bins, double* out, void* workspace,
                             size_t workspace_bytes, clipmi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIPMI_H */
