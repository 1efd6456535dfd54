/*
 * pram_hip.h — C ABI of libpram_hip.so, the MI355X (gfx950) kernels underneath the PRAM
 * per-query hot path (SFD2 extract -> SegNetViT recognise -> GML/AdaGML match + Sinkhorn).
 *
 * The reference (feixue94/pram) is pure Python on stock torch ops and has no FFI; the boundary
 * it exposes is dict-in/dict-out nn.Modules.  This header is the native
 * boundary a maintainer binds underneath those modules (ctypes stub in INTEGRATION.md); each
 * entry names the reference torch-op site (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless it says "host"; fp32 unless typed otherwise.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, nothing syncs.
 *   - no allocation inside; workspaces are passed in and sized by the *_workspace_bytes query.
 *   - return 0 on success, negative on error (PRAM_E_*); pram_last_error() gives the text.
 *   - ragged batches: `*_lens` are per-batch-element int32 device arrays (NULL = every
 *     element has the padded max length).  The reference has no masks; a padded row/key is
 *     never read into a softmax, so each element computes exactly its B=1 result.
 *   - token matrices are row-major [rows][ld]; heads are 64-wide column blocks.
 *
 * Limits (each is checked and comes back as PRAM_E_ARG with a message, never as a wrong result):
 *   - attention heads are exactly 64 wide (the shipped models: hidden 256 = 4 heads; pram_amd's Python layer raises on any
 *     other hidden_dim before it gets here);
 *   - keypoint selection sorts a top-k of up to 8192 keypoints per frame in LDS; larger bounds sort in the caller's workspace
 *     (pram_select_keypoints_workspace_bytes accounts for it) and max_keypoints >= h * w keeps everything unsorted;
 *   - AdaGML pruning handles token sets of at most 8192 tokens (pram_adagml_prune_f32);
 *   - Sinkhorn / dual-softmax matching handles at most 8191 rows (m_max) and 4351 columns (n_max) per pair, the dust-bin row
 *     and column excluded (pram_sinkhorn_match_f32, pram_dual_softmax_match_f32);
 *   - k-means labelling takes at most PRAM_KMEANS_MAX_K = 4096 clusters and fewer than 2^31 points (the pram_kmeans entries);
 *   - statistical outlier removal keeps at most PRAM_KNN_MAX_K = 32 neighbours per point, in registers, and takes fewer than
 *     2^31 points (pram_knn_mean_distance, pram_sor_select);
 *   - LayerNorm rows are at most 1024 wide; the split-fp16 GEMMs need K % 32 == 0 (other shapes: the exact-fp32 entry);
 *   - the split-fp16 operands carry value * s in fp16 (s = 16 by default, pram_x3_set_act_scale): a finite |x| >= 65520 / s
 *     (4094.97) does not fit.  This one is NOT a silent limit
 *     either: see "range guard" below (pram_set_status_word) — the kernels report it, and pram_amd's Python layer re-runs the
 *     call on the exact-fp32 entries (or raises).
 */
#ifndef PRAM_HIP_H
#define PRAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRAM_OK 0
#define PRAM_E_ARG (-1)      /* bad shape / alignment / null pointer */
#define PRAM_E_LAUNCH (-2)   /* hipLaunchKernel failed */
#define PRAM_E_UNSUPPORTED (-3)

int pram_hip_version(void);
const char* pram_last_error(void);
/* Which kernel instantiation the last size-dependent launch of the CALLING HOST THREAD took, e.g. "conv_x3<2,1>",
 * "linear_x3w<4,2,4,planes>", "attention_x3_pipe<ps,mode0,w8,phases>" ("" before the first one).  The GEMM, convolution and
 * attention entries pick their tile from the launch grid; this is how a test knows which one it exercised.  Entries whose
 * kernel is fixed by the entry leave the record alone.  The string is valid until the thread's next call of this function. */
const char* pram_last_kernel(void);

/* ---------------------------------------------------------------- range guard of the split-fp16 ("x3") entries
 * The x3 entries carry every fp32 activation as two fp16 parts of value * s (s = the activation scale below, 16 by default).  A finite
 * value with |s x| >= 65520 rounds to
 * +-inf in its hi part and the result of the launch is garbage (usually NaN — but NaN scores turn into ordinary-looking
 * indices further down).  Kernel launches are asynchronous, so this cannot come back as a return code of the launch: every x3
 * kernel that splits fp32 values (GEMM / convolution operand staging, the plane-writing epilogues) ORs PRAM_STATUS_X3_RANGE
 * into a caller-owned DEVICE status word when it meets such a value.  The word is sticky until reset.  NaN inputs are not
 * flagged: they propagate as NaN, exactly as in the reference's fp32 arithmetic; +-inf inputs are flagged.
 *   pram_set_status_word : registers the word for the CURRENT device (NULL detaches; without a word nothing is reported).
 *   pram_read_status_word: enqueues a copy of the word to *host_out on `stream`, waits for the stream, and (reset != 0) clears
 *                          the word if it was set.  A caller that sees PRAM_STATUS_X3_RANGE re-runs on the *_f32 entries. */
#define PRAM_STATUS_X3_RANGE 1u
int pram_set_status_word(unsigned int* device_word);
/* Activation scale.  The planes carry value * s with s = 16 by default: the range is |x| < 65520 / s = 4094.97 and values down
 * to 2^-25 / s keep their last bit (the lo part is an fp16 subnormal below 2^-14).  A model whose activations are larger (trained
 * checkpoints; the range guard trips) lowers s instead of leaving the split path: s = 1 carries |x| < 65520 with an absolute floor
 * of 3e-8, s = 2^-4 a million with 4.8e-7 — the pair (hi, lo) is a 22-bit significand whatever the scale, only the floor moves.
 *   pram_x3_set_act_scale(s): s = a power of two in [2^-12, 2^4] -> sets the scale for the CALLING HOST THREAD and returns the
 *   previous one; s <= 0 only queries; anything else returns -1 and changes nothing.  Every x3 entry reads it at launch and
 *   hands it to its kernel by value: planes written under one setting must be consumed under the same setting (pram_amd's models
 *   set it around their forward, nets/_blocks.py); a captured hipGraph replays with the value it was captured under. */
float pram_x3_set_act_scale(float scale);
int pram_read_status_word(unsigned int* host_out, int reset, void* stream);

/* ---------------------------------------------------------------- token linear algebra */

/* flags for pram_linear_f32 */
#define PRAM_LIN_ROTARY 1  /* rotate column pairs (c, c+32) of each 64-wide head for c < rot_cols */

/* out[m][n] = alpha * ( [A0 | A1] · Wᵀ + bias ) + residual          (nn.Linear sites:
 * nets/segnetvit.py:87-95,157-164; nets/gml.py:118-126,151-159,220,235; K6 in SURVEY.md §2.1)
 *   A0 [m][lda0] supplies k in [0,k0), A1 [m][lda1] supplies k in [k0,k0+k1) (the torch.cat of
 *   segnetvit.py:106); a1 may be NULL with k1 = 0.  W is [n][k0+k1] (torch layout).
 *   PRAM_LIN_ROTARY: W rows were pre-permuted so that within each 64-wide head the even
 *   rotary dims are columns 0..31 and the odd dims 32..63; cos/sin are [m][32]
 *   (apply_cached_rotary_emb, segnetvit.py:21-23).
 * Constraints: k0 % 32 == 0 when k1 > 0; (k0+k1) % 4 == 0; lda % 4 == 0. */
int pram_linear_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                    const float* w, const float* bias, const float* residual, int ldr,
                    float* out, int ldo, int m, int n, float alpha, int flags,
                    const float* rot_cos, const float* rot_sin, int rot_cols, void* stream);

/* fp16-operand variant for BASELINE config C5 ("fp16 MFMA path"): identical contract, but `w16` is the weight
 * matrix pre-converted to IEEE fp16 ([n][k0+k1]) and the activations are rounded to fp16 on their way into LDS;
 * products on v_mfma_f32_32x32x16_f16, fp32 accumulate and epilogue.  Needs (k0+k1) % 8 == 0 and, with a
 * second segment, k0 % 64 == 0.  Not for the fp32 parity configurations. */
int pram_linear_f16_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                        const void* w16, const float* bias, const float* residual, int ldr,
                        float* out, int ldo, int m, int n, float alpha, int flags,
                        const float* rot_cos, const float* rot_sin, int rot_cols, void* stream);

/* pram_linear_f16_f32 on a ragged token matrix, as pram_linear_ragged_f32 / pram_linear_x3_ragged_f32: rows are sequences of
 * t_pad rows, sequence s has lens[s] (device int32) valid ones; output tiles without a valid row are skipped and only valid rows
 * are stored (`out` may be a persistent buffer whose other rows belong to someone else: AdaGML commits the matching descriptors
 * of the pairs that stop at a layer, nets/adagml.py:386-396).  lens == NULL: pram_linear_f16_f32. */
int pram_linear_f16_ragged_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                               const void* w16, const float* bias, const float* residual, int ldr,
                               float* out, int ldo, int m, int n, float alpha, int flags,
                               const float* rot_cos, const float* rot_sin, int rot_cols,
                               const int* lens, int t_pad, void* stream);

/* pram_linear_f16_f32 that also (or only: out may be NULL) writes the result rounded to fp16 — the q / k / v operand
 * of pram_attention_h16_f32, which would otherwise round the fp32 result itself while staging it (same values). */
int pram_linear_f16_h16(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                        const void* w16, const float* bias, const float* residual, int ldr,
                        float* out, int ldo, void* out16, int ldo16, int m, int n, float alpha, int flags,
                        const float* rot_cos, const float* rot_sin, int rot_cols, void* stream);

/* Split-fp16 ("x3") variant: fp32-class results on the fp16 matrix pipe (same nn.Linear sites; default path).
 * Every fp32 operand x is carried as two fp16 numbers, x * s = hi + lo (s a power of two), and every product as
 * three v_mfma_f32_32x32x16_f16 accumulated in fp32: a.b ~= (a_hi.b_hi + a_hi.b_lo + a_lo.b_hi) / (s_a s_b) — the
 * dropped lo.lo term and the truncation of hi + lo are 2^-22 relative, the class of fp32 rounding itself.
 *   w_hi / w_lo : the weight matrix [n][k0+k1] * w_scale split on the host into two fp16 planes
 *                 (pram_amd/ops.py::split_weight; w_scale = the power of two that puts max|w| in [2^13, 2^14));
 *   activations : fp32 in HBM, split with s = 16 while they are staged (|x| must stay below 4094);
 *   out_hi / out_lo (optional, both or neither; then `out` may be NULL): the result * 16 as split planes
 *                 [m][ldo16] fp16 — the q / k / v operand format of pram_attention_x3_f32.
 * Needs (k0+k1) % 8 == 0 and, with a second segment, k0 % 32 == 0. */
int pram_linear_x3_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                       const void* w_hi, const void* w_lo, float w_scale, const float* bias,
                       const float* residual, int ldr, float* out, int ldo, void* out_hi, void* out_lo,
                       int ldo16, int m, int n, float alpha, int flags, const float* rot_cos,
                       const float* rot_sin, int rot_cols, void* stream);

/* Profiling aid (no product caller): with PRAM_GEMM_ABLATE=4 in the environment the wide split-fp16 GEMM adds, per workgroup,
 * the shader-clock cycles of each main-loop phase to eight device counters: [0] issue + MFMA k-steps, [1] wait for the
 * chunk's loads, [2] commit (split + LDS writes), [3] barrier, [4] whole main loop, [5] workgroups, [6] epilogue;
 * [8 + 8 w + i] = eight time stamps of wave w of workgroup 0 in its fourth chunk (gemm_core_x3w.h).
 * out72 = HOST array of 72 counters; reset != 0 clears them after the read. */
int pram_debug_gemm_phases(unsigned long long* out72, int reset);

/* The q | k | v projection of an attention block in one call (nets/segnetvit.py:87-95, nets/gml.py:151-159), split-fp16 path:
 * columns [0, vt_col0) leave as row-major split planes [m][ldo16] (out_hi / out_lo: the q / k operands of pram_attention_x3_f32,
 * rotary applied to the first rot_cols of them when PRAM_LIN_ROTARY is set); the last heads * 64 columns — the values — leave
 * as the transposed, key-permuted planes [m / t_seq][heads][64][t_seq] that pram_attention_x3_vt would build from them (zeros
 * for tokens >= lens[s]; lens may be NULL).  Rows are sequences of t_seq tokens, t_seq % 64 == 0; n == vt_col0 + heads * 64. */
int pram_linear_x3_qkv_f32(const float* a0, int lda0, int k0, const void* w_hi, const void* w_lo, float w_scale,
                           const float* bias, void* out_hi, void* out_lo, int ldo16, void* vt_hi, void* vt_lo, int vt_col0,
                           int heads, int t_seq, int m, int n, int flags, const float* rot_cos, const float* rot_sin,
                           int rot_cols, const int* lens, void* stream);

/* pram_linear_x3_f32 with the activations already split: [A0 | A1] given as fp16 planes (value * s = hi + lo, s = pram_x3_set_act_scale's value in force at the PRODUCER's launch and here, 16 by default; [m][lda]
 * halves) written by the epilogues of pram_linear_x3[p]_f32 / pram_attention_x3_f32 / pram_layernorm_gelu_x3.  Both operands are
 * then staged with plain 16-byte copies (the fp32-input form splits A again in every column tile and is instruction-issue
 * bound).  k0, k1 multiples of 32; lda multiples of 8. */
int pram_linear_x3p_f32(const void* a0_hi, const void* a0_lo, int lda0, int k0, const void* a1_hi, const void* a1_lo,
                        int lda1, int k1, const void* w_hi, const void* w_lo, float w_scale, const float* bias,
                        const float* residual, int ldr, float* out, int ldo, void* out_hi, void* out_lo, int ldo16,
                        int m, int n, float alpha, int flags, const float* rot_cos, const float* rot_sin, int rot_cols,
                        void* stream);

/* Ragged token matrices (AdaGML's pruned / stopped pairs): rows are sequences of t_pad rows, sequence s has lens[s] (device
 * int32) valid ones.  Output tiles that contain no valid row are skipped and their outputs left untouched; everything else is
 * the un-ragged call.  (The reference shrinks its tensors with boolean indexing instead, nets/adagml.py:354-372.) */
int pram_linear_ragged_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                           const float* w, const float* bias, const float* residual, int ldr,
                           float* out, int ldo, int m, int n, float alpha, int flags,
                           const float* rot_cos, const float* rot_sin, int rot_cols,
                           const int* lens, int t_pad, void* stream);
int pram_linear_x3_ragged_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1,
                              const void* w_hi, const void* w_lo, float w_scale, const float* bias,
                              const float* residual, int ldr, float* out, int ldo, void* out_hi, void* out_lo,
                              int ldo16, int m, int n, float alpha, int flags, const float* rot_cos,
                              const float* rot_sin, int rot_cols, const int* lens, int t_pad, void* stream);

/* Batched C_b = alpha * A_b · B_bᵀ (einsum 'bmd,bnd->bmn', nets/gml.py:282; K12).
 * A_b = a + b*stride_a, [m_max][lda]; B_b [n_max][ldb]; C_b [m_max][ldc]. */
int pram_bgemm_nt_f32(const float* a, int lda, long long stride_a, const float* b, int ldb,
                      long long stride_b, float* c, int ldc, long long stride_c, int batch,
                      int m_max, int n_max, int k, float alpha, void* stream);

/* pram_bgemm_nt_f32 on the split-fp16 path: both operands as split planes (value * s = hi + lo at the activation scale in force, what the projection epilogues
 * write: pram_linear_x3_f32 out_hi / out_lo): a [m_max][lda], b [n_max][ldb == k] per batch element; strides in halves for the
 * planes, in floats for c.  k % 32 == 0, lda and the plane strides % 8 == 0.  Three fp16 MFMAs per product, fp32-class result. */
int pram_bgemm_nt_x3p_f32(const void* a_hi, const void* a_lo, int lda, long long stride_a, const void* b_hi, const void* b_lo,
                          int ldb, long long stride_b, float* c, int ldc, long long stride_c, int batch, int m_max, int n_max,
                          int k, float alpha, void* stream);

/* y = GELU(LayerNorm(x)) rowwise, eps 1e-5, exact erf GELU (nn.LayerNorm + nn.GELU,
 * nets/segnetvit.py:92-93,161-162; K11).  In place when y == x.  cols <= 1024, cols % 4 == 0 */
int pram_layernorm_gelu_f32(const float* x, int ldx, float* y, int ldy, const float* gamma,
                            const float* beta, int rows, int cols, float eps, void* stream);

/* the same, skipping the rows beyond their sequence's length (see pram_linear_ragged_f32) */
int pram_layernorm_gelu_ragged_f32(const float* x, int ldx, float* y, int ldy, const float* gamma, const float* beta,
                                   int rows, int cols, float eps, const int* lens, int t_pad, void* stream);

/* Fourier positional encoding (normalize_keypoints nets/utils.py:17-24 +
 * LearnableFourierPositionalEncoding nets/segnetvit.py:35-40; K7):
 *   nk = (kpts - (cx,cy)) / scale ; proj = Wr·nk ; cos_out/sin_out [rows][32].
 * Pass cx = cy = 0, scale = 1 for pre-normalised keypoints. */
int pram_fourier_encoding_f32(const float* kpts, const float* wr, float cx, float cy, float scale,
                              float* cos_out, float* sin_out, int rows, void* stream);

/* ---------------------------------------------------------------- attention (graded kernel) */

/* Flash-style multi-head attention, head_dim 64, exact-fp32 MFMA (Attention.forward
 * nets/segnetvit.py:73-76; for cross attention (nets/gml.py:175-179) see pram_attention_cross_f32 below; K8/K9):
 *   out[b, i, h*64:(h+1)*64] = softmax_j( scale * q[b,i,h]·k[b,j,h] ) · v[b,j,h]
 * q rows of batch b start at row b*m_max (k/v: b*n_max).  lse2 (optional) receives
 * log2-domain log-sum-exp [batch][heads][m_max] for pram_attention_colmean_f32. */
int pram_attention_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                       float* out, int ldo, float* lse2, const int* q_lens, const int* k_lens,
                       int batch, int heads, int m_max, int n_max, float scale, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Keys are reduced in chunks of 512 folded in order.  A launch with fewer than 512 (batch, head, 128-row) units
 * — one to four query frames — cannot fill the chip, so when the caller passes a workspace of at least this many
 * bytes the chunks run as separate workgroups and a second kernel applies the same fold; the result is bit-identical
 * with or without the workspace.  Returns 0 when the launch would not be split (pass NULL / 0 then). */
size_t pram_attention_workspace_bytes(int batch, int heads, int m_max, int n_max);

/* The "fp16 MFMA path" of BASELINE config C5: same contract as pram_attention_f32 (fp32 tensors in HBM),
 * but Q/K/V and the probabilities are rounded to fp16 and multiplied on v_mfma_f32_32x32x16_f16 (fp32
 * accumulate, fp32 softmax).  ~1e-3 relative error: NOT for the fp32 parity configs. */
int pram_attention_f16_f32(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                           float* out, int ldo, float* lse2, const int* q_lens, const int* k_lens,
                           int batch, int heads, int m_max, int n_max, float scale, void* stream);

/* pram_attention_f16_f32 on q / k / v that are already fp16 in HBM (ld* in halves, multiples of 8): bit-identical
 * output, half the operand traffic, two K/V tiles in flight.  kv_shift = 0 for self attention; = pairs with
 * batch = 2*pairs for the single-launch cross attention (see pram_attention_cross_f32). */
int pram_attention_h16_f32(const void* q16, int ldq, const void* k16, int ldk, const void* v16, int ldv, float* out,
                           int ldo, float* lse2, const int* q_lens, const int* k_lens, int batch, int heads,
                           int m_max, int n_max, float scale, int kv_shift, void* stream);

/* Split-fp16 ("x3") flash attention — the default attention of the fp32 parity path (same einsum -> softmax -> einsum
 * sites as pram_attention_f32).  q / k are row-major split planes written by pram_linear_x3_f32 (value * s = hi + lo at the activation scale in force,
 * ld* in halves, multiples of 8; heads are 64-wide column blocks); vt_hi / vt_lo are the TRANSPOSED value planes of the
 * key side built by pram_attention_x3_vt: [batch][heads][64][tv], tv = n_max rounded up to 64.  S = K Q^T and O = P V are
 * fp16 MFMAs with fp32 accumulation: three per product for the scores and, by default, three per product for P V (the
 * probabilities enter as two fp16 parts like every other operand: 48 MFMAs per 64-key tile and 32-query wave);
 * pram_attention_x3_set_p_split(0) carries the probabilities as ONE fp16 from 1024 keys on (two MFMAs per P V product, 40 per
 * tile — not the default, see below); pram_attention_x3_mfma_per_tile reports what a launch issues.  Output fp32.
 * kv_shift as in pram_attention_h16_f32 (cross attention: batch = 2 * pairs, kv_shift = pairs).
 * Key chunks: from 1024 keys on the keys are reduced in chunks (pram_attention_x3_set_chunk_keys: default 4096 keys, i.e. one chunk for every shipped configuration), each chunk
 * normalised and all chunks folded in chunk order.  One workgroup normally walks all chunks of its 128 query rows and folds them
 * in registers; an under-filled launch (pram_attention_x3_is_split: one or two query frames, the reference's online loop
 * localization/loc_by_rec_online.py:109-133) runs groups of chunks as a second grid dimension, parks them in `workspace`
 * (pram_attention_x3_workspace_bytes; 0 when a sequence is a single chunk) and folds them in a second kernel: the SAME fold in
 * the SAME order, so the output is bit-identical whichever mode ran.  workspace == NULL (or too small): always fused. */
size_t pram_attention_x3_workspace_bytes(int batch, int heads, int m_max, int n_max);
int pram_attention_x3_is_split(int batch, int heads, int m_max, int n_max);
/* tuning / test knob: under-filled launches are split along the keys into as many groups of 512-key chunks as bring the grid to
 * `workgroups` (default 256 = one per CU; 0 = never; negative restores the default); returns the previous value.  The mode never
 * changes a result bit.  pram_attention_x3_is_split returns the number of groups (1 = fused). */
int pram_attention_x3_set_split_target(int workgroups);
/* keys per chunk (a multiple of 128; default 4096), process-wide: set it before the first
 * launch — it fixes where EVERY launch folds its partial soft-maxes (results move in their last bits, consistently for all batch
 * sizes).  Smaller chunks let shorter key sets use the split mode; a fused walk pays a spill round trip at every chunk end
 * (+17 % kernel time at 512 keys per chunk for 2048-key sets, +6 % at 2048 for 4096-key sets).  0 = query; returns the value. */
int pram_attention_x3_set_chunk_keys(int keys);
int pram_attention_x3_mfma_per_tile(int n_max);
/* probabilities in P V from 1024 keys on: 1 = two fp16 parts (three MFMAs per product; default), 0 = one fp16 (two MFMAs, ~15 % less
 * attention time, 2^-12 relative rounding per probability: logits 7e-4..1.3e-3 instead of 4e-5 from the fp32 oracle on flat attention: outside the 1e-3 parity bar on some shapes, an opt-in that is NOT parity-gated).
 * Process-wide, this setter only.  Negative = query; returns the value in force. */
int pram_attention_x3_set_p_split(int split);
int pram_attention_x3_f32(const void* q_hi, const void* q_lo, int ldq, const void* k_hi, const void* k_lo, int ldk,
                          const void* vt_hi, const void* vt_lo, float* out, int ldo, float* lse2,
                          const int* q_lens, const int* k_lens, int batch, int heads, int m_max, int n_max,
                          float scale, int kv_shift, void* workspace, size_t workspace_bytes, void* stream);

/* Column means of the soft-max matrix of the pram_attention_x3_f32 call that produced lse2 (AdaGML's token scores,
 * nets/adagml.py:92-104): colmean[kb][j] = mean over heads and over the q_lens[b] query rows of softmax_row(scale q k^T)[i][j],
 * kb = (b + kv_shift) % batch, [batch][n_max] fp32; entries j >= k_lens[kb] are left untouched.  q / k: the same split planes,
 * lse2: [batch][heads][m_max] (log2 domain).  Second Q K^T pass on the fp16 matrix pipe, three MFMAs per product; no atomics. */
int pram_attention_x3_colmean_f32(const void* q_hi, const void* q_lo, int ldq, const void* k_hi, const void* k_lo, int ldk,
                                  const float* lse2, float* colmean, const int* q_lens, const int* k_lens, int batch,
                                  int heads, int m_max, int n_max, float scale, int kv_shift, void* stream);

/* Single-product ("fp16 MFMA path", BASELINE C5) flash attention on the software-pipelined kernel of the split path: q / k = fp16
 * row-major [rows][ld] (pram_linear_f16_h16), vt16 = the transposed, key-permuted fp16 values [batch][heads][64][tv] written by
 * pram_attention_x3_vt with NULL lo planes.  One fp16 MFMA per product; the probabilities are rounded to fp16 like the inputs
 * (this path's own, looser tolerance).  Output fp32; lse2 / lens / kv_shift as pram_attention_x3_f32. */
int pram_attention_h16t_f32(const void* q16, int ldq, const void* k16, int ldk, const void* vt16, float* out, int ldo,
                            float* lse2, const int* q_lens, const int* k_lens, int batch, int heads, int m_max,
                            int n_max, float scale, int kv_shift, void* stream);

/* Row-major value planes [seqs * t_max][ldv] (head h at columns 64 h ..) -> the transposed, key-permuted planes
 * pram_attention_x3_f32 stages with plain 16-byte copies: [seqs][heads][64][tv], tv = t_max rounded up to 64, position of
 * token t = 64 (t / 64) + perm(t % 64) (the order in which the S^T accumulator registers hold the keys); tokens
 * t >= lens[seq] (NULL: t_max) are written as zeros.  v_lo == vt_lo == NULL: one plane only (the fp16 values of
 * pram_attention_h16t_f32). */
int pram_attention_x3_vt(const void* v_hi, const void* v_lo, int ldv, void* vt_hi, void* vt_lo, const int* lens,
                         int seqs, int heads, int t_max, void* stream);

/* Both directions of CrossMultiHeadAttention.forward (nets/gml.py:175-179; adagml.py:222-231) in ONE launch:
 * 2*pairs sequences of t_max rows each, sequences 0..pairs-1 = set 0, pairs..2*pairs-1 = set 1; sequence s takes
 * its queries from rows s*t_max.. of qk (the shared to_qk projection) and its keys / values from sequence
 * (s + pairs) mod 2*pairs of qk / v.  lens [2*pairs] (optional).  Per sequence the arithmetic is exactly
 * pram_attention_f32's (same kernel, same tiling), so the result equals two separate calls bit for bit. */
int pram_attention_cross_f32(const float* qk, int ldqk, const float* v, int ldv, float* out, int ldo, float* lse2,
                             const int* lens, int pairs, int heads, int t_max, float scale, void* workspace,
                             size_t workspace_bytes /* pram_attention_workspace_bytes(2*pairs, heads, t_max, t_max) */, void* stream);
int pram_attention_cross_f16_f32(const float* qk, int ldqk, const float* v, int ldv, float* out, int ldo, float* lse2,
                                 const int* lens, int pairs, int heads, int t_max, float scale, void* stream);
/* Column means for the same pairing: colmean [2*pairs][t_max]; row kb holds, per token of sequence kb, the mean
 * over heads and over the queries of sequence (kb + pairs) mod 2*pairs (adagml.py:229). */
int pram_attention_cross_colmean_f32(const float* qk, int ldqk, const float* lse2, float* colmean, const int* lens,
                                     int pairs, int heads, int t_max, float scale, void* stream);

/* Column means of the attention matrix (AdaGML Attention.forward nets/adagml.py:148,229; K10):
 *   colmean[b][j] = 1/(heads*m_b) * sum_h sum_i softmax(scale q k^T)[b,h,i,j] */
int pram_attention_colmean_f32(const float* q, int ldq, const float* k, int ldk, const float* lse2,
                               float* colmean, const int* q_lens, const int* k_lens, int batch,
                               int heads, int m_max, int n_max, float scale, void* stream);

/* ---------------------------------------------------------------- optimal transport + matches */

size_t pram_sinkhorn_workspace_bytes(int batch, int m_max, int n_max);

/* sink_algorithm (nets/gml.py:27-46; K13): plain-domain Sinkhorn on the dustbin-augmented
 * (m+1)x(n+1) matrix, `iters` iterations, eps 1e-8.  dist [batch][m_max][ldd].
 * bin_score: device pointer to the scalar parameter.  Outputs:
 *   p_out (optional) [batch][m_max+1][ldp] the final P*u*v (for parity with sink_algorithm)
 *   compute_matches (nets/gml.py:304-319; K14) fused into the last pass:
 *   matches0 [batch][m_max] int64 (-1 none), matches1 [batch][n_max], mscores0/1 fp32.
 * Rows >= m_b / cols >= n_b of the outputs are filled with -1 / 0.
 * m_max <= 8191 and n_max <= 4351; a larger problem is refused with PRAM_E_ARG. */
int pram_sinkhorn_match_f32(const float* dist, int ldd, const int* m_lens, const int* n_lens,
                            const float* bin_score, int iters, float match_threshold,
                            float* p_out, int ldp, long long* matches0, long long* matches1,
                            float* mscores0, float* mscores1, int batch, int m_max, int n_max,
                            void* workspace, void* stream);

/* dual_softmax (nets/gml.py:20-24; K15) + compute_matches; same outputs as above. */
int pram_dual_softmax_match_f32(const float* dist, int ldd, const int* m_lens, const int* n_lens,
                                const float* bin_score, float match_threshold, float* p_out, int ldp,
                                long long* matches0, long long* matches1, float* mscores0,
                                float* mscores1, int batch, int m_max, int n_max, void* workspace,
                                void* stream);

/* ---------------------------------------------------------------- AdaGML token pruning (K10) */

/* PoolingLayer tail + pruning bookkeeping (nets/adagml.py:137,354-372,516-531), one token set per
 * workgroup: conf = sigmoid(logit); n_below[s] = #(conf < thr) over the set's current tokens (the
 * check_if_stop numerator).  If lens_in[s] >= n_min_tokens the tokens with conf > thr are compacted,
 * order preserved, into x_out / cos_out / sin_out / ind_out (else all are copied); lens_out[s] = kept.
 * x [sets][t_max][ldx], cos/sin [sets][t_max][32], ind [sets][t_max] (original token ids).
 * Out-of-place only; rows at and beyond lens_out[s] of the outputs are not written.  conf_out (optional) [sets][t_max]
 * receives the confidences.  row_map: scratch, int32 [sets][t_max] (source row of every destination row). */
int pram_adagml_prune_f32(const float* conf_logit, float thr, int n_min_tokens, const int* lens_in,
                          const float* x_in, const float* cos_in, const float* sin_in, const int* ind_in,
                          float* x_out, float* cos_out, float* sin_out, int* ind_out, int* lens_out,
                          int* n_below, float* conf_out, int* row_map, int sets, int t_max, int ldx, void* stream);

/* Scatter the matches of the pruned sets back to full size (nets/adagml.py:382-396):
 * out_matches[b][ind0[i]] = ind1[matches0[i]] where matches0[i] >= 0; out_scores[b][ind0[i]] = mscores0[i].
 * out_* [batch][m_full] must be pre-filled with -1 / 0. */
int pram_adagml_scatter_f32(const long long* matches0, const float* mscores0, const int* ind0, const int* ind1,
                            const int* lens0, int batch, int t_max, int m_full, long long* out_matches,
                            float* out_scores, void* stream);

/* ---------------------------------------------------------------- SFD2 (NHWC feature maps) */

/* Implicit-GEMM convolution, NHWC, exact-fp32 MFMA (ResNet4x conv stack nets/sfd2.py:281-293,
 * 331-333; K1):  out = act( (conv(in, w) + bias) * scale + shift + residual )
 *   in [b][h][w][cin]; w [cout][ks][ks][cin] (repacked OIHW); out [b][ho][wo][cout],
 *   ho = (h + 2*pad - ks)/stride + 1.  ks in {1,3}; pad = ks/2; cin % 32 == 0, or cin == 4
 *   (conv1a, RGB + zero channel).  scale/shift = folded eval BatchNorm (NULL = identity). */
int pram_conv2d_nhwc_f32(const float* in, int batch, int h, int w, int cin, const float* wgt,
                         const float* bias, const float* scale, const float* shift,
                         const float* residual, float* out, int cout, int ks, int stride, int relu,
                         void* stream);

/* fp16-operand variant (BASELINE C5): wgt16 = [cout][ks][ks][cin] in fp16, cin % 64 == 0. */
int pram_conv2d_nhwc_f16_f32(const float* in, int batch, int h, int w, int cin, const void* wgt16,
                             const float* bias, const float* scale, const float* shift,
                             const float* residual, float* out, int cout, int ks, int stride, int relu,
                             void* stream);

/* Split-fp16 ("x3") variant (see pram_linear_x3_f32): wgt_hi / wgt_lo = [cout][ks][ks][cin] * w_scale as two fp16
 * planes, cin % 32 == 0; the im2col rows are split (s = 16) while they are staged.  fp32 in, fp32 out. */
int pram_conv2d_nhwc_x3_f32(const float* in, int batch, int h, int w, int cin, const void* wgt_hi, const void* wgt_lo,
                            float w_scale, const float* bias, const float* scale, const float* shift,
                            const float* residual, float* out, int cout, int ks, int stride, int relu, void* stream);

/* Grouped 3x3 convolution of the ResBlock (groups = 32, 8 ch/group; nets/sfd2.py:98-99,113-115).
 * w [c][3][3][c/groups]. */
int pram_conv3x3_grouped_nhwc_f32(const float* in, int batch, int h, int w, int c, const float* wgt,
                                  const float* scale, const float* shift, float* out, int groups,
                                  int relu, void* stream);

/* pram_conv2d_nhwc_x3_f32 followed, in the same kernel, by F.normalize over the channels of every output pixel (x / max(||x||, 1e-12)):
 * SFD2's descriptor head (convDb -> normalize, reference nets/sfd2.py:331-333) without the second pass over the map.  cout <= 128 (one
 * workgroup holds a pixel's whole channel vector), cin % 32 == 0.  The squared sums are added in another order than
 * pram_l2norm_rows_f32 adds them: the two agree to rounding, not bit for bit. */
int pram_conv2d_nhwc_x3_l2norm_f32(const float* in, int batch, int h, int w, int cin, const void* wgt_hi, const void* wgt_lo,
                                   float w_scale, const float* bias, const float* scale, const float* shift, const float* residual,
                                   float* out, int cout, int ks, int stride, int relu, void* stream);

/* pram_conv2d_nhwc_x3_f32 whose result leaves as the split operand of the next split-fp16 layer instead of fp32: out_hi =
 * fp16(s y), out_lo = fp16(s y - out_hi) (s = the activation scale in force, 16 by default), [batch][ho][wo][cout] each — the same four bytes per value, and the consumer needs
 * neither registers nor vector instructions to stage it (LDS-DMA).  cin % 32 == 0, cout even; |y| >= 4095 is reported through the
 * range guard (status word).  Used between a ResBlock's first 1x1 and its grouped 3x3. */
int pram_conv2d_nhwc_x3_planes(const float* in, int batch, int h, int w, int cin, const void* wgt_hi, const void* wgt_lo,
                               float w_scale, const float* bias, const float* scale, const float* shift, const float* residual,
                               void* out_hi, void* out_lo, int cout, int ks, int stride, int relu, void* stream);

/* The grouped 3x3 (8 channels per group) on the split-fp16 path: a block-diagonal product on the matrix pipe (a 32-channel block
 * is four groups; a 16-deep k-step carries one tap of two groups), the input taken as the planes above, windows double-buffered in
 * LDS by DMA under the MFMAs of a persistent workgroup per CU, weights in registers — the vector-ALU kernel above is bound by the
 * LDS broadcasts of its weights.  w_hi / w_lo: the [c][3][3][8] weights * w_scale as fp16 planes; c % 64 == 0.  fp32-class (three
 * fp16 products, fp32 accumulation): ~3e-7 relative from pram_conv3x3_grouped_nhwc_f32. */
int pram_conv3x3_grouped_planes_x3_f32(const void* in_hi, const void* in_lo, int batch, int h, int w, int c, const void* w_hi,
                                       const void* w_lo, float w_scale, const float* scale, const float* shift, float* out,
                                       int groups, int relu, void* stream);

/* SFD2's first two convolutions (nets/sfd2.py:135-139,281-282: conv1a 3 -> 64 3x3 stride 1, conv1b 64 -> 64 3x3 stride 2, each bias
 * -> BN -> ReLU) in ONE launch on the split-fp16 path: the 480 x 640 x 64 map between them (1.26 GB for 16 frames: the largest
 * round trip of the step) never exists — a workgroup computes the (2 * 8 + 1) x (2 * 16 + 1) window of conv1a outputs it needs
 * from the image, in LDS.  img: NHWC4 fp32 (pram_image_to_nhwc4_f32), or with img_nchw3 != 0 the reference's own NCHW layout
 * [batch][3][h][w] (the repack kernel is then not needed); out [batch][(h - 1) / 2 + 1][(w - 1) / 2 + 1][64].
 * wa: conv1a's [64][3][3][4] weights flattened to [64][36], zero-padded to [64][48], * wa_scale, as (hi, lo) fp16 planes;
 * wb: conv1b's [64][3][3][64] weights * wb_scale as (hi, lo) planes (the operand of pram_conv2d_nhwc_x3_f32); b? / s? / t?: bias and
 * eval-mode BatchNorm scale / shift of each layer.  fp32-class, not bit-identical to the two-kernel form (whose conv1a is the
 * exact-fp32 MFMA kernel). */
int pram_sfd2_conv1_x3_f32(const float* img, int batch, int h, int w, const void* wa_hi, const void* wa_lo, float wa_scale,
                           const float* ba, const float* sa, const float* ta, const void* wb_hi, const void* wb_lo, float wb_scale,
                           const float* bb, const float* sb, const float* tb, float* out, int img_nchw3, void* stream);

/* NCHW [b][3][h][w] -> NHWC4 [b][h][w][4] (zero 4th channel) */
int pram_image_to_nhwc4_f32(const float* img, float* out, int batch, int h, int w, void* stream);
/* NHWC [b][h][w][c] -> NCHW [b][c][h][w] (for the reference-layout dict entries); any extent = 0: PRAM_OK, nothing written */
int pram_nhwc_to_nchw_f32(const float* in, float* out, int batch, int h, int w, int c, void* stream);

/* softmax over 65 channels, drop dustbin, 8x8 depth-to-space (nets/sfd2.py:294-300; K2).
 * logits NHWC [b][hc][wc][65] -> score [b][8hc][8wc] */
int pram_score_map_f32(const float* logits, float* score, int batch, int hc, int wc, void* stream);

/* simple_nms (nets/sfd2.py:20-35; K3): 1 + 2 suppression rounds, window 2r+1 (r <= 4), exact equality.
 * workspace: pram_simple_nms_workspace_bytes (four fp32 images per frame); its contents on entry do not matter.
 * batch, h or w = 0: returns PRAM_OK, launches and writes nothing. */
size_t pram_simple_nms_workspace_bytes(int batch, int h, int w);
int pram_simple_nms_f32(const float* score, float* nms, int batch, int h, int w, int radius,
                        void* workspace, void* stream);

size_t pram_select_keypoints_workspace_bytes(int batch, int h, int w, int max_keypoints);

/* threshold / min-keypoint fallback / remove_borders / top-k (nets/sfd2.py:306-329,38-50; K4).
 * Canonical order: if more than max_keypoints candidates survive, (score desc, flat index asc);
 * otherwise row-major.  fallback_ref: -1 = each image tests its own count (per-query
 * semantics), >= 0 = every image uses that image's count (reference tests element 0).
 * kpts [b][max_keypoints][2] (x,y) fp32, scores [b][max_keypoints], counts [b].
 * max_keypoints > 0: up to 8192 the top-k is sorted in LDS, beyond that in the workspace (the reference has no bound,
 * nets/sfd2.py:38-50); >= h*w = keep all (the reference's max_keypoints < 0, nets/sfd2.py:324: row-major order, never sorted).
 * Rows of kpts / scores at and beyond counts[b] are not written.  batch, h or w = 0: returns PRAM_OK, launches and writes nothing,
 * counts included (there is no pixel to count). */
int pram_select_keypoints_f32(const float* nms, int batch, int h, int w, float conf_th,
                              int min_keypoints, int border, int max_keypoints, int fallback_ref,
                              float* kpts, float* scores, int* counts, void* workspace, void* stream);

/* sample_descriptors / ResNet4x.sample (nets/sfd2.py:53-64,348-369; K5): bilinear
 * grid_sample(align_corners=True, zero pad) of an NHWC map at keypoints, optional L2 norm,
 * optional per-pixel pre-normalisation of the map taps is NOT applied (pass a normalised map).
 * fmap [b][fh][fw][c]; kpts [b][n_max][2]; out [b][n_max][c].  c in {128, 256}. */
int pram_sample_nhwc_f32(const float* fmap, int batch, int fh, int fw, int c, const float* kpts,
                         const int* lens, int n_max, int s, int l2norm, float* out, void* stream);

/* ---- the descriptor head at the sampled pixels only.  A frame's keypoints read at most four map pixels each; the head's last two
 * layers (convDa.3, convDb + normalize) are row-wise independent, so they run on the list of those pixels instead of the map:
 * pram_sfd2_row_list -> pram_conv3x3_rows_x3_f32 -> pram_conv1x1_rows_x3_l2norm_f32 -> pram_sample_rows_f32 gives the bits of
 * pram_conv2d_nhwc_x3_f32 -> pram_conv2d_nhwc_x3_l2norm_f32 -> pram_sample_nhwc_f32.  No host synchronisation anywhere. */

/* The pixels pram_sample_nhwc_f32 would read for kpts [b][n_max][2] (lens [b] or NULL) on an fh x fw map at stride s — the same
 * coordinate arithmetic and validity tests, corners outside the map are not listed.  rows [b][rlen]: the distinct pixels
 * (y * fw + x) in ascending order, then -1;  n_rows [b]: how many;  pix2row [b][fh * fw]: a listed pixel's position in rows
 * (entries of other pixels are left as they are).  rlen >= min(4 n_max, fh * fw); fh * fw <= 2^18.  The layout is deterministic. */
int pram_sfd2_row_list(const float* kpts, const int* lens, int batch, int n_max, int fh, int fw, int s, int* rows,
                       int* n_rows, int* pix2row, int rlen, void* stream);

/* 3x3 / stride 1 split-fp16 convolution of in [batch][h][w][cin] at the listed pixels: out [batch * rlen][cout], row b * rlen + r =
 * pixel rows[b][r], bit for bit what pram_conv2d_nhwc_x3_f32 gives that pixel.  Tiles of 256 rows: a tile whose first row is
 * >= n_rows[b] is neither computed nor written; the dead rows of a partly live tile repeat the last live pixel.  rlen % 256 == 0,
 * cin % 32 == 0. */
int pram_conv3x3_rows_x3_f32(const float* in, int batch, int h, int w, int cin, const void* wgt_hi, const void* wgt_lo,
                             float w_scale, const float* bias, const int* rows, const int* n_rows, int rlen, float* out,
                             int cout, int relu, void* stream);

/* 1x1 split-fp16 convolution + F.normalize over the channels (pram_conv2d_nhwc_x3_l2norm_f32's arithmetic) of the rows matrix
 * in [batch * rlen][cin] -> out [batch * rlen][cout]; the rows of the 256-row tiles the producer skipped are neither read nor
 * written.  cout <= 128, cin % 32 == 0, rlen % 256 == 0. */
int pram_conv1x1_rows_x3_l2norm_f32(const float* in, int batch, int rlen, int cin, const void* wgt_hi, const void* wgt_lo,
                                    float w_scale, const float* bias, const int* n_rows, float* out, int cout, void* stream);

/* pram_sample_nhwc_f32 on a map that exists at the listed pixels only: rowmap [b * rlen][c], a tap at pixel p reads row
 * b * rlen + pix2row[b][p].  Same taps in the same order (nw, ne, sw, se), same weights, same normalisation. */
int pram_sample_rows_f32(const float* rowmap, const int* pix2row, int batch, int rlen, int fh, int fw, int c, const float* kpts,
                         const int* lens, int n_max, int s, int l2norm, float* out, void* stream);

/* F.normalize(x, dim=channel) of an NHWC map in place (nets/sfd2.py:333). rows = b*h*w */
int pram_l2norm_rows_f32(float* x, int rows, int cols, void* stream);

/* score lookup of ResNet4x.sample (nets/sfd2.py:367): out[b][i] = score_map[b*map_stride + y_i*w + x_i]
 * (map_stride = 0 reproduces the reference's score_map[0, ...]).  kpts [b][n_max][2], out [b][n_max]; lens [b] or NULL: frame b
 * has min(lens[b], n_max) live keypoints (a negative length: none), the rows of out beyond them are not written.  A keypoint
 * outside the map — x < 0, x >= w, y < 0, y >= h, tested on the float coordinates before the truncation, so a NaN is outside
 * too — scores 0; nothing is read for it. */
int pram_score_lookup_f32(const float* score_map, long long map_stride, int h, int w, const float* kpts,
                          const int* lens, int batch, int n_max, float* out, void* stream);

/* ---------------------------------------------------------------- edges of the path ("next" rows) */

/* F.interpolate(mode='bilinear', align_corners=True) on planar maps [planes][h][w] -> [planes][oh][ow]
 * (score map of frames whose sides are not multiples of 8, nets/sfd2.py:301-303; multi-scale
 * extraction nets/sfd2.py:412-415). */
int pram_resize_bilinear_f32(const float* in, float* out, int planes, int h, int w, int oh, int ow,
                             void* stream);

/* Recogniser epilogue (Frame.add_segmentations, localization/frame.py:96-121): per token
 * seg_scores = softmax(logits) (optional output), non_bg_mask = seg_scores[0] < bg_threshold,
 * seg_ids = argmax(logits) - 1 (first occurrence), n_non_bg[b] = sum(non_bg_mask). */
int pram_seg_epilogue_f32(const float* logits, const int* lens, int batch, int n_max, int n_class,
                          float bg_threshold, float* seg_scores, int* seg_ids, int* non_bg_mask,
                          int* n_non_bg, void* stream);

/* torch.topk(x, k = cols, dim = -1) = full descending sort of each row (MultiMap3D.process_segmentations,
 * localization/multimap3d.py:348-350); ties in canonical (value desc, index asc) order. cols <= 1024. */
int pram_row_sort_desc_f32(const float* x, int ld, int rows, int cols, float* vals, long long* idx,
                           void* stream);

/* Landmark vote of MultiMap3D.process_segmentations (localization/multimap3d.py:348-379) on the sorted class lists of
 * pram_row_sort_desc_f32 (sorted_ids / sorted_vals [n][c], c <= 1024): rank by rank, the landmarks that tokens put at sorted
 * position k — background 0 and landmarks seen at an earlier rank skipped — ordered by token count (descending, ties by
 * ascending id), until `topk` are collected.  Outputs (device): win_sid / win_rank / win_count [topk], *n_win, the winners'
 * tokens in ascending order tokens [topk][n] (first win_count[w] of row w valid) and the mean of their rank-k scores. */
int pram_seg_vote(const long long* sorted_ids, const float* sorted_vals, int n, int c, int topk, int* win_sid, int* win_rank,
                  int* win_count, int* n_win, int* tokens, float* mean_score, void* stream);

/* Row top-2 of a batched matrix (largest = 1: sim.topk(2), nearest_neighbor.py:5-17; largest = 0:
 * topk(largest=False), singlemap3d.py:428).  v0/v1 best and second best values, i0 index of the best
 * (lowest index on ties).  x [batch][m_max][ld]. */
int pram_row_top2_f32(const float* x, int ld, long long stride, const int* row_lens, const int* col_lens,
                      int batch, int m_max, int n_max, int largest, float* v0, float* v1, long long* i0,
                      void* stream);

/* Projection-refinement matching (SingleMap3D.refine_pose_by_projection, singlemap3d.py:416-433):
 * dist[i][j] = sqrt(2 - 2*sim[i][j] + 1e-6) + (||kpts[i] - proj_uv[:, j]|| >= range ? 100 : 0); per query
 * row the two smallest distances d0 <= d1 and the index of d0.  sim [m][ld] (= q_descs @ ref_descs^T),
 * kpts [m][2], proj_uv [2][n] (u row then v row). */
int pram_proj_dist_top2_f32(const float* sim, int ld, const float* kpts, const float* proj_uv, int m, int n,
                            float range, float* d0, float* d1, long long* i0, void* stream);

/* The same with the projected points in float64 (what the reference actually holds: it projects in float64, so the pixel
 * error and its `>= 2 * threshold` test are float64): proj_uv = [2][ldu] doubles, first n columns valid. */
int pram_proj_dist_top2_f64uv(const float* sim, int ld, const float* kpts, const double* proj_uv, int ldu, int m, int n,
                              double range, float* d0, float* d1, long long* i0, void* stream);

/* Projection of the map points into the query camera + frustum test + ordered compaction
 * (SingleMap3D.refine_pose_by_projection, localization/singlemap3d.py:405-415), float64 like the reference:
 *   p = K (Tcw [X 1])[:3];  u = p0 / p2,  v = p1 / p2;  keep = 0 < p2 < 100, 0 <= u < im_w, 0 <= v < im_h.
 * xyz [n][3]; K [3][3], Tcw [4][4] row-major (device); uvd [3][n] = u, v, depth of EVERY point; mask [n] int32;
 * keep_idx [n] = original indices of the survivors in their original order, uv_keep [2][n] their (u, v) (first *count
 * columns valid); count = number of survivors (device int). */
int pram_project_points_f64(const double* xyz, const double* K, const double* Tcw, int n, double im_w, double im_h,
                            double* uvd, int* mask, int* keep_idx, double* uv_keep, int* count, void* stream);

/* Per-layer bookkeeping of the batched AdaGML loop (nets/adagml.py:352-380 per pair; here `pairs` pairs at once, no host read):
 * commits the pruned token counts (lens_new / n_below of pram_adagml_prune_f32; NULL on layer 0) for the still-active pairs,
 * evaluates check_if_stop (adagml.py:522-531: 1 - below / (m + n) > 0.95, fp32) — every active pair stops when `last` — and lets the
 * pairs that stop here commit lens_final / ind_final / stop_layer.  Token sets 0..pairs-1 are the query sets, pairs..2*pairs-1 the
 * reference sets.  Outputs: lens_out (current counts), lens_stop (counts of the pairs stopping at this layer, 0 elsewhere: the
 * ragged out_proj GEMM), lens_eff (counts of the pairs still active afterwards, 0 elsewhere: the next layer).  The *_in / *_out
 * state buffers must differ (ping-pong). */
int pram_adagml_layer_state(const int* active_in, int* active_out, const int* lens_in, int* lens_out, const int* lens_new,
                            const int* n_below, const float* num_points, int* tiny, int* stop_layer, int* lens_final,
                            int* lens_stop, int* lens_eff, const int* ind, int* ind_final, int pairs, int t_max, int layer,
                            int last, void* stream);
/* score4[token] = (col_self, col_cross, 0, 0): the two attention scores per token the pooling head reads (adagml.py:132). */
int pram_adagml_scores4_f32(const float* col_self, const float* col_cross, float* score4, long long tokens, void* stream);
/* pram_adagml_prune_f32 with the logits at a stride (column 0 of the pooling head's padded [rows][4] output). */
int pram_adagml_prune_ld_f32(const float* conf_logit, int ld_logit, float thr, int n_min_tokens, const int* lens_in,
                             const float* x_in, const float* cos_in, const float* sin_in, const int* ind_in,
                             float* x_out, float* cos_out, float* sin_out, int* ind_out, int* lens_out,
                             int* n_below, float* conf_out, int* row_map, int sets, int t_max, int ldx, void* stream);

/* ---------------------------------------------------------------- MLP tail as a GEMM pair with the LayerNorm between them
 * Linear -> LayerNorm -> GELU -> Linear (+ residual): the tail of every attention block (nets/segnetvit.py:87-95,104-106;
 * nets/gml.py:118-126,151-162), SegNetViT's seg / sc heads (segnetvit.py:157-172) — without a stand-alone LayerNorm + GELU pass
 * over the hidden layer.  The first GEMM's weights are centred over its outputs on the host (w[j] - mean_j w[j], b[j] - mean b:
 * LayerNorm is invariant to the shift), so its output is h - mean(h); it also writes the rows' sums of squares, one partial per
 * 64-column block (row_ssq [parts][m], parts = pram_linear_x3_ssq_parts(m, n, k0 + k1) = ceil(n / 64); the consumer adds them in
 * ascending order, so the statistics do not depend on the tile configuration a launch picked).  The second GEMM applies
 * GELU(hidden * rstd * gamma + beta), rstd = 1 / sqrt(sum_p row_ssq[p][row] / k + eps), to its A operand while staging it
 * (GELU = t Phi(t) through a degree-7 fit of the Gaussian tail, |error| <= 7.5e-8 |t|).  Split-fp16 path; lens / t_pad as pram_linear_x3_ragged_f32. */
int pram_linear_x3_ssq_parts(int m, int n, int k);
int pram_linear_x3_ssq_f32(const float* a0, int lda0, int k0, const float* a1, int lda1, int k1, const void* w_hi, const void* w_lo,
                           float w_scale, const float* bias, float* out, int ldo, float* row_ssq, int m, int n,
                           const int* lens, int t_pad, void* stream);
int pram_linear_x3_lngelu_f32(const float* hidden, int ldh, int k, const void* w_hi, const void* w_lo, float w_scale, const float* bias,
                              const float* residual, int ldr, float* out, int ldo, int m, int n, const float* ln_ssq, int parts,
                              const float* gamma, const float* beta, float eps, const int* lens, int t_pad, void* stream);

/* Fixed-size per-query result record rec [batch][k][6] fp32 = x, y, score, landmark id, match index, match score — what the
 * single all-gather of the query-sharded job carries (the reference hands the same fields to its pose solver,
 * localization/singlemap3d.py:155-170).  landmark (int32 [batch][k]) and matches0 / mscores0 (int64 / fp32 [batch][km], km <= k:
 * only the first km keypoints of a query went through the matcher) may be NULL: 0, and -1 / 0 beyond km. */
int pram_pack_record_f32(const float* kpts, const float* scores, const int* landmark, const long long* matches0,
                         const float* mscores0, int batch, int k, int km, float* rec, void* stream);

/* Frame staging — replaces, per query frame, `torch.from_numpy(img / 255).permute(2, 0, 1).cuda().float()` followed by
 * `tvf.Normalize(mean, std)` (localization/loc_by_rec_online.py:98-106, nets/sfd2.py:14-17): frames_hwc3 = uint8 [batch][h][w][3] as
 * cv2.imread delivers them (channel order untouched, like the reference), lut = fp32 [3][256] with lut[c][v] = ((v / 255) - mean[c]) /
 * std[c] computed by the caller with the reference's own operations, out = fp32 [batch][3][h][w].  h * w a multiple of 4. */
int pram_stage_frames_u8(const void* frames_hwc3, const float* lut, float* out_nchw, int batch, int h, int w, void* stream);

/* dst[0 .. count) <- value, 32-bit words, on the stream (torch.zeros / torch.full of the host-side glue without a framework kernel). */
int pram_fill_u32(void* dst, unsigned int value, size_t count, void* stream);

/* ---------------------------------------------------------------- candidate-landmark matching: vote -> pairs -> 2D-3D matches
 * The loop of MultiMap3D.run (localization/multimap3d.py:110-145) around SingleMap3D.localize_with_ref_frame
 * (singlemap3d.py:127-162) for a whole batch of queries, without the host: for each of the seg_k best-voted landmarks of a query
 * (pram_seg_vote) decide the two keypoint sets (pram_cand_plan), fill the grouped matcher's inputs (pram_cand_gather), and turn
 * its matches0 into correspondences (pram_cand_correspond).  pairs = batch * seg_k, pair p = query p / seg_k, candidate p % seg_k.
 *
 * Reference store (one map; pram_amd/localization/candidates.py::ReferenceStore builds it): the reference frames' rows
 * concatenated in their original order, frame f = rows frame_off[f] .. frame_off[f + 1]: r_desc [rows][128], r_kpts [rows][2],
 * r_scores [rows], r_xyz [rows][3] float64, r_point3d_ids [rows] int64, r_segs [rows] int32 (in-map landmark of the row's 3D point);
 * frame_norm [frames][3] = (cx, cy, scale) of normalize_keypoints for the frame's camera; per in-map landmark l: lm_frame[l] (its
 * reference frame, -1 = none) and the rows of that frame with r_segs == l, in their original order, as sel_rows[lm_sel_off[l] ..
 * + lm_sel_len[l]] (RefFrame.get_keypoints_by_sid, refframe.py:34-43); per frame the label histogram hist_label / hist_cnt
 * [hist_off[f] .. hist_off[f + 1]] (distinct r_segs values of the frame and how many rows carry each).
 *
 * Plan table: int32 [PRAM_CAND_PLAN_COLS][pairs] (one contiguous column per field, so lens0 / lens1 go to the matcher as they are) = query, global landmark id (vote id - 1; -1 = no candidate), reference frame
 * (-1 = none: an empty pair), semantic flag, lens0, lens1, offset of the pair's token list in `tokens` (-1 = all keypoints of the
 * query in order), first row of the frame, offset of the pair's row list in sel_rows (-1 = the whole frame in order), vote order. */
#define PRAM_CAND_PLAN_COLS 10

/* sorted_ids [batch][n][c] (pram_row_sort_desc_f32 over a batch of padded queries): the ids of the rows t >= counts[b] become 0
 * at every rank — such a token names only the background, which is never a candidate, so pram_seg_vote(n) over the padded query
 * equals the vote over its first counts[b] tokens and its token lists keep the common stride n. */
int pram_cand_mask_ranks(long long* sorted_ids, const int* counts, int batch, int n, int c, void* stream);

/* One workgroup per (query, candidate).  win_sid / win_count [batch][seg_k], n_win [batch]: pram_seg_vote's outputs (topk = seg_k)
 * per query; seg_ids [batch][n] = pram_seg_epilogue_f32's (argmax - 1), counts [batch] keypoints per query.  multimap3d.py:114-139:
 * landmark = vote id - 1, in-map id = landmark - start_sid, its reference frame; semantic = semantic_matching && tokens >=
 * min_kpts && check_semantic_consistency (singlemap3d.py:513-532: labels present on both sides, min of the two sides' shares
 * >= overlap_ratio, float64); query side = the voted tokens when semantic, else all keypoints; reference side = the frame's rows of
 * that landmark when semantic and in-map id > 0 (singlemap3d.py:130), else the whole frame.  Candidates beyond n_win[b] and
 * landmarks without a reference frame give lens0 = lens1 = 0. */
int pram_cand_plan(const int* win_sid, const int* win_count, const int* n_win, const int* seg_ids, const int* counts,
                   int batch, int n, int n_class, int seg_k, const int* lm_frame, const int* lm_sel_off,
                   const int* lm_sel_len, int n_landmarks, int start_sid, const int* frame_off, const int* hist_off,
                   const int* hist_label, const int* hist_cnt, int n_frames, int min_kpts, double overlap_ratio,
                   int semantic_matching, int* plan, void* stream);

/* pram_cand_plan over the tables of SEVERAL maps (pram_amd/localization/multimap.py::MultiMapStore; MultiMap3D.run picks the map
 * by sid_scene_name[sid] and the in-map id by scene_name_start_sid, multimap3d.py:119-123): lm_frame / lm_sel_off / lm_sel_len
 * [n_landmarks] are indexed by the GLOBAL landmark id g = vote id - 1 (frames and rows numbered over all maps), and lm_start[g] is
 * the start_sid of the map that owns g, so in-map id = g - lm_start[g] and the frame's labels are compared as hist_label +
 * lm_start[g].  g outside [0, n_landmarks), lm_frame[g] < 0 (no map owns g, or no reference frame) and lm_frame[g] >= n_frames
 * give the empty pair.  Everything else, the checks and statuses included, as pram_cand_plan; the sid column stays g. */
int pram_cand_plan_maps(const int* win_sid, const int* win_count, const int* n_win, const int* seg_ids, const int* counts,
                        int batch, int n, int n_class, int seg_k, const int* lm_frame, const int* lm_sel_off,
                        const int* lm_sel_len, int n_landmarks, const int* lm_start, const int* frame_off, const int* hist_off,
                        const int* hist_label, const int* hist_cnt, int n_frames, int min_kpts, double overlap_ratio,
                        int semantic_matching, int* plan, void* stream);

/* The grouped matcher's inputs from the plan, one wave per row: desc0 / desc1 [pairs][t_pad][128], scores0 / scores1
 * [pairs][t_pad], nkpts0 / nkpts1 [pairs][t_pad][2] = keypoints already normalised per pair, (k - (cx, cy)) / scale in fp32 (the
 * operation order of pram_fourier_encoding_f32): the query side with (q_cx, q_cy, q_scale), the reference side with its frame's
 * frame_norm.  Rows at and beyond a pair's lens are written as zeros.  Query side from the extractor's batched outputs q_desc
 * [batch][n][128], q_kpts [batch][n][2], q_scores [batch][n]; tokens = pram_seg_vote's [batch][seg_k][n].  The descriptor buffers
 * must be 16-byte aligned; t_pad >= every lens0 / lens1 of the plan (rows beyond t_pad are not written). */
int pram_cand_gather(const int* plan, const int* tokens, const int* sel_rows, const float* q_desc, const float* q_kpts,
                     const float* q_scores, int n, const float* r_desc, const float* r_kpts, const float* r_scores,
                     const float* frame_norm, int ref_rows, float q_cx, float q_cy, float q_scale, float* desc0, float* nkpts0,
                     float* scores0, float* desc1, float* nkpts1, float* scores1, int pairs, int t_pad, void* stream);

/* matches0 [pairs][ldm] (the matcher's, -1 = none; the first min(lens0, t0) entries of a row are read) -> per pair the matched
 * rows in ascending query position (indices0 >= 0, singlemap3d.py:156-162), out buffers [pairs][cap]...: m_kpt_ids int64 (index
 * into the query's full keypoint list), m_kpts [..][2] (q_kpts rows, pixels), m_ref_kpts [..][2], m_point3d_ids int64, m_xyz
 * [..][3] float64 (copied bit for bit), m_sids int32 (r_segs), m_count [pairs].  A match index outside [0, lens1) is dropped. */
int pram_cand_correspond(const long long* matches0, int ldm, const int* plan, const int* tokens, const int* sel_rows,
                         const float* q_kpts, int n, const float* r_kpts, const double* r_xyz, const long long* r_point3d_ids,
                         const int* r_segs, int ref_rows, int pairs, int t0, int cap, long long* m_kpt_ids, float* m_kpts,
                         float* m_ref_kpts, long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_count, void* stream);

/* ---------------------------------------------------------------- batched absolute pose: P3P RANSAC, refinement, selection
 * What SingleMap3D.localize_with_ref_frame asks of pycolmap.absolute_pose_estimation (singlemap3d.py:168-193) and the candidate
 * loop's verify_and_update with its early exit (multimap3d.py:183-239, 294-313), for all pairs of a batch at once, straight from
 * pram_cand_correspond's padded outputs: m_kpts [pairs][t0][2] float32 (pixels; + 0.5 is added here, as every call site of the
 * reference does), m_xyz [pairs][t0][3] float64, count [pairs] (rows at and beyond count[p] are never read).  pairs = batch *
 * seg_k, pair p = query p / seg_k.  float64 arithmetic throughout; every loop has a compile-time or argument-given bound.
 *
 * Cameras: one row per query, cam_model [batch] int32 (COLMAP's model ids below) and cam_params [batch][PRAM_POSE_CAM_PARAMS]
 * float64 in COLMAP's parameter order, zero padded: SIMPLE_PINHOLE f cx cy, PINHOLE fx fy cx cy, SIMPLE_RADIAL f cx cy k,
 * RADIAL f cx cy k1 k2, OPENCV fx fy cx cy k1 k2 p1 p2.
 *
 * The sampler is a pure function of (seed, p, trial, draw): with sm64(x) = { x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) *
 * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31; } on uint64, key = sm64(sm64(seed) ^ (p << 32
 * | trial)) and word(draw) = sm64(key + draw).  With n = count[p]: i0 = mulhi64(word(0), n), i1 = mulhi64(word(1), n - 1), i2 =
 * mulhi64(word(2), n - 2) (mulhi64 = the high 64 bits of the 128-bit product); i1 += (i1 >= i0); lo = min(i0, i1), hi = max(i0,
 * i1); i2 += (i2 >= lo); i2 += (i2 >= hi).
 *
 * Workspaces (the caller allocates; nothing is allocated here): norm_pts pairs * t0 * 2 doubles; poses pairs * trials * 48
 * doubles; n_sol pairs * trials ints; h_inliers pairs * trials * 4 ints; h_resid pairs * trials * 4 doubles; best pairs ints. */
#define PRAM_CAM_SIMPLE_PINHOLE 0
#define PRAM_CAM_PINHOLE 1
#define PRAM_CAM_SIMPLE_RADIAL 2
#define PRAM_CAM_RADIAL 3
#define PRAM_CAM_OPENCV 4
#define PRAM_POSE_CAM_PARAMS 8
#define PRAM_POSE_UNDISTORT_STEPS 10

/* One thread per (pair, row < count): norm_pts [pairs][t0][2] = the keypoint + 0.5 on the normalised camera plane; distorted
 * models are inverted by PRAM_POSE_UNDISTORT_STEPS Newton steps on COLMAP's distortion function.  cam_model_host: a HOST copy of
 * cam_model, checked here without touching the device: an id outside the five models above -> PRAM_E_UNSUPPORTED. */
int pram_pose_prepare(const float* m_kpts, const int* count, const int* cam_model, const double* cam_params,
                      const int* cam_model_host, int batch, int seg_k, int t0, double* norm_pts, void* stream);

/* One thread per (pair, trial): three distinct rows below count[p] from the sampler above, then P3P by Grunert's quartic (the
 * law-of-cosines system reduced to one quartic in the distance ratio v = s3 / s1; Ferrari's closed form, then 3 Newton steps per
 * root) and the rigid motion from the three point pairs.  poses [pairs][trials][4][12] (row-major R | t, cam_from_world; the
 * first n_sol slots hold solutions, the rest zeros), n_sol [pairs][trials].  count < 3, collinear or duplicate triples: n_sol =
 * 0; a root that puts a point behind the camera is dropped.  triples (may be NULL) [pairs][trials][3]: the sampled rows. */
int pram_pose_hypotheses(const double* norm_pts, const double* m_xyz, const int* count, int pairs, int t0, int trials,
                         unsigned long long seed, double* poses, int* n_sol, int* triples, void* stream);

/* One workgroup per (pair, 16 trials): rows through LDS in chunks of 768 (30 KB, always chunked), each wave takes 4 trials in
 * turn per chunk, the 4 slots of a trial in registers.  Squared reprojection error on the normalised plane; inlier if <= (threshold_px / mean focal)^2 and depth
 * > 0.  h_inliers [pairs][trials * 4] (-1 = empty slot), h_resid = sum of the inliers' squared errors.  Then per pair best [pairs]
 * = the slot with (most inliers, then smaller residual sum, then smaller index), -1 if every slot is empty. */
int pram_pose_score(const double* norm_pts, const double* m_xyz, const int* count, const double* poses, const int* n_sol,
                    const int* cam_model, const double* cam_params, int pairs, int seg_k, int t0, int trials,
                    double threshold_px, int* h_inliers, double* h_resid, int* best, void* stream);

/* One workgroup per pair.  From the best hypothesis: refine_iters Levenberg-Marquardt iterations (initial damping 1e-3, x 0.1
 * on an accepted step, x 10 otherwise) over rotation (left axis-angle increment) and translation on the hypothesis' inliers,
 * residuals in pixels through the full camera model, Cauchy loss of scale 1 px as weights 1 / (1 + r^2); re-score all rows,
 * refine again on the new inliers, re-score.  A refined pose with fewer inliers than the hypothesis had is discarded for the
 * hypothesis.  qvec [pairs][4] (w, x, y, z; w >= 0), tvec [pairs][3], inliers [pairs][t0] bytes, num_inliers, success [pairs].
 * count < 3, best < 0 or a best support below max(3, min_inlier_ratio * count): success = 0 and zeros everywhere. */
int pram_pose_refine(const float* m_kpts, const double* norm_pts, const double* m_xyz, const int* count, const double* poses,
                     const int* h_inliers, const int* best, const int* cam_model, const double* cam_params, int pairs, int seg_k,
                     int t0, int trials, double threshold_px, double min_inlier_ratio, int refine_iters, double* qvec, double* tvec,
                     unsigned char* inliers, int* num_inliers, int* success, void* stream);

/* One thread per query over its seg_k candidates in vote order: a failed candidate is skipped; a successful one is kept if none
 * is kept yet or the kept one has fewer inliers; the walk stops at the first with num_inliers >= min_inliers.  chosen [batch][3]
 * = kept candidate (-1 = none), tracking status (1 = a candidate reached min_inliers, 0 = some succeeded, -1 = none did), order
 * of the kept candidate (the reference's ret['order'], the position in the vote: by construction the same number as column 0;
 * kept as a column of its own so that the row reads like the reference's result). */
int pram_pose_select(const int* success, const int* num_inliers, int batch, int seg_k, int min_inliers, int* chosen, void* stream);

/* ---------------------------------------------------------------- pose refinement by matching over covisible frames
 * SingleMap3D.refine_pose_by_matching (singlemap3d.py:268-365) for a whole batch of located queries: ALL keypoints of a query are
 * matched against the WHOLE of each frame covisible with the localisation's reference frame, the matches are stacked in list
 * order with the localisation's own matches last, one pose is estimated on the stack, and find_reference_frames (singlemap3d.py:
 * 500-511) votes for the new reference frames.  A refinement pair is a row of the plan table above with token offset -1 and
 * sel_rows offset -1, so pram_cand_gather and pram_cand_correspond run on pram_refine_plan's table unchanged (they take the
 * query from the plan's column), and pram_pose_* run on pram_refine_merge's list with seg_k = 1.  refine pairs = batch * n_cov,
 * pair p = query p / n_cov, slot p % n_cov.
 *
 * Store tables (ReferenceStore builds them): the covisibility graph in CSR form, covis_frames[covis_off[f] .. covis_off[f + 1]]
 * = the frames sharing most points with frame f in (count descending, frame index ascending), empty for a frame that is no
 * landmark's reference frame ("vrf"), n_covis entries in all; the point table pt_ids [n_points] int64 (sorted, unique, no -1)
 * with pt_frames[pt_off[i] .. pt_off[i + 1]] = the frames observing point i (duplicates counted), n_entries in all; is_vrf
 * [n_frames] int32.  Every index read from a table is checked against the size given beside it before it is used.
 *
 * One thread per (query, slot).  chosen [batch][3] = pram_pose_select's; loc_plan = the localisation's plan table [..][batch *
 * seg_k] (its frame and sid columns at pair b * seg_k + kept); counts [batch]; enable [batch] (NULL = every located query).
 * plan [PRAM_CAND_PLAN_COLS][batch * n_cov]: query b, the kept candidate's sid, frame = entry j of the covisible list of the
 * kept candidate's frame (the list cut to n_cov), semantic 0, lens0 = counts[b], lens1 = the frame's rows, token offset -1,
 * first row of the frame, sel offset -1, order j; beyond the list, for a query that is not located (kept < 0) or not enabled:
 * frame -1 and lens0 = lens1 = 0.  Per query ref_frame (store index of the kept candidate's frame, -1 = not refined),
 * n_cov_used (slots in use) and init_on = 1 iff tracking status is 1 and the reference frame is in its own (cut) list — then
 * singlemap3d.py:273-278 keeps the localisation's matches, and, its remove() acting on a copy, matches the frame again. */
int pram_refine_plan(const int* chosen, const int* loc_plan, const int* counts, const int* enable, const int* frame_off,
                     const int* covis_off, const int* covis_frames, int batch, int seg_k, int n_cov, int n_frames, int n_covis,
                     int* plan, int* ref_frame, int* n_cov_used, int* init_on, void* stream);

/* One workgroup per query.  r_*: pram_cand_correspond's outputs for the refinement pairs, [batch * n_cov][t0]... with r_count;
 * a_*: the same for the localisation's pairs, [batch * seg_k][t0a]... with a_count.  Per query ONE list [batch][cap]..., cap >=
 * n_cov * t0 + t0a: the slots in ascending order, inside a slot the order pram_cand_correspond left, then (init_on[b]) the rows
 * of the kept candidate.  m_kpt_ids int64, m_kpts / m_ref_kpts [..][2], m_point3d_ids int64, m_xyz [..][3] float64 (copied as
 * 64-bit words), m_sids, m_src int32 (slot of origin; n_cov = the localisation's), m_count [batch].  Offsets = the exclusive scan
 * of the counts; an empty slot costs one load; rows at and beyond m_count[b] are not written. */
int pram_refine_merge(const long long* r_kpt_ids, const float* r_kpts, const float* r_ref_kpts, const long long* r_point3d_ids,
                      const double* r_xyz, const int* r_sids, const int* r_count, int t0, const long long* a_kpt_ids,
                      const float* a_kpts, const float* a_ref_kpts, const long long* a_point3d_ids, const double* a_xyz,
                      const int* a_sids, const int* a_count, int t0a, const int* chosen, const int* init_on, int batch,
                      int seg_k, int n_cov, int cap, long long* m_kpt_ids, float* m_kpts, float* m_ref_kpts,
                      long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_src, int* m_count, void* stream);

/* find_reference_frames, one workgroup per query: over the rows r < m_count[b] of m_point3d_ids [batch][cap] — those with
 * inliers [batch][cap] != 0 when success[b], all of them otherwise (singlemap3d.py:353-359) — the point id is looked up in pt_ids
 * by binary search (an unknown id votes for nothing) and every entry of its frame list that is_vrf gets + 1 by an integer atomic
 * in hist [batch][n_frames], a workspace of the caller in global memory which the entry zeroes (no limit on the map's size from
 * LDS).  Then k selection rounds over the histogram: best_frames [batch][k] = the first k frames in (count descending, frame
 * index ascending) with count > 0, -1 padded, best_counts [batch][k] (0 padded), n_best [batch].  1 <= k <= n_frames. */
int pram_refine_frame_vote(const long long* m_point3d_ids, const int* m_count, const unsigned char* inliers, const int* success,
                           int batch, int cap, const long long* pt_ids, const int* pt_off, const int* pt_frames, int n_points,
                           int n_entries, const int* is_vrf, int n_frames, int k, int* hist, int* best_frames, int* best_counts,
                           int* n_best, void* stream);

/* ---------------------------------------------------------------- pose refinement by projection over covisible frames
 * SingleMap3D.refine_pose_by_projection (singlemap3d.py:367-498) for a whole batch of located queries, on the localisation's
 * device-side state (chosen, loc_plan and the per-pair qvec / tvec of pram_pose_refine) and the store's tables above plus the
 * per-point values aligned with pt_ids: pt_xyz [n_points][3] float64, pt_desc [n_points][128] float32, pt_sid [n_points] int32
 * (point3Ds[pid].xyz / .descriptor / .seg_id).  Four entries, run in this order; pram_pose_* (seg_k = 1) and
 * pram_refine_frame_vote then run on pram_projref_correspond's lists unchanged.  n_points >= 1 everywhere.
 *
 * Deviations: a row whose point id is -1 or is not in pt_ids marks nothing (the reference raises KeyError at :392); the
 * reference's in-place append of the reference frame to its graph list (:381) is not reproduced, the frame is one more slot.
 *
 * singlemap3d.py:378-387.  Grid (n_cov + 1, batch), one workgroup per (slot, query), threads over the rows of the slot's frame.
 * Slots j < n_cov: entry j of the covisible list of the kept candidate's frame, the list cut to n_cov (chosen, loc_plan, enable,
 * covis_* as in pram_refine_plan); slot n_cov: that frame itself when the cut list does not hold it (:380-381).  Every row's
 * point id (point3d_ids [n_rows], rows frame_off[g] .. frame_off[g + 1]) is looked up in pt_ids by binary search and its bit set
 * in bitmap [batch][ceil(n_points / 32)] (bit i & 31 of word i >> 5), which the entry zeroes, by an integer atomic OR.  A query
 * that is not located or not enabled marks nothing; ref_frame [batch] = the kept frame's store index, or -1. */
int pram_projref_mark(const int* chosen, const int* loc_plan, const int* enable, const int* frame_off, const int* covis_off,
                      const int* covis_frames, const long long* point3d_ids, const long long* pt_ids, int batch, int seg_k,
                      int n_cov, int n_frames, int n_covis, int n_rows, int n_points, unsigned int* bitmap, int* ref_frame,
                      void* stream);

/* singlemap3d.py:369-377, 387-415.  One workgroup per query: the marked points in ascending table index (= ascending point id,
 * np.unique's order at :387), n_union [batch] of them; each projected in float64, p = K (R X + t) in pram_project_points_f64's
 * operation order, R from qvec [batch * seg_k][4] (w, x, y, z) by qvec2rotmat's formula in its operation order and t = tvec
 * [batch * seg_k][3] of pair b * seg_k + chosen[b][0]; K from cam_model / cam_params [batch][PRAM_POSE_CAM_PARAMS] by
 * Frame.get_intrinsics' mapping (frame.py:154-175: f, cx, cy for SIMPLE_PINHOLE, SIMPLE_RADIAL, RADIAL; fx, fy, cx, cy for
 * PINHOLE, OPENCV; no distortion, :401).  Kept: 0 < p2 < 100, 0 <= u < width, 0 <= v < height with image_size [batch][2] int32
 * (width, height).  Ordered compaction into cand_pt [batch][cap] (point-table indices), cand_uv [batch][2][cap] (u row, v row),
 * n_cand [batch].  cap >= the marked points of any query (min(n_points, (n_cov + 1) * the largest frame) always is; marks beyond
 * cap are dropped).  Entries of cand_pt / cand_uv at and beyond n_cand[b] are unspecified. */
int pram_projref_project(const unsigned int* bitmap, int n_points, const double* pt_xyz, const int* chosen, const double* qvec,
                         const double* tvec, const int* cam_model, const double* cam_params, const int* image_size, int batch,
                         int seg_k, int cap, int* cand_pt, double* cand_uv, int* n_union, int* n_cand, void* stream);

/* singlemap3d.py:423-437, fused: no [keypoints][candidates] matrix is written.  One wave per (query b, keypoint i < n); a keypoint
 * i >= counts[b] gets best -1, d0 = d1 = +inf, accept 0.  Over the query's candidates c < n_cand[b] in ascending order: the pixel
 * error sqrt((kx - u)^2 + (ky - v)^2) in float64, the float32 keypoint (q_kpts [batch][n][2]) widened first; c is in range when
 * that error is NOT >= 2 * threshold.  For in-range candidates only: sim = the 128-term fp32 dot product of q_desc [batch][n][128]
 * row i with pt_desc row cand_pt[b][c] in ONE fixed order — lane l of the wave forms (q[2l] * r[2l]) + (q[2l + 1] * r[2l + 1]),
 * then the 64 lane values are summed by a butterfly, lane l adding the value of lane l ^ 32, then ^ 16, 8, 4, 2, 1 — and
 * d = sqrtf((2 - 2 sim) + 1e-6f); top-2 update with strict <, so the lowest index wins ties.  best [batch][n] = the candidate
 * index of the smallest d (-1: none in range), d0 / d1 [batch][n] the smallest and second smallest (+inf where there is none),
 * accept [batch][n] = 1 iff n_cand[b] >= 2 and (exactly one candidate is in range, or two or more and d0 / d1 <= 0.995f).
 * Those are the reference's decisions: an out-of-range candidate carries + 100 there, so it never displaces an in-range one from
 * the top-2, and against it the ratio is at most about 0.02.  threshold > 0, finite. */
int pram_projref_match(const float* q_kpts, const float* q_desc, const int* counts, int batch, int n, const int* cand_pt,
                       const double* cand_uv, const int* n_cand, int cap, const float* pt_desc, int n_points, double threshold,
                       int* best, float* d0, float* d1, unsigned char* accept, void* stream);

/* singlemap3d.py:446-450.  One workgroup per query: the accepted keypoints i < counts[b] in ascending index, in
 * pram_cand_correspond's layout with n rows per query: m_kpt_ids [batch][n] int64, m_kpts [batch][n][2] float32, m_point3d_ids
 * [batch][n] int64 (pt_ids), m_xyz [batch][n][3] float64 (pt_xyz, copied as 64-bit words), m_sids [batch][n] int32 (pt_sid),
 * m_count [batch]; rows at and beyond m_count[b] are not written. */
int pram_projref_correspond(const unsigned char* accept, const int* best, const int* counts, const float* q_kpts, int batch, int n,
                            const int* cand_pt, const int* n_cand, int cap, const long long* pt_ids, const double* pt_xyz,
                            const int* pt_sid, int n_points, long long* m_kpt_ids, float* m_kpts, long long* m_point3d_ids,
                            double* m_xyz, int* m_sids, int* m_count, void* stream);

/* ---------------------------------------------------------------- tracking the last frame, for a batch of streams
 * Tracker.track_last_frame (localization/tracker.py:162-233), Frame.initialize_localization_variables / update_point3ds
 * (frame.py:84-89, 191-195) and the hand-over mTracker.last_frame = curr_frame (loc_by_rec_online.py:193-197) for n_slots
 * independent streams.  The state (pram_amd/localization/tracker.py::TrackState owns it) holds the last frame of every stream,
 * slot s = rows s * n_max .. s * n_max + n_max of st_kpts [..][2], st_scores, st_desc [..][128] (16-byte aligned), st_xyz [..][3]
 * float64, st_point3d_ids int64 (-1 = the row has no point), st_segs int32, with st_counts [n_slots] (rows in use), st_ref_frame
 * [n_slots] (store index of the frame's reference frame) and st_frame_norm [n_slots][3] (normalize_keypoints' constants of the
 * frame's camera).  slot [batch] names the state slot of query b (-1 = none; a value outside [0, n_slots) counts as none).  A
 * tracking pair is a row of the plan table above with the slot in its frame column, so pram_cand_gather runs on
 * pram_track_plan's table unchanged with the state's arrays as r_desc / r_kpts / r_scores / frame_norm and ref_rows = n_slots *
 * n_max, and pram_pose_* (seg_k = 1) run on pram_track_correspond's lists.  float64 is moved as 64-bit words; every index read
 * from a table is checked against the size given beside it before it is used.
 *
 * One thread per pair; counts [batch] keypoints per query (stride n).  plan [PRAM_CAND_PLAN_COLS][batch]: query b, sid -1, frame
 * = slot[b], semantic 0, lens0 = counts[b], lens1 = st_counts[slot[b]], token offset -1, first row slot[b] * n_max, sel offset
 * -1, order 0; a query without a slot: frame -1, lens0 = lens1 = 0.  loc_plan: the same table with frame = st_ref_frame[slot[b]]
 * — the one-pair-per-query localisation plan pram_refine_plan and pram_projref_mark read (seg_k = 1).  The padded size of the
 * grouped matcher call, max(64, round_up(max(n, n_max), 64)), is known on the host: no table is read back. */
int pram_track_plan(const int* counts, const int* slot, const int* st_counts, const int* st_ref_frame, int batch, int n,
                    int n_slots, int n_max, int* plan, int* loc_plan, void* stream);

/* tracker.py:195-205.  One workgroup per pair (pairs = batch, pair p = query p).  matches0 [pairs][ldm] (-1 = none; the first
 * min(lens0, t0) entries of a row are read) -> the query rows i with 0 <= j = matches0[p][i] < lens1 AND st_point3d_ids[slot][j]
 * >= 0, in ascending i (ordered compaction by ballot and prefix), in pram_cand_correspond's layout [pairs][cap]...: m_kpt_ids
 * int64 (= i), m_kpts (q_kpts [batch][n][2] rows), m_ref_kpts (the last frame's keypoints), m_point3d_ids, m_xyz (bit for
 * bit), m_sids (st_segs), m_count [pairs].  Rows at and beyond cap are dropped; rows at and beyond m_count[p] are not written. */
int pram_track_correspond(const long long* matches0, int ldm, const int* plan, const float* q_kpts, int n, const float* st_kpts,
                          const double* st_xyz, const long long* st_point3d_ids, const int* st_segs, int n_slots, int n_max,
                          int pairs, int t0, int cap, long long* m_kpt_ids, float* m_kpts, float* m_ref_kpts,
                          long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_count, void* stream);

/* tracker.py:154-160 (ret[...][inliers]).  One workgroup per query: of the first count[b] rows of the six lists [batch][cap]...
 * those with mask [batch][cap] != 0 (bytes), in order, into lists of the same layout, with o_count [batch].  The outputs must
 * not be the inputs; rows at and beyond o_count[b] are not written. */
int pram_track_filter(const long long* kpt_ids, const float* kpts, const float* ref_kpts, const long long* point3d_ids,
                      const double* xyz, const int* sids, const int* count, const unsigned char* mask, int batch, int cap,
                      long long* o_kpt_ids, float* o_kpts, float* o_ref_kpts, long long* o_point3d_ids, double* o_xyz,
                      int* o_sids, int* o_count, void* stream);

/* The located frame becomes its stream's last frame.  For every query b with a slot: (one wave per row, 16-byte loads) the
 * query's counts[b] keypoints, scores and descriptors (q_* [batch][n]..., n <= n_max) go to the slot's first rows; ALL n_max
 * rows of the slot get xyz 0 and point id -1; st_segs = seg_ids [batch][n] on the first counts[b] rows (NULL: -1) and -1 beyond;
 * st_counts = counts[b], st_ref_frame = ref_frame[b], st_frame_norm = (q_cx, q_cy, q_scale).  Then (one workgroup per query) the
 * list rows r < m_count[b] of m_* [batch][cap]... — with mask [batch][cap] non-NULL only those with mask != 0 — are scattered
 * to row m_kpt_ids[r] of the slot: xyz, point id and landmark.  A keypoint id outside [0, counts[b]) writes nothing.  Of the
 * rows naming one keypoint the LAST in list order writes (numpy's fancy assignment, frame.py:87-89), whatever the scheduling:
 * winner [batch][n] int32, a workspace of the caller which the entry sets to -1, takes an integer atomic max of r per keypoint
 * id, and after a workgroup barrier the row that equals its keypoint's winner writes.  Slots no query names are not touched,
 * rows at and beyond counts[b] keep their keypoints, scores and descriptors.  slot_host: a HOST copy of slot, checked here
 * without touching the device: a slot >= n_slots, or two queries naming one slot -> PRAM_E_ARG. */
int pram_track_commit(const float* q_kpts, const float* q_scores, const float* q_desc, const int* counts, const int* seg_ids,
                      const int* slot, const int* slot_host, const int* ref_frame, int batch, int n, float q_cx, float q_cy,
                      float q_scale, const long long* m_kpt_ids, const long long* m_point3d_ids, const double* m_xyz,
                      const int* m_sids, const int* m_count, const unsigned char* mask, int cap, float* st_kpts, float* st_scores,
                      float* st_desc, int* st_counts, double* st_xyz, long long* st_point3d_ids, int* st_segs, int* st_ref_frame,
                      float* st_frame_norm, int n_slots, int n_max, int* winner, void* stream);

/* ---- The query pre-filter (csrc/prefilter.hip; pram_amd/localization/localizer.py drives it): Frame.add_segmentations' optional
 * filtering of the query (frame.py:102-116) for a padded batch.  keypoints [batch][n][2], scores [batch][n], descriptors
 * [batch][n][desc_dim], logits [batch][n][n_class], and pram_seg_epilogue_f32's outputs at the filtering threshold: seg_ids,
 * non_bg_mask [batch][n], n_non_bg [batch]; counts [batch] real rows per query (clamped to [0, n]); enable = the threshold is
 * > 0.  Query b FIRES when enable != 0 and 5 * n_non_bg[b] >= 2 * counts[b] — frame.py:106's `>= 0.4 * n` in float64, which
 * this integer form equals for every n an int holds (csrc/prefilter.hip) — and then keeps the rows i < counts[b] with
 * non_bg_mask != 0, in their order; otherwise it keeps all counts[b] rows.  counts[b] == 0 fires (0 >= 0.0).  Outputs, out of
 * place, same shapes: the five row arrays compacted (kept rows bit for bit, NaN payloads and negative zeros included; rows j >=
 * o_counts[b] zero, o_seg_ids -2 there), o_counts [batch], kept [batch][n] = the input row of output row j (-1 for j >=
 * o_counts[b]), filtered [batch] = 1 where the query fired.  Every element of every output is written whatever the inputs hold
 * beyond counts[b].  One workgroup per query plans (ordered compaction by ballot and prefix), one wave per output row moves
 * (descriptors as 16-byte vectors: desc_dim % 4 == 0 and 16-byte aligned descriptor buffers; a logits row as 32-bit words, since
 * an odd n_class leaves it 4-byte aligned only).  No atomics, no host synchronisation.  batch == 0 or n == 0: PRAM_OK, nothing
 * is launched and nothing written (with n == 0 the caller owns o_counts = 0 and filtered = enable != 0). */
int pram_query_prefilter(const float* keypoints, const float* scores, const float* descriptors, const float* logits,
                         const int* seg_ids, const int* non_bg_mask, const int* n_non_bg, const int* counts, int enable, int batch,
                         int n, int n_class, int desc_dim, float* o_keypoints, float* o_scores, float* o_descriptors,
                         float* o_logits, int* o_seg_ids, int* o_counts, int* kept, int* filtered, void* stream);

/* ---- Map building (csrc/mapbuild.hip; pram_amd/localization/mapbuild.py drives these): the two inputs of a ReferenceStore that
 * the reference computes offline on the CPU (recognition/recmap.py).  Both take tables of the store as they lie on the device.
 * An offset table also comes as a HOST copy: the workspace size and the table's shape are checked from it without touching the
 * device, and nothing is read back. */
#define PRAM_MAPBUILD_SHORT_TRACK 32   /* tracks up to this many entries: Gram matrix and rank selection in LDS */
#define PRAM_MAPBUILD_ROW_LDS 512      /* longer tracks up to this many entries keep the current Gram row in LDS, beyond: workspace */
#define PRAM_MAPBUILD_MAX_VRF 64
#define PRAM_MAPBUILD_CAM_COLS 13      /* qw qx qy qz tx ty tz fx fy cx cy width height */

/* RecMap.assign_point3D_descriptor (recmap.py:124-194).  One workgroup per point p, whose track is the entries trk_off[p] ..
 * trk_off[p + 1] of trk_frame (store frame index; -1: an image the map does not hold) and trk_kpt (keypoint index inside the
 * frame).  An entry with frame -1, a frame outside [0, n_frames) or a keypoint outside its frame is dropped.  Over the kept
 * entries i: d_ij = 2 - 2 <a_i, a_j> in float64 (the products of the fp32 rows are exact and are added in one fixed order for
 * every pair — four dimensions to a lane in ascending order, then a butterfly over 32 lanes: d_ij == d_ji bit for bit), m_i = numpy's median of row i, and the FIRST i with the smallest
 * m_i is chosen.  pt_choice [n_points]: its position in the track, -1 when nothing was kept; pt_desc [n_points][128]: a bit copy
 * of its row of descriptors [n_rows][128] (16-byte aligned), zeros for -1.  Descriptors are finite.  workspace: 12 bytes per
 * entry up to the end of the last track longer than PRAM_MAPBUILD_SHORT_TRACK, as the size function says. */
size_t pram_mapbuild_desc_workspace_bytes(const int* trk_off_host, int n_points);
int pram_mapbuild_assign_descriptors(const float* descriptors, const int* frame_off, int n_frames, int n_rows, const int* trk_off,
                                     const int* trk_off_host, const int* trk_frame, const int* trk_kpt, int n_points, void* workspace,
                                     size_t workspace_bytes, float* pt_desc, int* pt_choice, void* stream);

/* find_best_vrf_by_covisibility with the filter of RecMap.create_virtual_frame_3 around it (recmap.py:263-355, 369-403).  One
 * workgroup per landmark l, whose points are lm_points[lm_off[l] .. lm_off[l + 1]) in the label file's order (ids the point
 * table lacks and repeated ids allowed).  point3d_ids [n_rows] / frame_off: the store's rows; pt_ids (ascending) / pt_off /
 * pt_frames / pt_xyz [n_points][3]: its point table; frame_ignored [n_frames]; frame_cams [n_frames][PRAM_MAPBUILD_CAM_COLS]
 * float64.  A frame's observation count is the number of its rows with id > 0.  Candidates: the frames listed by the landmark's
 * points that the table holds, minus ignored ones; those with count >= min_obs by count descending, then by first encounter in
 * the double loop over the points and each point's frame list, cut at topk_imgs; when no frame reaches min_obs every
 * encountered frame by first encounter.  A candidate's mask has a bit per list position whose id (> 0; a repeated id: its first
 * position) a row of the frame carries.  Greedy cover: the first candidate with the largest popcount(mask & unobserved), a gain
 * of 0 allowed; stop at coverage >= min_cover_ratio, after a pick with gain / len < gain_floor, at n_vrf picks or when no
 * candidate is left.  A picked frame is dropped unless a point of the list with id >= 0 that the table holds is a row of the
 * frame and K (R x + t) / z lies inside [0, width) x [0, height) (float64, no depth test).  lm_vrf [n_landmarks][n_vrf]: store
 * frame indices in pick order, padded with -1; lm_vrf_n [n_landmarks]. */
size_t pram_mapbuild_vrf_workspace_bytes(int n_landmarks, int n_lm_points, int n_frames);
int pram_mapbuild_select_frames(const long long* point3d_ids, const int* frame_off, int n_frames, int n_rows, const long long* pt_ids,
                                const int* pt_off, const int* pt_frames, int n_points, int n_entries, const double* pt_xyz,
                                const int* lm_off, const int* lm_off_host, const long long* lm_points, int n_landmarks,
                                const int* frame_ignored, const double* frame_cams, int min_obs, int topk_imgs, int n_vrf,
                                double min_cover_ratio, double gain_floor, void* workspace, size_t workspace_bytes, int* lm_vrf,
                                int* lm_vrf_n, void* stream);

/* ---- Map compression (csrc/compress.hip; pram_amd/localization/compress.py drives these): RecMap.compress_map_by_projection_v2
 * (recmap.py:668-922) and the rows RefFrame.associate_keypoints_with_point3Ds (refframe.py:99-147) gives a compressed frame.
 * Frames, rows and the point table are a ReferenceStore's, as they lie on the device; frame_cams as for map building.  Tables
 * the host walks to enqueue the steps come as HOST arrays; nothing is read back. */
#define PRAM_COMPRESS_ROW_TILE 256     /* candidate rows per workgroup of the test step */
#define PRAM_COMPRESS_KPT_TILE 256     /* kept keypoints of a chain frame per LDS tile */

/* One workspace serves the selection and the sparsification: 24 bytes per row, 4 (covisibility_frame + 1) + 16 besides. */
size_t pram_compress_workspace_bytes(int n_rows, int covisibility_frame);

/* Selection (recmap.py:695-828).  A row is valid when its id is not -1 and pt_ids (ascending) holds it.  vrf_host [n_vrf]: the
 * reference frames in order (a repeated one is taken again); covis_off_host [n_frames + 1] / covis_frames_host: every frame's
 * candidates in order, at most covisibility_frame each, at least one for every frame of vrf_host.  For each v of vrf_host: v is
 * retained with all its valid rows kept (over an earlier partial retention; its place in the retained order stays) and starts
 * the chain; then each candidate c != v in order: a retained c joins the chain; otherwise a valid row of c with xyz x is
 * discarded when for some chain frame k, p = R_k x + t_k, u = (fx p_x + cx p_z) / p_z, v likewise, 0 <= u < width,
 * 0 <= v < height, p_z > 0 and sqrt(dx * dx + dy * dy) <= radius for a KEPT row of k with keypoint xys [n_rows][2] (float64);
 * with a row left c is retained with the rows left and joins the chain, with none nothing happens.  A chain frame without kept
 * rows discards nothing; a candidate without valid rows is never retained.  Launches: one begin per v, a test (row tiles x
 * covisibility_frame + 1 chain slots) and a commit per candidate; the kernels read the state to decide what a step does; no
 * workgroup waits for another.  ret_order [n_frames]: the frame's place in the retained order, -1 when not retained; list_cnt
 * [n_frames] and list_pt [n_rows]: frame f's kept rows as indices into pt_ids, in row order, at list_pt[frame_off[f] ..]. */
int pram_compress_select(const long long* point3d_ids, const int* frame_off, const int* frame_off_host, int n_frames, int n_rows,
                         const long long* pt_ids, int n_points, const double* pt_xyz, const double* xys, const double* frame_cams,
                         const int* covis_off_host, const int* covis_frames_host, int covisibility_frame, const int* vrf_host,
                         int n_vrf, double radius, void* workspace, size_t workspace_bytes, int* ret_order, int* list_cnt,
                         int* list_pt, void* stream);

/* sparsify_by_grid (recmap.py:670-693, 852-860) in place on the lists of pram_compress_select, for every frame listing more
 * than nkpts points; one workgroup per frame.  A listed point projects with the frame's own pose (no in-image or depth test)
 * into cell iw = rint(u // radius), ih likewise (numpy's float floor division), key ih * ceil(width / radius) + iw in 64 bits.
 * Per key the highest pt_score [n_points] wins, the earlier position on a tie; the winners leave in the order in which their
 * keys first appear.  A point whose projection is not finite is dropped. */
int pram_compress_sparsify(const int* frame_off, int n_frames, int n_rows, const double* frame_cams, const double* pt_xyz,
                           const int* pt_score, int n_points, double radius, int nkpts, void* workspace, size_t workspace_bytes,
                           int* list_pt, int* list_cnt, void* stream);

/* The rows of the compressed frames: row i is point row_point[i] (an index into the point table) seen from frame row_frame[i].
 * out_kpts [n_out][3] float64: the projection and the score 1 / clip(5 pt_err, 1, 20); out_xyz, out_desc [n_out][128], out_sid,
 * out_ids: the point's values.  An index out of range gives zeros and id -1. */
int pram_compress_rows(const int* row_frame, const int* row_point, int n_out, int n_frames, int n_points, const double* frame_cams,
                       const long long* pt_ids, const double* pt_xyz, const float* pt_desc, const int* pt_sid, const double* pt_err,
                       double* out_kpts, double* out_xyz, float* out_desc, int* out_sid, long long* out_ids, void* stream);

/* ---- K-means labelling of a map's points (csrc/kmeans.hip; pram_amd/localization/labelling.py drives these): the labels that
 * RecMap.cluster(method='kmeans') (recmap.py:85-122) takes from sklearn's KMeans(n_clusters=k, random_state=0): k-means++
 * seeding, Lloyd iterations, sklearn's stopping rules and its relocation of empty clusters.  x [n][3] float64: the points as the
 * host centred them (sklearn subtracts the mean); centers [k][3] float64 in the same coordinates.  Every floating-point sum has
 * one fixed order, so a result is the same bits on every run and equals the numpy restatement tests/kmeans_ref.py:
 *   - distance ((x0 - c0)^2 + (x1 - c1)^2) + (x2 - c2)^2, products and sums written out; the lowest centre index wins a tie;
 *   - a sum over points cuts them into blocks of PRAM_KMEANS_BLOCK consecutive indices: inside a block the terms are added to 0.0
 *     in ascending index (cluster sums: per cluster), the block partials are added to 0.0 in ascending block index.  Results
 *     depend on PRAM_KMEANS_BLOCK.  No floating-point atomics; counts are integers.
 * Every entry refuses (PRAM_E_ARG) n < 1, k < 1, k > n, k > PRAM_KMEANS_MAX_K, a null or misaligned pointer (float64 buffers 8
 * bytes, the others 4), a workspace that is too small and n >= 2^31 (n travels as long long so that this is a refusal and not a
 * wrapped int).  Coordinates are finite.  No workgroup waits for another: every step is a launch of its own and
 * every loop is bounded by an argument. */
#define PRAM_KMEANS_BLOCK 1024         /* points per block of every reduction over points; the results depend on it */
#define PRAM_KMEANS_MAX_K 4096         /* the per-block histogram and cursors of the cluster sums are LDS tables of this size */
#define PRAM_KMEANS_MAX_TRIALS 10      /* candidates per k-means++ step: sklearn's 2 + int(ln k) is 10 at k = 4096 */
#define PRAM_KMEANS_STATE_WORDS 8      /* done, n_iter, strict, relocations, changed, three spare */

/* One workspace serves seeding and iterations.  0 for arguments the entries refuse. */
size_t pram_kmeans_workspace_bytes(long long n, int k);

/* sklearn's k-means++ (_kmeans_plusplus) with the host's random numbers: first: the first seed's index; rand [k - 1][n_trials]
 * float64 (device): the uniform numbers of every step, n_trials in [1, PRAM_KMEANS_MAX_TRIALS].  closest[i] is the squared
 * distance of point i to its nearest seed, pot its blocked sum.  A step's candidate t is the first i with
 * run[b] + within[i] >= rand[t] * pot, clipped to n - 1, where within is the running sum of closest inside block b and run the
 * running sum of the block totals; its potential is the blocked sum of min(closest[i], d2(x_i, x_cand)); the smallest potential
 * wins, the lowest t on a tie.  Three launches per step (pick the winner and the next targets' blocks: one workgroup; update
 * closest and walk the targets' blocks; the candidates' potentials per block), nothing is read back.  seeds [k] int32: the chosen
 * points; centers [k][3]: their coordinates. */
int pram_kmeans_init_pp(const double* x, long long n, int k, int first, const double* rand, int n_trials, void* workspace,
                        size_t workspace_bytes, int* seeds, double* centers, void* stream);

/* Lloyd iterations first_iter .. first_iter + n_iters - 1 on `centers` (in place), four launches each: assign every point (one
 * thread per point, the centres through LDS); the cluster sums and counts of every block (the block's points ordered by label in
 * LDS, stably, every run added in index order); the block partials added in block order; and one workgroup that relocates empty
 * clusters (ascending cluster index; each takes the next of the points farthest from their own centre, in descending distance,
 * lowest index on ties, which leaves its old cluster's sum and count), divides the sums by the counts (a cluster left without a
 * point keeps its sum), adds the squared centre moves in ascending index and decides: the labels equal the previous iteration's
 * (strict) -> done; else shift <= tol_abs -> done; else iteration max_iter - 1 -> done.  state [PRAM_KMEANS_STATE_WORDS] int32
 * (device) carries this between calls: state[0] done, [1] iterations run, [2] strict, [3] relocations so far; first_iter == 0
 * resets it.  Once done, the launches of later iterations return at once, so a caller enqueues iterations in groups and reads
 * state[0] once per group.  finish != 0 (after the iterations, valid once done is set): without strict convergence one more
 * assignment; labels [n] int32, dist [n] float64 (squared distance to the point's own centre; also the iterations' scratch) and
 * inertia [2] float64: the blocked sum of dist, and the last iteration's shift.  Nothing waits for the stream. */
int pram_kmeans_lloyd(const double* x, long long n, int k, double* centers, double tol_abs, int max_iter, int first_iter, int n_iters,
                      int finish, void* workspace, size_t workspace_bytes, int* labels, double* dist, int* state, double* inertia,
                      void* stream);

/* One assignment step: labels [n] int32 and dist [n] float64 of x against centers [k][3].  Needs no workspace. */
int pram_kmeans_assign(const double* x, long long n, const double* centers, int k, int* labels, double* dist, void* stream);

/* ---- triangulation (csrc/triangulate.hip): a map's points from pairwise matches and known poses ------------------------------
 * What localization/triangulation.py of the reference does with COLMAP: verify every pair's matches against the epipolar geometry
 * of the two known poses, join the kept matches into tracks, triangulate every track.  NOT COLMAP's incremental triangulator: a
 * batched one with fixed budgets (DESIGN.md 4.21 lists the deviations).  float64; nothing here has been timed.
 *
 * The stages share one frame table, laid out as the store's: keypoints [n_rows][2] float32 of all frames concatenated, frame_off
 * [n_frames + 1] int32; a "row" is a keypoint's index in it.  Cameras are per frame: cam_model [n_frames] (PRAM_CAM_*), cam_params
 * [n_frames][PRAM_POSE_CAM_PARAMS], cam_model_host a HOST copy the launcher validates (PRAM_E_UNSUPPORTED).  Poses are
 * cam_from_world: qvec [n_frames][4] (w, x, y, z; normalised inside), tvec [n_frames][3].  Every entry refuses (PRAM_E_ARG) a null
 * or misaligned pointer (float64 buffers 8 bytes, int32 4) and a negative size; none waits for the stream; a buffer of zero
 * logical length still needs a valid pointer. */
#define PRAM_TRI_GN_STEPS 5            /* Gauss-Newton steps of the point-only refit */
#define PRAM_TRI_FRAME_COLS 16         /* R [9] row-major, t [3], C = -R^T t [3], mean focal length */
#define PRAM_TRI_CC_STATE_WORDS 4      /* hooked this round, done, rounds run, spare */

/* table [n_frames][PRAM_TRI_FRAME_COLS]: what verification and triangulation read of a frame's pose and camera. */
int pram_tri_frames(const double* qvec, const double* tvec, const int* cam_model, const double* cam_params,
                    const int* cam_model_host, int n_frames, double* table, void* stream);

/* norm [n_rows][2]: every keypoint (x + pixel_offset, y + pixel_offset) through its frame's inverse camera model, with
 * pram_pose_prepare's undistortion (PRAM_POSE_UNDISTORT_STEPS Newton steps).  The reference verifies with offset 0 and
 * triangulates with offset 0.5. */
int pram_tri_normalize(const float* keypoints, const int* frame_off, const int* cam_model, const double* cam_params,
                       const int* cam_model_host, int n_frames, int n_rows, double pixel_offset, double* norm, void* stream);

/* pairs [n_pairs][2] frame indices; match_off [n_pairs + 1] and matches [n_matches][2] (keypoint index in frame 0, in frame 1):
 * the matches of every pair as CSR.  E = [t / |t|]x R of cam1_from_cam0; a match is kept when its two epipolar errors
 * (colmap_utils/geometry.py compute_epipolar_errors) are <= max_error / mean focal length of their frame.  keep [n_matches]: the
 * mask; kept [n_matches][2]: the kept matches of pair p in their original order from match_off[p] on, count [n_pairs] of them;
 * edges [n_matches][2]: the rows a kept match joins, (-1, -1) for a dropped one.  A match with an index outside its frame, and
 * every match of a pair that names a frame outside the table, is dropped without being dereferenced. */
int pram_tri_verify(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                    const double* table, int n_frames, int n_pairs, int n_matches, double max_error, unsigned char* keep,
                    int* kept, int* edges, int* count, void* stream);

/* Connected components over the rows with `edges` [n_edges][2] (an edge with an end outside [0, n_rows) is ignored): rounds
 * first_round .. first_round + n_rounds - 1 of (hook the larger root to the smaller with an atomic min; jump every pointer to its
 * root; close the round), three launches each.  first_round == 0 sets label[i] = i and clears state
 * [PRAM_TRI_CC_STATE_WORDS] (device): [0] hooked this round, [1] done, [2] rounds run.  Once done is set the launches of later
 * rounds return at once, so a caller enqueues rounds in groups and reads state[1] once per group.  At the end label[i] is the
 * smallest row of i's component, whatever order the atomics landed in.  n_rows <= 2^30, n_rounds <= 1024. */
int pram_tri_components(const int* edges, int n_edges, int n_rows, int first_round, int n_rounds, int* label, int* state,
                        void* stream);

/* The tracks of `label` as CSR: a track is a component of two rows or more, tracks in ascending label, entries in ascending row.
 * trk_off [n_rows / 2 + 2], trk_label [n_rows / 2 + 1], trk_row / trk_frame / trk_kpt [n_rows] are sized for the worst case;
 * sizes [2] (device) = (tracks, entries) says how much of them is written.  Counts, a scan over the labels, a cursor fill and a
 * bitonic sort of every track by one wave, in place: no cap on a track's length.  workspace: 256-byte aligned. */
size_t pram_tri_tracks_workspace_bytes(int n_rows);
int pram_tri_tracks(const int* label, const int* frame_off, int n_frames, int n_rows, void* workspace, size_t workspace_bytes,
                    int* trk_off, int* trk_label, int* trk_row, int* trk_frame, int* trk_kpt, int* sizes, void* stream);

/* One wave per track (trk_off [n_tracks + 1], trk_label [n_tracks], trk_row / trk_frame [n_entries]; norm: pram_tri_normalize
 * with the offset 0.5).  Hypotheses: every pair of entries in lexicographic order when there are at most `trials`, else `trials`
 * pairs from the pose stage's sampler keyed by (seed, trk_label, trial), smaller entry first; a pair of one frame is skipped.  A
 * hypothesis is the midpoint of the two rays, refused when a depth is not positive or the rays meet below min_tri_angle
 * (radians); its score is the number of entries with positive depth and a reprojection error (pixels, full camera model, keypoint
 * + 0.5) <= max_reproj_error, which must be 2 at least; most inliers win, then the smaller sum of squared errors, then the lower
 * index (best [n_tracks], -1: none).  Refit on the winner's inliers: the least-squares point of their rays, then
 * PRAM_TRI_GN_STEPS Gauss-Newton steps on the pixel error (a step that is not finite or not positive definite is not taken).
 * Inliers are marked again at the refit point; of a frame's several inliers the one with the smallest error stays, the lowest
 * row on a tie.  accept [n_tracks]: two kept entries at least and some two of them seeing the point under min_tri_angle or
 * more; xyz [n_tracks][3]; error [n_tracks]: the mean reprojection error of the kept entries; kept [n_tracks]: their number;
 * entry_keep [n_entries] uint8; entry_error [n_entries]: the final inliers' error in pixels, -1 for the others.  An entry naming
 * a row or frame outside the tables is never an inlier. */
int pram_tri_triangulate(const double* norm, const float* keypoints, const double* table, const int* cam_model,
                         const double* cam_params, const int* trk_off, const int* trk_label, const int* trk_row,
                         const int* trk_frame, int n_tracks, int n_entries, int n_frames, int n_rows, int trials,
                         unsigned long long seed, double min_tri_angle, double max_reproj_error, int* accept, double* xyz,
                         double* error, int* kept, int* best, unsigned char* entry_keep, double* entry_error, void* stream);

/* Stage 2b, between pram_tri_verify and pram_tri_components: a match joins the track graph only when observations of third frames
 * agree with it.  pram_tri_adjacency builds the rows' adjacency over `edges` [n_edges][2] as CSR: adj_off [n_rows + 1], adj
 * [2 * n_edges] of which adj_off[n_rows] entries are written, every row's list ascending with duplicates kept, and row_frame
 * [n_rows], each row's frame.  An edge counts when both ends are in [0, n_rows) and differ; any other, (-1, -1) included, is
 * skipped and never dereferenced.  Degrees by integer atomics, a scan, a cursor fill and the tracks' sort of every list: the
 * table is a function of the set of edges alone; no cap on a degree.  n_edges < 2^30, n_rows <= 2^30; workspace: 256-byte
 * aligned.  Without edges adj_off is all zero and adj is not touched. */
size_t pram_tri_adjacency_workspace_bytes(int n_rows, int n_edges);
int pram_tri_adjacency(const int* edges, int n_edges, const int* frame_off, int n_frames, int n_rows, void* workspace,
                       size_t workspace_bytes, int* adj_off, int* adj, int* row_frame, void* stream);

/* One wave per edge (u, v).  support [n_edges] is 0 for an edge that does not count or whose rows share a frame.  Otherwise a
 * witness is a distinct row w of adj(u) or adj(v) other than u and v, in a frame that is neither u's nor v's; a row in both
 * lists, or twice in one, is one witness.  Of the pairs (u, v), (u, w), (v, w) the one whose rays (norm: offset 0.5) meet under
 * the largest angle is taken, the first in that order on a tie; below min_tri_angle (radians) w does not confirm; X is the
 * midpoint of that pair's rays as pram_tri_triangulate forms a hypothesis; w confirms when u, v and w all have positive depth at
 * X and a reprojection error (pixels, full camera model, keypoint + 0.5) <= max_reproj_error.  support counts the confirming
 * witnesses; edges_out [n_edges][2] is the edge where support >= min_support and (-1, -1) elsewhere, the layout
 * pram_tri_components takes.  adj_off is clamped into [0, 2 * n_edges] and a w outside [0, n_rows) or with a frame outside the
 * table is skipped, so a caller's own table cannot lead out of bounds.  Integer counts only: the result repeats bit for bit. */
int pram_tri_support(const double* norm, const float* keypoints, const double* table, const int* cam_model,
                     const double* cam_params, const int* edges, int n_edges, const int* adj_off, const int* adj,
                     const int* row_frame, int n_frames, int n_rows, double min_tri_angle, double max_reproj_error,
                     int min_support, int* support, int* edges_out, void* stream);

/* Between one round's pram_tri_triangulate and the next round's pram_tri_components: what a round left over becomes the next
 * round's match graph.  state [n_rows] holds one byte per row, PRAM_TRI_ROW_*; first == 1 sets every row DEAD before anything
 * else.  Marking, one thread per entry of the round's track table (trk_off [n_tracks + 1], trk_row [n_entries]) with its results
 * (accept [n_tracks], entry_keep [n_entries] of pram_tri_triangulate): the entry's row becomes TAKEN when its track was accepted
 * and the entry kept, FREE when the track was accepted and the entry not kept, DEAD when the track was not accepted (it would
 * come back identical).  The thread finds its track by bisection in trk_off; offsets are clamped into [0, n_entries], an entry
 * outside its track's clamped range and a row outside [0, n_rows) are skipped.  A table of pram_tri_tracks holds a row once, so
 * every byte has one writer; in a caller's table that names a row twice one of the writes stays.  Filtering, one thread per edge
 * of `edges` [n_edges][2]: edges_out [n_edges][2] is the edge when both ends are in [0, n_rows) and FREE, and (-1, -1)
 * otherwise; n_live [1] (device) counts the survivors, by a ballot per wave and one integer atomic.  Bytes and integers only:
 * the result repeats bit for bit.  n_entries, n_rows <= 2^30, n_edges < 2^30. */
#define PRAM_TRI_ROW_FREE 0
#define PRAM_TRI_ROW_TAKEN 1
#define PRAM_TRI_ROW_DEAD 2
int pram_tri_split(const int* trk_off, const int* trk_row, int n_tracks, int n_entries, const int* accept,
                   const unsigned char* entry_keep, const int* edges, int n_edges, int n_rows, int first, unsigned char* state,
                   int* edges_out, int* n_live, void* stream);

/* ---- two-view geometry without poses (csrc/twoview.hip; pram_amd/localization/twoview.py drives these) ------------------------
 * The other branch of the reference's triangulation.main (estimation_and_geometric_verification, pycolmap.verify_matches): per
 * pair an essential matrix by RANSAC over five-point samples, the mask of the matches that agree with it and the relative pose it
 * decomposes to.  NOT COLMAP's estimator: a fixed trial budget, the calibrated case only, no local optimisation (DESIGN.md 4.24
 * lists the deviations).  float64; profiles/twoview_timing.md has the time of every stage.
 *
 * The entries read the triangulation's frame table and match layout: norm [n_rows][2] is pram_tri_normalize with the offset 0.5,
 * frame_off [n_frames + 1], pairs [n_pairs][2] frame indices, match_off [n_pairs + 1] and matches [n_matches][2] the matches as
 * CSR, cam_model [n_frames] / cam_params [n_frames][PRAM_POSE_CAM_PARAMS] the cameras (a model id outside PRAM_CAM_* reads as
 * SIMPLE_PINHOLE; pram_tri_normalize has refused it before).  Index rules, in every entry: match_off is clamped into
 * [0, n_matches]; a pair naming a frame outside [0, n_frames) has no usable match; a match with an index outside its frame is
 * never dereferenced, is no inlier of anything, and a sample that draws it yields no hypothesis.  E is row-major with
 * x1^T E x0 = 0 for x0 = (u0, v0, 1) of frame 0 and x1 of frame 1.  Every entry refuses (PRAM_E_ARG) a null or misaligned pointer
 * (float64 8 bytes, int32 4), n_pairs > 65535, trials outside [1, 2^20] and a negative size; none waits for the stream. */
#define PRAM_TWOVIEW_MAX_SOL 10        /* real solutions of a five-point sample */

/* One lane per (pair, trial), the trial's working set in LDS ([element][lane], 141312 bytes of dynamic LDS per wave).  Sampler:
 * key = sm64(sm64(seed) ^ ((first_pair + p) << 32 | trial)) with splitmix64's output function sm64 (pram_pose_hypotheses');
 * pick k = 0 .. 4 is mulhi64(sm64(key + k), n - k), n the pair's clamped match count, then stepped over the earlier picks in
 * ascending order (+1 for every earlier pick <= it): five distinct indices below n.  first_pair is the position of pairs[0] among
 * all processed pairs, so a batch cut into chunks draws what the whole batch draws.  Solver: the null space of the 5 x 9
 * epipolar system by Gauss-Jordan with complete pivoting (rank-deficient when a pivot falls below 1e-10 of the first), the ten
 * cubic constraints det E = 0 and 2 E E^T E - tr(E E^T) E = 0 as a 10 x 20 matrix in Nister's column order, Gauss-Jordan with
 * partial pivoting, the degree-10 polynomial det B(z) of the hidden variable z, its real roots in ascending order by 48
 * bisection steps each on the Sturm count inside the Cauchy bound, 4 Newton steps on det B(z), (x, y) from the null vector of
 * B(z).  A root is kept when E is finite and |det E| and every entry of 2 E E^T E - tr(E E^T) E are <= 1e-6 at |E|_F = 1.
 * E [n_pairs][trials][PRAM_TWOVIEW_MAX_SOL][9]: Frobenius-normalised, the kept roots first, zeros behind; n_sol
 * [n_pairs][trials]; fives [n_pairs][trials][5] (may be NULL): the sampled match indices, -1 when n < 5.  n_sol = 0 for n < 5, a
 * sample naming an unusable match, a rank-deficient sample (duplicates) and a chain that is not finite. */
int pram_twoview_hypotheses(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                            int n_frames, int n_pairs, int n_matches, int first_pair, int trials, unsigned long long seed,
                            double* E, int* n_sol, int* fives, void* stream);

/* Every slot against every match of its pair: the squared Sampson error on the normalised plane, an inlier when it is <=
 * (max_error * 0.5 * (1 / f0 + 1 / f1))^2 with f the mean focal length of each frame's camera; no cheirality.  h_inliers
 * [n_pairs][trials][PRAM_TWOVIEW_MAX_SOL] (-1 for a slot >= n_sol), h_resid (same shape): the sum of the inliers' errors; best
 * [n_pairs]: the slot with most inliers, then the smaller sum, then the smaller index (-1: no slot).  The matches go through LDS
 * in chunks of 768 whatever their number; sums are per lane in ascending order and combined by the wave's butterfly. */
int pram_twoview_score(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                       const int* cam_model, const double* cam_params, int n_frames, int n_pairs, int n_matches, const double* E,
                       const int* n_sol, int trials, double max_error, int* h_inliers, double* h_resid, int* best, void* stream);

/* One workgroup per pair.  The best E is decomposed into its four (R, t) (t: the largest cross product of two columns; R =
 * cof(E') -+ [t]x E', E' = sqrt(2) E, re-orthonormalised to det R = +1), the one with most inliers at positive depth in both
 * frames is taken (lowest index on a tie), refined by refine_iters Levenberg-Marquardt iterations over 5 parameters (a left
 * axis-angle increment on R, two tangent directions of the unit sphere for t; Cauchy weights of scale 1 pixel on the signed
 * Sampson distance; pram_pose_refine's damping and acceptance rule), inliers marked again, refined again; a refined model with
 * fewer inliers than the hypothesis had is dropped for the hypothesis.  success [n_pairs]: the pair has 5 matches at least, some
 * trial gave a solution and the final support is >= max(min_num_inliers, min_inlier_ratio * count).  E_out [n_pairs][9]
 * (Frobenius norm 1), qvec [n_pairs][4] (w, x, y, z; w >= 0), tvec [n_pairs][3] (unit; frame 1 from frame 0), num_inliers,
 * num_front [n_pairs] (the inliers at positive depth in both frames); keep / kept / edges / count: pram_tri_verify's outputs
 * under the final E.  A failed pair has zeros everywhere, keeps no match and has count 0. */
int pram_twoview_finish(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* matches,
                        const int* cam_model, const double* cam_params, int n_frames, int n_pairs, int n_matches, const double* E,
                        const int* h_inliers, const int* best, int trials, double max_error, double min_inlier_ratio,
                        int min_num_inliers, int refine_iters, double* E_out, double* qvec, double* tvec, int* num_inliers,
                        int* num_front, int* success, unsigned char* keep, int* kept, int* edges, int* count, void* stream);

/* ---- statistical outlier removal of a map's points (csrc/knn.hip; pram_amd/localization/outliers.py drives these) -------------
 * What RecMap.remove_statics_outlier (recmap.py:43-61) takes from Open3D's PointCloud::RemoveStatisticalOutliers, written from
 * knowledge of its source and NOT pinned to it (Open3D was never run beside this).  x [n][3] float64.
 *   1. for every point i its kk = min(k, n) nearest points, ITSELF INCLUDED at distance 0; avg[i] is the mean of the kk Euclidean
 *      distances.  The search is all-pairs and exact.  Ties at the kk-th distance do not matter: the multiset of the kk smallest
 *      distances is unique.  No neighbour index is returned;
 *   2. a point is valid when avg[i] > 0 (a point with kk - 1 exact duplicates or more is not); nv is the number of valid points;
 *   3. over the valid points mean = sum(avg) / nv, std = sqrt(sum((avg - mean)^2) / (nv - 1)), threshold = mean + std_ratio * std;
 *   4. the inliers are the valid points with avg[i] < threshold (strict), in ascending index.  With nv < 2 there is no threshold
 *      (std and threshold are NaN) and no point is an inlier.
 * One fixed arithmetic, so a result is the same bits on every run and equals the numpy restatement tests/outliers_ref.py:
 *   - d2 = (dx * dx + dy * dy) + dz * dz with dx = x[j] - x[i], products and sums written out;
 *   - a point's kk smallest d2 in ascending order, each square-rooted, added to 0.0 in that order, the sum divided by (double)kk;
 *   - the two sums over points follow the k-means rule above with blocks of PRAM_SOR_BLOCK consecutive indices: inside a block the
 *     terms are added to 0.0 in ascending index (an invalid point contributes nothing), the block sums are added to 0.0 in
 *     ascending block index; two passes, the mean first, then the squared deviations (d * d with d = avg - mean).  Results depend
 *     on PRAM_SOR_BLOCK.  No floating-point atomics; counts are integers.
 * Both entries refuse (PRAM_E_ARG) n < 1, n >= 2^31 (n travels as long long so that this is a refusal and not a wrapped int), a
 * null or misaligned pointer (float64 buffers and the workspace 8 bytes, int32 4); k > n is allowed (kk is the algorithm's own
 * rule).  Coordinates are finite: a NaN d2 fails every `<`, so a candidate with a non-finite coordinate is never kept and a
 * query with one keeps nothing finite (its avg is then inf or NaN, which is not an inlier); pram_amd's Python layer refuses such
 * input before it gets here.  Nothing waits for the stream. */
#define PRAM_KNN_TILE 1024             /* candidates per LDS tile of the all-pairs search: three planes of float64 */
#define PRAM_KNN_MAX_K 32              /* a thread's sorted list of smallest d2 lives in registers: this many entries at most */
#define PRAM_SOR_BLOCK 1024            /* points per block of the two sums over points; the results depend on it */

/* avg [n] float64: step 1.  One thread per query point, the candidates streamed through LDS in tiles of PRAM_KNN_TILE.  Refuses
 * k < 1 and k > PRAM_KNN_MAX_K as well.  Needs no workspace. */
int pram_knn_mean_distance(const double* x, long long n, int k, double* avg, void* stream);

/* 0 for an n the entries refuse. */
size_t pram_sor_workspace_bytes(long long n);

/* Steps 2 to 4 on avg [n]: stats [4] float64 = (mean, std, threshold, nv); mask [n] uint8 (1: inlier); inlier_idx [n] int32: the
 * inliers' indices in ascending order, entries beyond the count unspecified; count [2] int32 = (inliers, nv).  nv == 0 gives a
 * NaN mean too.  Refuses a std_ratio that is not > 0 and a workspace that is too small. */
int pram_sor_select(const double* avg, long long n, double std_ratio, void* workspace, size_t workspace_bytes, double* stats,
                    unsigned char* mask, int* inlier_idx, int* count, void* stream);

/* ---- localisation against retrieved database frames (csrc/retrieval.hip; pram_amd/localization/retrieval.py drives these) -----
 * The reference's offline localizer (localization/pose_estimator.py): every (query, retrieved frame) pair is a plan row of the
 * candidate stage — all keypoints of the query against the frame's rows that carry a 3D point.  The store adds valid_rows [n_valid]
 * / valid_off [n_frames + 1]: per frame the rows (indices into the concatenated arrays, original order) whose point id is not -1
 * and is in the point table pt_ids.  pram_cand_gather and pram_cand_correspond run on pram_retr_plan's table unchanged when they
 * are handed valid_rows as sel_rows; pram_refine_merge with init_on all 0 stacks a query's slots; pram_pose_* solve either the
 * stack (seg_k = 1) or every pair (seg_k = n_db).  Every entry refuses (PRAM_E_ARG) a null or misaligned pointer and a negative
 * size; nothing waits for the stream and nothing is allocated. */

/* retrieval [batch][n_db] store frame indices (-1 padded), counts [batch] query keypoints, enable [batch] or null -> plan
 * [PRAM_CAND_PLAN_COLS][batch * n_db].  A live slot: query b, sid -1, frame, semantic 0, lens0 = counts[b], lens1 = the frame's valid
 * rows, tok_off -1, row0 = frame_off[frame], sel_off = valid_off[frame], order = slot.  An empty pair (frame -1, both lengths 0,
 * row0 0, sel_off -1): a slot < 0 or >= n_frames, a frame without valid rows (pose_estimator.py:65-66), counts[b] <= 0, enable[b]
 * == 0.  The covisibility stage is planned by the same entry: its retrieval list is pram_covis_topk's.  Needs n_db > 0. */
int pram_retr_plan(const int* retrieval, const int* counts, const int* enable, const int* frame_off, const int* valid_off,
                   int batch, int n_db, int n_frames, int n_valid, int* plan, void* stream);

/* Per pair, the rows of pram_cand_correspond's list [pairs][t0] whose point has obs_th observations or more
 * (pose_estimator.py:122), in their order, into m_* [pairs][t0]; m_count [pairs].  Observations of a point: pt_off[i + 1] - pt_off[i]
 * (duplicates counted), 0 for an id pt_ids does not hold; obs_th <= 0 keeps every row.  Rows beyond m_count are not written.  The
 * output must not be the input. */
int pram_retr_filter(const long long* r_kpt_ids, const float* r_kpts, const float* r_ref_kpts, const long long* r_point3d_ids,
                     const double* r_xyz, const int* r_sids, const int* r_count, int pairs, int t0, const long long* pt_ids,
                     const int* pt_off, int n_points, int obs_th, long long* m_kpt_ids, float* m_kpts, float* m_ref_kpts,
                     long long* m_point3d_ids, double* m_xyz, int* m_sids, int* m_count, void* stream);

/* pose_estimator_iterative's choice among a query's slots (pose_estimator.py:429-556, 558) from the per-pair success, num_inliers
 * and filtered count [batch][n_db]: walk the slots in order, pass over count < 8 or success == 0, remember as best the strictly
 * largest num_inliers above 0 (the first wins a tie), accept the first slot with num_inliers >= inlier_th; with none accepted
 * the best is taken when its num_inliers >= min_best_inliers.  chosen [batch][3] = (kept slot or -1, status 1 accepted / 2 best
 * taken / 0 failed, best slot met up to the end of the walk or -1).  Needs n_db > 0. */
int pram_retr_select(const int* success, const int* num_inliers, const int* count, int batch, int n_db, int inlier_th,
                     int min_best_inliers, int* chosen, void* stream);

/* get_covisibility_frames (pose_estimator.py:18-42) for n store frames at once: for every valid row of frames[s], every entry of
 * its point's frame list counts once (duplicates counted), the frame itself only with include_self != 0.  best_frames
 * [n][k] (-1 padded), best_counts [n][k] (0 padded), n_found [n]; order: count descending, then store frame index ascending, at the
 * cut too.  A frames[s] outside [0, n_frames) finds nothing.  hist [n][n_frames] int32 is the caller's workspace, zeroed by the
 * entry.  Needs k >= 1 (k may exceed n_frames) and n_frames >= 1. */
int pram_covis_topk(const int* frames, int n, const int* valid_off, const int* valid_rows, const long long* point3d_ids, int n_rows,
                    int n_valid, const long long* pt_ids, const int* pt_off, const int* pt_frames, int n_points, int n_entries,
                    int n_frames, int k, int include_self, int* hist, int* best_frames, int* best_counts, int* n_found,
                    void* stream);

/* ---- bundle adjustment (csrc/bundle.hip): a map's poses refined with its points --------------------------------------------
 * Levenberg-Marquardt over the frames' poses (cam_from_world, the tangent of pram_pose_refine: R <- exp([w]x) R, t <- t + d) and
 * the points (additive), intrinsics constant, under the robust cost of pram_pose_refine at scale loss_scale: per observation
 * s = |r|^2 / loss_scale^2, cost log1p(s), weight 1 / (1 + s); the residual goes through the full camera model against keypoint
 * + 0.5.  The reduced camera system of the Schur complement is solved by conjugate gradients with the block-Jacobi preconditioner,
 * matrix-free.  Damping is pram_pose_refine's, H + lam diag(H), on the point blocks and on the frame blocks.  NOT Ceres / COLMAP's
 * bundle adjuster: DESIGN.md 4.25 lists the deviations and every fixed summation order.  float64; no floating-point atomics.
 *
 * The tables.  An observation is a row (keypoint) with a point: obs_row / obs_frame / obs_point [n_obs] in ascending row, so that
 * frame f's observations are frm_off[f] .. frm_off[f + 1] (frm_off [n_frames + 1]); pt_off [n_points + 1] / pt_obs [n_obs] is the
 * CSR of observation indices per point, ascending.  frozen [n_frames]: six bits per frame, bit a freezes tangent parameter a
 * (0..2 rotation, 3..5 translation): its Jacobian column is zero and its diagonal 1, so its step is exactly 0.  A frame without
 * observations is frozen.  table [n_frames][PRAM_TRI_FRAME_COLS] is pram_tri_frames' and xyz [n_points][3] the points.
 * pram_ba_begin checks every index of the tables on the device before any kernel reads through it: a table that fails ends the
 * run with PRAM_BA_REASON_TABLES and nothing else is written.
 *
 * The state record lives in the workspace: float64 [PRAM_BA_STATE_F64] and int32 [PRAM_BA_STATE_I32 + 2 * max_iters]; behind the
 * fixed words the CG iterations of every LM iteration, then its accept flag.  Every kernel reads it; once `done` is set (or, for
 * the CG kernels, the solve has stopped) the launches still enqueued return at once, so a caller enqueues LM iterations in groups
 * and reads PRAM_BA_SI_DONE once per group.  pram_ba_layout gives the byte offsets of the workspace's arrays
 * [PRAM_BA_ARRAYS + 1] (the last is the total) in the order of bundle.hip's enum: tests and the timing tool read the stages there.
 *
 * pram_ba_begin fills `context` [PRAM_BA_CONTEXT_BYTES] (HOST memory: the pointers and sizes of the problem), copies table and
 * xyz into the workspace and computes the initial cost; the problem's arrays and the workspace must outlive the context.
 * pram_ba_iterate enqueues n_iters LM iterations of at most cg_iters CG iterations each (a CG solve stops at
 * |r| <= cg_tol |b|); stages: PRAM_BA_STAGE_ALL, or single stages for tests and timing.  A step is accepted when the cost falls
 * (a NaN cost rejects), lam x 0.1 on accept (not below 1e-15), x 10 on reject; the run ends at max_iters iterations or at an
 * accepted relative decrease of the cost below ftol.  A point whose damped block has a pivot that is not positive, or fewer than
 * two observations of weight above 0, stays where it is.  An observation with depth <= 1e-12 or a residual that is not finite
 * has weight 0.  pram_ba_finish writes the poses (a frame that never moved keeps qvec_in / tvec_in bit for bit), the points and
 * the filter: obs_keep [n_obs] (depth > 0 and reprojection error <= max_reproj_error), obs_error [n_obs] (pixels), pt_keep
 * [n_points] (two kept observations at least and a largest angle between the rays of two of them of min_tri_angle radians or
 * more), pt_error [n_points] (the mean error of the kept), pt_angle [n_points] (that largest angle, -1 without a pair), pt_kept
 * [n_points], counts [2] = (observations of weight 0 at the final state, observations not kept).  Limits: n_frames <= 2^24,
 * n_points <= 2^28, n_obs <= 2^26, max_iters <= 4096, cg_iters <= 65536; workspace 256-byte aligned. */
#define PRAM_BA_OBS_DOUBLES 20         /* per observation: sqrt(w) J_c [2][6], sqrt(w) J_p [2][3], sqrt(w) r [2] */
#define PRAM_BA_BLOCK 64               /* frames per block of the sums over frames */
#define PRAM_BA_ARRAYS 25
#define PRAM_BA_CONTEXT_BYTES 512
#define PRAM_BA_STATE_F64 16
#define PRAM_BA_STATE_I32 16
#define PRAM_BA_SD_COST 0
#define PRAM_BA_SD_LAM 2
#define PRAM_BA_SD_COST0 9
#define PRAM_BA_SI_DONE 0
#define PRAM_BA_SI_REASON 1
#define PRAM_BA_SI_LM_ITER 2
#define PRAM_BA_SI_ACCEPTED 3
#define PRAM_BA_SI_CG_FAIL 9
#define PRAM_BA_REASON_MAX_ITERS 1
#define PRAM_BA_REASON_FTOL 2
#define PRAM_BA_REASON_TABLES 3
#define PRAM_BA_STAGE_LINEARISE 1
#define PRAM_BA_STAGE_BLOCKS 2
#define PRAM_BA_STAGE_CG_INIT 4
#define PRAM_BA_STAGE_CG 8
#define PRAM_BA_STAGE_STEP 16
#define PRAM_BA_STAGE_ALL 31

size_t pram_ba_workspace_bytes(int n_frames, int n_points, int n_obs, int max_iters);
int pram_ba_layout(int n_frames, int n_points, int n_obs, int max_iters, size_t* offsets);
int pram_ba_begin(const float* keypoints, const int* cam_model, const double* cam_params, const int* cam_model_host,
                  const double* table, const double* xyz, const int* obs_row, const int* obs_frame, const int* obs_point,
                  const int* frm_off, const int* pt_off, const int* pt_obs, const int* frozen, int n_frames, int n_points,
                  int n_obs, int n_rows, int max_iters, double loss_scale, double lam0, double cg_tol, double ftol,
                  void* workspace, size_t workspace_bytes, void* context, void* stream);
int pram_ba_iterate(const void* context, int n_iters, int cg_iters, int stages, void* stream);
int pram_ba_finish(const void* context, const double* qvec_in, const double* tvec_in, double max_reproj_error, double min_tri_angle,
                   double* qvec, double* tvec, double* xyz, unsigned char* obs_keep, double* obs_error, int* pt_keep,
                   double* pt_error, double* pt_angle, int* pt_kept, int* counts, void* stream);

/* ---- bundle adjustment with camera groups (csrc/bundle.hip): the intrinsics refined with the poses and the points ------------
 * The adjustment above with a second kind of unknown: the parameters of camera GROUPS.  A group is a set of frames that share one
 * physical camera, hence one model and one parameter vector grp_params [n_groups][PRAM_BAC_GROUP_PARAMS]: the model's own
 * parameters in COLMAP's order (3 for SIMPLE_PINHOLE, 4 for PINHOLE and SIMPLE_RADIAL, 5 for RADIAL, 8 for OPENCV), zero padded;
 * a step is additive.  The reduced system has 6 n_frames + 8 n_groups unknowns; its preconditioner is block-Jacobi (a 6 x 6 block
 * per frame, an 8 x 8 block per group, no coupling between them), its matvec exact.  DESIGN.md 4.27 has the passes, the fixed
 * orders and the deviations from COLMAP.  The pram_ba_* entries are untouched by this; the state record, the stages, the reasons
 * and the decision are theirs.
 *
 * The tables are pram_ba_begin's (there is no per-frame cam_params: a frame's parameters are its group's) and the groups':
 * frm_grp [n_frames] the group of every frame, and its inverse as a CSR, grp_off [n_groups + 1] / grp_frame [n_frames], the frames
 * of a group ascending.  grp_mask [n_groups]: eight bits per group, bit a freezes parameter a of the model's order; a parameter
 * the model does not have and every parameter of a group without observations are frozen by the entry.  A frozen parameter's
 * column is zero and its diagonal 1, so its step is exactly 0.  pram_bac_begin checks the group tables on the device as it checks
 * the observation tables (every grp_frame in range, every frame in exactly one group, one model per group): a failure ends the run
 * with PRAM_BA_REASON_TABLES before any kernel reads through them.
 *
 * Per observation the workspace holds PRAM_BAC_OBS_DOUBLES: sqrt(w) J_c [2][6], sqrt(w) J_k [2][8], sqrt(w) J_p [2][3],
 * sqrt(w) r [2].  pram_bac_layout gives the offsets of the workspace's arrays [PRAM_BAC_ARRAYS + 1]: the first PRAM_BA_ARRAYS are
 * pram_ba_layout's arrays, then the per-frame parameters (accepted, candidate), the groups' parameters (accepted, candidate), the
 * groups' blocks [36], diag U_k, b_k, the groups' rows of cg_x / cg_r / cg_z / cg_p / cg_q, their dot products [2 n_groups] and
 * block partials, the frames' partial sums [n_frames][60] and [n_frames][8], the groups' mask, candidate flag and model, and the
 * block sums of the groups' folds [n_frames / PRAM_BA_BLOCK + n_groups + 1][60].
 * A group's sum over its frames is the blocked order of PRAM_BA_BLOCK over grp_frame; a dot product adds the frames' total and
 * the groups' total, frames first.  A candidate with a focal length that is not finite or not above 0 has cost NaN and is
 * rejected.  pram_bac_finish writes pram_ba_finish's outputs, evaluated with the refined parameters, and grp_params
 * [n_groups][PRAM_BAC_GROUP_PARAMS]: a group that never moved returns its input bit for bit.  `context`
 * [PRAM_BAC_CONTEXT_BYTES] is HOST memory.  Limits: pram_ba_begin's, and 1 <= n_groups <= n_frames. */
#define PRAM_BAC_OBS_DOUBLES 36
#define PRAM_BAC_GROUP_PARAMS 8
#define PRAM_BAC_ARRAYS 45
#define PRAM_BAC_CONTEXT_BYTES 1024

size_t pram_bac_workspace_bytes(int n_frames, int n_points, int n_obs, int n_groups, int max_iters);
int pram_bac_layout(int n_frames, int n_points, int n_obs, int n_groups, int max_iters, size_t* offsets);
int pram_bac_begin(const float* keypoints, const int* cam_model, const int* cam_model_host, const double* table, const double* xyz,
                   const int* obs_row, const int* obs_frame, const int* obs_point, const int* frm_off, const int* pt_off,
                   const int* pt_obs, const int* frozen, const int* frm_grp, const int* grp_off, const int* grp_frame,
                   const double* grp_params, const int* grp_mask, int n_frames, int n_points, int n_obs, int n_rows, int n_groups,
                   int max_iters, double loss_scale, double lam0, double cg_tol, double ftol, void* workspace, size_t workspace_bytes,
                   void* context, void* stream);
int pram_bac_iterate(const void* context, int n_iters, int cg_iters, int stages, void* stream);
int pram_bac_finish(const void* context, const double* qvec_in, const double* tvec_in, double max_reproj_error, double min_tri_angle,
                    double* qvec, double* tvec, double* xyz, unsigned char* obs_keep, double* obs_error, int* pt_keep,
                    double* pt_error, double* pt_angle, int* pt_kept, int* counts, double* grp_params, void* stream);

/* ---- incremental mapping (csrc/mapper.hip; pram_amd/localization/mapper.py drives these) ---------------------------------------
 * The glue that turns pram_twoview_*, pram_pose_*, pram_tri_* and pram_ba_* into a mapper that needs no poses: a seed pair, then
 * rounds of registration against the points so far, triangulation and adjustment.  NOT COLMAP's incremental mapper: every
 * eligible frame of a round is registered at once, the model is re-triangulated in full and adjusted globally every round, the
 * budgets are fixed (DESIGN.md 4.26 lists the deviations).  The entries read the triangulation's frame table (frame_off
 * [n_frames + 1], keypoints [n_rows][2], norm [n_rows][2] = pram_tri_normalize with the offset 0.5), the match CSR and
 * pram_twoview_finish's outputs, and pram_tri_adjacency's table.  A "row" is a keypoint's index in the frame table, a "point" an
 * index into the current model's xyz [n_points][3].  Index rules, in every entry: an offset pair is clamped into its table; a frame,
 * row or point outside its table is never dereferenced and yields nothing.  float64 where a coordinate is involved, integer sums
 * only, no floating-point atomics; the result of every entry is a function of its inputs alone.  Every entry refuses (PRAM_E_ARG)
 * a null or misaligned pointer (float64 and the workspace 8 bytes, int32 4), a negative size and a workspace that is too small;
 * none waits for the stream and none allocates. */
#define PRAM_MAP_MAX_LINKS 8           /* distinct points a keypoint may bring to its frame's correspondences */

/* Seed scores, one workgroup per processed pair.  kept / count: pram_twoview_finish's (pair p's kept matches stand at
 * kept[match_off[p] ..], count[p] of them); qvec [n_pairs][4], tvec [n_pairs][3], success [n_pairs]: its relative poses (frame 1
 * from frame 0).  Per kept match: d0 the unit ray of frame 0, d1 = R^T times the unit ray of frame 1, X the midpoint of the two
 * rays from the centres 0 and -R^T t, formed as pram_tri_triangulate forms a hypothesis; the match counts when X has positive
 * depth in both frames; its angle is atan2(|d0 x d1|, d0 . d1).  n_tri [n_pairs]: the matches that count; tri_angle [n_pairs]: the
 * LOWER median of their angles, element (n_tri - 1) / 2 in ascending order, found by bisection on the doubles' bit patterns (64
 * counting passes over the workspace's word per match; no sort), 0 for n_tri = 0.  A pair with success == 0 has n_tri 0. */
size_t pram_map_pair_angles_workspace_bytes(int n_matches);
int pram_map_pair_angles(const double* norm, const int* frame_off, const int* pairs, const int* match_off, const int* kept,
                         const int* count, const double* qvec, const double* tvec, const int* success, int n_frames, int n_pairs,
                         int n_matches, void* workspace, size_t workspace_bytes, int* n_tri, double* tri_angle, void* stream);

/* One workgroup.  seed [1]: among the pairs with success != 0, n_tri >= min_num_inliers and tri_angle >= min_tri_angle (radians) the
 * one with the largest n_tri, the lowest position on a tie; -1 when none is eligible. */
int pram_map_seed(const int* success, const int* n_tri, const double* tri_angle, int n_pairs, int min_num_inliers,
                  double min_tri_angle, int* seed, void* stream);

/* 2D-3D correspondences of the frames that are not registered, one workgroup per frame: a count pass, the offsets, a fill pass.
 * adj_off [n_rows + 1] / adj [n_adj] / row_frame [n_rows]: pram_tri_adjacency's; registered [n_frames] uint8; row_point [n_rows]:
 * the row's point in the current model or -1.  For every row u of an unregistered frame: the distinct row_point[v] in
 * [0, n_points) over the v of adj(u) whose frame is registered, ascending, the PRAM_MAP_MAX_LINKS smallest of them.  n_corr
 * [n_frames] (0 for a registered frame), corr_off [n_frames + 1], corr_row / corr_point [capacity] ordered by (row, point); a
 * position at or beyond capacity is not written (n_corr and corr_off still say what there is).  dropped [n_frames]: per frame the
 * entries of its rows' adjacency lists whose point is beyond the kept ones (an entry, not a distinct point: a point linked twice
 * counts twice). */
int pram_map_correspond(const int* adj_off, const int* adj, const int* row_frame, int n_adj, const int* frame_off,
                        const unsigned char* registered, const int* row_point, int n_frames, int n_rows, int n_points, int capacity,
                        int* n_corr, int* corr_off, int* dropped, int* corr_row, int* corr_point, void* stream);

/* One workgroup.  The unregistered frames with n_corr >= max(min_corr, 1) and tries < max_reg_trials, ordered by (n_corr descending,
 * frame ascending), at most round_frames of them (0: all): chosen [n_frames] (-1 padded), chosen_count [n_frames] (0 padded),
 * n_chosen [1].  Selection rounds on a packed key, as pram_covis_topk. */
int pram_map_choose(const int* n_corr, const unsigned char* registered, const int* tries, int n_frames, int min_corr,
                    int max_reg_trials, int round_frames, int* chosen, int* chosen_count, int* n_chosen, void* stream);

/* The chosen frames' correspondences as pram_pose_* take them: matched_keypoints [n_chosen][t0][2] (the keypoints as stored),
 * matched_xyzs [n_chosen][t0][3], counts [n_chosen] = min(n_corr, t0); rows beyond t0 are dropped in table order and counted in
 * cut [n_chosen]; the rows behind counts are zero.  A chosen frame outside [0, n_frames) has count 0. */
int pram_map_pack(const int* chosen, int n_chosen, const int* corr_off, const int* corr_row, const int* corr_point, int n_corr_total,
                  const float* keypoints, const double* xyz, int n_frames, int n_rows, int n_points, int t0,
                  float* matched_keypoints, double* matched_xyzs, int* counts, int* cut, void* stream);

/* One thread per edge: edges_out [n_edges][2] is the edge when the frames of both ends are registered, (-1, -1) otherwise. */
int pram_map_live_edges(const int* edges, int n_edges, const int* row_frame, const unsigned char* registered, int n_frames,
                        int n_rows, int* edges_out, void* stream);

/* ---- image retrieval (csrc/imgret.hip; pram_amd/localization/image_retrieval.py drives these) ----------------
 * A VLAD vector per image (Jegou et al.; intra-normalisation after Arandjelovic and Zisserman) from its 128-D local descriptors
 * and a vocabulary of k centres, and the best database images of every query by the inner product of two such vectors.  Not a
 * restatement of anything in the reference, which ships no retrieval network.  desc float32 [n_rows][PRAM_IMGRET_DIM], centres
 * float32 [k][PRAM_IMGRET_DIM], 1 <= k <= PRAM_IMGRET_MAX_K (the centres are staged in LDS: 128 KB at 256).  The result of every
 * entry is a function of its inputs alone: every sum has the order written here, there are no floating-point atomics.  Every
 * entry refuses (PRAM_E_ARG) a null or misaligned pointer (descriptor and vector rows 16 bytes, float64 and the workspace 8, int32
 * 4), a size out of range and a workspace that is too small; none waits for the stream and none allocates. */
#define PRAM_IMGRET_DIM 128
#define PRAM_IMGRET_MAX_K 256
#define PRAM_IMGRET_MAX_TOPK 64        /* a list slot per lane of the wave that keeps a query's list */
#define PRAM_IMGRET_MAX_SPLITS 1024

/* labels [n_rows]: the nearest centre of every row, the lowest index on a tie; dist float64 [n_rows]: its squared distance,
 * the sum over d ascending of the square of double(x_d) - double(c_d), added to 0.0 (float64 on purpose: the products of fp32
 * inputs are exact, so a numpy restatement reproduces every bit).  Every row of desc is read. */
int pram_imgret_assign(const float* desc, int n_rows, const float* centres, int k, int* labels, double* dist, void* stream);

/* Image i is the rows first[i] .. first[i] + count[i] - 1 of desc (clamped into [0, n_rows): no other row is read), which serves
 * the stores' flat layout (frame_off) and a padded batch [B][N][128] with counts (first = b N) alike.  sums float64
 * [n_img][k][128]: per image, centre c and dimension d the sum of double(x_d) - double(c_d) over the image's rows with
 * labels == c, in ascending row index, added to 0.0; n_assigned [n_img][k]: how many rows that is.  A label outside [0, k)
 * belongs to no centre. */
int pram_imgret_aggregate(const float* desc, const int* labels, int n_rows, const float* centres, int k, const int* first,
                          const int* count, int n_img, double* sums, int* n_assigned, void* stream);

/* The Lloyd step of the vocabulary, from the two entries above with the "images" being blocks of consecutive rows: fold adds
 * the blocks' sums [n_blk][k][128] and n_assigned [n_blk][k] onto total float64 [k][128] and total_n [k] in ascending block
 * order (the caller zeroes both before an iteration and may hand its blocks over in several calls, in order); update then sets
 * c <- float(double(c) + total / total_n) for every centre with total_n > 0; a centre without a row keeps its value. */
int pram_imgret_fold(const double* sums, const int* n_assigned, int n_blk, int k, double* total, int* total_n, void* stream);
int pram_imgret_update(float* centres, const double* total, const int* total_n, int k, void* stream);

/* out float32 [n_img][k * 128] from sums: the block of centre c is v / n_c with n_c = sqrt of the sum over d ascending of v^2 (a
 * zero block stays zero); g = sqrt of the sum, ONE chain over c ascending then d ascending, of the squares of those entries; out =
 * float(entry / g).  An image whose sums are all zero (no rows) is all zeros. */
int pram_imgret_normalize(const double* sums, int n_img, int k, float* out, void* stream);

/* The best k database vectors of every query: q float32 [nq][L], db float32 [nd][L], L a multiple of 128, 1 <= k <=
 * PRAM_IMGRET_MAX_TOPK, nd >= 1.  exclude [nq] or null: a database index the query may not return (-1: none); db_valid uint8
 * [nd] or null: 0 bars a database vector for everybody.  idx [nq][k], sim [nq][k]: similarity descending, then database index
 * ascending, at the cut too; entries beyond the allowed vectors hold -1 and 0.  A NaN similarity is never returned; -0.0 ranks
 * as +0.0.  The similarity is exact fp32 on v_mfma_f32_32x32x2_f32: per (query, database vector) ONE accumulator chain over the
 * whole of L in ascending index, from 0.0f, so a value depends neither on the tile it falls in nor on splits.  The grid is (tiles
 * of 32 queries) x splits, each split a range of 128-row database tiles that leaves a list [nq][splits][k] of packed 64-bit keys
 * in the workspace (the ordered float bits, then 0x7fffffff - index); a second launch merges them.  The order is total, so idx
 * and sim are the same bits for every 1 <= splits <= PRAM_IMGRET_MAX_SPLITS.  The queries x database matrix is never written.
 * The workspace size is 0 for sizes the entry refuses. */
size_t pram_imgret_topk_workspace_bytes(int nq, int k, int splits);
int pram_imgret_topk(const float* q, int nq, const float* db, int nd, int L, const int* exclude, const unsigned char* db_valid,
                     int k, int splits, void* workspace, size_t workspace_bytes, int* idx, float* sim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRAM_HIP_H */
