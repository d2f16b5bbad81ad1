/*
 * valle_hip.h — C ABI of libvalle_hip.so: the MI355X (gfx950) kernels behind the AR + NAR
 * codec-token transformer path of KubiakJakub01/Valle2.
 *
 * The reference has no native layer and no FFI (SURVEY.md §2.1): its hot path is PyTorch ops
 * issued from valle/models/ (*.py).  Each entry point below therefore cites the reference
 * *call site* whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions (every entry point):
 *   - returns 0 when the work was enqueued, a negative VH_E* code when an argument is rejected
 *     (nothing is launched then); vh_last_error() gives the thread-local reason string;
 *   - no allocation, no synchronisation, no host read of device memory: every call may be
 *     captured in a hipGraph; the caller owns all buffers including workspaces;
 *   - all tensors fp32, contiguous in the stated layout, base pointers 16-byte aligned,
 *     leading dimensions multiples of 4 elements; token ids int64; lengths int32;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream);
 *   - one device per process; calls are thread-safe for distinct streams.
 *
 * Arithmetic is fp32 end to end (fp32 MFMA v_mfma_f32_32x32x2_f32 / 16x16x4_f32, exact f32
 * FMA chains) because greedy-token parity with the reference needs it (SURVEY.md §7).
 */
#ifndef VALLE_HIP_H
#define VALLE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VH_VERSION 146            /* 0.2.22: packed AR prompt pass in perf mode — vh_attn_rows_packed_lm_bf16 (vh_attn_rows_packed_bf16 under the prefix-LM mask of every segment, seg_x_len), vh_transformer_forward_packed_lm_bf16 (the perf-mode prompt pass of a ragged batch with no padding rows) and vh_kv_unpack_bf16 (vh_kv_unpack for 16-bit streams); nothing earlier changes; 0.2.21: packed AR prompt pass — vh_transformer_forward_packed_lm (vh_transformer_forward_packed under the prefix-LM mask of every segment, seg_x_len and a scratch lse2) and vh_kv_unpack (the K/V rows of a packed stream copied bit for bit to rows of a per-row or grouped cache, all layers and both of K and V in one launch); nothing earlier changes; 0.2.20: packed NAR training — vh_embed_nar_packed and vh_embed_nar_packed_bwd (the NAR model input over packed rows: text rows and audio rows of every segment in one launch, the codebook count changing at each segment's own prefix boundary; the backward reads every gradient row once for all its tables); nothing earlier changes; 0.2.19: packed AR training — vh_attn_rows_packed_lse (vh_attn_rows_packed with a mask mode, per-segment text lengths and lse2), vh_attn_rows_bwd_packed + vh_attn_rows_bwd_packed_ws_bytes (the five-product backward over segments); nothing earlier changes; 0.2.18: per-row length bounds for AR decoding — vh_row_limits records of (min_new, max_new), vh_sample_step_rows_bounded / vh_sample_step_wide_rows_bounded and vh_ar_decoder_set_row_limits (EOS outside the support below min_new, forced at max_new; NULL or zero records: bit for bit as before); 0.2.17: repetition-aware sampling per row — the two reserved words of vh_row_sampling are read as (window, max_repeats) by vh_sample_step_rows / vh_sample_step_wide_rows and the decoder's row_sampling (zeros: off, bit for bit as before; no new symbol, no new field); 0.2.16: packed NAR decoding in perf mode — vh_attn_rows_packed_bf16 (the 16-bit many-row attention over the segments of one K/V stream) and vh_transformer_forward_packed_bf16 (the perf-mode stage forward of a ragged batch with no padding rows); 0.2.15: vh_attn_decode_form — which kernels a decode-attention call launches for a shape, or the entry point's refusal (read-only; one call record, one check, one plan and one launcher behind the seven vh_attn_decode* entries); 0.2.14: vh_linear_form and vh_linear_form_row — which compiled form a decode GEMM takes for a shape, or the entry point's refusal (read-only; one dispatch plan and one table of compiled forms behind every vh_linear* entry); 0.2.13: NAR decoding over packed rows — vh_attn_rows_packed (many-row attention over the segments of one K/V stream) and vh_transformer_forward_packed (the stage forward of a ragged batch with no padding rows); 0.2.12: per-request NAR sampling — vh_categorical_rows_keyed (the stage sampler keyed on (request, frame) with one vh_row_sampling record per request, tokens stored straight into the codes tensor); 0.2.11: per-row sampling — vh_row_sampling, vh_sample_step_rows and vh_sample_step_wide_rows (seed, draw key, top-k, top-p and temperature per row), vh_ar_decoder_desc gains row_sampling at its end; 0.2.10: queued decoding — vh_decode_groups_poll and vh_decode_group_reset (a finished group's rows go to a waiting utterance between graph replays), and vh_attn_decode_shared_groups takes prefix_len[g] == 0 as a PARKED group (no K/V read, rows exactly 0.0); 0.2.9: the folded-LayerNorm decode GEMMs (vh_linear_folded, vh_linear_qkv_folded, vh_linear_qkv_folded_kv16) and vh_ffn_decode also serve K = d_model in {640, 768, 896} (10, 12 and 14 heads of width 64): accepted shapes of existing symbols only; 0.2.8: grouped shared-prompt decode attention (vh_attn_decode_shared_groups: the beams of several utterances, each group over its own prompt; vh_ar_decoder_desc gains n_groups, beams_per_group, prefix_cap, prefix_lens at its end); 0.2.7: perf mode of the decode step with key splits and with a shared prompt (vh_attn_decode_kv16_split, vh_attn_decode_shared_kv16; vh_ar_decoder takes kv_bf16 with n_split > 1 and with prefix_len > 0); 0.2.6: the folded-LayerNorm decode GEMMs (vh_linear_folded, vh_linear_qkv_folded) take K in {1280, 1536, 1792, 2048, 2560, 3072, 3584, 4096} and vh_ar_decoder serves d_model <= 4096 at head width 64; 0.2.5: up to 32 codebooks in vh_embed_sum_pe (VH_MAX_TABLES) and vh_sample_step_wide for vocabularies up to VH_SAMPLE_MAX_V (the decoder samples through it when V > 2048); 0.2.4: KV-cached decoding at head widths other than 64 (vh_attn_decode_hd, vh_linear_qkv[_folded]_hd, vh_kv_store; the decoder derives the width from d_model / n_heads); 0.2.3: perf-mode q is PRE-SCALED by 1/sqrt(64) log2(e) between vh_linear_qkv_bf16 and vh_attn_rows_bf16; 0.2.2: head + greedy step in one launch (vh_head_greedy, opt-in: vh_ar_decoder_desc.head_ws); 0.2.1: shared-prompt decode attention (vh_attn_decode_shared); 0.2.0: bf16-MFMA perf mode of the prompt pass / NAR stage (vh_*_bf16); 0.1.2: five-product attention backward (vh_attn_rows_bwd_ws); 0.1.1: dropout fields (vh_dropout_spec) */
#define VH_MAX_TABLES 32          /* EnCodec: 8 codebooks at 6 kbps (valle/config.py:15-17), 16 at 12 kbps, 32 at 24 kbps */
#define VH_SAMPLE_MAX_V 16384     /* widest row vh_sample_step_wide takes (num_audio_tokens <= 16383); vh_sample_step: 2048 */
#define VH_HEAD_DIM 64            /* every configuration of the path has d_model/n_heads = 64 */

enum { VH_OK = 0, VH_EINVAL = -1, VH_EALIGN = -2, VH_EUNSUPPORTED = -3, VH_ELAUNCH = -4,
       VH_ESTATE = -5 };

/* activation fused in a GEMM epilogue */
enum { VH_ACT_NONE = 0, VH_ACT_GELU_ERF = 1,
       VH_ACT_GELU_BWD = 2,   /* vh_linear_ex only: out = acc * gelu'(residual) (backward through the activation) */
       VH_ACT_GELU_ERF_D = 3, /* vh_linear_ex only: out = gelu(acc + bias), pre_out = gelu'(acc + bias) — the forward keeps
                                 the DERIVATIVE instead of the pre-activation (erf is evaluated once for both) ... */
       VH_ACT_MUL = 4         /* ... so that the backward is out = acc * residual[m][n], no transcendental in its epilogue */ };

/* attention mask modes (analytic; no (B,h,T,T) tensor is ever materialised) */
enum {
    VH_MASK_FULL = 0,    /* every key < kv_len visible                (NAR, valle_nar.py:94-96) */
    VH_MASK_PREFIX = 1,  /* prefix-LM of build_attn_mask(x_len, y_len) (valle/models/utils.py:17-43):
                            keys < x_len visible to all rows; rows >= x_len also see keys <= row */
    VH_MASK_EXPLICIT = 2 /* caller-supplied u8 (Tq,Tk) mask + optional u8 (B,Tk) key padding,
                            nonzero = masked (API mask convention, valle/models/modules.py:160-164) */
};

int vh_version(void);
const char* vh_last_error(void);

/* Kernel-selection knobs for benchmarking A/B runs in one process (0 = built-in default).
 * Results are identical up to fp32 summation order whatever the setting. */
enum { VH_TUNE_DECODE_VARIANT = 0,  /* decode attention: 0 = default (the ring kernel, 8 waves x 2 register sets of 32 keys, when there
                                       is one (b, head) per CU and no key split; else the 32-key burst kernel), 1 = always the burst
                                       kernel */
       VH_TUNE_DECODE_WAVES = 1,    /* waves per workgroup of the burst kernel: 4, 8 or 16 (nonzero also selects the burst kernel) */
       VH_TUNE_ROW_GROUPS = 2,      /* decode GEMMs (16 < M <= 64): 1 (default) = one workgroup per 16 rows x 16 columns,
                                       (8 rows while the grid stays within the CUs), 2 = one workgroup per
                                       16 columns (all rows), 3 = groups of 16 rows only */
       VH_TUNE_TILE_DMA = 4,        /* large-M GEMM operand staging: 0 (default) = LDS-DMA when K % 32 == 0,
                                       1 = always through registers, 2 = LDS-DMA whenever eligible */
       VH_TUNE_REDUCE_BLOCK = 3,    /* threads per workgroup of the split-K reduce: 64, 128 (default), 256 */
       VH_TUNE_FFN_FUSED = 5,       /* decode step FeedForward: 0 (default) = vh_ffn_decode (one launch split over dim_feedforward
                                       + the slab reduce) when the weights are folded and d_model <= 512 (measured slower at
                                       1024), 1 = always linear_1 and linear_2 as separate launches (vh_linear_folded +
                                       vh_linear_ws), 2 = vh_ffn_decode wherever it is supported */
       VH_TUNE_GRAPH_STEPS = 6,     /* decode graph: 0 (default) = replay in graphs of 8 consecutive steps (+ single-step graphs
                                       for the remainder); 1 = one graph launch per step */
       VH_TUNE_FFN_SLICE = 7,       /* vh_ffn_decode: hidden columns per workgroup, 0 (default) = chosen from the shape, else 16 / 32 */
       VH_TUNE_FFN_ROWS = 8,        /* vh_ffn_decode: rows per workgroup, 0 (default) = chosen from the shape, else 8 / 16 */
       VH_TUNE_LN_STATS = 9,        /* folded-LayerNorm decode GEMMs on <= 16 rows per workgroup: 0 (default) = row statistics from
                                       the operand fragments (no second read of the rows), 1 = from their own row loads */
       VH_TUNE_TAIL_SPLIT = 10,     /* vh_linear_ex with a workspace: 0 (default) = the tiles beyond the last multiple of 256 are
                                       computed as K slices + a fix-up launch when they would fill <= half of the CUs, 1 = never */
       VH_TUNE_TN_WGS = 11,         /* vh_gemm_tn: workgroups the contraction split aims at, 0 (default) = 256 (one per CU) */
       VH_TUNE_DECODE_COMBINE = 12, /* decode attention with key splits: 1 = the last workgroup of a (b, head) to arrive adds the split
                                       records in the same launch, 2 = a second launch does (same bits: split order either way);
                                       0 (default) = as measured: in the same launch at two splits (configs[4], 8 rows x 16 heads:
                                       13 us per step faster at context 2.7 k), a second launch at more (13 us per step slower at
                                       4 beams x 8 splits) */
       VH_TUNE_ATTN_BWD = 13,       /* vh_attn_rows_bwd_ws: 0 (default) / 2 = the five-product kernel + slab reduce, 1 = the two-kernel,
                                       seven-product form of vh_attn_rows_bwd (its D scratch taken from the workspace) */
       VH_TUNE_ATTN_BWD_CHUNKS = 14, /* five-product attention backward: key chunks per (batch row, head); 0 (default) = chosen from the
                                       shape (bwd_chunks in csrc/attention.hip), else that many (at least ceil(T / 256)) */
       VH_TUNE_BF16_GEMM = 15,      /* perf-mode tile GEMM: 0 (default) = form 4 where the shape allows it (N % 256 == 0, K % 128 == 0,
                                       >= 128 tiles), else per output type (16-bit outputs: form 3; fp32 output + residual: form 1);
                                       1 = 128^2 tiles, two slabs of 64 k (two workgroups per CU), 3 = one slab of 64 k, no software
                                       pipeline, four workgroups per CU, 4 = one persistent workgroup per CU, 256^2 tiles, 8 waves
                                       taking turns on the matrix pipe, requests in flight across barriers and tiles
                                       (csrc/gemm16p.hip); 2 (round 5's ring of three slabs of 32 k, removed: slower on 7 of 8 shapes)
                                       = the default */
       VH_TUNE_COUNT = 16 };
int vh_set_tuning(int knob, int value);

/* ---- dropout field of the training path -------------------------------------------------------------
 * replaces nn.Dropout at its four call sites of a training step: PositionalEncoding (valle/models/modules.py:56-58,
 * 78-80: p = 0.1 whatever config.dropout says), FeedForward (:219), EncoderLayer.dropout1 / dropout2 (:277-278, p =
 * config.dropout, default 0.1 valle/config.py:26) and TokenEmbedding (:35).  The field is never stored: it is a pure
 * function of (seed, site, row, column) that every kernel regenerates where it needs it — forward epilogue and
 * backward alike — so a training step with dropout reads and writes no mask tensors.
 *   keep(row, col) = philox4x32_7(key = (seed lo, seed hi), counter = (col / 4, row, site lo, site hi))[col % 4]
 *                    >= round(p * 2^32)                                   (Philox: Salmon et al., SC'11; 7 rounds)
 *   dropped value  = keep ? value / (1 - p) : 0                           (torch.nn.functional.dropout's scaling)
 * `row` / `col` index the logical (rows, cols) matrix the site covers (cols % 4 == 0); `site` tells the fields of one
 * step apart (layer, call site), `seed` the steps.  A NULL spec or p == 0 means "no dropout" everywhere below; p must
 * be < 1.  The stream differs from torch's generators: parity with the reference is through the exported mask
 * (vh_dropout_mask) handed to the oracle, and distributional. */
typedef struct { uint64_t seed; uint64_t site; float p; } vh_dropout_spec;
/* out[r][c] = keep(r, c) ? x[r][c] / (1 - p) : 0 for a (rows, cols) matrix (row strides ldx / ldo, multiples of 4);
 * out may be x.  Forward and backward of a free-standing nn.Dropout are this same call. */
int vh_dropout(const float* x, int ldx, float* out, int ldo, int64_t rows, int cols, const vh_dropout_spec* spec,
               void* stream);
/* keep[r * cols + c] = 1 / 0: the field itself, for tests and for handing the very same mask to a CPU oracle */
int vh_dropout_mask(uint8_t* keep, int64_t rows, int cols, const vh_dropout_spec* spec, void* stream);

/* ---- K1/K2: embedding gather (sum over n_tables codebooks) + sinusoidal position add --------
 * replaces TokenEmbedding.forward + PositionalEncoding.forward (valle/models/modules.py:33-37,
 * 78-80) and the 8-codebook sum of ValleNAR._prepare_audio_codes (valle/models/valle_nar.py:
 * 179-185).  For b<B, t<T (t < lens[b] when lens != NULL):
 *   out[b*out_bstride + (out_t0 + t)*d + :] =
 *       sum_{j<n_tables} tables[j][ ids[b*ids_bstride + t*ids_tstride + j*ids_jstride] ][:]
 *       + pe[(pos0 + t)*d + :]                      (pe == NULL: no position term)
 * `tables` is a HOST array of n_tables device pointers, each (vocab[j], d); `vocab` is a HOST array of
 * the n_tables row counts.  An id outside [0, vocab[j]) reads row 0 instead (never out of bounds) and
 * ORs VH_DEVERR_EMBED_ID into *err_flag (device int32, may be NULL); the reference's nn.Embedding raises
 * IndexError there — the host side turns the flag into that exception at its next synchronisation.
 * row_pos0 / row_t0 (device int32 (B), each may be NULL): per-row overrides of pos0 / out_t0 — a ragged batch whose
 * rows sit at different offsets (text | prompt | target per utterance) is embedded by one launch.
 * drop (NULL: none): the dropout that follows the position add (modules.py:80) applied to the sum before it is stored;
 * the field's row index is the row's offset in `out` / d (= b * (out_bstride / d) + out_t0 + t; out_bstride % d == 0
 * then), its column the column — what vh_embed_bwd regenerates from the same spec. */
enum { VH_DEVERR_EMBED_ID = 1, VH_DEVERR_TARGET = 2 };
int vh_embed_sum_pe(const int64_t* ids, int64_t ids_bstride, int64_t ids_tstride,
                    int64_t ids_jstride, const float* const* tables, const int32_t* vocab, int n_tables,
                    const float* pe, int pos0, const int32_t* lens, float* out,
                    int64_t out_bstride, int out_t0, int B, int T, int d, int32_t* err_flag,
                    const int32_t* row_pos0, const int32_t* row_t0, const vh_dropout_spec* drop, void* stream);

/* PositionalEncoding.forward as a module call (valle/models/modules.py:78-80; its dropout is vh_dropout):
 *   out[b, t, :] = x[b, t, :] + pe[(pos0 + t) * d + :]   for (B, T, d) contiguous x / out (out may be x); d % 4 == 0;
 * the caller guarantees pos0 + T rows in `pe`.  (The model paths add the position inside vh_embed_sum_pe.) */
int vh_add_pe(const float* x, const float* pe, float* out, int B, int T, int d, int pos0, void* stream);

/* ---- K3/K4: LayerNorm (eps) with optional adaptive scale/shift ------------------------------
 * replaces nn.LayerNorm (valle/models/modules.py:284) and AdaptiveLayerNorm.forward (:93-99):
 *   out[r,:] = ada_scale[:] * (gamma * (x[r,:]-mean)/sqrt(var+eps) + beta) + ada_shift[:]
 * ada_scale/ada_shift (d) may both be NULL (plain LayerNorm). */
int vh_layernorm(const float* x, const float* gamma, const float* beta, const float* ada_scale,
                 const float* ada_shift, float* out, int rows, int d, float eps, void* stream);

/* ---- K5/K9/K10/K11: out = act(LN?(A) W^T + bias) + residual ---------------------------------
 * replaces nn.Linear at valle/models/modules.py:146 (qkv), :171 (out), :221 (linear_1 +
 * exact-erf GELU, linear_2) and the heads valle_ar.py:83,158 / valle_nar.py:100.
 * A (M,K) lda; W (N,K) row-major (the nn.Linear weight as stored); bias (N)|NULL;
 * residual (M,N) ldr |NULL (may alias out); out (M,N) ldo.
 * ln_gamma/ln_beta (K)|NULL: when given (M <= 64 only) A's rows are LayerNorm-ed (eps ln_eps,
 * then optional ada_scale/ada_shift (K)) on the fly in the operand load — the decode path. */
int vh_linear(const float* A, int lda, const float* W, const float* bias, const float* residual,
              int ldr, float* out, int ldo, int M, int N, int K, int act, const float* ln_gamma,
              const float* ln_beta, const float* ada_scale, const float* ada_shift, float ln_eps,
              void* stream);

/* Same contract as vh_linear without the fused LayerNorm, plus a caller-owned workspace of
 * vh_linear_ws_bytes(M,N,K) bytes: for M <= 64 and K > 1024 (linear_2, K = dim_feedforward) the K
 * range is split over ~256 workgroups whose partial sums meet in the workspace and are added in
 * slice order by a second small kernel (bitwise reproducible; no floating-point atomics).  The same
 * is done for M > 64 when the (M,N) grid has at most 256 tiles of 128x128 and K >= 1024 (one
 * utterance through the NAR stack, a short prefill): K slices in the second grid dimension of the
 * tile kernel.  With MORE than 256 tiles the workspace serves the tile kernel's tail split instead (the tiles
 * beyond the last multiple of 256 as K slices + a fix-up launch when they would fill at most half of the CUs:
 * vh_linear_ex below) — a prompt pass of 8 x 1100 positions has 276 tiles per 512-wide projection, two rounds for
 * the work of 1.08.
 * Falls back to vh_linear when the shape does not split or workspace == NULL. */
size_t vh_linear_ws_bytes(int M, int N, int K);
int vh_linear_ws(const float* A, int lda, const float* W, const float* bias, const float* residual,
                 int ldr, float* out, int ldo, int M, int N, int K, int act, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- K5+K6: QKV projection with the K/V rows appended in place to the cache -----------------
 * replaces qkv Linear + chunk + rearrange + torch.cat cache growth (valle/models/modules.py:
 * 146-157).  A (M=B*T, K=d) lda; Wqkv (3d, d) rows [Q | K | V], head j = rows j*64..j*64+63.
 * q_out (M, d) ldq receives the Q columns; K and V columns of row (b,t) go to
 * kcache/vcache[(b*h + head)*S_max + pos0(b) + t][0..63] with pos0(b) = cache_len ? cache_len[b] : 0.
 * Optional fused LayerNorm on A's rows as in vh_linear (M <= 64 only). */
int vh_linear_qkv(const float* A, int lda, const float* Wqkv, float* q_out, int ldq, float* kcache,
                  float* vcache, const int32_t* cache_len, int B, int T, int d_model, int n_heads,
                  int S_max, const float* ln_gamma, const float* ln_beta, const float* ada_scale,
                  const float* ada_shift, float ln_eps, void* stream);

/* ---- LayerNorm folded into the weights (decode path, M <= 64) -------------------------------
 * The LayerNorm in front of a Linear (valle/models/modules.py:271 norm1 → qkv, :278 norm2 →
 * linear_1) is rewritten so the products do not wait for the row statistics:
 *   LN(x) W^T + b = rstd * (x Wf^T - mean * c1) + c2,
 *   Wf = W * gamma (per input column), c1[n] = sum_k Wf[n,k], c2[n] = sum_k beta[k] W[n,k] + b[n].
 * vh_ln_fold prepares Wf (N,K), c1 (N), c2 (N) once per weight set (bias may be NULL);
 * vh_linear_folded / vh_linear_qkv_folded are vh_linear / vh_linear_qkv with (Wf, c1, c2) in
 * place of (W, bias, ln_gamma, ln_beta): mean / rstd are computed beside the products and applied
 * in the epilogue.  Supported: M <= 64, N % 16 == 0, K in {128, 256, 512, 1024}; at head width 64 (vh_linear_folded,
 * vh_linear_qkv_folded, vh_linear_qkv_folded_kv16) also K in {640, 768, 896} (K = 128 PW, PW in 5..7, eight waves, one pass,
 * fp32 weights only); and for vh_linear_folded /
 * vh_linear_qkv_folded also K in {1280, 1536, 1792, 2048, 2560, 3072, 3584, 4096} (K = 256 PW passes, PW in 5..8, one or two passes): 16 waves per 16 output columns, one or
 * two passes over K, mean / variance from the operand fragments as one-pass sums about the mean of the row's first 32
 * elements (the products run on x - that shift too, so the epilogue's correction is a fraction of the row's deviation);
 * the shift being a mean of 32 of the row's own elements bounds the cancellation of the one-pass variance: (mean - shift)^2 <=
 * K/32 var, at most 7 bits lost of 24 at K = 4096 even for a row whose first 32 elements are outliers;
 * more than 16 rows run as row groups, so vh_linear_qkv_folded needs T == 1 there.  Deterministic (fixed summation
 * order, no atomics).  The _kv16 form and vh_ffn_decode keep K <= 1024 (with 640, 768 and 896), the _hd form K in {128, 256, 512, 1024}.  Anything else: VH_EUNSUPPORTED with a
 * message naming "folded LayerNorm". */
int vh_ln_fold(const float* W, const float* gamma, const float* beta, const float* bias, float* Wf,
               float* c1, float* c2, int N, int K, void* stream);
int vh_linear_folded(const float* A, int lda, const float* Wf, const float* c1, const float* c2,
                     const float* residual, int ldr, float* out, int ldo, int M, int N, int K,
                     int act, float ln_eps, void* stream);
int vh_linear_qkv_folded(const float* A, int lda, const float* Wf, const float* c1, const float* c2,
                         float* q_out, int ldq, float* kcache, float* vcache, const int32_t* cache_len, int B,
                         int T, int d_model, int n_heads, int S_max, float ln_eps, void* stream);

/* ---- the same two for a head width other than 64 (the decode step of such a model) --------------------------------
 * vh_linear_qkv / vh_linear_qkv_folded with the K and V rows appended to caches (B, h, S_max, head_dim), head_dim =
 * d_model / n_heads a multiple of 4 (a 4-column group never crosses a head).  The decode step's form only: T == 1 and
 * B <= 64 (anything else is refused with VH_EUNSUPPORTED); the folded form takes the K of vh_linear_qkv_folded. */
int vh_linear_qkv_hd(const float* A, int lda, const float* Wqkv, float* q_out, int ldq, float* kcache, float* vcache,
                     const int32_t* cache_len, int B, int T, int d_model, int n_heads, int S_max, const float* ln_gamma,
                     const float* ln_beta, const float* ada_scale, const float* ada_shift, float ln_eps, int head_dim,
                     void* stream);
int vh_linear_qkv_folded_hd(const float* A, int lda, const float* Wf, const float* c1, const float* c2, float* q_out, int ldq,
                            float* kcache, float* vcache, const int32_t* cache_len, int B, int T, int d_model, int n_heads,
                            int S_max, float ln_eps, int head_dim, void* stream);

/* ---- which compiled form a decode GEMM takes (ABI 138; read-only, launches nothing, touches no GPU state) ------------
 * vh_linear_form runs the named entry point's own argument checks and its dispatch plan for a shape, with the current
 * vh_set_tuning knobs, and returns what that entry point would return for well-formed pointers: VH_OK and the form in *out,
 * or the entry's refusal code with vh_last_error() set to the entry's own message (*out is zeroed).
 *   entry               asks                                                         M, N, K, T
 *   VH_ENTRY_LINEAR     vh_linear (ln_kind NONE / GAMMA), vh_linear_folded (FOLDED)  as the entry's; T ignored
 *   VH_ENTRY_QKV        vh_linear_qkv / vh_linear_qkv_folded                         M = B*T rows, K = d_model, N = 3 K
 *   VH_ENTRY_QKV_HD     vh_linear_qkv_hd / vh_linear_qkv_folded_hd                   the same (any valid head width)
 *   VH_ENTRY_QKV_KV16   vh_linear_qkv_folded_kv16 (FOLDED only; T == 1)              the same
 *   VH_ENTRY_LINEAR_WS  vh_linear_ws with a workspace of vh_linear_ws_bytes          as the entry's: the GEMM launch (the
 *                                                                                    split-K reduce and a tail split's extra slices are not described)
 *   VH_ENTRY_HEAD_GREEDY vh_head_greedy                                              M = B, N = V, K = d_model
 * w16 != 0 asks for the 16-bit-weight form the decoder of perf mode uses (VH_ENTRY_LINEAR without LayerNorm and
 * VH_ENTRY_QKV_KV16).  A combination no entry point has (an unknown entry, M % T != 0, N != 3 K for the QKV entries, w16
 * elsewhere) is VH_EINVAL.
 * out: family (VH_FORM_*; VH_FORM_NONE when M == 0), the template tuple of the kernel (gemm_skinny_fast<mt, nw, epi, pw, ln,
 * nj, w16>; gemm_skinny_kernel<mt, nw, epi, pw, ln>; gemm_head_greedy_kernel<pw>; the tile kernels are <epi>), the launch
 * grid and block and the rows per row group (0: none).
 * vh_linear_form_row(i, out) lists the compiled skinny forms, i = 0, 1, ...: the tuple and in out->epis the set of epilogues
 * (bit e = epilogue e) row i is built for; VH_EINVAL past the last row.  Every form vh_linear_form returns for a skinny
 * family is one of these rows. */
enum { VH_LN_NONE = 0, VH_LN_GAMMA = 1, VH_LN_FOLDED = 2 };
enum { VH_ENTRY_LINEAR = 0, VH_ENTRY_QKV = 1, VH_ENTRY_QKV_HD = 2, VH_ENTRY_QKV_KV16 = 3, VH_ENTRY_LINEAR_WS = 4,
       VH_ENTRY_HEAD_GREEDY = 5 };
enum { VH_FORM_NONE = 0, VH_FORM_SKINNY_FAST = 1, VH_FORM_SKINNY_GENERIC = 2, VH_FORM_TILE_DMA = 3, VH_FORM_TILE_REG = 4,
       VH_FORM_HEAD_GREEDY = 5 };
typedef struct vh_linear_form_info {
    int family;
    int mt, nw, epi, pw, ln, nj, w16;
    unsigned grid[3], block;
    int rg_rows;
    unsigned epis;                /* vh_linear_form: 1 << epi; vh_linear_form_row: every epilogue the row is built for */
} vh_linear_form_info;
int vh_linear_form(int entry, int M, int N, int K, int T, int ln_kind, int w16, vh_linear_form_info* out);
int vh_linear_form_row(int i, vh_linear_form_info* out);

/* ---- prompt pass at a head width other than 64: K / V of the QKV projection into the cache --------------------------
 * qkv (B*T, ld) holds [Q | K | V] column blocks of d = n_heads * head_dim columns (the projection the prompt's attention
 * used); K and V of row (b, t) go to kcache / vcache[(b*h + head)*S_max + t][0 .. head_dim-1], t < T <= S_max.  16-byte
 * loads and stores (head_dim % 4 == 0, ld % 4 == 0, 16-byte aligned pointers); a bit-exact copy. */
int vh_kv_store(const float* qkv, int ld, float* kcache, float* vcache, int B, int T, int n_heads, int head_dim, int S_max,
                void* stream);

/* ---- FeedForward + residual of the decode step as one launch split over dim_feedforward --------
 * replaces FeedForward.forward + the residual add of EncoderLayer.forward (valle/models/modules.py:215-221,
 * :278-279) for M <= 64 rows:   out = x + b2 + GELU(LN2(x) W1^T + b1) W2^T
 * with (w1f, c1, c2) = vh_ln_fold(W1, ln2_gamma, ln2_beta, b1).  Workgroup (slice, row group) owns SW
 * consecutive hidden columns and up to 16 rows: it computes that (rows x SW) tile of the hidden activation
 * (folded LayerNorm, exact-erf GELU), keeps it in LDS, multiplies it by W2[:, slice]^T and leaves a raw
 * (rows x d_model) partial in slab `slice` of the workspace — linear_1 -> linear_2 never crosses a kernel
 * boundary and the (M, dff) hidden activation never exists in memory.  A second small launch adds the slabs
 * in slice order (bitwise reproducible, no atomics) with b2 and the residual x.  out may alias x.
 * x (M, d_model) ldx; w1f (dff, d_model); w2 (d_model, dff) as stored; c1, c2 (dff); b2 (d_model) | NULL.
 * Supported: M <= 64, d_model in {128, 256, 512, 640, 768, 896, 1024}, dff % 16 == 0, dff / 16 <= 1024 slices.
 * workspace: vh_ffn_decode_ws_bytes(M, d_model, dff) bytes (no initialisation needed). */
size_t vh_ffn_decode_ws_bytes(int M, int d_model, int dff);
int vh_ffn_decode(const float* x, int ldx, const float* w1f, const float* c1, const float* c2, const float* w2,
                  const float* b2, float* out, int ldo, int M, int d_model, int dff, float ln_eps,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- K7+K8a: multi-row attention (prefill / NAR / training forward) -------------------------
 * replaces merge_masks + F.scaled_dot_product_attention (valle/models/modules.py:160-167,
 * 175-207).  q (B,Tq,ldq) heads at columns head*64; K/V from the cache layout (B,h,S_max,64);
 * out (B,Tq,ldo).  Query row i sits at key position q_off + i (q_off = Tk - Tq).
 *   VH_MASK_FULL   : key j visible iff j < kvl(b)
 *   VH_MASK_PREFIX : key j visible iff j < kvl(b) && (j < xl(b) || (q_off+i >= xl(b) && j <= q_off+i))
 *   VH_MASK_EXPLICIT: key j visible iff !mask[i*Tk+j] && !(pad && pad[b*Tk+j])
 * kvl(b) = kv_len ? kv_len[b] : Tk ; xl(b) = x_len_dev ? x_len_dev[b] : x_len.
 * softmax scale = 1/sqrt(64). */
int vh_attn_rows(const float* q, int ldq, const float* kcache, const float* vcache, float* out,
                 int ldo, int B, int n_heads, int Tq, int Tk, int S_max, int mode, int x_len,
                 const int32_t* x_len_dev, const int32_t* kv_len, const uint8_t* mask,
                 const uint8_t* pad, void* stream);

/* vh_attn_rows in VH_MASK_EXPLICIT mode with ONE MASK PER BATCH ROW: mask (B,Tq,Tk) u8, mask_batch_stride elements between the
 * rows' masks (0 = the same (Tq,Tk) mask for all) — the 3-D attn_mask MultiHeadAttention.forward accepts
 * (valle/models/modules.py:187-188: 'b t t -> b 1 t t'); key j of row b visible to query i iff
 * !mask[b*stride + i*Tk + j] && !(pad && pad[b*Tk + j]). */
int vh_attn_rows_bmask(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo, int B,
                       int n_heads, int Tq, int Tk, int S_max, const uint8_t* mask, int64_t mask_batch_stride,
                       const uint8_t* pad, void* stream);

/* vh_attn_rows that also writes lse2 (B, n_heads, Tq): log2 of the softmax denominator of every query row
 * in the scaled-score units the backward kernels use (lse2 = max + log2(sum 2^(s - max)), s = q.k/8*log2 e). */
int vh_attn_rows_lse(const float* q, int ldq, const float* kcache, const float* vcache, float* out,
                     int ldo, int B, int n_heads, int Tq, int Tk, int S_max, int mode, int x_len,
                     const int32_t* x_len_dev, const int32_t* kv_len, const uint8_t* mask,
                     const uint8_t* pad, float* lse2, void* stream);

/* vh_attn_rows over the SEGMENTS of one packed row stream, VH_MASK_FULL only: a ragged batch with no padding rows.
 * Utterance s owns rows seg_start[s] .. seg_start[s] + seg_len[s] - 1 of q (M, ldq), of out (M, ldo) and of ONE K/V stream
 * per head, kcache / vcache (1, h, S_max >= M, 64), M = the sum of the lengths: query row seg_start[s] + i attends keys seg_start[s] + j, j < seg_len[s],
 * of the same cache and nothing else.  One workgroup = the 128 queries from blocks[2 i + 1] on of segment blocks[2 i] x one
 * head, over that segment's keys in 32-key tiles counted from the segment's key 0 — vh_attn_rows' tile order, and its
 * arithmetic, for that utterance alone (B = 1, Tq = Tk = seg_len[s]): the same bits.  K/V rows past a segment's end are
 * clamped to its last row and masked; query rows past it are neither loaded nor stored.  Workgroups run in table order:
 * list the blocks of the longest segment first (they visit the most tiles).
 * seg_start, seg_len (n_seg) and blocks (n_blocks pairs) are DEVICE int32 arrays the host cannot check: the caller vouches
 * that the segments are disjoint and inside [0, M), that every block names a segment < n_seg and a first query
 * 0 <= q0 < seg_len, and that the blocks cover every query once (a query no block covers keeps its old `out` row).  Inside
 * such segments no row of another segment is read as a visible key and no row at or beyond M is touched.  (A block naming
 * no segment is skipped and a segment reaching past S_max is cut there, so the caches are never overrun; q and out have
 * no such guard.) */
int vh_attn_rows_packed(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                        int n_heads, int S_max, const int32_t* seg_start, const int32_t* seg_len, int n_seg,
                        const int32_t* blocks, int n_blocks, void* stream);

/* ---- backward of vh_attn_rows (training, Tq == Tk == T): dQ, dK, dV without materialising P -----
 * replaces the autograd backward of F.scaled_dot_product_attention (valle/models/modules.py:167) in
 * loss.backward() of training_step.  q (B*T, ldq) / kcache, vcache (B,h,S_max,64) / out (B*T, ldo) /
 * lse2 as produced by vh_attn_rows_lse, dout (B*T, lddo) the gradient of out; same mask arguments.
 * dq, dk, dv: (B*T, ldg) each with head h at columns h*64 (three column blocks of one (B*T, 3d) buffer
 * work: ldg = 3d).  dsum (B, n_heads, T) is scratch (D = rowsum(dout * out)).  Two launches, no atomics:
 * results are bitwise reproducible. */
int vh_attn_rows_bwd(const float* q, int ldq, const float* kcache, const float* vcache, const float* out,
                     int ldo, const float* dout, int lddo, const float* lse2, float* dsum, float* dq,
                     float* dk, float* dv, int ldg, int B, int n_heads, int T, int S_max, int mode,
                     int x_len, const int32_t* x_len_dev, const int32_t* kv_len, const uint8_t* mask,
                     const uint8_t* pad, void* stream);

/* The same gradients from FIVE products (round 4): one kernel with keys as lanes computes S, dP, dV, dK per (32-query tile,
 * 256-key chunk) and sends dS through LDS into the chunk's dQ partial (mfma 16x16x4 over all the chunk's keys, no cross-wave
 * sum); the partials of the ceil(T / 256) chunks land in slabs inside `ws` and a second launch adds them in chunk order
 * (T <= 256: dq is written directly, one launch).  No atomics: bitwise reproducible.  ws: vh_attn_rows_bwd_ws_bytes bytes,
 * 16-byte aligned, scratch.  D = rowsum(dout * out) is computed in the kernel (no dsum argument). */
size_t vh_attn_rows_bwd_ws_bytes(int B, int n_heads, int T);
/* the number of key chunks (= dQ slabs) vh_attn_rows_bwd_ws uses for this shape and mask family (tools, tests) */
int vh_attn_rows_bwd_chunks(int B, int n_heads, int T, int mode);
int vh_attn_rows_bwd_ws(const float* q, int ldq, const float* kcache, const float* vcache, const float* out,
                        int ldo, const float* dout, int lddo, const float* lse2, float* dq, float* dk, float* dv,
                        int ldg, int B, int n_heads, int T, int S_max, int mode, int x_len,
                        const int32_t* x_len_dev, const int32_t* kv_len, const uint8_t* mask,
                        const uint8_t* pad, void* ws, size_t ws_bytes, void* stream);

/* ---- packed AR training (ABI 143): the training forms of the attention over the SEGMENTS of one packed row stream -----
 * vh_attn_rows_packed plus a mask mode (VH_MASK_FULL or VH_MASK_PREFIX; anything else is VH_EINVAL), seg_x_len (device
 * int32 (n_seg), read only under the prefix mask: the text length inside segment s, clamped to 0 .. seg_len[s]) and lse2
 * (n_heads, M): the log2-sum-exp of the scaled scores of every packed row, as vh_attn_rows_lse writes it.  Segment s is a
 * sequence of its own: key j of it is visible to its query i when j < x_len || (i >= x_len && j <= i); no key is padding.
 * out and lse2 of a segment are bit for bit those of vh_attn_rows_lse on it alone (B = 1, Tq = Tk = seg_len[s], the same mode
 * and x_len).  M: rows of q / out / lse2 (S_max >= M); the tables are under vh_attn_rows_packed's contract, and a segment
 * reaching past M is cut there. */
int vh_attn_rows_packed_lse(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                            int n_heads, int M, int S_max, int mode, const int32_t* seg_start, const int32_t* seg_len,
                            const int32_t* seg_x_len, int n_seg, const int32_t* blocks, int n_blocks, float* lse2,
                            void* stream);
/* Its backward: vh_attn_rows_bwd_ws' five-product kernel (eight waves) with the sequence taken from the segment table.
 * q / out / dout (M, ld·), kcache / vcache (1, h, S_max >= M, 64), lse2 (n_heads, M) from vh_attn_rows_packed_lse; dq, dk,
 * dv (M, ldg) views.  Work items are (segment, key chunk) pairs x head: items[2 i], items[2 i + 1] (device int32, n_items
 * pairs), chunk c of a segment = its keys [c chunk_keys, (c + 1) chunk_keys); chunk_keys a multiple of 32, at most 256, one
 * per launch; workgroups run in table order (list the heaviest first).  max_chunks = the largest chunk count of a segment:
 * above 1 the dQ partials go to slabs (max_chunks, n_heads, M, 64) inside ws (vh_attn_rows_bwd_packed_ws_bytes, 16-byte
 * aligned) and a second launch adds them in chunk order over `blocks` (the forward's table: every query once); at 1 the
 * kernel writes dq itself and ws may be NULL.  No atomics: two runs give the same bits.  With tables that list every
 * (segment, chunk) and every query block once, every row of dq, dk and dv in [0, M) is written exactly once.  The tables are
 * DEVICE arrays the host cannot check: an entry out of range (segment >= n_seg, a segment outside [0, M), chunk >=
 * max_chunks or beyond the segment) makes its workgroup return without touching memory. */
size_t vh_attn_rows_bwd_packed_ws_bytes(int n_heads, int M, int max_chunks);
int vh_attn_rows_bwd_packed(const float* q, int ldq, const float* kcache, const float* vcache, const float* out,
                            int ldo, const float* dout, int lddo, const float* lse2, float* dq, float* dk, float* dv,
                            int ldg, int n_heads, int M, int S_max, int mode, const int32_t* seg_start,
                            const int32_t* seg_len, const int32_t* seg_x_len, int n_seg, const int32_t* items,
                            int n_items, int chunk_keys, int max_chunks, const int32_t* blocks, int n_blocks,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- K8b: single-row decode attention over the KV cache (HBM-bound) -------------------------
 * replaces SDPA with q-len 1 (valle/models/modules.py:167 reached via :336-338).
 * q (B, ldq); keys 0 .. cache_len[b] + len_bias - 1 of row b are attended (len_bias = 1 when the
 * new K/V row was just appended by vh_linear_qkv and cache_len is not yet incremented).
 * n_split >= 1 splits the key range of one (b,head) over n_split workgroups; then `partial`
 * must hold vh_attn_decode_ws_bytes(B, n_heads, n_split) bytes: the split records followed by one ticket word per
 * (b, head).  The records are combined in split order by a second launch (default) or, with VH_TUNE_DECODE_COMBINE = 1,
 * inside the same launch by whichever workgroup finishes last; for that form the TICKET WORDS (the last B * n_heads * 4
 * bytes, rounded up to 16) MUST BE ZERO before the first call on a workspace; every call leaves them zero (calls on one
 * workspace must be stream-ordered).  out (B, ldo). */
size_t vh_attn_decode_ws_bytes(int B, int n_heads, int n_split);
int vh_attn_decode(const float* q, int ldq, const float* kcache, const float* vcache, float* out,
                   int ldo, const int32_t* cache_len, int len_bias, int B, int n_heads, int S_max,
                   int n_split, void* partial, void* stream);
/* ---- decode attention over a shared prompt (the beams of ONE utterance) ------------------------------------------
 * replaces the same SDPA (valle/models/modules.py:167) for generate()'s num_beams rows, whose first prefix_len keys are the
 * same bits in every row (valle_ar.py:135-138 replicates one utterance): kprefix / vprefix (1, h, prefix_S, 64) are read
 * once per step for all B beams (a beam is a lane of the score tile), ksuffix / vsuffix (B, h, S_suf, 64) hold each
 * beam's generated rows, suffix_len[b] + len_bias of them attended.  Bytes per call: 2 (prefix_len + sum_b suffix) 64 h 4
 * instead of 2 B (prefix_len + suffix) 64 h 4.  Two launches: one whose workgroups take either four 32-key blocks of the
 * prefix for all beams or one (beam, head, key split) of the suffixes — a split record each — and one that merges the
 * records of every (beam, head).  fp32, deterministic (fixed merge order); results differ from vh_attn_decode's by
 * summation order only.  ceil(prefix_len / 32) + n_split_suffix <= 256.
 * partial: vh_attn_decode_shared_ws_bytes() bytes, no initialisation needed. */
size_t vh_attn_decode_shared_ws_bytes(int B, int n_heads, int prefix_len, int n_split_suffix);
int vh_attn_decode_shared(const float* q, int ldq, const float* kprefix, const float* vprefix, int prefix_len,
                          int prefix_S, const float* ksuffix, const float* vsuffix, float* out, int ldo,
                          const int32_t* suffix_len, int len_bias, int B, int n_heads, int S_suf, int n_split_suffix,
                          void* partial, size_t partial_bytes, void* stream);
/* ---- decode attention over several shared prompts (the beams of SEVERAL utterances) ------------------------------------
 * vh_attn_decode_shared for G = B / beams utterances in one call: row b is a beam of utterance (group) b / beams, and its
 * first prefix_len[b / beams] keys are that utterance's prompt.  kprefix / vprefix (G, h, prefix_S, 64): one prompt per group,
 * read once per step for the group's beams (the columns of a score tile are the beams of ONE group; a second pass serves beams
 * 32..63).  prefix_len: DEVICE int32 (G), 1 <= prefix_len[g] <= prefix_cap (a larger value is cut at prefix_cap) — a captured
 * step serves later calls whose prompts have other lengths.  prefix_cap (host, 1 <= prefix_cap <= prefix_S) sizes the grid
 * and the record stride: ceil(prefix_cap / 32) + n_split_suffix <= 256 slots per (row, head).  ksuffix / vsuffix, suffix_len,
 * len_bias, n_split_suffix and out as in vh_attn_decode_shared.  The same two launches: prefix workgroups (group, head, four
 * 32-key blocks) and suffix workgroups (row, head, split) in one, the merge per (row, head) in the other.  A block wholly
 * beyond its group's prefix_len loads nothing and writes no record, and the merge of a row reads only the slots its group
 * wrote: the workspace needs no initialisation and may hold anything, as may every cache row beyond a length.  fp32,
 * deterministic (no atomics, fixed merge order).  beams == 1 (no sharing) and G == 1 are legal; for G == 1 the records and
 * their order are vh_attn_decode_shared's.  B <= 64, B % beams == 0.
 * prefix_len[g] <= 0 PARKS group g (ABI 134; queued decoding keeps the rows of a group without an utterance in the launch):
 * neither its prefix nor its suffix workgroups load anything or write a record, and the merge writes exactly 0.0 into its
 * rows without reading a slot — no K/V bytes, and finite rows whatever the caches and the workspace hold.  For every group
 * with prefix_len[g] >= 1 the records, their order and the output bits are what they were before.
 * partial: vh_attn_decode_shared_groups_ws_bytes() = B h (ceil(prefix_cap / 32) + n_split_suffix) records of 72 floats. */
size_t vh_attn_decode_shared_groups_ws_bytes(int B, int n_heads, int prefix_cap, int n_split_suffix);
int vh_attn_decode_shared_groups(const float* q, int ldq, const float* kprefix, const float* vprefix,
                                 const int32_t* prefix_len, int prefix_cap, int prefix_S, const float* ksuffix,
                                 const float* vsuffix, float* out, int ldo, const int32_t* suffix_len, int len_bias, int B,
                                 int beams, int n_heads, int S_suf, int n_split_suffix, void* partial, size_t partial_bytes,
                                 void* stream);
/* ---- decode attention at a head width other than 64 ------------------------------------------------------------------
 * vh_attn_decode's contract over fp32 caches (B, h, S_max, head_dim): keys 0 .. cache_len[b] + len_bias - 1 of row b,
 * out (B, ldo) at columns head * head_dim.  scale is the softmax scale (callers pass (float)(1 / sqrt((double)head_dim)),
 * the reference's head_dim ** -0.5).  head_dim: a multiple of 4 from 16 to 256 (64 included, for comparisons; anything
 * else is refused with VH_EUNSUPPORTED).  n_split > 1 splits the key range of a (b, head) over n_split workgroups whose
 * records (round_up(head_dim + 2, 4) floats each) a second launch adds in split order: partial must hold
 * vh_attn_decode_hd_ws_bytes(B, n_heads, head_dim, n_split) bytes (partial_bytes says how many it holds), no
 * initialisation needed.  Deterministic. */
size_t vh_attn_decode_hd_ws_bytes(int B, int n_heads, int head_dim, int n_split);
int vh_attn_decode_hd(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                      const int32_t* cache_len, int len_bias, int B, int n_heads, int head_dim, int S_max, float scale,
                      int n_split, void* partial, size_t partial_bytes, void* stream);

/* ---- many-row attention (forward) at a head width other than 64 ------------------------------------------------------
 * vh_attn_rows without a cache layout: one flash kernel over fp32 q (B, h, Tq, head_dim), k / v (B, h, Tk, head_dim) and
 * out (B, h, Tq, head_dim) given as STRIDED VIEWS with unit stride in the last dimension — element (b, head, row, c) of an
 * operand lies at base + b * sb + head * sh + row * sr + c (strides in floats) — so the per-head column blocks of a
 * (rows, 3 d) QKV projection are read in place and out is the per-head columns of a (rows, d) buffer: no transposition
 * pass, no staging copy, and no (B, h, Tq, Tk) score map (scores live in registers, K / V tiles in LDS).
 * scale is the softmax scale (callers pass (float)(1 / sqrt((double)head_dim))).  A pure addition of ABI 146: no earlier
 * symbol, struct or behaviour changes, and VH_VERSION stays.
 * Masks: the analytic modes of vh_attn_rows with its exact semantics — query row i sits at key position q_off + i,
 * q_off = Tk - Tq; kvl(b) = kv_len ? min(kv_len[b], Tk) : Tk; xl(b) = x_len_dev ? x_len_dev[b] : x_len;
 *   VH_MASK_FULL   : key j visible iff j < kvl(b)
 *   VH_MASK_PREFIX : key j visible iff j < kvl(b) && (j < xl(b) || (q_off+i >= xl(b) && j <= q_off+i))   (causal: x_len = 0)
 *   VH_MASK_EXPLICIT is refused (VH_EUNSUPPORTED): caller-supplied masks keep the materialised route.
 * A row with kv_len[b] <= 0 has no visible key: its workgroups load no key tile and every query of the row gets NaN in all
 * its head_dim outputs (0 / 0 — what vh_attn_rows at width 64 and SDPA give for a fully masked row); with kv_len[b] >= 1
 * every query sees key 0 in either mode.  Keys kvl(b) .. Tk - 1 are read (they meet weight 0) and must be finite, as for
 * vh_attn_rows.
 * head_dim: a multiple of 4 from 16 to 128 (64 included, for comparisons); anything else — 132..256 too, which the decode
 * kernel takes — is VH_EUNSUPPORTED.  One body compiled for NB = ceil(head_dim / 32) in {1, 2, 3, 4}; columns head_dim ..
 * 32 NB - 1 are zero-filled on chip and never loaded or stored: nothing outside the operands' head_dim columns is touched.
 * All checks run before any launch: a null q / k / v / out, a mode that is not one of the three, B / n_heads / Tq <= 0 or
 * Tq > Tk, a stride that is not a multiple of 4 floats (rows must stay 16-byte aligned) -> VH_EINVAL; a q / k / v / out that
 * is not 16-byte aligned -> VH_EALIGN; a negative k / v row stride, or one that puts key row Tk - 1 more than 2^30 floats
 * after row 0 (the kernel's key offsets are 32-bit) -> VH_EUNSUPPORTED.  Deterministic (no atomics). */
int vh_attn_rows_hd(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                    const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                    const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                    float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                    int B, int n_heads, int head_dim, int Tq, int Tk, float scale,
                    int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len, void* stream);

/* ---- training on flash attention at a head width other than 64 (pure additions of ABI 146: VH_VERSION stays) ----------
 * vh_attn_rows_hd_lse: vh_attn_rows_hd — the same kernel body, checks and bits of `out` — that also stores, for every query
 *   row, lse2[(b * n_heads + head) * Tq + i] = log2(sum_j exp2(s_ij)) over the visible keys, s = scale * log2(e) * q k^T:
 *   vh_attn_rows_lse's units.  lse2 is (B, n_heads, Tq), contiguous, 16-byte aligned (null -> VH_EINVAL, misaligned ->
 *   VH_EALIGN); a query without a visible key gets -inf.
 * vh_attn_rows_hd_bwd: dq, dk, dv of that forward given dout, for Tq == Tk == T.  Two launches (queries as lanes: dQ and
 *   D = rowsum(dO o O); keys as lanes: dK, dV), P recomputed tile by tile from lse2, no (B, h, T, T) map, no atomics: the same
 *   call twice gives the same bits.  q / k / v / out / dout are strided views as above (batch, head, row strides in floats,
 *   unit stride in the last dimension); dq, dk and dv are views of the same shape that SHARE one stride set (g_sb, g_sh,
 *   g_sr): the column blocks of one (rows, 3 d) gradient buffer.  Every element of dq / dk / dv inside (B, h, T, head_dim)
 *   is written exactly once, zeros included (keys at or beyond kv_len[b], keys no query sees; a row with kv_len[b] <= 0 gets
 *   dq = dk = dv = 0 and no NaN): the caller may hand in uninitialised memory.  Nothing outside the views is written.
 *   ws: device scratch of vh_attn_rows_hd_bwd_ws_bytes(B, n_heads, T) bytes (the D vector, B h T floats), 16-byte aligned.
 *   Masks, head widths and the scale are vh_attn_rows_hd's.  All checks run before any launch: a null pointer (ws included),
 *   an unknown mode, B / n_heads / T <= 0, a stride that is not a multiple of 4 floats, a workspace smaller than needed,
 *   a grid that does not fit -> VH_EINVAL; VH_MASK_EXPLICIT, a head width outside the served set, a negative q / k / v /
 *   dout row stride or one that puts row T - 1 more than 2^30 floats after row 0 (those rows are addressed by 32-bit
 *   offsets) -> VH_EUNSUPPORTED; a pointer that is not 16-byte aligned -> VH_EALIGN. */
int vh_attn_rows_hd_lse(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                        const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                        const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                        float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                        int B, int n_heads, int head_dim, int Tq, int Tk, float scale,
                        int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len, float* lse2, void* stream);
size_t vh_attn_rows_hd_bwd_ws_bytes(int B, int n_heads, int T);
int vh_attn_rows_hd_bwd(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                        const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                        const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                        const float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                        const float* dout, int64_t d_sb, int64_t d_sh, int64_t d_sr,
                        const float* lse2, float* dq, float* dk, float* dv, int64_t g_sb, int64_t g_sh, int64_t g_sr,
                        int B, int n_heads, int head_dim, int T, float scale, int mode, int x_len,
                        const int32_t* x_len_dev, const int32_t* kv_len, void* ws, size_t ws_bytes, void* stream);

/* ---- perf mode of the decode step: bf16 K/V cache (opt-in; never the parity path) ---------------
 * SURVEY.md section 7's "perf mode": the K/V cache — 93 % of the bytes a decode step reads at configs[1] — stored
 * as bf16 (B, h, S_max, 64), everything else (weights, q, softmax, accumulators, residual stream) fp32 as in the parity
 * path.  Greedy tokens are NOT guaranteed to equal the reference's; teacher-forced logits agree to atol 5e-2.
 *   vh_kv_to_bf16            narrows the first `rows` rows of n_streams (b, head) streams of an fp32 cache (row stride
 *                            64, stream stride S_src * 64) into a bf16 cache (stream stride S_dst * 64), round to
 *                            nearest even: the prompt pass runs in fp32 and is narrowed once;
 *   vh_linear_qkv_folded_kv16  vh_linear_qkv_folded for one new row per sequence with the K / V rows appended as bf16;
 *   vh_attn_decode_kv16      vh_attn_decode (one (b, head) per workgroup, no key split) over the bf16 cache;
 *   vh_attn_decode_kv16_split  the same with the key range of a (b, head) split over n_split = 1..16 workgroups (ranges of
 *                            32-key chunks; n_split == 1 IS vh_attn_decode_kv16's launch, bit for bit).  For n_split > 1
 *                            `partial` must hold vh_attn_decode_ws_bytes(B, n_heads, n_split) bytes (partial_bytes says how
 *                            many it holds; no initialisation needed); the records are added in split order by a second
 *                            launch: deterministic, results differ from the unsplit form's by summation order only;
 *   vh_attn_decode_shared_kv16  vh_attn_decode_shared over 16-bit prefix and suffix caches: the prompt's K / V are read once
 *                            per step for all beams at half the bytes, widened to fp32 in registers (q is NOT rounded: fp32
 *                            arithmetic on the rounded cache).  Same records, same bound ceil(prefix_len / 32) +
 *                            n_split_suffix <= 256 (n_split_suffix = 1..16), same workspace (vh_attn_decode_shared_ws_bytes). */
int vh_kv_to_bf16(const float* src, uint16_t* dst, int n_streams, int rows, int S_src, int S_dst, void* stream);
int vh_linear_qkv_folded_kv16(const float* A, int lda, const float* Wf, const float* c1, const float* c2, float* q_out,
                              int ldq, uint16_t* kcache16, uint16_t* vcache16, const int32_t* cache_len, int B,
                              int d_model, int n_heads, int S_max, float ln_eps, void* stream);
int vh_attn_decode_kv16(const float* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, float* out, int ldo,
                        const int32_t* cache_len, int len_bias, int B, int n_heads, int S_max, void* stream);
int vh_attn_decode_kv16_split(const float* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, float* out, int ldo,
                              const int32_t* cache_len, int len_bias, int B, int n_heads, int S_max, int n_split,
                              void* partial, size_t partial_bytes, void* stream);
int vh_attn_decode_shared_kv16(const float* q, int ldq, const uint16_t* kprefix16, const uint16_t* vprefix16, int prefix_len,
                               int prefix_S, const uint16_t* ksuffix16, const uint16_t* vsuffix16, float* out, int ldo,
                               const int32_t* suffix_len, int len_bias, int B, int n_heads, int S_suf, int n_split_suffix,
                               void* partial, size_t partial_bytes, void* stream);

/* ---- which kernels a decode-attention call launches (ABI 139; read-only, launches nothing, touches no GPU state) ------
 * vh_attn_decode_form runs the named entry point's own argument check and its dispatch plan, with the current vh_set_tuning
 * knobs, as for a call with valid 16-byte-aligned pointers, ldq = ldo = n_heads * head_dim and len_bias = 1, and returns
 * what that entry point would return: VH_OK and the form in *out, or the entry's refusal code with vh_last_error() set to
 * the entry's own message (*out is zeroed).
 *   entry: VH_ATTN_ENTRY_* names one of the seven vh_attn_decode* functions; head_dim is read by VH_ATTN_ENTRY_HD only (the
 *   others are width 64); prefix is prefix_len (SHARED, SHARED_KV16) or prefix_cap (SHARED_GROUPS) and prefix_S the rows of the
 *   prefix cache; beams is read by SHARED_GROUPS only; S_max is the capacity of the rows' own cache (S_suf of the shared
 *   forms); ws_bytes is the partial_bytes argument (VH_ATTN_ENTRY_DECODE, whose signature has none, ignores it).
 * out: the kernel (VH_ATTN_K_*) with its template arguments (nw waves and d register sets of the width-64 kernels; lk lanes
 * per key and nv slots per lane of the hd kernel; 0 where the kernel has none), grid and block; whether the split records
 * are combined inside the launch and the byte offset of its ticket words in the workspace; the second launch (VH_ATTN_2ND_*)
 * with grid and block; records per (row, head), floats per record and the workspace bytes the form needs.
 * vh_attn_decode_form_row(i, out) lists the compiled first kernels, i = 0, 1, ...: kernel, nw, d, lk, nv (the rest zero);
 * VH_EINVAL past the last row.  Every form vh_attn_decode_form returns is one of these rows. */
enum { VH_ATTN_ENTRY_DECODE = 0, VH_ATTN_ENTRY_KV16 = 1, VH_ATTN_ENTRY_KV16_SPLIT = 2, VH_ATTN_ENTRY_SHARED = 3,
       VH_ATTN_ENTRY_SHARED_GROUPS = 4, VH_ATTN_ENTRY_SHARED_KV16 = 5, VH_ATTN_ENTRY_HD = 6 };
enum { VH_ATTN_K_NONE = 0, VH_ATTN_K_BURST = 1, VH_ATTN_K_RING = 2, VH_ATTN_K_RING16 = 3, VH_ATTN_K_RING16_SPLIT = 4,
       VH_ATTN_K_HD = 5, VH_ATTN_K_SHARED = 6, VH_ATTN_K_SHARED_GROUPS = 7, VH_ATTN_K_SHARED16 = 8 };
enum { VH_ATTN_2ND_NONE = 0, VH_ATTN_2ND_COMBINE = 1, VH_ATTN_2ND_HD_COMBINE = 2, VH_ATTN_2ND_MERGE = 3,
       VH_ATTN_2ND_MERGE_GROUPS = 4 };
typedef struct vh_attn_decode_form_info {
    int kernel;                   /* VH_ATTN_K_* */
    int nw, d, lk, nv;
    unsigned grid[3], block;
    int fused_combine;            /* the last workgroup of a (row, head) to arrive adds the split records */
    size_t ticket_offset;         /* fused_combine: where the ticket words start in the workspace */
    int second;                   /* VH_ATTN_2ND_* */
    unsigned second_grid, second_block;
    int records, record_floats;   /* per (row, head); 0 records: no workspace */
    size_t ws_bytes;
} vh_attn_decode_form_info;
int vh_attn_decode_form(int entry, int B, int n_heads, int head_dim, int S_max, int n_split, int prefix, int prefix_S,
                        int beams, size_t ws_bytes, vh_attn_decode_form_info* out);
int vh_attn_decode_form_row(int i, vh_attn_decode_form_info* out);

/* ---- K12/K13: greedy sampling + decode-state update + next-token embedding ------------------
 * replaces topk_sampling(top_k=1) (valle/models/utils.py:46-68: argmax, lowest index on ties),
 * the EOS bookkeeping valle/models/valle_ar.py:167-171 and the re-embedding :143-144 for the
 * next step.  `codes` (B, codes_stride) int64 is the growing `prompt_codes` of the reference
 * (BOS + prompt pre-filled); audio_pos[b] = index of the token produced now.  Per row b:
 *   p = audio_pos[b]; tok = (codes[b][p-1]==eos) ? eos : argmax(logits[b,:V]); codes[b][p] = tok;
 *   if (tok==eos) eos_count[p - (pos_base?pos_base[b]:0)] += 1;
 *   x_next[b,:] = audio_emb[tok,:] + pe[p*d + :]; audio_pos[b] = p+1; cache_len[b] += 1.
 * eos_count[s] == B means every row had finished at step s (the reference's break, :169-170);
 * the host polls it every few steps instead of synchronising every step. */
int vh_greedy_step(const float* logits, int ldl, int V, int eos, int64_t* codes,
                   int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base,
                   const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                   float* x_next, int B, int d, void* stream);

/* ---- queued decoding: poll and re-arm the groups of a decode launch (ABI 134) -------------------------------------------
 * The B rows of a grouped decode (vh_attn_decode_shared_groups) are G = B / beams groups, group g the rows g * beams ..
 * g * beams + beams - 1.  Between two replays of the captured step the host may hand a finished group's rows to another
 * utterance: every per-row quantity the step reads (codes, cache_len, audio_pos, pos_base, prefix_lens) is a device array.
 *
 * vh_decode_groups_poll (one launch, one wave per group, plain stores, deterministic):
 *   group_done[g]  = 1 when every beam's latest token codes[b][audio_pos[b] - 1] is eos, or when every beam has produced
 *                    audio_pos[b] - pos_base[b] >= max_new tokens; else 0 (an audio_pos outside 1 .. codes_width reads nothing
 *                    and counts as not finished);
 *   group_steps[g] = max over the group's beams of audio_pos[b] - pos_base[b];
 *   maxima[0..3]   = max cache_len and max audio_pos over ALL rows, then the same two over the rows of groups that are not
 *                    done (-2^30 when there is none).  The host re-arms or parks every done group before it replays, so
 *                    maxima[2] + n <= S_suf and maxima[3] + n <= codes_width bound the next n steps' K/V appends, token
 *                    writes and positional rows; maxima[0..1] are the high-water marks.
 * It replaces the eos_count[step] == B scan of the static schedule, which has no meaning once rows start at different steps.
 *
 * vh_decode_group_reset (one launch, one workgroup per row of the group):
 *   prompt_len >= 1 (BOS + prompt_len - 1 first-codebook ids in `prompt`, a device array): for the group's rows
 *     codes[b][0 .. codes_width) = BOS, prompt, then eos to the end; cache_len[b] = 0; audio_pos[b] = pos_base[b] =
 *     prompt_len; sum_logprobs[b] = 0; prefix_lens[group] = prefix_len (the keys of the group's region of the prefix cache:
 *     text + BOS + prompt, >= prompt_len).  The row's first sample (vh_greedy_step / vh_sample_step on the group's rows) then
 *     writes codes[b][prompt_len]; hand it a scratch counter in place of cache_len — the first sample appends no K/V row, and
 *     cache_len[b] = 0 is where the first replayed step appends.
 *   prompt_len == 0 parks the group: prefix_lens[group] = 0 (see vh_attn_decode_shared_groups) and for its rows
 *     codes[b][pos_base[b]] = eos, audio_pos[b] = pos_base[b] + 1, cache_len[b] = 0 — the state of a fresh row whose first
 *     token was EOS.  Nothing else of codes is touched: every further step finds EOS at audio_pos - 1 and writes EOS at
 *     audio_pos.  Called again at every poll it rewinds the rows, so a parked row never moves more than the steps between two
 *     polls from its base.  sum_logprobs is left as it is.  (A pos_base outside 1 .. codes_width - 2 is pulled into it.) */
int vh_decode_groups_poll(const int64_t* codes, int64_t codes_stride, int codes_width, const int32_t* cache_len,
                          const int32_t* audio_pos, const int32_t* pos_base, int eos, int B, int beams, int max_new,
                          int32_t* group_done, int32_t* group_steps, int32_t* maxima, void* stream);
int vh_decode_group_reset(int64_t* codes, int64_t codes_stride, int codes_width, const int64_t* prompt, int prompt_len,
                          int prefix_len, int bos, int eos, int group, int B, int beams, int32_t* cache_len,
                          int32_t* audio_pos, int32_t* pos_base, float* sum_logprobs, int32_t* prefix_lens, void* stream);

/* ---- K11 + K12/K13 in ONE launch (opt-in; DESIGN.md 3.20 has the A/B) -----------------------------
 * logits[b,:V] = x[b,:] . proj_w^T (the head: no bias, valle_ar.py:29,158) and, in the same launch, everything
 * vh_greedy_step does with them: every 16-column workgroup publishes its (largest logit, lowest column) per row, the
 * last workgroup to arrive per group of rows picks the tokens, does the EOS bookkeeping and builds x_next.  Same
 * results as vh_linear + vh_greedy_step bit for bit (the logits are the same sums, the arg-max has the same tie rule).
 * B <= 64, d in {128, 256, 512, 1024}; x_next may be x.  workspace: vh_head_greedy_ws_bytes(B, V) bytes, 16-byte
 * aligned, ZEROED once before the first call (the launches leave it zeroed where it matters). */
size_t vh_head_greedy_ws_bytes(int B, int V);
int vh_head_greedy(const float* x, int ldx, const float* proj_w, float* logits, int ldl, int V, int eos,
                   int64_t* codes, int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base,
                   const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len, float* x_next,
                   int B, int d, void* workspace, size_t workspace_bytes, void* stream);

/* ---- K12 (stochastic): temperature / top-k / top-p sampling + the same state update ----------
 * replaces topk_sampling (valle/models/utils.py:46-68) incl. the published semantics of
 * transformers==4.38.2 top_k_top_p_filtering (top-k keeps ties of the k-th score, top_k <= 0 keeps
 * all; top-p drops, from the smallest, entries whose cumulative probability is <= 1 - top_p and
 * always keeps the largest), torch.multinomial and the log-prob gather; then the bookkeeping of
 * vh_greedy_step plus sum_logprobs[b] += logprob while row b has not finished (valle_ar.py:167).
 * Randomness is a counter-based generator keyed on (seed, row, audio_pos[b]) — replaying a captured
 * graph draws fresh numbers; the stream is NOT torch's, so parity is distributional.  V <= 2048 (wider rows: vh_sample_step_wide).
 * One filter and one seed for every row of the launch, the row's index b as the generator's `row`; a seed, key and filter PER
 * ROW: vh_sample_step_rows below. */
int vh_sample_step(const float* logits, int ldl, int V, int eos, int top_k, float top_p,
                   float temperature, uint64_t seed, int64_t* codes, int64_t codes_stride,
                   int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                   const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                   float* x_next, int B, int d, void* stream);

/* ---- K12 (stochastic, wide): vh_sample_step for 1 <= V <= VH_SAMPLE_MAX_V --------------------------------
 * Same signature and semantics as vh_sample_step (temperature, top-k with ties, top_k <= 0 keeps all, top-p, the draw
 * from uniform01(seed, row, audio_pos[b]), the filtered log-prob, sum_logprobs, EOS, eos_count, the append, x_next,
 * audio_pos / cache_len) for vocabularies up to 16384 entries.  One 1024-thread workgroup per row with the row's scores
 * and indices in LDS (128 KiB); fast path (0 < top_k < V, top_p == 1): radix select of the k-th score and the draw over
 * the survivors in index order; otherwise the survivors are sorted (descending, lower index first on ties) and the
 * top-p cut and the draw are block-parallel scans.  Support and log-prob are vh_sample_step's; the token for a given
 * seed is too unless the draw falls within fp32 rounding of a CDF boundary (the sums run in another order). */
int vh_sample_step_wide(const float* logits, int ldl, int V, int eos, int top_k, float top_p,
                        float temperature, uint64_t seed, int64_t* codes, int64_t codes_stride,
                        int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                        const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                        float* x_next, int B, int d, void* stream);

/* ---- K12 (stochastic) with PER-ROW sampling: every row's seed, draw key and filter from device memory ----------
 * One record per row, indexed as logits / codes / audio_pos are.  32 bytes, 16-byte aligned (two 16-byte loads per
 * workgroup): seed at byte 0, key at 8, top_k at 12, top_p at 16, temperature at 20, reserved[0] at 24, reserved[1] at 28.
 *   seed         the row's own seed: the draw at audio position p is uniform01(seed, key, p) — nothing of the launch (its
 *                scalar seed, the decoder's seed_dev, the row's index in the launch) enters it;
 *   key          the `row` of the counter-based generator: the beam index WITHIN the request, so the beams of one request
 *                draw different numbers from one seed and the same numbers wherever the request's rows stand;
 *   top_k        as vh_sample_step's (<= 0 keeps all).  top_k == 1 is vh_greedy_step's token: the largest logit, the lowest
 *                index on ties (compared as values: -0.0 == +0.0), log-probability exactly 0, whatever top_p and temperature say;
 *   top_p        as vh_sample_step's;
 *   temperature  > 0 (NOT checked: the records live on the device); the kernel divides 1.0f by it in fp32, as the host does
 *                for vh_sample_step, so a record that holds a call's values filters exactly as that call.
 *   reserved[0]  window K of REPETITION-AWARE sampling (VALL-E 2); 0: off — the row samples exactly as above, bit for bit;
 *   reserved[1]  max_repeats R (read only when window != 0).  With window = K >= 1, at audio position p (BOS at 0):
 *                  1. the first draw is exactly the draw above: same filter, u1 = uniform01(seed, key, p), same token c;
 *                  2. n_c = how many of the row's own codes[max(1, p - K) .. p - 1] equal c (prompt codes count, BOS never
 *                     does, fewer than K entries early on);
 *                  3. n_c > R: the token is drawn again from softmax(logits / temperature) over all V entries — no top-k, no
 *                     top-p, walked in index order — with u2 = uniform01(seed, key, p | 0x40000000) (bit 30: apart from
 *                     every first draw and from the NAR stage's streams, bit 31).  It may be c again and may be EOS;
 *                     sum_logprobs takes ITS log-probability under the unfiltered distribution in place of the filtered one;
 *                  4. a finished row (codes[p - 1] == eos) skips 2 and 3 and writes EOS as ever;
 *                  5. top_k == 1 stays greedy whatever else the record says: the two words are ignored.
 *                The ratio threshold t_r of the paper over its window K is max_repeats = floor(t_r * K) (K = 10, t_r = 0.1:
 *                window 10, max_repeats 1).  The scalar entries (one filter for every row) and vh_categorical_rows_keyed (the
 *                NAR stage) do not read the two words.
 * The caller may rewrite records between launches (stream-ordered); a captured graph holds the pointer, not the values. */
typedef struct {
    uint64_t seed;
    uint32_t key;
    int32_t top_k;
    float top_p;
    float temperature;
    uint32_t reserved[2];
} vh_row_sampling;

/* vh_sample_step / vh_sample_step_wide with rs[b] in place of (top_k, top_p, temperature, seed) and of the row index as
 * the draw key; everything else as there (V <= 2048 / V <= VH_SAMPLE_MAX_V).  rs: device array of B records, not NULL. */
int vh_sample_step_rows(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs, int64_t* codes,
                        int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                        const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                        float* x_next, int B, int d, void* stream);
int vh_sample_step_wide_rows(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs, int64_t* codes,
                             int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                             const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                             float* x_next, int B, int d, void* stream);

/* ---- K12 (stochastic) with PER-ROW LENGTH BOUNDS: at least min_new, at most max_new audio tokens per row ----------
 * One record per decode row, a device array indexed like rs.  8 bytes, 8-byte aligned (one load per workgroup).  A bound
 * of 0 is off; an all-zero record changes nothing.  For row b let p = audio_pos[b] (the position of the token being drawn)
 * and n = p - pos_base[b] (the audio tokens the row has produced before this step):
 *   1. a finished row (codes[p - 1] == eos) writes EOS as ever and reads neither word;
 *   2. max_new > 0 and n >= max_new: the token is EOS, FORCED.  No draw, no repetition-aware count, no redraw;
 *      sum_logprobs[b] is unchanged (a forced token is not the model's choice); eos_count, the token write, x_next,
 *      audio_pos and cache_len behave as for any EOS.  The row produces at most max_new non-EOS tokens.  This test comes
 *      before 3: a record with min_new > max_new behaves as its max_new;
 *   3. n < min_new: EOS is OUTSIDE THE SUPPORT.  Its scaled score is -inf before top-k (ties included), top-p, the
 *      top_k == 1 arg-max and the draw, and in the repetition-aware redraw over all V entries; the row's log-probability is
 *      the one under the distribution without EOS.  The row produces at least min_new non-EOS tokens before EOS can
 *      appear; no path returns a suppressed EOS (not the walk's last entry when rounding leaves none, not the sorted path
 *      with top_k <= 0 or top_k >= V, where the -inf entry stays in the array);
 *   4. the draws stay uniform01(seed, key, p) and uniform01(seed, key, p | 0x40000000): a request's rows remain a function
 *      of the request alone. */
typedef struct {
    int32_t min_new, max_new;
} vh_row_limits;

/* vh_sample_step_rows / vh_sample_step_wide_rows with limits[b] beside rs[b].  limits == NULL: the _rows launch, bit for
 * bit.  With limits, pos_base must not be NULL and V >= 2 (VH_EINVAL), limits 8-byte aligned (VH_EALIGN). */
int vh_sample_step_rows_bounded(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs,
                                const vh_row_limits* limits, int64_t* codes, int64_t codes_stride, int32_t* eos_count,
                                const int32_t* pos_base, float* sum_logprobs, const float* audio_emb, const float* pe,
                                int32_t* audio_pos, int32_t* cache_len, float* x_next, int B, int d, void* stream);
int vh_sample_step_wide_rows_bounded(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs,
                                     const vh_row_limits* limits, int64_t* codes, int64_t codes_stride, int32_t* eos_count,
                                     const int32_t* pos_base, float* sum_logprobs, const float* audio_emb, const float* pe,
                                     int32_t* audio_pos, int32_t* cache_len, float* x_next, int B, int d, void* stream);

/* ---- composite: one AR decode step / hipGraph replay ----------------------------------------
 * The 5 launches per layer of one decode step (LN1+QKV+append, decode attention, out-proj+
 * residual, FeedForward slices, slab reduce + residual) plus head GEMM and vh_greedy_step, enqueued natively
 * (valle/models/valle_ar.py:141-171 with modules.py:336-352).  */
typedef struct {
    const float *ln1_g, *ln1_b, *wqkv, *wo, *bo, *ln2_g, *ln2_b, *w1, *b1, *w2, *b2;
    float *kcache, *vcache;           /* this layer's (B,h,S_max,head_dim) caches, head_dim = d_model / n_heads */
    /* optional vh_ln_fold outputs for (ln1, wqkv) and (ln2, w1, b1); all NULL → LayerNorm applied in
     * the operand load from ln*_g / ln*_b.  Used by the decode step only. */
    const float *wqkv_f, *qkv_c1, *qkv_c2, *w1_f, *w1_c1, *w1_c2;
    /* shared-prompt decoding (vh_ar_decoder_desc.prefix_len > 0): this layer's prompt K / V, (1, h, prefix_S, 64), written
     * once by a one-row prompt pass and read by every beam; kcache / vcache then hold only the beams' generated rows */
    const float *kprefix, *vprefix;
    /* perf mode of the decode step, second half (round 6; with vh_ar_decoder_desc.kv_bf16): h16 copies (vh_h16_format) of the four
     * matrices a step streams — wqkv_f16 (3d, d) and w1_f16 (dff, d) of the FOLDED weights above, wo16 (d, d), w2_16 (d, dff).
     * All four non-NULL: the step's QKV, out-projection and FeedForward launches read them (half the weight bytes; fp32
     * accumulators, fp32 rows, c1 / c2 / biases fp32); any NULL: the fp32 matrices, as before.  A caller that sets them should
     * point qkv_c1 / w1_c1 at the row sums of the ROUNDED matrices (sum_k wqkv_f16[n,k], sum_k w1_f16[n,k]): with the sums of the
     * fp32 fold the epilogue leaves rstd * mean * (rowsum(Wf16) - c1), which grows with a row's |mean| / std. */
    const uint16_t *wqkv_f16, *wo16, *w1_f16, *w2_16;
} vh_layer;

/* d_model: head width 64 (d_model = 64 n_heads) up to 4096; other head widths up to 1024.  At d_model > 1024 (width 64 only) a
 * layer with folded weights (d_model in the K set of vh_linear_folded) runs vh_linear_qkv_folded / vh_linear_folded at the wide K; a layer without
 * them runs vh_layernorm into `attn` (free before the attention writes it and after the out-projection has read it) and
 * the plain vh_linear_qkv / vh_linear: two more launches per layer, any d_model % 64 == 0.  kv_bf16, head_ws and the 16-bit
 * weight copies are d_model <= 1024 forms.  d_model > 4096 is refused with a message naming 4096. */
typedef struct {
    int B, d_model, n_heads, dff, n_layers, S_max, V, eos, n_split;
    float ln_eps;
    const vh_layer* layers;           /* host array of n_layers */
    const float *proj_w;              /* (V, d) */
    const float *audio_emb, *audio_pe;
    float *x;                         /* (B,d) residual stream, holds the current token's embedding */
    float *q, *attn, *hidden, *logits;/* (B,d) (B,d) (B,dff) (B,ldl) scratch; ldl = round_up(V,4) */
    void *attn_partial;               /* vh_attn_decode_ws_bytes() or NULL when n_split == 1 */
    void *gemm_ws;                    /* vh_linear_ws_bytes(B, d_model, dff) bytes or NULL */
    size_t gemm_ws_bytes;
    int32_t *cache_len, *audio_pos, *eos_count;
    const int32_t *pos_base;          /* (B) or NULL */
    int64_t *codes;                   /* (B, codes_stride) growing code sequence */
    int64_t codes_stride;
    /* sampling (valle/config.py:48-51): top_k == 1 → vh_greedy_step, else vh_sample_step (V <= 2048) or
     * vh_sample_step_wide (V <= VH_SAMPLE_MAX_V; a wider V is refused when the decoder is created); per row: row_sampling below */
    int top_k;
    float top_p, temperature;
    uint64_t seed;
    float *sum_logprobs;              /* (B) or NULL */
    /* optional: workspace of vh_ffn_decode_ws_bytes(B, d_model, dff) bytes; with it and folded weights in every
     * layer the FeedForward of a layer is vh_ffn_decode (two launches instead of three). */
    void *ffn_ws;
    size_t ffn_ws_bytes;
    /* perf mode (opt-in): nonzero = every layer's kcache / vcache point at bf16 caches (B,h,S_max,64) and the step
     * runs vh_linear_qkv_folded_kv16 + vh_attn_decode_kv16; needs folded weights in every layer.  n_split > 1: the attention is
     * vh_attn_decode_kv16_split and attn_partial must hold vh_attn_decode_ws_bytes(B, n_heads, n_split) bytes
     * (attn_partial_bytes says how many it holds).  With prefix_len > 0: see below. */
    int kv_bf16;
    /* shared prompt (the reference's generate(): ONE utterance replicated over num_beams rows, valle_ar.py:135-138 — every
     * beam's prompt K/V is the same bits).  prefix_len > 0: the first prefix_len keys of every row live ONCE in
     * layers[i].kprefix / vprefix ((1, h, prefix_S, 64)); layers[i].kcache / vcache are (B, h, S_max, 64) caches of the
     * GENERATED rows only, cache_len[b] counts those, and the step's attention is vh_attn_decode_shared (n_split = key
     * splits of the suffix part).  attn_partial must hold vh_attn_decode_shared_ws_bytes(B, n_heads, prefix_len, n_split)
     * bytes (attn_partial_bytes says how many it holds).  With kv_bf16 the prefix caches are 16-bit as well (kprefix / vprefix
     * then point at uint16_t data) and the attention is vh_attn_decode_shared_kv16: same bound, same workspace. */
    int prefix_len, prefix_S;
    size_t attn_partial_bytes;
    /* optional (opt-in): zeroed workspace of vh_head_greedy_ws_bytes(B, V) bytes; with it and top_k == 1 the head and the
     * greedy step are ONE launch (vh_head_greedy) instead of vh_linear + vh_greedy_step. */
    void *head_ws;
    size_t head_ws_bytes;
    /* optional: a device uint64 ADDED to `seed` by every sampling step (top_k != 1).  A captured graph freezes `seed`; a decoder
     * that serves many generate() calls keeps the call's seed here and rewrites it between calls (valle2_amd/valle_ar.py keeps
     * a decoder per shape: graphs, caches and workspaces survive the call). */
    const uint64_t *seed_dev;
    /* optional (with kv_bf16): an h16 copy of proj_w (V, d) for the head GEMM of the step */
    const uint16_t *proj_w16;
    /* grouped shared prompts (several utterances, each replicated over beams_per_group rows; 0 = the forms above).
     * n_groups > 0: B == n_groups * beams_per_group, row b belongs to group b / beams_per_group; layers[i].kprefix / vprefix
     * are (n_groups, h, prefix_S, 64) with group g's prompt in its first prefix_lens[g] rows (DEVICE int32 (n_groups), read
     * by every step: the caller rewrites it between calls); prefix_cap (<= prefix_S) bounds every length.  kcache / vcache,
     * cache_len and n_split as with prefix_len > 0, which must be 0 here.  The step's attention is
     * vh_attn_decode_shared_groups; attn_partial must hold vh_attn_decode_shared_groups_ws_bytes(B, n_heads, prefix_cap,
     * n_split) bytes.  fp32 caches at head width 64 only: kv_bf16 and other head widths are refused. */
    int n_groups, beams_per_group, prefix_cap;
    const int32_t *prefix_lens;
    /* optional: per-row sampling, a device array of B vh_row_sampling records (16-byte aligned) read by every step.  With it
     * the step samples through vh_sample_step_rows / vh_sample_step_wide_rows whatever top_k says (a record's top_k == 1 is that
     * row's greedy token); top_k, top_p, temperature, seed and seed_dev above are not read, V <= VH_SAMPLE_MAX_V.  Refused with
     * head_ws (the fused greedy head has no sampler behind it).  NULL: the forms above. */
    const vh_row_sampling *row_sampling;
} vh_ar_decoder_desc;

typedef struct vh_ar_decoder vh_ar_decoder;
vh_ar_decoder* vh_ar_decoder_create(const vh_ar_decoder_desc* desc);   /* NULL on bad desc */
void vh_ar_decoder_destroy(vh_ar_decoder* dec);
/* attach (or, with NULL, clear) the per-row length bounds the decoder's sample steps read: a device array of B
 * vh_row_limits records, 8-byte aligned (VH_EALIGN).  Needs a decoder with row_sampling and pos_base (VH_EINVAL) and
 * V >= 2.  Such a decoder always samples through vh_sample_step_rows / vh_sample_step_wide_rows: vh_ar_decoder_create
 * refuses row_sampling together with head_ws, so the fused greedy head (which reads no limits) is never its step.  The captured graphs hold the pointer, so it is set BEFORE vh_ar_decoder_capture (after it: VH_ESTATE); the
 * caller may rewrite the records between steps and replays (stream-ordered).  The descriptor keeps row_sampling as its
 * trailing field. */
int vh_ar_decoder_set_row_limits(vh_ar_decoder* dec, const vh_row_limits* limits);
/* enqueue one step eagerly (no graph) */
int vh_ar_decoder_step(vh_ar_decoder* dec, void* stream);
/* capture one step into a hipGraph on `stream` (which must be a non-null, idle stream) */
int vh_ar_decoder_capture(vh_ar_decoder* dec, void* stream);
/* replay the captured step n_steps times on `stream` */
int vh_ar_decoder_replay(vh_ar_decoder* dec, int n_steps, void* stream);
/* eager steps with hipEvents on every decode-attention launch.  *kernel_ms (optional): mean elapsed time between
 * the start and stop events attached to the kernel's own dispatch (hipExtLaunchKernelGGL) — the kernel's duration
 * as the profiler sees it.  *mean_ms: mean event-to-event time of marker events recorded before and after the
 * launch (an upper bound: it carries event + dispatch overhead); *floor_ms (optional): the same marker bracket
 * with nothing inside it, once per step.  All in milliseconds.  Synchronises the stream; measurement only. */
int vh_ar_decoder_profile_attn(vh_ar_decoder* dec, int n_steps, void* stream, float* mean_ms,
                               float* floor_ms, float* kernel_ms);

/* ---- training path: backward of the row ops (loss.backward() of valle/models/valle_ar.py:86) -----
 * The plain backward GEMMs (dX = dY.W, dW = dY^T.X and the five attention products) are library
 * GEMMs issued by the host; these entry points are the hand-written non-GEMM halves.  Gradient
 * buffers marked "+=" are accumulated with fp32 atomics: the caller zeroes them first. */
/* LayerNorm / AdaptiveLayerNorm backward (modules.py:284, :93-99).  y = s*(gamma*xhat+beta)+t:
 * dx written; dgamma += , dbeta += , and when ada_scale != NULL dscale += , dshift += (all (d)).
 * dres (rows, d) | NULL: added to dx — the gradient of the pre-norm block's residual branch, which bypasses the norm
 * (x feeds norm AND residual add, modules.py:271-279): no separate elementwise add.  dx must not alias dres.
 * dcolsum (d) | NULL: += the column sums of the rows written to dx — the bias gradient of the Linear whose output x
 * was (out-projection / linear_2), without a column-sum launch.
 * dx_drop (rows, d) + drop (both or neither): x = residual + dropout(branch) (modules.py:277-278): the gradient of the
 * BRANCH is the dropped dx.  It is written to dx_drop in the same pass (field row = row, column = column) and dcolsum
 * then sums dx_drop — the branch's Linear bias sits under the dropout — while dx stays the residual stream's gradient. */
int vh_layernorm_bwd(const float* x, const float* gamma, const float* beta, const float* ada_scale,
                     const float* dy, float* dx, float* dgamma, float* dbeta, float* dscale,
                     float* dshift, const float* dres, float* dcolsum, float* dx_drop, const vh_dropout_spec* drop,
                     int rows, int d, float eps, void* stream);
/* exact-erf GELU on a saved pre-activation: dh == NULL → out = gelu(pre); else out = dh*gelu'(pre) */
int vh_gelu(const float* pre, const float* dh, float* out, int64_t n, void* stream);
/* P = softmax(S*scale + mask) in place over rows of (B,h,Tq,Tk) with row stride ld >= Tk; same mask
 * semantics as vh_attn_rows */
int vh_softmax_rows(float* S, int ld, int B, int n_heads, int Tq, int Tk, float scale, int mode,
                    int x_len, const int32_t* x_len_dev, const int32_t* kv_len, const uint8_t* mask,
                    const uint8_t* pad, void* stream);
/* dS = scale * P o (dP - rowsum(dP o P)), in place on dP (both with row stride ld) */
int vh_softmax_bwd(const float* P, float* dP, int ld, int64_t rows, int Tk, float scale, void* stream);
/* mean cross entropy over `rows` rows of (rows, V) logits (F.cross_entropy, valle_ar.py:86):
 * *loss = mean(lse - logit[target]); dlogits (may be NULL) = (softmax - onehot) / rows.
 * A target outside [0, V) (this includes torch's ignore_index -100, which the collate format never
 * emits: it pads with 0, valle/collate.py:35,65) contributes lse only, gets no one-hot term and ORs
 * VH_DEVERR_TARGET into *err_flag (device int32, may be NULL). */
int vh_cross_entropy(const float* logits, int ld, int V, const int64_t* target, float* loss,
                     float* dlogits, int ldd, int rows, int32_t* err_flag, void* stream);
/* embedding backward: dtable[ids[b,t], :] += dout[b, out_t0 + t, :]; ids outside [0, vocab) are skipped
 * (and flagged as in vh_embed_sum_pe).  drop (NULL: none): the forward's vh_embed_sum_pe dropout — dout is multiplied
 * by the regenerated field on the way in (dout_bstride % d == 0 then). */
int vh_embed_bwd(const int64_t* ids, int64_t ids_bstride, int64_t ids_tstride, const float* dout,
                 int64_t dout_bstride, int out_t0, float* dtable, int vocab, int B, int T, int d,
                 int32_t* err_flag, const vh_dropout_spec* drop, void* stream);
/* ---- packed NAR training (ABI 144): the model input over the SEGMENTS of one packed row stream ----------------------
 * n_seg segments lie back to back in out (M, d): segment s starts at row seg_start[s] (ASCENDING in s: the kernels find a
 * row's segment by a binary search over seg_start) and holds x_len[s] text rows, then a_len[s] audio rows:
 *   text row i   = text_table[tokens[s, i]] + pe_text[i]
 *   audio row t  = sum_{j < n(t)} code_tables[j][codes[s, t, j]] + pe_audio[t],  n(t) = n_full for t < prefix[s], else n_rest
 * (the NAR training input: all codebooks for the acoustic prefix, the codebooks below the stage after it; positions restart
 * at 0 for each stream of each segment).  seg_start, x_len, a_len, prefix: device int32 (n_seg); tokens (n_seg, >= max_x_len)
 * int64 with a batch stride; codes (n_seg, >= max_a_len, >= n_full) int64 with batch, frame and codebook strides; code_tables
 * / code_vocab: HOST arrays of n_full device tables and their row counts, 1 <= n_rest <= n_full <= VH_MAX_TABLES.  The
 * additions are vh_embed_sum_pe's in its order — tables in ascending j, the position, then the dropout field of the row's
 * own stream (drop_text / drop_audio, NULL: none) whose row is the PACKED row — so every row of a segment is bit for bit
 * what vh_embed_sum_pe writes for that utterance alone at the same rows of out.  An id outside its table reads row 0 and
 * ORs VH_DEVERR_EMBED_ID into *err_flag.  max_x_len / max_a_len: the longest text / audio stream, which the host holds
 * against pe_text_rows / pe_audio_rows before any launch; a device length beyond them is cut there.  A row in [0, M) that
 * lies in no segment is left alone; no row at or beyond M is written.  VH_EINVAL names the argument for: a null pointer,
 * d not a positive multiple of 4, n_rest / n_full out of range, M <= 0, n_seg <= 0, a PE row count below the longest
 * stream. */
int vh_embed_nar_packed(const int64_t* tokens, int64_t tokens_bstride, const int64_t* codes, int64_t codes_bstride,
                        int64_t codes_tstride, int64_t codes_jstride, const float* text_table, int text_vocab,
                        const float* const* code_tables, const int32_t* code_vocab, int n_full, int n_rest,
                        const float* pe_text, int pe_text_rows, const float* pe_audio, int pe_audio_rows,
                        const int32_t* seg_start, const int32_t* x_len, const int32_t* a_len, const int32_t* prefix,
                        int n_seg, int max_x_len, int max_a_len, float* out, int M, int d, int32_t* err_flag,
                        const vh_dropout_spec* drop_text, const vh_dropout_spec* drop_audio, void* stream);
/* Its backward: dout (M, d) is multiplied by the regenerated field of each row's stream on the way in and every packed row is
 * ADDED (fp32 atomics, no promise of order, as vh_embed_bwd) into the table row its id names: dtext_table for a text row,
 * dcode_tables[j] for j < n(t) for an audio row, so tables j >= n_rest receive prefix frames only.  The gradient row is read
 * once for all its tables; consecutive packed rows that name the same row of a table are added up before the atomic is
 * issued.  dtext_table and any entry of dcode_tables (a HOST array of n_full device pointers) may be NULL: skipped.  Ids out
 * of range are skipped and flagged; nothing is scattered outside a table.  The same refusals as the forward. */
int vh_embed_nar_packed_bwd(const int64_t* tokens, int64_t tokens_bstride, const int64_t* codes, int64_t codes_bstride,
                            int64_t codes_tstride, int64_t codes_jstride, const float* dout, float* dtext_table,
                            int text_vocab, float* const* dcode_tables, const int32_t* code_vocab, int n_full, int n_rest,
                            int pe_text_rows, int pe_audio_rows, const int32_t* seg_start, const int32_t* x_len,
                            const int32_t* a_len, const int32_t* prefix, int n_seg, int max_x_len, int max_a_len, int M,
                            int d, int32_t* err_flag, const vh_dropout_spec* drop_text, const vh_dropout_spec* drop_audio,
                            void* stream);
/* bias gradient: out[c] += sum_r x[r, c] */
int vh_colsum(const float* x, int ld, float* out, int rows, int cols, void* stream);

/* ---- AdaptiveLayerNorm projections of a whole stack (training) ------------------------------------
 * out[i, :] = emb W_i^T + b_i for the n project_layer Linears of a stack (valle/models/modules.py:94-96; n = 2 per
 * EncoderLayer), one (1, K) stage embedding for all, in ONE launch; and their backward in one launch:
 *   dw_i (N, K) = dout_i^T emb (an outer product: the Linear saw one input row), db_i = dout_i   — both WRITTEN,
 *   demb (K) += sum_i dout_i W_i   (fp32 atomics; the caller zeroes it; NULL: not wanted).
 * items: DEVICE array of n descriptors; dw / db / b may be NULL.  N = 2 K for the reference's modules; K % 4 == 0,
 * K <= 2048. */
typedef struct { const float* w; const float* b; float* dw; float* db; } vh_adaproj_item;
int vh_adaproj_fwd(const vh_adaproj_item* items, int n, const float* emb, float* out, int N, int K, void* stream);
int vh_adaproj_bwd(const vh_adaproj_item* items, int n, const float* emb, const float* dout, float* demb, int N, int K,
                   void* stream);

/* ---- NAR stage sampler -------------------------------------------------------------------------
 * replaces `Categorical(logits=logits / temperature).sample()` of ValleNAR.generate
 * (valle/models/valle_nar.py:160) for `rows` rows of (rows, V) logits (row stride ld):
 *   tokens[r * tokens_stride] ~ softmax(logits[r] / temperature)     (inverse CDF in index order, counter
 *   RNG keyed on (seed, r, stream_id): the stream differs from torch's, parity is distributional), or
 *   the arg-max with the lowest index on ties when greedy != 0 (what the parity tests pin).
 * logprob (rows floats, may be NULL) receives log p(token) (0 when greedy). */
int vh_categorical_rows(const float* logits, int ld, int V, int rows, float temperature, int greedy,
                        uint64_t seed, uint32_t stream_id, int64_t* tokens, int64_t tokens_stride,
                        float* logprob, void* stream);

/* vh_categorical_rows keyed on the REQUEST, not on the row's place in the launch (ABI 136).  Packed row r belongs to request
 * g = row_request[r] and is its frame t = row_key[r] (int32 device arrays of `rows` entries); rq = requests[g] is one of
 * n_requests vh_row_sampling records in device memory (16-byte aligned):
 *   the draw      u = uniform01(rq.seed, t, stream_id): the generator of the other samplers, keyed on the frame index inside
 *                 the request — which rows share the launch, their order and their count do not enter;
 *   the scale     rq.top_k == 1: the arg-max over the unscaled logits, the lowest index on ties, log-probability exactly 0;
 *                 otherwise 1.0f / rq.temperature, the fp32 division vh_sample_step_rows does.  rq.temperature > 0 is NOT
 *                 checked: the records live on the device;
 *   not read      rq.key, rq.top_p and any other value of rq.top_k (the reference's NAR stage has no filter, valle_nar.py:160);
 *   the token     goes to tokens[g * request_stride + t * key_stride] (element strides >= 1): codebook n of a (B, Ty_max, Q)
 *                 codes tensor is tokens = codes + n, request_stride = Ty_max * Q, key_stride = Q, n_keys = Ty_max;
 *   guards        a row with g outside [0, n_requests) or t outside [0, n_keys) reads no record and writes nothing.
 * The arithmetic of a row is vh_categorical_rows': one request with row_key[r] = r draws that launch's tokens and
 * log-probabilities bit for bit.  logprob (rows floats, indexed by packed row, may be NULL).  rows == 0 is VH_OK. */
int vh_categorical_rows_keyed(const float* logits, int ld, int V, int rows,
                              const vh_row_sampling* requests, int n_requests,
                              const int32_t* row_request, const int32_t* row_key, int n_keys,
                              uint32_t stream_id,
                              int64_t* tokens, int64_t request_stride, int64_t key_stride,
                              float* logprob /* rows, may be NULL */, void* stream);

/* ---- optimizer step over one flat fp32 buffer ------------------------------------------------
 * replaces optim.AdamW(fused) (valle/models/valle_ar.py:182-194), the global-norm clip
 * `gradient_clip_val` of the Trainer (valle/train_model.py:31-32) and the 1/world scale after the
 * gradient all-reduce, in two launches with no host read:
 *   norm = grad_scale * ||grad||_2 (double accumulation, fixed order: reproducible);
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1;   g = grad * grad_scale * coef;
 *   p *= 1 - lr*wd;  m += (g - m)(1-b1);  v = b2 v + (1-b2) g^2;
 *   p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)       (torch.optim.AdamW, amsgrad off).
 * param/grad/exp_avg/exp_avg_sq: n floats each (n % 4 == 0); zero_grad != 0 clears grad afterwards;
 * norm_out (1 float, optional) receives norm; workspace: vh_adamw_ws_bytes() bytes.
 * block_slot / slot_step (both NULL: every element updates with `step`): torch.optim.AdamW keeps a step
 * count per parameter and skips parameters whose grad is None (NAR trains one stage per step: the other
 * stages' heads and embeddings receive nothing, valle_nar.py:76).  block_slot (n / 64 int32, device) maps
 * each 64-float block to its parameter slot, slot_step (device) holds the slot's own step count for this
 * update, 0 = skip the slot entirely (no decay, no moments, no move).  Needs n % 64 == 0.
 * guard (optional, one int32 on the device): nonzero when the update launch starts = parameters and moments are not
 * touched (the error flag of the range-checking kernels: a step that saw a bad id never reaches the parameters, and
 * the host can read the flag a step later instead of synchronising every step); the gradient is still cleared when
 * zero_grad != 0, so the buffer the next backward accumulates into is zero either way. */
size_t vh_adamw_ws_bytes(void);
int vh_adamw_flat(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                  float max_norm, int zero_grad, void* workspace, float* norm_out, const int32_t* block_slot,
                  const int32_t* slot_step, const int32_t* guard, void* stream);

/* ---- training forward / backward products on the LDS-DMA tile machine --------------------------
 * vh_linear_ex = vh_linear (same tile kernels, M of any size) with the two epilogues training needs:
 *   pre_out != NULL : the pre-activation acc + bias is ALSO stored to pre_out (row stride ldp) — the
 *                     forward of FeedForward.linear_1 keeps it for the GELU backward (modules.py:221);
 *   act == VH_ACT_GELU_ERF_D (pre_out required) / VH_ACT_MUL (residual required, no bias, no pre_out): the pair the
 *                     training step uses — forward stores gelu'(pre) in pre_out, backward multiplies by it; the
 *                     GELU'-epilogue of VH_ACT_GELU_BWD (erf + exp on 64 values per lane and tile) held the biggest
 *                     product of the backward at 75 % MFMA-busy against 84 % for a plain epilogue.
 *   act == VH_ACT_GELU_BWD : out = acc * gelu'(residual[m][n]) — the backward through nn.GELU fused into
 *                     the dX = dY . W product of linear_2 (residual = the saved pre-activation).
 *   dcolsum != NULL (N % 128 == 0): the column sums of `out` are ADDED to dcolsum (N floats, fp32 atomics, one per
 *                     column and tile) — the gradient of linear_1's bias falls out of the product that makes its
 *                     pre-activation's gradient, without a column-sum launch.
 * The backward's dX = dY . W products run on this NT form with W handed over transposed (vh_transpose),
 * so K here is the forward's N: pad it to a multiple of 32 with zero columns for the fast kernel.
 *   workspace (optional, vh_linear_ex_ws_bytes(M, N, K) bytes, 16-byte aligned): lets the product split its TAIL.
 *                     128 x 128 tiles are dealt to 256 CUs, so T tiles cost ceil(T / 256) rounds: 320 tiles (10240
 *                     training positions x a 512-wide projection) take as long as 512.  With a workspace the tiles
 *                     beyond the last multiple of 256 — when they would occupy at most half of the CUs — are computed
 *                     as 2..8 K slices each (one workgroup per slice, raw sums to the workspace) and a small second
 *                     launch adds the slices in slice order and applies the epilogue: deterministic, but those tiles'
 *                     sums are associated differently from an unsplit run.  vh_linear_ex_ws_bytes returns 0 for a
 *                     shape that is not split (<= 16 MiB otherwise); NULL or a smaller workspace = never split. */
/*   drop (NULL: none; act NONE / GELU_ERF / GELU_ERF_D, N % 4 == 0, K % 32 == 0): out = dropout(act(acc + bias)) +
 *                     residual with the field indexed by (m, n) — dropout1 / dropout2 inside the out-projection's /
 *                     linear_2's epilogue (modules.py:277-278) and FeedForward's dropout inside linear_1's (:219).
 *                     With VH_ACT_GELU_ERF_D the stored derivative is multiplied by the same keep / (1 - p) factor, so
 *                     the backward's VH_ACT_MUL epilogue already yields the gradient through dropout AND GELU. */
size_t vh_linear_ex_ws_bytes(int M, int N, int K);
int vh_linear_ex(const float* A, int lda, const float* W, const float* bias, const float* residual, int ldr,
                 float* out, int ldo, float* pre_out, int ldp, float* dcolsum, int M, int N, int K, int act,
                 const vh_dropout_spec* drop, void* workspace, size_t workspace_bytes, void* stream);

/* out (cols, ldo) = in (rows, cols)^T; out rows are zero-filled from `rows` up to ldo. */
int vh_transpose(const float* in, int ldi, int rows, int cols, float* out, int ldo, void* stream);
/* The same for n matrices in ONE launch (every Linear weight of the stack, once per optimizer step, for the dX
 * products of the backward): `items` is a DEVICE array of n descriptors; tile0 = number of 32x32 output tiles of the
 * items before this one (tiles of an item: ceil(cols / 32) * ceil(ldo / 32)), total_tiles their sum. */
typedef struct { const float* in; float* out; int32_t ldi, rows, cols, ldo, tile0, pad_; } vh_transpose_item;
int vh_transpose_many(const vh_transpose_item* items, int n, int total_tiles, void* stream);

/* Weight gradient dW = dY^T . X of `loss.backward()` (valle/models/valle_ar.py:86):
 *   C (NI, NJ) = A^T . B,  A (M, NI) row stride lda, B (M, NJ) row stride ldb — both stored with the
 * contraction index (the token) as the row, read in place (no transposed copies).  The contraction is cut
 * into slices whose partial tiles are summed in fixed order from `workspace` (vh_gemm_tn_ws_bytes; bitwise
 * reproducible, no atomics).  lda/ldb/ldc multiples of 4 covering the row padded to 4 floats. */
size_t vh_gemm_tn_ws_bytes(int M, int NI, int NJ);
int vh_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int NI, int NJ,
               void* workspace, size_t workspace_bytes, void* stream);

/* General batched fp32 GEMM of the backward pass: C[b,h] = op(A[b,h]) . op(B[b,h]) on the fp32 matrix
 * cores (128x128x32 tiles).  a_kmajor = 0: A stored (M,K) k contiguous; 1: stored (K,M) m contiguous.
 * b_kmajor = 0: B stored (N,K) (an nn.Linear weight as stored); 1: stored (K,N).  C is (M,N) ldc.
 * Two-level batch index (b < batch, h < H) with element strides, so attention operands are read in
 * place from (B,T,h,64) / (B,h,T,64) / (B,h,T,T) tensors.  Leading dimensions and strides must be
 * multiples of 4; ragged M/N/K are guarded (buffers padded to the leading dimension).
 * k_splits > 1 cuts K into that many slices handled by separate workgroups whose partial tiles are
 * ADDED to C with fp32 atomics (the caller zeroes C; summation order is not fixed) — for weight
 * gradients, where the output is a few tiles and K is the whole token count. */
int vh_gemm_batched(const float* A, int lda, int64_t sAb, int64_t sAh, int a_kmajor, const float* B,
                    int ldb, int64_t sBb, int64_t sBh, int b_kmajor, float* C, int ldc, int64_t sCb,
                    int64_t sCh, int M, int N, int K, int batch, int H, int k_splits, void* stream);

/* ---- composite: full-sequence transformer forward (prefill / NAR stage / training forward) --
 * valle/models/modules.py:305-352 without cache input: x (B*T, d) in/out in place, every
 * layer's K/V written to its cache at positions 0..T-1.  scratch: xn (B*T,d), q (B*T,d),
 * attn (B*T,d), hidden (B*T,dff).  ada_* per layer (L,2,2,d) = [layer][norm1|norm2][scale|shift]
 * or NULL for plain LayerNorm. */
typedef struct {
    int B, T, d_model, n_heads, dff, n_layers, S_max, mode, x_len;
    float ln_eps;
    const vh_layer* layers;
    const float* ada;                 /* (L,2,2,d) or NULL */
    const int32_t *x_len_dev, *kv_len;
    const uint8_t *mask, *pad;
    float *x, *xn, *q, *attn, *hidden;
    /* optional split-K workspace for the out-projection and linear_2 when B*T is small (few 128x128 tiles,
     * long K): the largest of vh_linear_ws_bytes(B*T, d_model, d_model), (B*T, d_model, dff), (B*T, dff, d_model) */
    void *gemm_ws;
    size_t gemm_ws_bytes;
    /* optional: the stack's INPUT rows (B*T, d) when they must stay untouched (the module API returns a new
     * tensor, modules.py:341-349): layer 0 reads its LayerNorm input and its residual from x_in and the stack
     * writes its output to x — no copy of the input.  NULL: x is input and output. */
    const float *x_in;
} vh_forward_desc;
int vh_transformer_forward(const vh_forward_desc* desc, void* stream);
/* vh_transformer_forward over packed rows (the NAR stage of a ragged batch): desc->B = 1, desc->T = the sum of the segment
 * lengths, desc->mode = VH_MASK_FULL, kv_len / x_len_dev / mask / pad NULL (anything else is refused: VH_EINVAL for B,
 * VH_EUNSUPPORTED for the mask fields); x (T, d) holds utterance s at rows seg_start[s] .. + seg_len[s] - 1 and every layer's
 * K/V lands at the same rows of its (1, h, S_max, 64) cache.  The launches of vh_transformer_forward with
 * vh_attn_rows_packed for vh_attn_rows; the segment and block arrays are its arguments, under its contract. */
int vh_transformer_forward_packed(const vh_forward_desc* desc, const int32_t* seg_start, const int32_t* seg_len, int n_seg,
                                  const int32_t* blocks, int n_blocks, void* stream);
/* vh_transformer_forward_packed under the PREFIX-LM mask (the AR prompt pass of a ragged batch): desc->mode = VH_MASK_PREFIX,
 * segment s attends under the prefix mask of its own text length seg_x_len[s] (clamped to 0 .. seg_len[s]) — the attention is
 * vh_attn_rows_packed_lse, so the caller lends lse2, (n_heads, T) floats it need not read.  fp32, head width 64, LayerNorm
 * (desc->ada NULL); B != 1 and bad dimensions are VH_EINVAL, another mode, the mask fields, ada or another head width
 * VH_EUNSUPPORTED, a misaligned q / attn / lse2 / cache VH_EALIGN — all before any launch. */
int vh_transformer_forward_packed_lm(const vh_forward_desc* desc, const int32_t* seg_start, const int32_t* seg_len,
                                     const int32_t* seg_x_len, int n_seg, const int32_t* blocks, int n_blocks, float* lse2,
                                     void* stream);
/* The K/V rows of packed streams to the rows of a cache: src (n_streams, n_heads, S_src, 64) fp32 — n_streams = layers x 2,
 * what a packed forward wrote — dst (n_streams, B_dst, n_heads, S_dst, 64) fp32.  Rows seg_start[s] .. + seg_len[s] - 1 of
 * every (stream, head) go to positions 0 .. seg_len[s] - 1 of row dst_row[s], bit for bit (16-byte loads and stores); nothing
 * else of dst is written.  seg_start / seg_len / dst_row: device int32 (n_seg).  A segment reaching past S_src is cut there, a
 * length beyond S_dst is cut there, a segment that starts outside [0, S_src) or names a row outside [0, B_dst) writes nothing.
 * Refused before the launch: null pointers, non-positive dimensions or n_seg (VH_EINVAL), src / dst not 16-byte aligned
 * (VH_EALIGN), n_seg > 65535 or more than 2^26 rows per stream (VH_EUNSUPPORTED). */
int vh_kv_unpack(const float* src, float* dst, int n_streams, int n_heads, int S_src, int B_dst, int S_dst,
                 const int32_t* seg_start, const int32_t* seg_len, const int32_t* dst_row, int n_seg, void* stream);

/* ---- perf mode of the MFMA-bound legs: bf16 operands, fp32 accumulate (opt-in; never the parity path) ------------
 * SURVEY.md section 7's "perf mode" for the prompt pass (valle/models/valle_ar.py:141-158 at kv_cache=None) and the NAR
 * stage forward (valle_nar.py:87-100): every matrix product on v_mfma_f32_32x32x16_bf16 with bf16 operands and fp32
 * accumulators; the residual stream, LayerNorm statistics, biases, softmax and the heads stay fp32.  The reference itself
 * asks for reduced-precision matmuls on a GPU (valle/utils.py:11, set_float32_matmul_precision('high')).  Teacher-forced
 * logits agree with the reference to atol 5e-2 (SURVEY.md 8c); greedy tokens are NOT guaranteed.  bf16 = the upper 16 bits
 * of an fp32, round to nearest even, passed as uint16_t.
 *   vh_to_bf16              narrows a (rows, cols) fp32 matrix (weights: once per weight set); cols % 8 == 0.
 *   vh_layernorm_bf16       vh_layernorm with a bf16 output (the A operand of the product that follows); d % 8 == 0.
 *   vh_linear_bf16          out = act(A W^T + bias) + residual, A (M,K) lda and W (N,K) bf16, bias (N) / residual (M,N) ldr
 *                           fp32; out fp32 (M,N) ldo, or bf16 when out_bf16 != 0 (no residual then).  N % 128 == 0,
 *                           K % 64 == 0, act NONE / GELU_ERF.
 *   vh_linear_qkv_bf16      vh_linear_qkv with bf16 operands: q_out (M, d) ldq bf16, K / V rows appended to bf16 caches
 *                           (B,h,S_max,64) — the layout vh_attn_decode_kv16 streams, so a perf-mode generate needs no
 *                           narrowing pass.  d_model % 128 == 0.  q_out holds q' = q / sqrt(64) * log2(e), scaled in fp32
 *                           before the one narrowing (since 0.2.3): the form vh_attn_rows_bf16 consumes.
 *   vh_attn_rows_bf16       vh_attn_rows over bf16 q' / K / V with a bf16 output; analytic masks only (FULL / PREFIX).
 *                           q' is PRE-SCALED (above): the weights are 2^(q'.k - max), i.e. softmax(q.k / 8) of the unscaled q. */
/* The 16-bit operand format ("h16") of everything called *bf16 / *kv16 / *16 in this header — operands of the perf-mode kernels and
 * the narrow K/V cache of the decode step: 0 = IEEE fp16 (the default build: same MFMA rate as bf16, 11 bits of significand
 * against 8 — teacher-forced logits of the 24-layer stack 5.5e-3 from the reference against 4.2e-2), 1 = bf16 (the round-5
 * format, -DVH_PERF_BF16).  The entry points keep their round-5 names; the narrowing is IEEE (overflow -> infinity, NaN stays NaN). */
int vh_h16_format(void);
int vh_to_bf16(const float* src, int64_t lds, uint16_t* dst, int64_t ldd, int64_t rows, int cols, void* stream);
int vh_layernorm_bf16(const float* x, const float* gamma, const float* beta, const float* ada_scale,
                      const float* ada_shift, uint16_t* out, int rows, int d, float eps, void* stream);
int vh_linear_bf16(const uint16_t* A, int lda, const uint16_t* W, const float* bias, const float* residual, int ldr,
                   void* out, int ldo, int out_bf16, int M, int N, int K, int act, void* stream);
int vh_linear_qkv_bf16(const uint16_t* A, int lda, const uint16_t* Wqkv, uint16_t* q_out, int ldq, uint16_t* kcache16,
                       uint16_t* vcache16, const int32_t* cache_len, int B, int T, int d_model, int n_heads, int S_max,
                       void* stream);
int vh_attn_rows_bf16(const uint16_t* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, uint16_t* out, int ldo,
                      int B, int n_heads, int Tq, int Tk, int S_max, int mode, int x_len, const int32_t* x_len_dev,
                      const int32_t* kv_len, void* stream);

/* vh_transformer_forward in perf mode.  `layers` supplies the fp32 LayerNorm parameters and biases (its weight matrices
 * and caches are not touched); layers16[i] the bf16 copies of the four matrices (vh_to_bf16) and the layer's bf16 caches.
 * x (B*T, d) fp32 in/out (x_in as in vh_forward_desc); scratch: xn16, q16, attn16 (B*T, d) and hidden16 (B*T, dff) bf16. */
typedef struct { const uint16_t *wqkv, *wo, *w1, *w2; uint16_t *kcache16, *vcache16; } vh_layer16;
typedef struct {
    int B, T, d_model, n_heads, dff, n_layers, S_max, mode, x_len;
    float ln_eps;
    const vh_layer* layers;
    const vh_layer16* layers16;
    const float* ada;                 /* (L,2,2,d) or NULL */
    const int32_t *x_len_dev, *kv_len;
    float* x;
    const float* x_in;
    uint16_t *xn16, *q16, *attn16, *hidden16;
} vh_forward16_desc;
int vh_transformer_forward_bf16(const vh_forward16_desc* desc, void* stream);

/* vh_attn_rows_bf16 over the SEGMENTS of one packed row stream, VH_MASK_FULL only: vh_attn_rows_packed in the 16-bit format.
 * Utterance s owns rows seg_start[s] .. seg_start[s] + seg_len[s] - 1 of q' (M, ldq; PRE-SCALED as for vh_attn_rows_bf16), of
 * out (M, ldo) and of ONE 16-bit K/V stream per head, kcache16 / vcache16 (1, h, S_max >= M, 64), M = the sum of the lengths:
 * query row seg_start[s] + i attends keys seg_start[s] + j, j < seg_len[s], of the same cache and nothing else.  One
 * workgroup = the 128 queries from blocks[2 i + 1] on of segment blocks[2 i] x one head, over that segment's keys in 64-key
 * tiles counted from the segment's key 0 — vh_attn_rows_bf16's tile order, and its arithmetic, for that utterance alone
 * (B = 1, Tq = Tk = seg_len[s], full mask): the same bits.  K/V rows past a segment's end are clamped to its last row and
 * masked (a tail tile re-reads the segment's own last row, never a row of the next segment or one at or beyond M); query
 * rows past it are not stored.  Workgroups run in table order, workgroup id = block * n_heads + head: list the blocks of the
 * longest segment first.  ldq, ldo: multiples of 8, >= n_heads * 64; q, out and the caches 16-byte aligned.
 * seg_start, seg_len (n_seg) and blocks (n_blocks pairs) are DEVICE int32 arrays the host cannot check: the caller vouches
 * that the segments are disjoint and inside [0, M), that every block names a segment < n_seg and a first query
 * 0 <= q0 < seg_len, and that the blocks cover every query once (a query no block covers keeps its old `out` row).  Inside
 * such segments no row of another segment is read as a visible key and no row at or beyond M is touched.  (A block naming
 * no segment is skipped and a segment reaching past S_max is cut there, so the caches are never overrun; q and out have
 * no such guard.) */
int vh_attn_rows_packed_bf16(const uint16_t* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, uint16_t* out,
                             int ldo, int n_heads, int S_max, const int32_t* seg_start, const int32_t* seg_len, int n_seg,
                             const int32_t* blocks, int n_blocks, void* stream);
/* vh_transformer_forward_bf16 over packed rows (the perf-mode NAR stage of a ragged batch): desc->B = 1, desc->T = the sum of
 * the segment lengths, desc->mode = VH_MASK_FULL, kv_len / x_len_dev NULL (anything else is refused: VH_EINVAL for B,
 * VH_EUNSUPPORTED for the mask fields and for a d_model / dff vh_transformer_forward_bf16 does not take); x (T, d) holds
 * utterance s at rows seg_start[s] .. + seg_len[s] - 1 and every layer's K/V lands at the same rows of its 16-bit
 * (1, h, S_max, 64) cache.  The launches of vh_transformer_forward_bf16 with vh_attn_rows_packed_bf16 for vh_attn_rows_bf16;
 * the segment and block arrays are its arguments, under its contract.  A null or misaligned pointer in the descriptor or in
 * either layer table is refused here, before any launch, not by the launch that would meet it. */
int vh_transformer_forward_packed_bf16(const vh_forward16_desc* desc, const int32_t* seg_start, const int32_t* seg_len, int n_seg,
                                       const int32_t* blocks, int n_blocks, void* stream);
/* vh_attn_rows_packed_bf16 under the PREFIX-LM mask (ABI 146): segment s attends under the prefix mask of its own text length
 * seg_x_len[s], clamped to 0 .. seg_len[s] — query i sees key j iff j < x_len or (i >= x_len and j <= i).  Per segment the
 * output is bit for bit vh_attn_rows_bf16(B = 1, Tq = Tk = seg_len[s], VH_MASK_PREFIX, x_len = seg_x_len[s]) on that segment
 * alone: the same body over the same keys in the same tile order.  Layout, alignment, the tail-tile clamp and the refusals are
 * vh_attn_rows_packed_bf16's, plus a null seg_x_len (VH_EINVAL); seg_x_len is a DEVICE int32 array of n_seg entries, and the
 * caller vouches for the segment and block arrays exactly as there: the segments disjoint and inside [0, M), every block
 * naming a segment < n_seg and a first query 0 <= q0 < seg_len, the blocks covering every query once.  Workgroups run in table
 * order: under this mask a segment's LAST query block visits the most key tiles. */
int vh_attn_rows_packed_lm_bf16(const uint16_t* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, uint16_t* out,
                                int ldo, int n_heads, int S_max, const int32_t* seg_start, const int32_t* seg_len,
                                const int32_t* seg_x_len, int n_seg, const int32_t* blocks, int n_blocks, void* stream);
/* vh_transformer_forward_packed_bf16 under the PREFIX-LM mask (the perf-mode AR prompt pass of a ragged batch, ABI 146):
 * desc->mode = VH_MASK_PREFIX, segment s attends under the prefix mask of its own text length seg_x_len[s] — the launches of
 * vh_transformer_forward_bf16 with vh_attn_rows_packed_lm_bf16 for vh_attn_rows_bf16.  LayerNorm stacks (desc->ada NULL).
 * B != 1, S_max < T and bad dimensions are VH_EINVAL; another mode, kv_len, x_len_dev, ada, or a d_model / dff
 * vh_transformer_forward_bf16 does not take VH_EUNSUPPORTED; null or misaligned pointers in the descriptor or in either layer
 * table VH_EINVAL / VH_EALIGN — all before any launch. */
int vh_transformer_forward_packed_lm_bf16(const vh_forward16_desc* desc, const int32_t* seg_start, const int32_t* seg_len,
                                          const int32_t* seg_x_len, int n_seg, const int32_t* blocks, int n_blocks, void* stream);
/* vh_kv_unpack for 16-bit streams (ABI 146): src (n_streams, n_heads, S_src, 64) and dst (n_streams, B_dst, n_heads, S_dst, 64)
 * uint16_t (a row is 128 bytes, moved with 16-byte loads and stores).  The same tables, the same cuts and the same refusals as
 * vh_kv_unpack; the copy is bit for bit and nothing else of dst is written. */
int vh_kv_unpack_bf16(const uint16_t* src, uint16_t* dst, int n_streams, int n_heads, int S_src, int B_dst, int S_dst,
                      const int32_t* seg_start, const int32_t* seg_len, const int32_t* dst_row, int n_seg, void* stream);

/* ---- the decoder of the 24 kHz EnCodec family: codes -> waveform (additions under ABI 146; csrc/codec.hip) -----------------
 * Replaces the arithmetic behind EncodecPip.decode (valle/models/encodec_pip.py:59-72): the residual vector quantiser's
 * decode and the causal SEANet decoder.  Activations are channels-last (B, T, C) fp32: a time step is a row.  Every shape,
 * alignment and pointer fault is refused before any launch. */
enum { VH_PAD_ZERO = 0, VH_PAD_REFLECT = 1 };
/* out[b, t, :] = sum over q < Q of codebooks[q][codes[b, q, t]], added in codebook order 0 .. Q-1 starting from 0.0f (fp32
 * torch adding in that order is bit-equal).  codes (B, Q, T) int64; codebooks (n_books, K, D), Q <= n_books; out (B, T, D);
 * D % 4 == 0.  An id outside [0, K) is never read: it contributes nothing and ORs VH_DEVERR_EMBED_ID into *err_flag (device
 * int32, may be NULL). */
int vh_rvq_decode(const int64_t* codes, const float* codebooks, float* out, int B, int Q, int T, int n_books, int K, int D,
                  int32_t* err_flag, void* stream);
/* The causal windowed GEMM of every convolution of the decoder, on v_mfma_f32_32x32x2_f32:
 *   out[b, t, co] = bias[co] + sum_k sum_ci act(xpad[b, t + k dilation, ci]) w[co, k, ci]  (+ residual[b, t, co])
 * x (B, T, C_in); w (C_out, taps, C_in) — nn.Conv1d's (C_out, C_in, taps) with its last two dimensions swapped, so that the
 * reduction runs along memory; bias (C_out) or NULL; residual (B, T, C_out) or NULL; out (B, T, C_out).  xpad is x with
 * (taps - 1) dilation rows of LEFT padding per batch row (row b's window never reads row b - 1): zeros (VH_PAD_ZERO), or the
 * reflection xpad[i] = x[pad - i] (VH_PAD_REFLECT), where an x row >= T reads as zero — the reference's small-input branch
 * (zero-extend to pad + 1, reflect, cut the extension off) for T <= pad.  elu = 1 applies ELU (alpha 1, expm1 for x <= 0) to
 * every x on load; act is the identity otherwise.  A ConvTranspose1d(C_in, C, 2 r, stride r) trimmed by r on the right is
 * this entry with taps 2, VH_PAD_ZERO, C_out = r C and w[(p, co), 0, ci] = wt[ci, co, p + r], w[(p, co), 1, ci] =
 * wt[ci, co, p]: its (B, T, r C) output IS the (B, T r, C) layout.  C_in % 4 == 0; C_out % 4 == 0 or C_out == 1 (the
 * waveform); anything else is VH_EUNSUPPORTED by name.  An output element's sum order depends on (taps, C_in) alone: a row of
 * a right-padded batch has the bits of the same row decoded alone — with lens (device int32 (B), or NULL: every batch row holds
 * T rows): batch row b holds lens[b] len_scale valid rows (clamped to 0 .. T), and the reflection, which reads FORWARD at the
 * start of a row, reads zero beyond them, exactly what the small-input branch gives that utterance alone.  Rows t >= the
 * valid length are computed from whatever x holds there. */
int vh_conv1d_causal(const float* x, const float* w, const float* bias, const float* residual, float* out, int B, int T,
                     int C_in, int C_out, int taps, int dilation, int pad_mode, int elu, const int32_t* lens, int len_scale,
                     void* stream);
/* One nn.LSTM layer over T steps, zero initial state, gate order i, f, g, o: T launches, one per step (no workgroup waits
 * for another inside a launch).  xproj (B, T, 4 H): W_ih x_t + b_ih + b_hh of every frame (one vh_conv1d_causal with taps 1);
 * w_hh (4 H, H); h_seq (B, T, H) receives h_t; c (B, H) is scratch (the cell state; needs no initialisation); skip and y
 * (B, T, H), both or neither: y = h_t + skip, the residual the decoder's LSTM block ends with.  H % 4 == 0, H <= 1024. */
int vh_lstm_layer(const float* xproj, const float* w_hh, float* h_seq, float* c, const float* skip, float* y, int B, int T,
                  int H, void* stream);

/* ---- the encoder of the same family: waveform -> codes (additions under ABI 146: VH_VERSION stays; csrc/codec.hip) -------
 * Replaces the arithmetic behind EncodecPip.encode (valle/models/encodec_pip.py): the causal SEANet encoder and the residual
 * vector quantiser's encode.  The stride-1 convolutions, the residual blocks and the LSTM are vh_conv1d_causal and
 * vh_lstm_layer; these three are what the encoder adds.  Every shape, alignment and pointer fault is refused before any
 * launch. */
/* The first convolution, C_in = 1: x (B, L) -> out (B, L, C_out), out[b, t, co] = bias[co] + sum_k xpad[b, t + k] w[co, k].
 * w (C_out, taps); bias (C_out) or NULL; taps - 1 samples of LEFT reflection per batch row (xpad[i] = x[pad - i]); lens
 * (device int32 (B)) or NULL: batch row b holds lens[b] valid samples (clamped to 0 .. L) and a FORWARD read beyond them
 * reads zero, exactly as vh_conv1d_causal treats it (the reference's small-input branch for that utterance alone).  One lane
 * computes 4 output channels: fma over the taps in order from 0, then + bias — the sum order depends on taps alone.
 * C_out % 4 == 0; 1 <= taps <= 64. */
int vh_conv1d_wave(const float* x, const float* w, const float* bias, float* out, int B, int L, int C_out, int taps,
                   const int32_t* lens, void* stream);
/* The strided, downsampling causal convolution (EncodecConv1d with stride > 1) on v_mfma_f32_32x32x2_f32:
 *   out[b, t', co] = bias[co] + sum_k sum_ci act(xpad_b[t' stride + k, ci]) w[co, k, ci],  t' < T_out = ceil(T / stride)
 * x (B, T, C_in); w (C_out, taps, C_in); bias (C_out) or NULL; out (B, T_out, C_out).  xpad_b is the reference's causal
 * padding of batch row b over its own valid length len_b = lens ? clamp(lens[b], 0, T) : T:  taps - stride rows of left
 * reflection (xpad[left - i] = x[i]), then the len_b rows, then ceil(len_b / stride) stride - len_b rows of right reflection
 * (xpad[left + len_b + i] = x[len_b - 2 - i]); when len_b <= max(left, right) the reference's small-input rule holds: the
 * row is zero-extended to max(left, right) + 1 rows, reflected, and the extension cut off the end.  elu = 1 applies ELU on
 * load.  Output rows t' >= ceil(len_b / stride) of a batch row are written as zeros; no valid row of a later layer reads
 * them.  The kernel is vh_conv1d_causal's (same tiles, same fragment order): an output's sum order depends on
 * (taps, C_in) alone and a row of a padded batch has the bits of the same utterance alone.  C_in % 4 == 0, C_out % 4 == 0,
 * 1 <= stride <= taps <= 64. */
int vh_conv1d_down(const float* x, const float* w, const float* bias, float* out, int B, int T, int C_in, int C_out, int taps,
                   int stride, int elu, const int32_t* lens, void* stream);
/* The residual vector quantiser's encode, all Q stages in ONE launch: x (B, T, D) -> codes (B, Q, T) int64, the layout
 * vh_rvq_decode reads.  Stage q picks id = argmax_k 2 r.E[q][k] - e_sq[q][k] (the nearest entry; the LOWEST index of equal
 * scores; a row whose scores are not finite still gets an id inside [0, K)), then r -= E[q][id] in plain fp32 — the
 * reference's residual - quantized.  codebooks (n_books, K, D), Q <= n_books; e_sq (n_books, K) = |E[q][k]|^2, precomputed
 * by the caller.  A workgroup keeps the residual of 128 rows in registers across the stages, streams each codebook through
 * LDS in chunks of 32 entries and forms the scores on v_mfma_f32_32x32x2_f32; a row's codes depend on that row alone.
 * D % 4 == 0, D <= 128, K <= 16384; beyond them VH_EUNSUPPORTED. */
int vh_rvq_encode(const float* x, const float* codebooks, const float* e_sq, int64_t* codes, int B, int T, int D, int Q,
                  int n_books, int K, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VALLE_HIP_H */
