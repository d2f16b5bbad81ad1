// Native composition of the primitives: one AR decode step (eager / hipGraph-captured) and the
// full-sequence transformer forward.  Host code only — every launch goes through the C-ABI
// primitives so that what the tests check piecewise is exactly what the composites run.
#include <stdarg.h>

#include <vector>

#include "vh_common.h"

static thread_local char g_err[512] = "";

void vh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int g_tuning[VH_TUNE_COUNT] = {0};
extern "C" int vh_h16_format(void) { return VH_H16_IS_BF16; }     // 0 = IEEE fp16 (default), 1 = bf16 (-DVH_PERF_BF16)
int vh_tuning(int knob) { return (knob >= 0 && knob < VH_TUNE_COUNT) ? g_tuning[knob] : 0; }
extern "C" int vh_set_tuning(int knob, int value) {
    VH_REQUIRE(knob >= 0 && knob < VH_TUNE_COUNT, VH_EINVAL, "vh_set_tuning: knob=%d", knob);
    g_tuning[knob] = value;
    return VH_OK;
}

extern "C" const char* vh_last_error(void) { return g_err; }
extern "C" int vh_version(void) { return VH_VERSION; }

#define HIP_TRY(call)                                                             \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        VH_REQUIRE(e_ == hipSuccess, VH_ELAUNCH, #call ": %s", hipGetErrorString(e_)); \
    } while (0)

#define TRY(call) VH_TRY(call)

// ---------------------------------------------------------------------------------------------
// AR decoder
// ---------------------------------------------------------------------------------------------
struct vh_ar_decoder {
    vh_ar_decoder_desc d;
    std::vector<vh_layer> layers;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipGraph_t graph_n = nullptr;        // VH_GRAPH_STEPS consecutive steps in one graph (fewer graph launches per generate)
    hipGraphExec_t exec_n = nullptr;
    int ldl = 0;
    const vh_row_limits* row_limits = nullptr;   // vh_ar_decoder_set_row_limits: the rows' length bounds, beside d.row_sampling
};

// The decode attention of one layer as attention.hip's call record: any head width or 64, 16-bit or fp32 caches, one shared
// prompt (the beams of one utterance: prompt K/V read once, each beam's own rows after it), one per group (the beams of
// several utterances) or none.  The plain fp32 form at width 64 is vh_attn_decode's call, which takes no workspace size.
static DecodeAttnCall decoder_attn_call(const vh_ar_decoder_desc& d, const vh_layer& L, void* stream) {
    const int D = d.d_model, hd = D / d.n_heads;
    const bool any_width = hd != VH_HEAD_DIM;
    const int kind = any_width ? ATTN_PREFIX_NONE : d.n_groups > 0 ? ATTN_PREFIX_GROUPS : d.prefix_len > 0 ? ATTN_PREFIX_ONE : ATTN_PREFIX_NONE;
    const bool sized = any_width || d.kv_bf16 || kind != ATTN_PREFIX_NONE;
    void* const ws = d.n_split > 1 || kind != ATTN_PREFIX_NONE ? d.attn_partial : nullptr;   // an unsplit call leaves no records
    const char* const ws_name = any_width                    ? "attn_partial, vh_attn_decode_hd_ws_bytes()"
                                : kind == ATTN_PREFIX_GROUPS ? "attn_partial, vh_attn_decode_shared_groups_ws_bytes()"
                                : kind == ATTN_PREFIX_ONE    ? "attn_partial, vh_attn_decode_shared_ws_bytes()"
                                                             : "attn_partial, vh_attn_decode_ws_bytes()";
    return DecodeAttnCall{"vh_ar_decoder", ws_name, d.q, D, d.attn, D, d.cache_len, 1, d.B, d.n_heads, any_width, hd,
                          (float)(1.0 / sqrt((double)hd)), d.kv_bf16 != 0, L.kcache, L.vcache, d.S_max, kind, L.kprefix, L.vprefix,
                          kind == ATTN_PREFIX_GROUPS ? d.prefix_cap : d.prefix_len, d.prefix_S, d.prefix_lens, d.beams_per_group,
                          d.n_split, ws, sized ? d.attn_partial_bytes : ATTN_WS_SIZE_NOT_GIVEN, stream};
}

static int decoder_check(const vh_ar_decoder_desc* d) {
    VH_REQUIRE(d, VH_EINVAL, "vh_ar_decoder: null desc");
    VH_REQUIRE(d->B > 0 && d->B <= 64, VH_EUNSUPPORTED,
               "vh_ar_decoder: B=%d (decode rows per GPU must be 1..64)", d->B);
    VH_REQUIRE(d->n_layers > 0 && d->layers, VH_EINVAL, "vh_ar_decoder: no layers");
    VH_REQUIRE(d->n_heads > 0 && d->d_model > 0 && d->d_model % d->n_heads == 0, VH_EUNSUPPORTED,
               "vh_ar_decoder: d_model=%d is not a multiple of n_heads=%d", d->d_model, d->n_heads);
    const int hd = d->d_model / d->n_heads;
    if (hd != VH_HEAD_DIM) {          // a head width other than 64: vh_linear_qkv[_folded]_hd + vh_attn_decode_hd
        VH_REQUIRE(hd % 4 == 0 && hd >= 16 && hd <= 256, VH_EUNSUPPORTED,
                   "vh_ar_decoder: head width %d (d_model=%d / n_heads=%d): the cached decoder serves 64 and multiples of 4 "
                   "from 16 to 256", hd, d->d_model, d->n_heads);
        VH_REQUIRE(d->d_model % 16 == 0 && d->d_model <= 1024, VH_EUNSUPPORTED,
                   "vh_ar_decoder: head width %d needs d_model %% 16 == 0 and d_model <= 1024 (got %d)", hd, d->d_model);
        VH_REQUIRE(!d->kv_bf16, VH_EUNSUPPORTED, "vh_ar_decoder: the bf16 K/V cache (perf mode) is width 64 only (head width %d)",
                   hd);
        VH_REQUIRE(d->prefix_len == 0, VH_EUNSUPPORTED,
                   "vh_ar_decoder: the shared prompt (prefix_len=%d) is width 64 only (head width %d)", d->prefix_len, hd);
        VH_REQUIRE(d->n_groups == 0, VH_EUNSUPPORTED,
                   "vh_ar_decoder: grouped shared prompts (n_groups=%d) are width 64 only (head width %d)", d->n_groups, hd);
    } else {
        // width 64: the prompt pass (vh_layernorm) and the folded decode GEMMs end at 4096
        VH_REQUIRE(d->d_model <= 4096, VH_EUNSUPPORTED, "vh_ar_decoder: d_model=%d: the cached decoder serves d_model <= 4096",
                   d->d_model);
    }
    VH_REQUIRE(d->dff % 16 == 0 && d->V > 0 && d->S_max > 0 && d->n_split >= 1, VH_EINVAL,
               "vh_ar_decoder: bad dff/V/S_max/n_split");
    VH_REQUIRE(d->proj_w && d->audio_emb && d->audio_pe && d->x && d->q && d->attn && d->hidden &&
                   d->logits && d->cache_len && d->audio_pos && d->eos_count && d->codes,
               VH_EINVAL, "vh_ar_decoder: null buffer in desc");
    VH_REQUIRE(d->prefix_len >= 0, VH_EINVAL, "vh_ar_decoder: prefix_len=%d", d->prefix_len);
    if (d->ffn_ws) {
        VH_REQUIRE(d->ffn_ws_bytes >= vh_ffn_decode_ws_bytes(d->B, d->d_model, d->dff) && d->ffn_ws_bytes > 0, VH_EINVAL,
                   "vh_ar_decoder: ffn_ws needs vh_ffn_decode_ws_bytes() bytes");
        for (int i = 0; i < d->n_layers; ++i)
            VH_REQUIRE(d->layers[i].w1_f && d->layers[i].w1_c1 && d->layers[i].w1_c2, VH_EINVAL,
                       "vh_ar_decoder: ffn_ws needs the folded linear_1 weights (layer %d)", i);
    }
    if (d->kv_bf16) {
        VH_REQUIRE(d->d_model <= 1024, VH_EUNSUPPORTED, "vh_ar_decoder: the bf16 K/V cache (perf mode) serves d_model <= 1024 (got %d)",
                   d->d_model);
        for (int i = 0; i < d->n_layers; ++i)
            VH_REQUIRE(d->layers[i].wqkv_f, VH_EINVAL, "vh_ar_decoder: the bf16 K/V cache needs folded weights (layer %d)", i);
    }
    if (d->prefix_len > 0) {
        for (int i = 0; i < d->n_layers; ++i)
            VH_REQUIRE(d->layers[i].kprefix && d->layers[i].vprefix, VH_EINVAL,
                       "vh_ar_decoder: shared prompt needs kprefix / vprefix in every layer (layer %d)", i);
    }
    VH_REQUIRE(d->n_groups >= 0, VH_EINVAL, "vh_ar_decoder: n_groups=%d", d->n_groups);
    if (d->n_groups > 0) {
        VH_REQUIRE(!d->kv_bf16, VH_EUNSUPPORTED,
                   "vh_ar_decoder: grouped shared prompts (n_groups=%d) with kv_bf16 (perf mode) are not served: fp32 caches only",
                   d->n_groups);
        VH_REQUIRE(d->prefix_len == 0, VH_EINVAL, "vh_ar_decoder: n_groups=%d with prefix_len=%d (one form or the other)",
                   d->n_groups, d->prefix_len);
        VH_REQUIRE(d->beams_per_group >= 1 && d->B == d->n_groups * d->beams_per_group, VH_EINVAL,
                   "vh_ar_decoder: B=%d is not n_groups=%d x beams_per_group=%d", d->B, d->n_groups, d->beams_per_group);
        VH_REQUIRE(d->prefix_cap >= 1 && d->prefix_cap <= d->prefix_S && d->prefix_lens, VH_EINVAL,
                   "vh_ar_decoder: grouped shared prompts need prefix_lens and 1 <= prefix_cap=%d <= prefix_S=%d", d->prefix_cap,
                   d->prefix_S);
        for (int i = 0; i < d->n_layers; ++i)
            VH_REQUIRE(d->layers[i].kprefix && d->layers[i].vprefix, VH_EINVAL,
                       "vh_ar_decoder: grouped shared prompts need kprefix / vprefix in every layer (layer %d)", i);
    }
    // the attention's own rules (the n_split range of the cache type, the record bound of a shared prompt, attn_partial and its
    // size): the check of the call every step will make.  Layer 0 stands for every layer: no pointer is looked at.
    TRY(vh_internal_attn_decode_check(decoder_attn_call(*d, d->layers[0], nullptr), false));
    VH_REQUIRE(d->top_k == 1 || d->row_sampling || d->temperature > 0.f, VH_EINVAL,
               "vh_ar_decoder: sampling (top_k=%d) needs temperature > 0", d->top_k);
    VH_REQUIRE((d->top_k == 1 && !d->row_sampling) || d->V <= VH_SAMPLE_MAX_V, VH_EUNSUPPORTED,
               "vh_ar_decoder: sampling (top_k=%d%s) serves V <= %d (VH_SAMPLE_MAX_V), got V=%d", d->top_k,
               d->row_sampling ? ", row_sampling" : "", VH_SAMPLE_MAX_V, d->V);
    if (d->row_sampling) {
        // the fused greedy head has no sampler behind it: a row of the records could not sample
        VH_REQUIRE(!d->head_ws, VH_EUNSUPPORTED,
                   "vh_ar_decoder: row_sampling with head_ws: per-row sampling runs the sampler on every row, head_ws (head + "
                   "greedy step in one launch) has none — set one or the other");
        VH_REQUIRE(vh_aligned16(d->row_sampling), VH_EALIGN, "vh_ar_decoder: row_sampling must be 16-byte aligned");
    }
    if (d->head_ws) {
        VH_REQUIRE(d->top_k == 1 && d->B <= 64 && d->d_model <= 1024, VH_EUNSUPPORTED,
                   "vh_ar_decoder: head_ws (head + greedy step in one launch) is for top_k == 1, B <= 64, d_model <= 1024");
        VH_REQUIRE(d->head_ws_bytes >= vh_head_greedy_ws_bytes(d->B, d->V) && vh_aligned16(d->head_ws), VH_EINVAL,
                   "vh_ar_decoder: head_ws needs vh_head_greedy_ws_bytes() = %zu bytes, 16-byte aligned (got %zu)",
                   vh_head_greedy_ws_bytes(d->B, d->V), d->head_ws_bytes);
    }
    return VH_OK;
}

extern "C" void vh_ar_decoder_destroy(vh_ar_decoder* dec);

extern "C" vh_ar_decoder* vh_ar_decoder_create(const vh_ar_decoder_desc* desc) {
    if (decoder_check(desc) != VH_OK) return nullptr;
    auto* dec = new vh_ar_decoder();
    dec->d = *desc;
    dec->layers.assign(desc->layers, desc->layers + desc->n_layers);
    dec->d.layers = dec->layers.data();
    dec->ldl = (desc->V + 3) & ~3;
    return dec;
}

extern "C" void vh_ar_decoder_destroy(vh_ar_decoder* dec) {
    if (!dec) return;
    if (dec->exec) (void)hipGraphExecDestroy(dec->exec);
    if (dec->graph) (void)hipGraphDestroy(dec->graph);
    if (dec->exec_n) (void)hipGraphExecDestroy(dec->exec_n);
    if (dec->graph_n) (void)hipGraphDestroy(dec->graph_n);
    delete dec;
}

// One decode step for every row: x (B,d) holds the new token's embedding on entry and the NEXT
// token's embedding on exit.  `ev` (optional) brackets each decode-attention launch.
void vh_internal_attn_decode_events(hipEvent_t start, hipEvent_t stop);   // attention.hip
int vh_internal_linear_w16(const float* A, int lda, const uint16_t* W16, const float* bias, const float* residual, int ldr,
                           float* out, int ldo, int M, int N, int K, void* stream);                                   // gemm.hip
int vh_internal_linear_qkv_folded_kv16_w16(const float* A, int lda, const uint16_t* Wf16, const float* c1, const float* c2,
                                           float* q_out, int ldq, uint16_t* kcache16, uint16_t* vcache16, const int32_t* cache_len,
                                           int B, int d_model, int n_heads, int S_max, float ln_eps, void* stream);   // gemm.hip
int vh_internal_ffn_decode_w16(const float* x, int ldx, const uint16_t* w1f16, const float* c1, const float* c2,
                               const uint16_t* w2_16, const float* b2, float* out, int ldo, int M, int d_model, int dff,
                               float ln_eps, void* workspace, size_t workspace_bytes, void* stream);                  // ffn.hip
int vh_internal_sample_step(const float* logits, int ldl, int V, int eos, int top_k, float top_p, float temperature, uint64_t seed,
                            const uint64_t* seed_dev, const vh_row_sampling* rs, const vh_row_limits* limits, int64_t* codes,
                            int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                            const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len, float* x_next, int B,
                            int d, void* stream);   // elementwise.hip
int vh_internal_sample_step_wide(const float* logits, int ldl, int V, int eos, int top_k, float top_p, float temperature,
                                 uint64_t seed, const uint64_t* seed_dev, const vh_row_sampling* rs, const vh_row_limits* limits,
                                 int64_t* codes, int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base,
                                 float* sum_logprobs, const float* audio_emb, const float* pe, int32_t* audio_pos,
                                 int32_t* cache_len, float* x_next, int B, int d, void* stream);   // elementwise.hip

static int decoder_enqueue(vh_ar_decoder* dec, hipStream_t s, std::vector<hipEvent_t>* ev,
                           std::vector<hipEvent_t>* kev = nullptr) {
    const vh_ar_decoder_desc& d = dec->d;
    const int B = d.B, D = d.d_model;
    const int hd = D / d.n_heads;       // 64: the kernels below as always; otherwise the _hd forms (decoder_check)
    // FeedForward as one launch split over dim_feedforward + the slab reduce (vh_ffn_decode) when the caller gave
    // the workspace and the folded weights; else linear_1 and linear_2 (split-K + reduce) as separate launches
    // measured: +1.6 us per step at 12L/512d x 32 rows, but 1.2 us per LAYER slower at 24L/1024d x 8 rows (256 slices of
    // 16 columns, 8 MB of slabs: profiles/r3_ab_config5_ffn.log) — the default follows the measurements
    const int ffn_knob = vh_tuning(VH_TUNE_FFN_FUSED);
    // (640 / 768 / 896 take it as 512 does: their unfused route is linear_1 + split-K linear_2 + reduce, one launch more)
    const bool ffn_fused = d.ffn_ws && ffn_knob != 1 && (d.d_model <= 512 || d.d_model == 640 || d.d_model == 768 || d.d_model == 896 ||
                                                        (ffn_knob == 2 && d.d_model <= 1024));
    // d_model > 1024 (width 64): the LayerNorm-in-the-operand-load GEMMs end at K = 1024.  Folded weights (d_model 1280 .. 2048 in steps of 256, 2560 .. 4096 in steps of 512)
    // run the wide folded GEMMs; without them the step normalises into d.attn — free before the attention writes it and again
    // once the out-projection has read it — and runs the plain GEMMs on that: two more launches per layer, any d_model % 64 == 0.
    const bool ln_apart = D > 1024;
    // decode attention of one layer, optionally bracketed by events (vh_ar_decoder_profile_attn)
    auto attention = [&](const vh_layer& L) -> int {
        return vh_internal_attn_decode(decoder_attn_call(d, L, s));
    };
    auto run_attention = [&](const vh_layer& L) -> int {
        if (!ev) return attention(L);
        hipEvent_t e0, e1;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            vh_set_error("vh_ar_decoder: hipEventCreate failed");
            return VH_ELAUNCH;
        }
        hipEvent_t k0 = nullptr, k1 = nullptr;
        if (kev && hipEventCreate(&k0) == hipSuccess && hipEventCreate(&k1) == hipSuccess) {
            vh_internal_attn_decode_events(k0, k1);
            kev->push_back(k0);
            kev->push_back(k1);
        }
        (void)hipEventRecord(e0, s);
        const int arc = attention(L);
        (void)hipEventRecord(e1, s);
        vh_internal_attn_decode_events(nullptr, nullptr);
        ev->push_back(e0);
        ev->push_back(e1);
        return arc;
    };
    for (int i = 0; i < d.n_layers; ++i) {
        const vh_layer& L = dec->layers[i];
        // LN1 fused into the QKV GEMM; K/V rows appended at cache_len[b]  (modules.py:146-157,271)
        // (perf mode with h16 copies of the step's four matrices: the same launches over half the weight bytes)
        const bool w16 = d.kv_bf16 && L.wqkv_f16 && L.wo16 && L.w1_f16 && L.w2_16 && D <= 1024;
        if (hd != VH_HEAD_DIM && L.wqkv_f)
            TRY(vh_linear_qkv_folded_hd(d.x, D, L.wqkv_f, L.qkv_c1, L.qkv_c2, d.q, D, L.kcache, L.vcache, d.cache_len, B, 1, D,
                                        d.n_heads, d.S_max, d.ln_eps, hd, s));
        else if (hd != VH_HEAD_DIM)
            TRY(vh_linear_qkv_hd(d.x, D, L.wqkv, d.q, D, L.kcache, L.vcache, d.cache_len, B, 1, D, d.n_heads, d.S_max, L.ln1_g,
                                 L.ln1_b, nullptr, nullptr, d.ln_eps, hd, s));
        else if (w16)
            TRY(vh_internal_linear_qkv_folded_kv16_w16(d.x, D, L.wqkv_f16, L.qkv_c1, L.qkv_c2, d.q, D, (uint16_t*)L.kcache,
                                                       (uint16_t*)L.vcache, d.cache_len, B, D, d.n_heads, d.S_max, d.ln_eps, s));
        else if (d.kv_bf16)
            TRY(vh_linear_qkv_folded_kv16(d.x, D, L.wqkv_f, L.qkv_c1, L.qkv_c2, d.q, D, (uint16_t*)L.kcache,
                                          (uint16_t*)L.vcache, d.cache_len, B, D, d.n_heads, d.S_max, d.ln_eps, s));
        else if (L.wqkv_f)
            TRY(vh_linear_qkv_folded(d.x, D, L.wqkv_f, L.qkv_c1, L.qkv_c2, d.q, D, L.kcache, L.vcache,
                                     d.cache_len, B, 1, D, d.n_heads, d.S_max, d.ln_eps, s));
        else if (ln_apart) {
            TRY(vh_layernorm(d.x, L.ln1_g, L.ln1_b, nullptr, nullptr, d.attn, B, D, d.ln_eps, s));
            TRY(vh_linear_qkv(d.attn, D, L.wqkv, d.q, D, L.kcache, L.vcache, d.cache_len, B, 1, D, d.n_heads,
                              d.S_max, nullptr, nullptr, nullptr, nullptr, 0.f, s));
        } else
            TRY(vh_linear_qkv(d.x, D, L.wqkv, d.q, D, L.kcache, L.vcache, d.cache_len, B, 1, D, d.n_heads,
                              d.S_max, L.ln1_g, L.ln1_b, nullptr, nullptr, d.ln_eps, s));
        TRY(run_attention(L));
        // out-proj + bias + residual (modules.py:171,277)
        if (w16)
            TRY(vh_internal_linear_w16(d.attn, D, L.wo16, L.bo, d.x, D, d.x, D, B, D, D, s));
        else
            TRY(vh_linear(d.attn, D, L.wo, L.bo, d.x, D, d.x, D, B, D, D, VH_ACT_NONE, nullptr, nullptr,
                          nullptr, nullptr, 0.f, s));
        // LN2 + linear_1 + exact GELU + linear_2 + bias + residual (modules.py:215-221,278-279)
        if (w16 && d.ffn_ws) {             // (the fused FeedForward is the only 16-bit-weight form: taken at every width)
            TRY(vh_internal_ffn_decode_w16(d.x, D, L.w1_f16, L.w1_c1, L.w1_c2, L.w2_16, L.b2, d.x, D, B, D, d.dff, d.ln_eps, d.ffn_ws,
                                           d.ffn_ws_bytes, s));
            continue;
        }
        if (ffn_fused) {
            TRY(vh_ffn_decode(d.x, D, L.w1_f, L.w1_c1, L.w1_c2, L.w2, L.b2, d.x, D, B, D, d.dff, d.ln_eps, d.ffn_ws,
                              d.ffn_ws_bytes, s));
            continue;
        }
        if (L.w1_f)
            TRY(vh_linear_folded(d.x, D, L.w1_f, L.w1_c1, L.w1_c2, nullptr, 0, d.hidden, d.dff, B, d.dff, D,
                                 VH_ACT_GELU_ERF, d.ln_eps, s));
        else if (ln_apart) {
            TRY(vh_layernorm(d.x, L.ln2_g, L.ln2_b, nullptr, nullptr, d.attn, B, D, d.ln_eps, s));
            TRY(vh_linear(d.attn, D, L.w1, L.b1, nullptr, 0, d.hidden, d.dff, B, d.dff, D, VH_ACT_GELU_ERF,
                          nullptr, nullptr, nullptr, nullptr, 0.f, s));
        } else
            TRY(vh_linear(d.x, D, L.w1, L.b1, nullptr, 0, d.hidden, d.dff, B, d.dff, D, VH_ACT_GELU_ERF,
                          L.ln2_g, L.ln2_b, nullptr, nullptr, d.ln_eps, s));
        TRY(vh_linear_ws(d.hidden, d.dff, L.w2, L.b2, d.x, D, d.x, D, B, D, d.dff, VH_ACT_NONE, d.gemm_ws,
                         d.gemm_ws_bytes, s));
    }
    // head (no bias, no final norm: valle_ar.py:29,158) then sampling + state update
    if (d.top_k == 1 && d.head_ws) {      // opt-in: one launch for both (the descriptor check made sure the shape is served)
        TRY(vh_head_greedy(d.x, D, d.proj_w, d.logits, dec->ldl, d.V, d.eos, d.codes, d.codes_stride, d.eos_count, d.pos_base,
                           d.audio_emb, d.audio_pe, d.audio_pos, d.cache_len, d.x, B, D, d.head_ws, d.head_ws_bytes, s));
        return VH_OK;
    }
    if (d.kv_bf16 && d.proj_w16 && D <= 1024)
        TRY(vh_internal_linear_w16(d.x, D, d.proj_w16, nullptr, nullptr, 0, d.logits, dec->ldl, B, d.V, D, s));
    else
        TRY(vh_linear(d.x, D, d.proj_w, nullptr, nullptr, 0, d.logits, dec->ldl, B, d.V, D, VH_ACT_NONE,
                      nullptr, nullptr, nullptr, nullptr, 0.f, s));
    if (d.top_k == 1 && !d.row_sampling)
        TRY(vh_greedy_step(d.logits, dec->ldl, d.V, d.eos, d.codes, d.codes_stride, d.eos_count,
                           d.pos_base, d.audio_emb, d.audio_pe, d.audio_pos, d.cache_len, d.x, B, D, s));
    else if (d.V > 2048)              // wider than vh_sample_step's LDS row (decoder_check bounds V by VH_SAMPLE_MAX_V)
        TRY(vh_internal_sample_step_wide(d.logits, dec->ldl, d.V, d.eos, d.top_k, d.top_p, d.temperature, d.seed, d.seed_dev,
                                         d.row_sampling, dec->row_limits, d.codes, d.codes_stride, d.eos_count, d.pos_base,
                                         d.sum_logprobs, d.audio_emb, d.audio_pe, d.audio_pos, d.cache_len, d.x, B, D, s));
    else
        TRY(vh_internal_sample_step(d.logits, dec->ldl, d.V, d.eos, d.top_k, d.top_p, d.temperature, d.seed, d.seed_dev,
                                    d.row_sampling, dec->row_limits, d.codes, d.codes_stride, d.eos_count, d.pos_base,
                                    d.sum_logprobs, d.audio_emb, d.audio_pe, d.audio_pos, d.cache_len, d.x, B, D, s));
    return VH_OK;
}

// The per-row length bounds of the decoder's sample steps (elementwise.hip, ROW_LIMITS_LOAD).  Not a descriptor field: the
// descriptor keeps row_sampling as its trailing field.  The captured graphs hold the pointer, so it cannot change under them.
extern "C" int vh_ar_decoder_set_row_limits(vh_ar_decoder* dec, const vh_row_limits* limits) {
    VH_REQUIRE(dec, VH_EINVAL, "vh_ar_decoder_set_row_limits: null decoder");
    VH_REQUIRE(!dec->exec && !dec->exec_n, VH_ESTATE,
               "vh_ar_decoder_set_row_limits: called after vh_ar_decoder_capture (the graphs hold the pointer: set it before capture)");
    // (with row_sampling the step is the sampler on every row: decoder_check refuses row_sampling with head_ws, so no decoder
    // that passes here enqueues vh_head_greedy or vh_greedy_step, which read no limits)
    VH_REQUIRE(dec->d.row_sampling, VH_EINVAL,
               "vh_ar_decoder_set_row_limits: a decoder without row_sampling (the length bounds sit beside per-row sampling records)");
    VH_REQUIRE(dec->d.pos_base, VH_EINVAL,
               "vh_ar_decoder_set_row_limits: a decoder without pos_base (a row's tokens are counted from it)");
    VH_REQUIRE(dec->d.V >= 2, VH_EINVAL, "vh_ar_decoder_set_row_limits: V=%d (a token besides EOS to draw below min_new: V >= 2)",
               dec->d.V);
    VH_REQUIRE(((uintptr_t)limits & 7u) == 0, VH_EALIGN, "vh_ar_decoder_set_row_limits: limits must be 8-byte aligned");
    dec->row_limits = limits;
    return VH_OK;
}

extern "C" int vh_ar_decoder_step(vh_ar_decoder* dec, void* stream) {
    VH_REQUIRE(dec, VH_EINVAL, "vh_ar_decoder_step: null decoder");
    return decoder_enqueue(dec, (hipStream_t)stream, nullptr);
}

#define VH_GRAPH_STEPS 8

static int capture_steps(vh_ar_decoder* dec, hipStream_t s, int n_steps, hipGraph_t* graph, hipGraphExec_t* exec) {
    if (*exec) { (void)hipGraphExecDestroy(*exec); *exec = nullptr; }
    if (*graph) { (void)hipGraphDestroy(*graph); *graph = nullptr; }
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    VH_REQUIRE(e == hipSuccess, VH_ELAUNCH, "hipStreamBeginCapture: %s", hipGetErrorString(e));
    int rc = VH_OK;
    for (int i = 0; i < n_steps && rc == VH_OK; ++i) rc = decoder_enqueue(dec, s, nullptr);
    e = hipStreamEndCapture(s, graph);
    if (rc != VH_OK) return rc;
    VH_REQUIRE(e == hipSuccess && *graph, VH_ELAUNCH, "hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(exec, *graph, nullptr, nullptr, 0);
    VH_REQUIRE(e == hipSuccess, VH_ELAUNCH, "hipGraphInstantiate: %s", hipGetErrorString(e));
    return VH_OK;
}

extern "C" int vh_ar_decoder_capture(vh_ar_decoder* dec, void* stream) {
    VH_REQUIRE(dec, VH_EINVAL, "vh_ar_decoder_capture: null decoder");
    VH_REQUIRE(stream, VH_EINVAL, "vh_ar_decoder_capture: capture needs a non-null stream");
    hipStream_t s = (hipStream_t)stream;
    // the step advances device-side state only, so N captured steps are the same step N times: one graph of a
    // single step (remainders) and one of VH_GRAPH_STEPS steps (the bulk: an eighth of the graph launches)
    TRY(capture_steps(dec, s, 1, &dec->graph, &dec->exec));
    if (vh_tuning(VH_TUNE_GRAPH_STEPS) != 1) TRY(capture_steps(dec, s, VH_GRAPH_STEPS, &dec->graph_n, &dec->exec_n));
    return VH_OK;
}

extern "C" int vh_ar_decoder_replay(vh_ar_decoder* dec, int n_steps, void* stream) {
    VH_REQUIRE(dec && dec->exec, VH_ESTATE, "vh_ar_decoder_replay: capture first");
    VH_REQUIRE(n_steps >= 0, VH_EINVAL, "vh_ar_decoder_replay: n_steps=%d", n_steps);
    hipStream_t s = (hipStream_t)stream;
    int i = 0;
    if (dec->exec_n)
        for (; i + VH_GRAPH_STEPS <= n_steps; i += VH_GRAPH_STEPS) HIP_TRY(hipGraphLaunch(dec->exec_n, s));
    for (; i < n_steps; ++i) HIP_TRY(hipGraphLaunch(dec->exec, s));
    return VH_OK;
}

static float mean_event_pairs(std::vector<hipEvent_t>& ev) {
    double total = 0.0;
    int n = 0;
    for (size_t i = 0; i + 1 < ev.size(); i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) { total += ms; ++n; }
    }
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
    return n ? (float)(total / n) : 0.f;
}

extern "C" int vh_ar_decoder_profile_attn(vh_ar_decoder* dec, int n_steps, void* stream,
                                          float* mean_ms, float* floor_ms, float* kernel_ms) {
    VH_REQUIRE(dec && mean_ms && n_steps > 0, VH_EINVAL, "vh_ar_decoder_profile_attn: bad args");
    hipStream_t s = (hipStream_t)stream;
    std::vector<hipEvent_t> ev, fl, kev;
    int rc = VH_OK;
    for (int i = 0; i < n_steps && rc == VH_OK; ++i) {
        rc = decoder_enqueue(dec, s, &ev, kernel_ms ? &kev : nullptr);
        // measurement floor: the same bracket with nothing inside, once per step
        hipEvent_t f0, f1;
        if (floor_ms && hipEventCreate(&f0) == hipSuccess && hipEventCreate(&f1) == hipSuccess) {
            (void)hipEventRecord(f0, s);
            (void)hipEventRecord(f1, s);
            fl.push_back(f0);
            fl.push_back(f1);
        }
    }
    (void)hipStreamSynchronize(s);
    if (floor_ms) *floor_ms = mean_event_pairs(fl);
    if (kernel_ms) *kernel_ms = mean_event_pairs(kev);
    *mean_ms = mean_event_pairs(ev);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// full-sequence forward (prefill / NAR stage / training forward)
// ---------------------------------------------------------------------------------------------
// the layers of both forwards: the same launches in the same order, the packed one with vh_attn_rows_packed for vh_attn_rows
static int forward_layers(const vh_forward_desc* f, const vh_segments* pk, void* stream) {
    const int B = f->B, T = f->T, D = f->d_model, M = B * T;
    for (int i = 0; i < f->n_layers; ++i) {
        const vh_layer& L = f->layers[i];
        const float* ada = f->ada ? f->ada + (int64_t)i * 4 * D : nullptr;
        const float* src = (i == 0 && f->x_in) ? f->x_in : f->x;     // layer 0 may read a caller-owned input
        TRY(vh_layernorm(src, L.ln1_g, L.ln1_b, ada, ada ? ada + D : nullptr, f->xn, M, D, f->ln_eps,
                         stream));
        TRY(vh_linear_qkv(f->xn, D, L.wqkv, f->q, D, L.kcache, L.vcache, nullptr, B, T, D, f->n_heads,
                          f->S_max, nullptr, nullptr, nullptr, nullptr, 0.f, stream));
        if (pk && pk->seg_x_len)
            TRY(vh_attn_rows_packed_lse(f->q, D, L.kcache, L.vcache, f->attn, D, f->n_heads, T, f->S_max, VH_MASK_PREFIX,
                                        pk->seg_start, pk->seg_len, pk->seg_x_len, pk->n_seg, pk->blocks, pk->n_blocks, pk->lse2,
                                        stream));
        else if (pk)
            TRY(vh_attn_rows_packed(f->q, D, L.kcache, L.vcache, f->attn, D, f->n_heads, f->S_max, pk->seg_start, pk->seg_len,
                                    pk->n_seg, pk->blocks, pk->n_blocks, stream));
        else
            TRY(vh_attn_rows(f->q, D, L.kcache, L.vcache, f->attn, D, B, f->n_heads, T, T, f->S_max,
                             f->mode, f->x_len, f->x_len_dev, f->kv_len, f->mask, f->pad, stream));
        TRY(vh_linear_ws(f->attn, D, L.wo, L.bo, src, D, f->x, D, M, D, D, VH_ACT_NONE, f->gemm_ws,
                         f->gemm_ws_bytes, stream));
        TRY(vh_layernorm(f->x, L.ln2_g, L.ln2_b, ada ? ada + 2 * D : nullptr, ada ? ada + 3 * D : nullptr,
                         f->xn, M, D, f->ln_eps, stream));
        TRY(vh_linear_ws(f->xn, D, L.w1, L.b1, nullptr, 0, f->hidden, f->dff, M, f->dff, D, VH_ACT_GELU_ERF,
                         f->gemm_ws, f->gemm_ws_bytes, stream));
        TRY(vh_linear_ws(f->hidden, f->dff, L.w2, L.b2, f->x, D, f->x, D, M, D, f->dff, VH_ACT_NONE, f->gemm_ws,
                         f->gemm_ws_bytes, stream));
    }
    return VH_OK;
}

extern "C" int vh_transformer_forward(const vh_forward_desc* f, void* stream) {
    VH_REQUIRE(f && f->layers && f->x && f->xn && f->q && f->attn && f->hidden, VH_EINVAL,
               "vh_transformer_forward: null pointer in desc");
    VH_REQUIRE(f->B > 0 && f->T > 0 && f->n_layers > 0 && f->S_max >= f->T, VH_EINVAL,
               "vh_transformer_forward: bad dims B=%d T=%d L=%d S_max=%d", f->B, f->T, f->n_layers,
               f->S_max);
    VH_REQUIRE(f->d_model == f->n_heads * VH_HEAD_DIM, VH_EUNSUPPORTED,
               "vh_transformer_forward: d_model=%d != n_heads=%d x 64", f->d_model, f->n_heads);
    return forward_layers(f, nullptr, stream);
}

// What both packed forwards refuse alike past vh_common.h's vh_packed_front / vh_packed_stream / vh_packed_mask, under the name of
// the entry point that was called: the masks of the padded forward (packed_no_masks) ...
static int packed_no_masks(const char* name, const vh_forward_desc* f) {
    VH_REQUIRE(!f->mask, VH_EUNSUPPORTED, "%s: mask is set (no explicit mask over segments)", name);
    VH_REQUIRE(!f->pad, VH_EUNSUPPORTED, "%s: pad is set (packed rows have no padding)", name);
    return VH_OK;
}

// ... and the head width, and what the packed attention would refuse inside layer 0 (lse2 where there is one), said before
// anything is launched (packed_back)
static int packed_back(const char* name, const vh_forward_desc* f, const vh_segments& sg) {
    VH_REQUIRE(f->d_model == f->n_heads * VH_HEAD_DIM, VH_EUNSUPPORTED, "%s: d_model=%d != n_heads=%d x 64", name, f->d_model,
               f->n_heads);
    VH_REQUIRE(vh_aligned16(f->q), VH_EALIGN, "%s: q must be 16-byte aligned", name);
    VH_REQUIRE(vh_aligned16(f->attn), VH_EALIGN, "%s: attn must be 16-byte aligned", name);
    VH_REQUIRE((reinterpret_cast<uintptr_t>(sg.lse2) & 3u) == 0, VH_EALIGN, "%s: lse2 must be 4-byte aligned", name);
    TRY(vh_packed_workgroups(name, sg.n_blocks, f->n_heads));
    for (int i = 0; i < f->n_layers; ++i) {
        VH_REQUIRE(f->layers[i].kcache && f->layers[i].vcache, VH_EINVAL, "%s: null kcache / vcache (layer %d)", name, i);
        VH_REQUIRE(vh_aligned16(f->layers[i].kcache) && vh_aligned16(f->layers[i].vcache), VH_EALIGN,
                   "%s: kcache and vcache must be 16-byte aligned (layer %d)", name, i);
    }
    return VH_OK;
}

static bool desc_complete(const vh_forward_desc* f) { return f && f->layers && f->x && f->xn && f->q && f->attn && f->hidden; }

extern "C" int vh_transformer_forward_packed(const vh_forward_desc* f, const int32_t* seg_start, const int32_t* seg_len, int n_seg,
                                             const int32_t* blocks, int n_blocks, void* stream) {
    const char* name = "vh_transformer_forward_packed";
    const vh_segments sg{seg_start, seg_len, blocks, n_seg, n_blocks, nullptr, nullptr};
    TRY(vh_packed_front(name, f, desc_complete(f), sg));
    TRY(vh_packed_mask(name, f, false));
    TRY(packed_no_masks(name, f));
    TRY(packed_back(name, f, sg));
    return forward_layers(f, &sg, stream);
}

// The prompt pass of a ragged batch over packed rows: vh_transformer_forward_packed's launches under the prefix-LM mask of
// every segment.  The attention is the packed TRAINING forward (attn_rows_packed_lse_kernel: attn_rows_body.inc takes the mask
// mode and seg_x_len only in the instantiation that also writes lse2), so the caller lends an (n_heads, T) lse2 it never reads.
extern "C" int vh_transformer_forward_packed_lm(const vh_forward_desc* f, const int32_t* seg_start, const int32_t* seg_len,
                                                const int32_t* seg_x_len, int n_seg, const int32_t* blocks, int n_blocks,
                                                float* lse2, void* stream) {
    const char* name = "vh_transformer_forward_packed_lm";
    const vh_segments sg{seg_start, seg_len, blocks, n_seg, n_blocks, seg_x_len, lse2};
    VH_REQUIRE(desc_complete(f), VH_EINVAL, "vh_transformer_forward_packed_lm: null pointer in desc");
    VH_REQUIRE(seg_start && seg_len && seg_x_len && blocks, VH_EINVAL,
               "vh_transformer_forward_packed_lm: null pointer (seg_start, seg_len, seg_x_len or blocks)");
    VH_REQUIRE(lse2, VH_EINVAL, "vh_transformer_forward_packed_lm: null pointer (lse2: (n_heads, T) floats of scratch)");
    TRY(vh_packed_stream(name, f, n_seg, n_blocks));
    TRY(vh_packed_mask(name, f, true));
    TRY(packed_no_masks(name, f));
    VH_REQUIRE(!f->ada, VH_EUNSUPPORTED, "vh_transformer_forward_packed_lm: ada is set (LayerNorm stacks only)");
    TRY(packed_back(name, f, sg));
    return forward_layers(f, &sg, stream);
}
