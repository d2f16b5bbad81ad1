// The model input of PACKED NAR training (ValleNAR.training_step_packed), forward and backward, over the packed rows
// themselves: segment s of `out` (M, d) starts at row seg_start[s] and holds x_len[s] text rows, then a_len[s] audio rows.
//   text row i   = text_table[tokens[s, i]] + pe_text[i]
//   audio row t  = sum_{j < n(t)} code_tables[j][codes[s, t, j]] + pe_audio[t],  n(t) = n_full for t < prefix[s], else n_rest
// Both kernels find a row's segment by a binary search over seg_start (ascending, as engine.PackedRows builds it): n_seg
// wave-uniform loads of an array that stays in the scalar / L1 cache, no host-built row table to keep in step with M.
// A row the search cannot place inside its segment (a gap between segments, a table out of order, a position beyond the
// caller's max_x_len / max_a_len) is neither read nor written.  The forward is an HBM-bound row kernel, float4 per lane; the
// backward is bound by its atomics and gives a thread a column, so that a wave adds into consecutive floats.
#include "vh_common.h"

struct NarTables {
    const float* t[VH_MAX_TABLES];
    int vocab[VH_MAX_TABLES];
};
struct NarGradTables {
    float* t[VH_MAX_TABLES];             // nullptr: that table takes no gradient
    int vocab[VH_MAX_TABLES];
};
struct NarSegs {
    const int32_t* seg_start;
    const int32_t* x_len;
    const int32_t* a_len;
    const int32_t* prefix;
    int n_seg, max_x_len, max_a_len;
};

enum { NAR_ROW_NONE = -1, NAR_ROW_TEXT = 0, NAR_ROW_AUDIO = 1 };

// packed row r -> (segment, stream, position in the stream, tables the row sums).  NAR_ROW_NONE: r belongs to no segment.
__device__ __forceinline__ int nar_locate(const NarSegs& g, int r, int n_full, int n_rest, int& seg, int& pos, int& n) {
    int lo = 0, hi = g.n_seg;                                     // largest s with seg_start[s] <= r
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.seg_start[mid] <= r) lo = mid; else hi = mid;
    }
    seg = lo;
    const int i = r - g.seg_start[lo];
    const int xl = min(max(g.x_len[lo], 0), g.max_x_len), al = min(max(g.a_len[lo], 0), g.max_a_len);
    if (i < 0 || i >= xl + al) return NAR_ROW_NONE;
    if (i < xl) {
        pos = i;
        n = 1;
        return NAR_ROW_TEXT;
    }
    pos = i - xl;
    n = pos < g.prefix[lo] ? n_full : n_rest;
    return NAR_ROW_AUDIO;
}

// ---------------------------------------------------------------------------------------------
// Forward.  grid ceil(M / 4), block 256 = 4 waves, one wave per packed row.  Lane j < n(t) reads and range-checks the id of
// table j once; the column loop takes table j's row from lane j (v_readlane: j is wave-uniform), so one form serves 1 ..
// VH_MAX_TABLES tables without a per-table array.  The additions are vh_embed_sum_pe's, in its order — tables in
// ascending j, then the position row, then the dropout field of the row's own stream keyed on the PACKED row — so a
// segment's rows are bit for bit what vh_embed_sum_pe writes for that utterance alone at the same rows of `out`.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_nar_packed_kernel(
    const int64_t* __restrict__ tokens, int64_t tok_bs, const int64_t* __restrict__ codes, int64_t codes_bs, int64_t codes_ts,
    int64_t codes_js, const float* __restrict__ text_table, int text_vocab, NarTables tabs, int n_full, int n_rest,
    const float* __restrict__ pe_text, const float* __restrict__ pe_audio, NarSegs segs, float* __restrict__ out, int M, int d,
    int32_t* __restrict__ err_flag, DropArgs drop_text, DropArgs drop_audio) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= M) return;
    int seg, pos, n;
    const int kind = nar_locate(segs, r, n_full, n_rest, seg, pos, n);
    if (kind == NAR_ROW_NONE) return;
    int row = 0;                                                  // lane j: the row of table j this packed row reads
    bool ok = true;
    if (lane < n) {
        int64_t id;
        int vocab;
        if (kind == NAR_ROW_TEXT) {
            id = tokens[seg * tok_bs + pos];
            vocab = text_vocab;
        } else {
            id = codes[seg * codes_bs + pos * codes_ts + lane * codes_js];
            vocab = tabs.vocab[lane];
        }
        ok = id >= 0 && id < vocab;                               // an id outside its table reads row 0 and raises the flag
        row = ok ? (int)id : 0;
    }
    if (__ballot(!ok) && err_flag && lane == 0) atomicOr(err_flag, VH_DEVERR_EMBED_ID);
    const bool text = kind == NAR_ROW_TEXT;
    const float* prow = (text ? pe_text : pe_audio) + (int64_t)pos * d;
    const DropArgs drop = text ? drop_text : drop_audio;
    float* orow = out + (int64_t)r * d;
    const float* t0 = text ? text_table : tabs.t[0];
    const int64_t row0 = __builtin_amdgcn_readlane(row, 0);
    for (int c = lane * 4; c < d; c += 256) {
        const f32x4 acc = ld4(prow + c);
        f32x4 e = ld4(t0 + row0 * d + c);
        for (int j = 1; j < n; ++j) e += ld4(tabs.t[j] + (int64_t)__builtin_amdgcn_readlane(row, j) * d + c);
        e += acc;
        if (drop.thresh) e = e * vh_dropmul4(drop, (uint32_t)r, (uint32_t)c >> 2);
        st4(orow + c, e);
    }
}

static int nar_packed_check(const char* name, const void* tokens, const void* codes, const void* text_table, int text_vocab,
                            const void* const* code_tables, const int32_t* code_vocab, int n_full, int n_rest,
                            int pe_text_rows, int pe_audio_rows, const int32_t* seg_start, const int32_t* x_len,
                            const int32_t* a_len, const int32_t* prefix, int n_seg, int max_x_len, int max_a_len,
                            const void* rows, const char* rows_name, int M, int d, const vh_dropout_spec* drop_text,
                            const vh_dropout_spec* drop_audio, bool tables_may_be_null) {
    const struct { const void* p; const char* what; } ptrs[] = {
        {tokens, "tokens"}, {codes, "codes"}, {text_table, "text_table"}, {code_tables, "code_tables"}, {code_vocab, "code_vocab"},
        {rows, rows_name}, {seg_start, "seg_start"}, {x_len, "x_len"}, {a_len, "a_len"}, {prefix, "prefix"}};
    for (const auto& a : ptrs) VH_REQUIRE(a.p, VH_EINVAL, "%s: null pointer: %s", name, a.what);
    VH_REQUIRE(n_full >= 1 && n_full <= VH_MAX_TABLES, VH_EINVAL, "%s: n_full=%d not in 1..%d", name, n_full, VH_MAX_TABLES);
    VH_REQUIRE(n_rest >= 1 && n_rest <= n_full, VH_EINVAL, "%s: n_rest=%d not in 1..n_full=%d", name, n_rest, n_full);
    VH_REQUIRE(M > 0, VH_EINVAL, "%s: M=%d must be positive", name, M);
    VH_REQUIRE(n_seg > 0, VH_EINVAL, "%s: n_seg=%d must be positive", name, n_seg);
    VH_REQUIRE(d > 0 && d % 4 == 0, VH_EINVAL, "%s: d=%d must be a positive multiple of 4 (float4 lanes, dropout fields)", name, d);
    VH_REQUIRE(text_vocab > 0, VH_EINVAL, "%s: text_vocab=%d", name, text_vocab);
    VH_REQUIRE(max_x_len >= 0 && max_a_len >= 0, VH_EINVAL, "%s: max_x_len=%d max_a_len=%d", name, max_x_len, max_a_len);
    VH_REQUIRE(pe_text_rows >= max_x_len, VH_EINVAL, "%s: pe_text_rows=%d below the longest text stream (max_x_len=%d)", name,
               pe_text_rows, max_x_len);
    VH_REQUIRE(pe_audio_rows >= max_a_len, VH_EINVAL, "%s: pe_audio_rows=%d below the longest audio stream (max_a_len=%d)", name,
               pe_audio_rows, max_a_len);
    VH_REQUIRE(VH_DROP_OK(drop_text) && VH_DROP_OK(drop_audio), VH_EINVAL, "%s: dropout p must be in [0, 1)", name);
    VH_REQUIRE(vh_aligned16(rows) && vh_aligned16(text_table), VH_EALIGN, "%s: %s / text_table must be 16-byte aligned", name, rows_name);
    for (int j = 0; j < n_full; ++j) {
        VH_REQUIRE(code_tables[j] || tables_may_be_null, VH_EINVAL, "%s: null pointer: code_tables[%d]", name, j);
        VH_REQUIRE(vh_aligned16(code_tables[j]), VH_EALIGN, "%s: code table %d must be 16-byte aligned", name, j);
        VH_REQUIRE(code_vocab[j] > 0, VH_EINVAL, "%s: code table %d has %d rows", name, j, code_vocab[j]);
    }
    return VH_OK;
}

extern "C" int vh_embed_nar_packed(const int64_t* tokens, int64_t tokens_bstride, const int64_t* codes, int64_t codes_bstride,
                                   int64_t codes_tstride, int64_t codes_jstride, const float* text_table, int text_vocab,
                                   const float* const* code_tables, const int32_t* code_vocab, int n_full, int n_rest,
                                   const float* pe_text, int pe_text_rows, const float* pe_audio, int pe_audio_rows,
                                   const int32_t* seg_start, const int32_t* x_len, const int32_t* a_len, const int32_t* prefix,
                                   int n_seg, int max_x_len, int max_a_len, float* out, int M, int d, int32_t* err_flag,
                                   const vh_dropout_spec* drop_text, const vh_dropout_spec* drop_audio, void* stream) {
    VH_REQUIRE(pe_text, VH_EINVAL, "vh_embed_nar_packed: null pointer: pe_text");
    VH_REQUIRE(pe_audio, VH_EINVAL, "vh_embed_nar_packed: null pointer: pe_audio");
    const int rc = nar_packed_check("vh_embed_nar_packed", tokens, codes, text_table, text_vocab, (const void* const*)code_tables,
                                    code_vocab, n_full, n_rest, pe_text_rows, pe_audio_rows, seg_start, x_len, a_len, prefix,
                                    n_seg, max_x_len, max_a_len, out, "out", M, d, drop_text, drop_audio, false);
    if (rc != VH_OK) return rc;
    VH_REQUIRE(vh_aligned16(pe_text) && vh_aligned16(pe_audio), VH_EALIGN, "vh_embed_nar_packed: pe tables must be 16-byte aligned");
    NarTables tp{};
    for (int j = 0; j < n_full; ++j) { tp.t[j] = code_tables[j]; tp.vocab[j] = code_vocab[j]; }
    DropArgs dt, da;
    vh_drop_args(drop_text, &dt);
    vh_drop_args(drop_audio, &da);
    const NarSegs segs{seg_start, x_len, a_len, prefix, n_seg, max_x_len, max_a_len};
    hipLaunchKernelGGL(embed_nar_packed_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, tokens, tokens_bstride,
                       codes, codes_bstride, codes_tstride, codes_jstride, text_table, text_vocab, tp, n_full, n_rest, pe_text,
                       pe_audio, segs, out, M, d, err_flag, dt, da);
    VH_CHECK_LAUNCH("vh_embed_nar_packed");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// Backward.  A workgroup owns NAR_RUN consecutive packed rows, a thread a column, as in embed_bwd_kernel: the lanes of a wave
// then add into 64 consecutive floats of a table row, two cache lines per atomic instruction (a thread owning a float4 spread
// every atomic instruction over eight lines and ran 1.7 x slower than the per-table launches it replaces).  It reads its
// column of every row ONCE (all in flight), multiplies the regenerated field of the row's stream, and then walks the rows once per table — the text
// table, then each code table with a gradient — adding up consecutive rows that name the SAME table row before the atomic
// is issued (embed_bwd_kernel's run collapsing: codec streams hold long runs of one id).  A row that does not read a table
// (another stream, j >= n(t), an id out of range, a row of no segment) carries -1 there and ends the run.  Two segments
// that meet inside the 16 rows are told apart by the row's own entry, so a run never crosses into another table.
// ---------------------------------------------------------------------------------------------
#define NAR_RUN 16
__global__ __launch_bounds__(256) void embed_nar_packed_bwd_kernel(
    const int64_t* __restrict__ tokens, int64_t tok_bs, const int64_t* __restrict__ codes, int64_t codes_bs, int64_t codes_ts,
    int64_t codes_js, float* __restrict__ dtext_table, int text_vocab, NarGradTables tabs, int n_full, int n_rest, NarSegs segs,
    const float* __restrict__ dout, int M, int d, int32_t* __restrict__ err_flag, DropArgs drop_text, DropArgs drop_audio) {
    __shared__ int s_kind[NAR_RUN], s_seg[NAR_RUN], s_pos[NAR_RUN], s_n[NAR_RUN];
    __shared__ int s_text[NAR_RUN];                               // the text table's row per packed row, -1 = none
    __shared__ int s_code[VH_MAX_TABLES][NAR_RUN];                // code table j's row per packed row, -1 = none
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * NAR_RUN;
    if (tid < NAR_RUN) {
        const int r = r0 + tid;
        int seg = 0, pos = 0, n = 0, kind = NAR_ROW_NONE, trow = -1;
        if (r < M) kind = nar_locate(segs, r, n_full, n_rest, seg, pos, n);
        if (kind == NAR_ROW_TEXT) {
            const int64_t id = tokens[seg * tok_bs + pos];
            if (id >= 0 && id < text_vocab) trow = (int)id;       // never scatter outside the table
            else if (err_flag) atomicOr(err_flag, VH_DEVERR_EMBED_ID);
        }
        s_kind[tid] = kind; s_seg[tid] = seg; s_pos[tid] = pos; s_n[tid] = n; s_text[tid] = trow;
    }
    __syncthreads();
    for (int e = tid; e < n_full * NAR_RUN; e += blockDim.x) {
        const int j = e / NAR_RUN, i = e % NAR_RUN;
        int crow = -1;
        if (s_kind[i] == NAR_ROW_AUDIO && j < s_n[i]) {
            const int64_t id = codes[s_seg[i] * codes_bs + s_pos[i] * codes_ts + j * codes_js];
            if (id >= 0 && id < tabs.vocab[j]) crow = (int)id;
            else if (err_flag) atomicOr(err_flag, VH_DEVERR_EMBED_ID);
        }
        s_code[j][i] = crow;
    }
    __syncthreads();
    const float* src = dout + (int64_t)r0 * d;
    for (int c = tid; c < d; c += blockDim.x) {
        float v[NAR_RUN];
#pragma unroll
        for (int i = 0; i < NAR_RUN; ++i)                          // the gradient row, read once for all its tables
            v[i] = s_kind[i] != NAR_ROW_NONE ? src[(int64_t)i * d + c] : 0.f;
        if (drop_text.thresh | drop_audio.thresh) {              // (a thread owns a column: one of the four words of a Philox call)
#pragma unroll
            for (int i = 0; i < NAR_RUN; ++i) {
                const DropArgs dr = s_kind[i] == NAR_ROW_TEXT ? drop_text : drop_audio;
                if (dr.thresh && s_kind[i] != NAR_ROW_NONE) v[i] *= vh_dropmul4(dr, (uint32_t)(r0 + i), (uint32_t)c >> 2)[c & 3];
            }
        }
        auto scatter = [&](float* __restrict__ table, const int* rows) {
            int cur = -1;
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i <= NAR_RUN; ++i) {
                const int id = i < NAR_RUN ? rows[i] : -1;
                if (id == cur) {
                    if (i < NAR_RUN) acc += v[i];
                    continue;
                }
                if (cur >= 0) atomicAdd(table + (int64_t)cur * d + c, acc);
                cur = id;
                if (i < NAR_RUN) acc = v[i];
            }
        };
        if (dtext_table) scatter(dtext_table, s_text);
        for (int j = 0; j < n_full; ++j)
            if (tabs.t[j]) scatter(tabs.t[j], s_code[j]);
    }
}

extern "C" int vh_embed_nar_packed_bwd(const int64_t* tokens, int64_t tokens_bstride, const int64_t* codes, int64_t codes_bstride,
                                       int64_t codes_tstride, int64_t codes_jstride, const float* dout, float* dtext_table,
                                       int text_vocab, float* const* dcode_tables, const int32_t* code_vocab, int n_full,
                                       int n_rest, int pe_text_rows, int pe_audio_rows, const int32_t* seg_start,
                                       const int32_t* x_len, const int32_t* a_len, const int32_t* prefix, int n_seg,
                                       int max_x_len, int max_a_len, int M, int d, int32_t* err_flag,
                                       const vh_dropout_spec* drop_text, const vh_dropout_spec* drop_audio, void* stream) {
    // dtext_table and the entries of dcode_tables may be NULL (no gradient wanted there); the array itself may not
    static const float aligned_dummy __attribute__((aligned(16))) = 0.f;
    const int rc = nar_packed_check("vh_embed_nar_packed_bwd", tokens, codes, dtext_table ? (const void*)dtext_table : &aligned_dummy,
                                    text_vocab, (const void* const*)dcode_tables, code_vocab, n_full, n_rest, pe_text_rows,
                                    pe_audio_rows, seg_start, x_len, a_len, prefix, n_seg, max_x_len, max_a_len, dout, "dout", M, d,
                                    drop_text, drop_audio, true);
    if (rc != VH_OK) return rc;
    NarGradTables tp{};
    for (int j = 0; j < n_full; ++j) { tp.t[j] = dcode_tables[j]; tp.vocab[j] = code_vocab[j]; }
    DropArgs dt, da;
    vh_drop_args(drop_text, &dt);
    vh_drop_args(drop_audio, &da);
    const NarSegs segs{seg_start, x_len, a_len, prefix, n_seg, max_x_len, max_a_len};
    const int lanes = (d + 63) / 64 * 64;                          // a thread owns a column (and every 256th after it)
    const int block = lanes > 256 ? 256 : lanes;
    hipLaunchKernelGGL(embed_nar_packed_bwd_kernel, dim3((M + NAR_RUN - 1) / NAR_RUN), dim3(block), 0, (hipStream_t)stream, tokens,
                       tokens_bstride, codes, codes_bstride, codes_tstride, codes_jstride, dtext_table, text_vocab, tp, n_full,
                       n_rest, segs, dout, M, d, err_flag, dt, da);
    VH_CHECK_LAUNCH("vh_embed_nar_packed_bwd");
    return VH_OK;
}
