// Embedding-sum + position add, LayerNorm / adaptive LayerNorm, greedy step.
// All HBM-bound row kernels: one wave64 per row, float4 per lane, wave-shuffle reductions.
#include "vh_common.h"

template <int CAP>
struct TablePtrs {
    const float* t[CAP];
    int vocab[CAP];
};

// ---------------------------------------------------------------------------------------------
// K1/K2  out[b, out_t0+t, :] = sum_j tables[j][ids[b,t,j], :] + pe[pos0+t, :]
// grid: (ceil(T/4), B), block 256 = 4 waves, one wave per (b,t) row.
// Two forms: embed_sum_pe_kernel<8> (up to 8 tables: every id read and checked once into a per-table array) and
// embed_sum_pe_many_kernel (9 to VH_MAX_TABLES tables: no per-table array, which at 32 entries would live in scratch).
// Both sum the codebooks in table order, then add the position row, then apply dropout: the same bits.
// ---------------------------------------------------------------------------------------------
template <int CAP>
__global__ __launch_bounds__(256) void embed_sum_pe_kernel(
    const int64_t* __restrict__ ids, int64_t ids_bs, int64_t ids_ts, int64_t ids_js, TablePtrs<CAP> tabs,
    int n_tables, const float* __restrict__ pe, int pos0, const int32_t* __restrict__ lens,
    float* __restrict__ out, int64_t out_bs, int out_t0, int T, int d, int32_t* __restrict__ err_flag,
    const int32_t* __restrict__ row_pos0, const int32_t* __restrict__ row_t0, DropArgs drop) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (t >= T) return;
    if (lens && t >= lens[b]) return;
    if (row_pos0) pos0 = row_pos0[b];               // ragged batches: every row its own position / output offset
    if (row_t0) out_t0 = row_t0[b];
    const int64_t* idp = ids + b * ids_bs + t * ids_ts;
    // ids are range-checked here (the reference's nn.Embedding raises IndexError): an id outside its
    // table reads row 0 and raises the device flag the host polls at its next synchronisation
    int64_t row[CAP];
    bool bad = false;
    for (int j = 0; j < n_tables; ++j) {
        const int64_t id = idp[j * ids_js];
        const bool ok = id >= 0 && id < tabs.vocab[j];
        bad |= !ok;
        row[j] = ok ? id : 0;
    }
    if (bad && err_flag && lane == 0) atomicOr(err_flag, VH_DEVERR_EMBED_ID);
    float* orow = out + b * out_bs + (int64_t)(out_t0 + t) * d;
    const float* prow = pe ? pe + (int64_t)(pos0 + t) * d : nullptr;
    // dropout after the position add (modules.py:80): the field's row is this row's index in `out`
    const uint32_t frow = (uint32_t)((b * out_bs) / d + out_t0 + t);
    for (int c = lane * 4; c < d; c += 256) {
        f32x4 acc = prow ? ld4(prow + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 e = ld4(tabs.t[0] + row[0] * d + c);
        // sum the codebooks first, then add the position row: same order as the reference
        // (emb0 + emb1 + ... then + pe), so fp32 rounding matches op for op.
        for (int j = 1; j < n_tables; ++j) e += ld4(tabs.t[j] + row[j] * d + c);
        e += acc;
        if (drop.thresh) e = e * vh_dropmul4(drop, frow, (uint32_t)c >> 2);
        st4(orow + c, e);
    }
}

// 9..VH_MAX_TABLES tables (EnCodec at 12 / 24 kbps: 16 / 32 codebooks): each table's id is read where it is used (one
// wave-uniform load per table and column pass, from the L1 after the first pass) and range-checked there.
__global__ __launch_bounds__(256) void embed_sum_pe_many_kernel(
    const int64_t* __restrict__ ids, int64_t ids_bs, int64_t ids_ts, int64_t ids_js, TablePtrs<VH_MAX_TABLES> tabs,
    int n_tables, const float* __restrict__ pe, int pos0, const int32_t* __restrict__ lens,
    float* __restrict__ out, int64_t out_bs, int out_t0, int T, int d, int32_t* __restrict__ err_flag,
    const int32_t* __restrict__ row_pos0, const int32_t* __restrict__ row_t0, DropArgs drop) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y;
    if (t >= T) return;
    if (lens && t >= lens[b]) return;
    if (row_pos0) pos0 = row_pos0[b];
    if (row_t0) out_t0 = row_t0[b];
    const int64_t* idp = ids + b * ids_bs + t * ids_ts;
    float* orow = out + b * out_bs + (int64_t)(out_t0 + t) * d;
    const float* prow = pe ? pe + (int64_t)(pos0 + t) * d : nullptr;
    const uint32_t frow = (uint32_t)((b * out_bs) / d + out_t0 + t);
    bool bad = false;
    for (int c = lane * 4; c < d; c += 256) {
        f32x4 acc = prow ? ld4(prow + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        auto gather = [&](int j) {
            const int64_t id = idp[j * ids_js];
            const bool ok = id >= 0 && id < tabs.vocab[j];
            bad |= !ok;
            return ld4(tabs.t[j] + (ok ? id : 0) * d + c);
        };
        f32x4 e = gather(0);
        for (int j = 1; j < n_tables; ++j) e += gather(j);   // table order, as the form above
        e += acc;
        if (drop.thresh) e = e * vh_dropmul4(drop, frow, (uint32_t)c >> 2);
        st4(orow + c, e);
    }
    if (bad && err_flag && lane == 0) atomicOr(err_flag, VH_DEVERR_EMBED_ID);
}

extern "C" int vh_embed_sum_pe(const int64_t* ids, int64_t ids_bstride, int64_t ids_tstride,
                               int64_t ids_jstride, const float* const* tables, const int32_t* vocab,
                               int n_tables, const float* pe, int pos0, const int32_t* lens, float* out,
                               int64_t out_bstride, int out_t0, int B, int T, int d, int32_t* err_flag,
                               const int32_t* row_pos0, const int32_t* row_t0, const vh_dropout_spec* drop,
                               void* stream) {
    VH_REQUIRE(ids && tables && vocab && out, VH_EINVAL, "vh_embed_sum_pe: null pointer");
    VH_REQUIRE(n_tables >= 1 && n_tables <= VH_MAX_TABLES, VH_EINVAL,
               "vh_embed_sum_pe: n_tables=%d not in 1..%d", n_tables, VH_MAX_TABLES);
    VH_REQUIRE(B >= 0 && T >= 0 && d > 0 && d % 4 == 0, VH_EINVAL,
               "vh_embed_sum_pe: bad dims B=%d T=%d d=%d (d must be a multiple of 4)", B, T, d);
    VH_REQUIRE(vh_aligned16(out) && (!pe || vh_aligned16(pe)) && out_bstride % 4 == 0, VH_EALIGN,
               "vh_embed_sum_pe: out/pe must be 16-byte aligned");
    DropArgs da;
    VH_REQUIRE(VH_DROP_OK(drop), VH_EINVAL, "vh_embed_sum_pe: dropout p must be in [0, 1)");
    if (vh_drop_args(drop, &da))
        VH_REQUIRE(out_bstride % d == 0 && (int64_t)B * (out_bstride / d) < (1ll << 32), VH_EINVAL,
                   "vh_embed_sum_pe: dropout needs out_bstride %% d == 0");
    if (B == 0 || T == 0) return VH_OK;
    for (int j = 0; j < n_tables; ++j) {
        VH_REQUIRE(tables[j] && vh_aligned16(tables[j]), VH_EALIGN,
                   "vh_embed_sum_pe: table %d null or unaligned", j);
        VH_REQUIRE(vocab[j] > 0, VH_EINVAL, "vh_embed_sum_pe: table %d has %d rows", j, vocab[j]);
    }
    dim3 grid((T + 3) / 4, B);
    if (n_tables <= 8) {
        TablePtrs<8> tp{};
        for (int j = 0; j < n_tables; ++j) { tp.t[j] = tables[j]; tp.vocab[j] = vocab[j]; }
        hipLaunchKernelGGL(embed_sum_pe_kernel<8>, grid, dim3(256), 0, (hipStream_t)stream, ids,
                           ids_bstride, ids_tstride, ids_jstride, tp, n_tables, pe, pos0, lens, out,
                           out_bstride, out_t0, T, d, err_flag, row_pos0, row_t0, da);
    } else {
        TablePtrs<VH_MAX_TABLES> tp{};
        for (int j = 0; j < n_tables; ++j) { tp.t[j] = tables[j]; tp.vocab[j] = vocab[j]; }
        hipLaunchKernelGGL(embed_sum_pe_many_kernel, grid, dim3(256), 0, (hipStream_t)stream, ids,
                           ids_bstride, ids_tstride, ids_jstride, tp, n_tables, pe, pos0, lens, out,
                           out_bstride, out_t0, T, d, err_flag, row_pos0, row_t0, da);
    }
    VH_CHECK_LAUNCH("vh_embed_sum_pe");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// out[b, t, :] = x[b, t, :] + pe[pos0 + t, :]: PositionalEncoding.forward called as a module (valle/models/modules.py:78-80);
// the model paths add the position inside embed_sum_pe_kernel.  One float4 per thread.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_pe_kernel(const float* __restrict__ x, const float* __restrict__ pe,
                                                     float* __restrict__ out, int64_t n4, int T, int d4, int pos0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int64_t row = i / d4;
    const int c = (int)(i - row * d4), t = (int)(row % T);
    st4(out + i * 4, ld4(x + i * 4) + ld4(pe + ((int64_t)(pos0 + t) * d4 + c) * 4));
}

extern "C" int vh_add_pe(const float* x, const float* pe, float* out, int B, int T, int d, int pos0, void* stream) {
    VH_REQUIRE(x && pe && out, VH_EINVAL, "vh_add_pe: null pointer");
    VH_REQUIRE(B >= 0 && T >= 0 && d > 0 && d % 4 == 0 && pos0 >= 0, VH_EINVAL, "vh_add_pe: bad dims B=%d T=%d d=%d pos0=%d", B, T,
               d, pos0);
    VH_REQUIRE(vh_aligned16(x) && vh_aligned16(pe) && vh_aligned16(out), VH_EALIGN, "vh_add_pe: pointers must be 16-byte aligned");
    const int64_t n4 = (int64_t)B * T * (d / 4);
    if (n4 == 0) return VH_OK;
    hipLaunchKernelGGL(add_pe_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, pe, out, n4, T,
                       d / 4, pos0);
    VH_CHECK_LAUNCH("vh_add_pe");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// Free-standing dropout (a module-level nn.Dropout outside the fused training step) and the field itself.
// One float4 per thread and Philox call; rows x cols/4 work items.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out,
                                                      int ldo, uint8_t* __restrict__ keep, int64_t rows, int c4n,
                                                      DropArgs drop) {
    const int64_t n = rows * c4n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / c4n;
        const int c4 = (int)(i - r * c4n);
        const f32x4 m = vh_dropmul4(drop, (uint32_t)r, (uint32_t)c4);
        if (keep) {
            *reinterpret_cast<uint32_t*>(keep + i * 4) = (m.x != 0.f ? 1u : 0u) | (m.y != 0.f ? 0x100u : 0u) |
                                                         (m.z != 0.f ? 0x10000u : 0u) | (m.w != 0.f ? 0x1000000u : 0u);
        } else {
            st4(out + r * ldo + 4 * c4, ld4(x + r * ldx + 4 * c4) * m);
        }
    }
}

extern "C" int vh_dropout(const float* x, int ldx, float* out, int ldo, int64_t rows, int cols,
                          const vh_dropout_spec* spec, void* stream) {
    VH_REQUIRE(x && out && rows >= 0 && rows < (1ll << 32) && cols > 0 && cols % 4 == 0 && ldx >= cols && ldo >= cols &&
                   ldx % 4 == 0 && ldo % 4 == 0,
               VH_EINVAL, "vh_dropout: bad dims rows=%lld cols=%d (cols and strides multiples of 4)", (long long)rows, cols);
    VH_REQUIRE(vh_aligned16(x) && vh_aligned16(out), VH_EALIGN, "vh_dropout: pointers must be 16-byte aligned");
    VH_REQUIRE(VH_DROP_OK(spec), VH_EINVAL, "vh_dropout: p must be in [0, 1)");
    if (rows == 0) return VH_OK;
    DropArgs da;
    hipStream_t st = (hipStream_t)stream;
    if (!vh_drop_args(spec, &da)) {                      // p == 0: the identity
        if (x != out && hipMemcpy2DAsync(out, (size_t)ldo * 4, x, (size_t)ldx * 4, (size_t)cols * 4, (size_t)rows,
                                         hipMemcpyDeviceToDevice, st) != hipSuccess) {
            vh_set_error("vh_dropout: copy failed");
            return VH_ELAUNCH;
        }
        return VH_OK;
    }
    const int64_t n = rows * (cols / 4);
    const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(dropout_kernel, dim3(blocks), dim3(256), 0, st, x, ldx, out, ldo, (uint8_t*)nullptr, rows, cols / 4, da);
    VH_CHECK_LAUNCH("vh_dropout");
    return VH_OK;
}

extern "C" int vh_dropout_mask(uint8_t* keep, int64_t rows, int cols, const vh_dropout_spec* spec, void* stream) {
    VH_REQUIRE(keep && rows >= 0 && rows < (1ll << 32) && cols > 0 && cols % 4 == 0, VH_EINVAL,
               "vh_dropout_mask: bad dims rows=%lld cols=%d", (long long)rows, cols);
    VH_REQUIRE((reinterpret_cast<uintptr_t>(keep) & 3u) == 0, VH_EALIGN, "vh_dropout_mask: keep must be 4-byte aligned");
    VH_REQUIRE(VH_DROP_OK(spec), VH_EINVAL, "vh_dropout_mask: p must be in [0, 1)");
    if (rows == 0) return VH_OK;
    DropArgs da;
    hipStream_t st = (hipStream_t)stream;
    if (!vh_drop_args(spec, &da)) {
        if (hipMemsetAsync(keep, 1, (size_t)rows * cols, st) != hipSuccess) {
            vh_set_error("vh_dropout_mask: memset failed");
            return VH_ELAUNCH;
        }
        return VH_OK;
    }
    const int64_t n = rows * (cols / 4);
    const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(dropout_kernel, dim3(blocks), dim3(256), 0, st, (const float*)nullptr, 0, (float*)nullptr, 0, keep,
                       rows, cols / 4, da);
    VH_CHECK_LAUNCH("vh_dropout_mask");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// K3/K4  LayerNorm (two-pass in registers: mean, then sum of squared deviations) + AdaLN affine
// NV = float4 chunks per lane (d <= 256*NV).  grid: ceil(rows/4), block 256.
// ---------------------------------------------------------------------------------------------
template <int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(
    const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ ada_scale, const float* __restrict__ ada_shift,
    float* __restrict__ out, int rows, int d, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (int64_t)row * d;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        v[i] = c < d ? ld4(xr + c) : f32x4{0.f, 0.f, 0.f, 0.f};
        s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) / (float)d;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < d) {
            f32x4 t = v[i] - mean;
            ss += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
        }
    }
    const float rstd = rsqrtf(wave_sum(ss) / (float)d + eps);
    float* orow = out + (int64_t)row * d;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < d) {
            f32x4 y = (v[i] - mean) * rstd * ld4(gamma + c) + ld4(beta + c);
            if (ada_scale) y = ld4(ada_scale + c) * y + ld4(ada_shift + c);
            st4(orow + c, y);
        }
    }
}

extern "C" int vh_layernorm(const float* x, const float* gamma, const float* beta,
                            const float* ada_scale, const float* ada_shift, float* out, int rows,
                            int d, float eps, void* stream) {
    VH_REQUIRE(x && gamma && beta && out, VH_EINVAL, "vh_layernorm: null pointer");
    VH_REQUIRE((ada_scale == nullptr) == (ada_shift == nullptr), VH_EINVAL,
               "vh_layernorm: ada_scale and ada_shift must be given together");
    VH_REQUIRE(rows >= 0 && d > 0 && d % 4 == 0 && d <= 4096, VH_EINVAL,
               "vh_layernorm: bad dims rows=%d d=%d (d multiple of 4, <= 4096)", rows, d);
    VH_REQUIRE(vh_aligned16(x) && vh_aligned16(out) && vh_aligned16(gamma) && vh_aligned16(beta) &&
                   vh_aligned16(ada_scale) && vh_aligned16(ada_shift),
               VH_EALIGN, "vh_layernorm: pointers must be 16-byte aligned");
    if (rows == 0) return VH_OK;
    dim3 grid((rows + 3) / 4), block(256);
    hipStream_t s = (hipStream_t)stream;
#define LN_LAUNCH(NV)                                                                            \
    hipLaunchKernelGGL(layernorm_kernel<NV>, grid, block, 0, s, x, gamma, beta, ada_scale,       \
                       ada_shift, out, rows, d, eps)
    if (d <= 256) LN_LAUNCH(1);
    else if (d <= 512) LN_LAUNCH(2);
    else if (d <= 1024) LN_LAUNCH(4);
    else if (d <= 2048) LN_LAUNCH(8);
    else LN_LAUNCH(16);
#undef LN_LAUNCH
    VH_CHECK_LAUNCH("vh_layernorm");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// K12/K13  greedy step: argmax (lowest index on ties, as torch.topk / multinomial over a one-hot),
// EOS bookkeeping, token append, next-token embedding + position.  One 256-thread block per row.
// The step index is derived from the row's own audio position, so the kernel carries no global
// counter and a captured graph can be replayed as is.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void greedy_step_kernel(
    const float* __restrict__ logits, int ldl, int V, int eos, int64_t* __restrict__ codes,
    int64_t codes_stride, int32_t* __restrict__ eos_count, const int32_t* __restrict__ pos_base,
    const float* __restrict__ audio_emb, const float* __restrict__ pe,
    int32_t* __restrict__ audio_pos, int32_t* __restrict__ cache_len, float* __restrict__ x_next, int d) {
    __shared__ float s_val[4];
    __shared__ int s_idx[4];
    __shared__ int s_tok;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* lr = logits + (int64_t)b * ldl;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = tid; i < V; i += 256) {
        const float v = lr[i];
        if (v > best || (v == best && i < bi)) { best = v; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if (lane == 0) { s_val[w] = best; s_idx[w] = bi; }
    __syncthreads();
    const int pos = audio_pos[b];  // index of the token being produced in row b's audio stream
    if (tid == 0) {
        for (int k = 1; k < 4; ++k)
            if (s_val[k] > best || (s_val[k] == best && s_idx[k] < bi)) { best = s_val[k]; bi = s_idx[k]; }
        int64_t* row = codes + (int64_t)b * codes_stride;
        int tok = bi;
        if (row[pos - 1] == (int64_t)eos) tok = eos;  // valle_ar.py:168: finished rows keep EOS
        row[pos] = tok;                               // valle_ar.py:171
        if (tok == eos) atomicAdd(&eos_count[pos - (pos_base ? pos_base[b] : 0)], 1);
        s_tok = tok;
    }
    __syncthreads();
    const int tok = s_tok;
    const float* er = audio_emb + (int64_t)tok * d;   // valle_ar.py:143-144 for the next step,
    const float* pr = pe + (int64_t)pos * d;          // only the new row (modules.py:337 keeps it)
    for (int c = tid * 4; c < d; c += 1024) {
        const f32x4 e = ld4(er + c) + ld4(pr + c);
        st4(x_next + (int64_t)b * d + c, e);
    }
    if (tid == 0) {
        audio_pos[b] = pos + 1;
        cache_len[b] += 1;
    }
}

extern "C" int vh_greedy_step(const float* logits, int ldl, int V, int eos, int64_t* codes,
                              int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base,
                              const float* audio_emb, const float* pe, int32_t* audio_pos,
                              int32_t* cache_len, float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(logits && codes && eos_count && audio_emb && pe && audio_pos && cache_len && x_next,
               VH_EINVAL, "vh_greedy_step: null pointer");
    VH_REQUIRE(B > 0 && V > 0 && ldl >= V && d > 0 && d % 4 == 0, VH_EINVAL,
               "vh_greedy_step: bad dims B=%d V=%d ldl=%d d=%d", B, V, ldl, d);
    VH_REQUIRE(vh_aligned16(audio_emb) && vh_aligned16(pe) && vh_aligned16(x_next), VH_EALIGN,
               "vh_greedy_step: audio_emb/pe/x_next must be 16-byte aligned");
    hipLaunchKernelGGL(greedy_step_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl,
                       V, eos, codes, codes_stride, eos_count, pos_base, audio_emb, pe, audio_pos,
                       cache_len, x_next, d);
    VH_CHECK_LAUNCH("vh_greedy_step");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// K12 (stochastic)  top-k / top-p / temperature sampling (valle/models/utils.py:46-68 with the
// published transformers==4.38.2 top_k_top_p_filtering semantics), fused with the same decode-state
// update as greedy_step_kernel.  One 256-thread block per row:
//   1. scores = logits / temperature into LDS (padded to a power of two with -inf), bitonic sort
//      descending (ties: lower index first);
//   2. top-k: keep every score >= the k-th largest (ties kept; top_k <= 0 keeps all);
//   3. top-p: walking from the smallest kept score, drop entries whose cumulative probability is
//      <= 1 - top_p, always keeping the largest one;
//   4. draw from the renormalised kept set with a counter-based RNG keyed on (seed, row, position)
//      — a captured graph replays with fresh randomness because the position advances;
//   5. logprob = log p(token) under the filtered distribution; sum_logprobs[b] += logprob while the
//      row has not finished (valle_ar.py:167);
//   6. per-row records only (rs != NULL) and only where the record asks for it: the repetition-aware redraw of a token
//      that fills too much of the row's last tokens (ROW_SAMPLING_LOAD below).
// The RNG stream differs from torch.multinomial's (CPU mt19937 / Philox): parity with the reference
// is distributional, not sample-exact (SURVEY.md §8c "parity unpinned" for top_k > 1).
// ---------------------------------------------------------------------------------------------
#define SAMPLE_MAXV 2048

__device__ __forceinline__ float uniform01(uint64_t seed, uint32_t row, uint32_t pos) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (((uint64_t)row << 32) | (uint64_t)(pos + 1u));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;     // splitmix64 finaliser
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);   // 24 random bits → [0, 1)
}

// order-preserving key of a float: a > b  <=>  okey(a) > okey(b)  (-inf lowest; no NaNs expected)
__device__ __forceinline__ uint32_t okey(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Per-row sampling (rs != NULL): the block of row b takes its seed, the `row` key of its draws and its filter from rs[b]
// (block-uniform: one block serves one row); the scalar seed and *seed_dev are not added.  1 / temperature is the host's
// fp32 division, so a record holding the call's values filters as the call does.  top_k == 1 is the arg-max with the lowest
// index on ties and a log-probability of exactly 0 (greedy_step_kernel's token): the scores stay unscaled (a scale could
// merge neighbouring logits into a tie), zeros of either sign become +0.0 (greedy_step_kernel compares values, for which
// -0.0 == +0.0; the radix keys would order them), top_p is off and only the first survivor in index order is kept.
//
// Repetition-aware sampling (reserved[0] = window K, reserved[1] = max_repeats R; K == 0: off, nothing below runs).  Once the
// filtered draw c is known, a row that has not finished counts c among its own codes[max(1, pos - K) .. pos - 1] (the prompt
// counts, BOS at 0 never does); more than R of them and the token is drawn again from softmax(logits / temperature) over all
// V entries in index order, with u2 = uniform01(seed, key, pos | RAS_STREAM), and the row's score takes the log-probability
// under that unfiltered distribution.  Everything the branch tests is block-uniform (one block, one row); top_k == 1 never
// takes it.
#define RAS_STREAM 0x40000000u    // bit 30: apart from every first draw (pos < 2^30) and from the NAR stage's streams (bit 31)
#define ROW_SAMPLING_LOAD(rec)                                            \
    do {                                                                  \
        const vh_row_sampling r_ = (rec);                                 \
        seed = r_.seed;                                                   \
        draw_key = r_.key;                                                \
        top_k = r_.top_k;                                                 \
        top_p = r_.top_p;                                                 \
        inv_temp = 1.0f / r_.temperature;                                 \
        ras_window = r_.reserved[0];                                      \
        ras_max = r_.reserved[1];                                         \
        greedy = top_k == 1;                                              \
        if (greedy) { top_p = 1.0f; inv_temp = 1.0f; }                    \
    } while (0)

// Per-row length bounds (limits != NULL, which the entry points allow only with rs and pos_base): the block of row b loads
// limits[b] once (block-uniform, 8 bytes) and, only where a word is set and the row has not finished, the two values that
// place the row: n = pos - pos_base[b] tokens produced so far.  force_eos (max_new > 0 and n >= max_new): the token is EOS
// with no draw, no repetition-aware count and no redraw, and the score does not move.  suppress_eos (otherwise, n <
// min_new): the EOS score is -inf wherever scores enter LDS, so top-k, top-p, the arg-max, the draw and the redraw run over
// the distribution without it.  An all-zero record sets neither.
#define ROW_LIMITS_LOAD(lim, hist_last)                                   \
    do {                                                                  \
        const vh_row_limits l_ = (lim);                                   \
        if ((l_.min_new | l_.max_new) != 0 && (hist_last) != (int64_t)eos) { \
            const int n_ = pos - pos_base[blockIdx.x];                    \
            force_eos = l_.max_new > 0 && n_ >= l_.max_new;               \
            suppress_eos = !force_eos && n_ < l_.min_new;                 \
        }                                                                 \
    } while (0)
// what a launch with limits needs (host side, before the launch): the records they sit beside, the base n is counted
// from, a vocabulary that holds a token besides EOS, and the alignment of the one 8-byte load
#define CHECK_ROW_LIMITS(name)                                                                                              \
    do {                                                                                                                    \
        VH_REQUIRE(!limits || rs, VH_EINVAL, name ": limits without rs (the length bounds sit beside per-row sampling records)"); \
        VH_REQUIRE(!limits || pos_base, VH_EINVAL, name ": limits need pos_base (a row's tokens are counted from it)");      \
        VH_REQUIRE(!limits || (V >= 2 && eos >= 0 && eos < V), VH_EINVAL,                                                   \
                   name ": limits need V >= 2 and 0 <= eos < V (a token besides EOS to draw below min_new), got V=%d eos=%d", V, eos); \
        VH_REQUIRE(((uintptr_t)limits & 7u) == 0, VH_EALIGN, name ": limits (vh_row_limits records) must be 8-byte aligned"); \
    } while (0)

// scan over a block of NW waves in thread order (the wide kernel's 16, the narrow kernel's 4 for its redraw): *excl / return
// value = the exclusive / inclusive prefix of v, *total = the sum over the block.  The values are consistent: a thread's
// excl is bit-equal to the previous thread's incl, the last thread's incl to *total.  s_w holds NW entries and may be
// reused once this returns.
template <int NW, typename T>
__device__ __forceinline__ T wide_block_scan(T v, T* s_w, T* excl, T* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    T prev = __shfl_up(incl, 1, 64);
    if (lane == 0) prev = 0;
    if (lane == 63) s_w[wv] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w == wv) before = all;
        all += s_w[w];
    }
    __syncthreads();
    *excl = before + prev;
    *total = all;
    return before + incl;
}

// inverse CDF over the weights exp(s_val[j] - m), j < n, in array order, by a block of NW waves: s_out[0] = the first j
// whose inclusive sum exceeds u01 * total (the last entry when rounding leaves none), s_tot[0] = total.  Ends with a barrier.
template <int NW>
__device__ __forceinline__ void wide_draw(const float* s_val, int n, float m, float u01, float* s_w, int* s_out,
                                          float* s_tot) {
    const int tid = threadIdx.x;
    const int per = (n + NW * 64 - 1) / (NW * 64);
    const int j0 = min(n, tid * per), j1 = min(n, j0 + per);
    float s = 0.f;
    for (int j = j0; j < j1; ++j) s += expf(s_val[j] - m);
    if (tid == 0) s_out[0] = n - 1;
    float excl, total;
    const float incl = wide_block_scan<NW>(s, s_w, &excl, &total);
    const float u = u01 * total;
    if (j1 > j0 && excl <= u && incl > u) {     // the intervals [excl, incl) tile [0, total): one owner at most
        float acc = excl;
        int pick = j1 - 1;
        for (int j = j0; j < j1; ++j) {
            acc += expf(s_val[j] - m);
            if (acc > u) { pick = j; break; }
        }
        s_out[0] = pick;
    }
    if (tid == 0) s_tot[0] = total;
    __syncthreads();
}

// how many of row[lo .. hi) equal tok, known to every thread of the NW-wave block; s_w holds NW entries and may be reused
// once this returns.  It holds two barriers: what any thread read from shared memory before the call has been read by the
// time another thread returns, so the caller may overwrite it.
template <int NW>
__device__ __forceinline__ int block_count_eq(const int64_t* row, int lo, int hi, int tok, int* s_w) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int c = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += NW * 64) c += row[i] == (int64_t)tok;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) s_w[wv] = c;
    __syncthreads();
    int n = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) n += s_w[w];
    __syncthreads();
    return n;
}

// BOUNDED: the instantiation that reads `limits` (launched only with limits != NULL).  Without it suppress_eos and force_eos
// are constants and the kernel is the one it was: a launch without limits pays nothing for them (one kernel with a run-time
// test of the pointer was measured once and not kept: its NULL launch cost 0.23 us more than the parent's at V = 1025,
// profiles/ab_length_bounds_untemplated.log).
template <bool BOUNDED>
__global__ __launch_bounds__(256) void sample_step_kernel(
    const float* __restrict__ logits, int ldl, int V, int eos, int top_k, float top_p, float inv_temp,
    uint64_t seed, int64_t* __restrict__ codes, int64_t codes_stride, int32_t* __restrict__ eos_count,
    const int32_t* __restrict__ pos_base, float* __restrict__ sum_logprobs,
    const float* __restrict__ audio_emb, const float* __restrict__ pe, int32_t* __restrict__ audio_pos,
    int32_t* __restrict__ cache_len, float* __restrict__ x_next, int d, int npow2, const uint64_t* __restrict__ seed_dev,
    const vh_row_sampling* __restrict__ rs, const vh_row_limits* __restrict__ limits) {
    uint32_t draw_key = blockIdx.x;   // the `row` of uniform01: the launch's row index, or the request's own key
    uint32_t ras_window = 0, ras_max = 0;
    bool greedy = false, suppress_eos = false, force_eos = false;
    if (rs) {
        ROW_SAMPLING_LOAD(rs[blockIdx.x]);
    } else if (seed_dev) {
        // a captured graph freezes `seed`; a decoder that outlives one generate() keeps the call's seed in device memory instead
        seed += *seed_dev;
    }
    __shared__ float s_val[SAMPLE_MAXV];
    __shared__ int s_idx[SAMPLE_MAXV];
    __shared__ int s_hist[256];
    __shared__ int s_sel[4];          // [0] chosen bin, [1] rank still wanted inside it, [2] survivors, [3] scratch
    __shared__ float s_red[8];
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* lr = logits + (int64_t)b * ldl;
    const int pos = audio_pos[b];
    int pick_tok = eos;               // (what a forced row writes)
    float pick_logprob = 0.f;
    if (BOUNDED) ROW_LIMITS_LOAD(limits[b], codes[(int64_t)b * codes_stride + pos - 1]);

    // ---- fast path: top-k only (top_p == 1, the reference's default top_k = 50, tok_p = 1.0) ---------------
    // No sort: the k-th largest score is found by a 4 x 8-bit radix select on order-preserving keys,
    // the survivors (>= k-th, ties kept) are compacted in index order and the draw walks their
    // cumulative probabilities.  (The sorted path below costs 66 barrier-separated bitonic stages and
    // serial exp loops on one thread: 89 us per launch against the 5 us of a greedy step.)
    // (a suppressed EOS is -inf and top_k < V, so it never survives the select: the walk's fallback cannot return it)
    const bool fast = top_k > 0 && top_k < V && top_p == 1.0f;
    if (force_eos) {
        // nothing is drawn
    } else if (fast) {
        float vmax = -INFINITY;
        for (int i = tid; i < V; i += 256) {
            float x = lr[i] * inv_temp;
            if (greedy) x += 0.0f;                      // -0.0 -> +0.0: the keys then order the scores as a float compare does
            if (suppress_eos && i == eos) x = -INFINITY;
            s_val[i] = x;
            vmax = fmaxf(vmax, x);
        }
        vmax = wave_max(vmax);
        if (lane == 0) s_red[wv] = vmax;
        uint32_t prefix = 0, mask = 0;
        int want = top_k;                               // rank (from the top) of the k-th value among candidates
        for (int shift = 24; shift >= 0; shift -= 8) {
            s_hist[tid] = 0;
            __syncthreads();
            for (int i = tid; i < V; i += 256) {
                const uint32_t key = okey(s_val[i]);
                if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
            }
            __syncthreads();
            if (wv == 0) {                              // lane l owns bins 255-4l .. 252-4l (descending)
                int c[4], tot = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = s_hist[255 - 4 * lane - j]; tot += c[j]; }
                int incl = tot;                          // inclusive prefix over lanes 0..lane
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += up;
                }
                const int before = incl - tot;           // candidates in higher bins than this lane's
                if (before < want && incl >= want) {     // exactly one lane
                    int acc = before;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (acc < want && acc + c[j] >= want) { s_sel[0] = 255 - 4 * lane - j; s_sel[1] = want - acc; }
                        acc += c[j];
                    }
                }
            }
            __syncthreads();
            prefix |= (uint32_t)s_sel[0] << shift;
            mask |= 255u << shift;
            want = s_sel[1];
        }
        // prefix == key of the k-th largest score.  Survivors: key >= prefix, kept in index order.
        const float m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        int mine = 0;                                    // each thread owns a contiguous index range
        const int per = (V + 255) / 256, i0 = tid * per, i1 = min(V, i0 + per);
        for (int i = i0; i < i1; ++i) mine += okey(s_val[i]) >= prefix;
        int incl = mine;                                 // block-wide exclusive prefix of `mine`
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_hist[wv] = incl;
        __syncthreads();
        int base = incl - mine;
        for (int ww = 0; ww < wv; ++ww) base += s_hist[ww];
        const int n_keep = greedy ? 1 : s_hist[0] + s_hist[1] + s_hist[2] + s_hist[3];   // (greedy: the lowest index of the ties)
        __syncthreads();                                 // s_hist / s_val are re-used below
        // compact (value, index); the survivor count is small (top_k plus ties) but may be anything <= V
        float kv[8];
        int ki[8], nk = 0;
        for (int i = i0; i < i1; ++i)
            if (okey(s_val[i]) >= prefix) { kv[nk & 7] = s_val[i]; ki[nk & 7] = i; ++nk; }   // per <= 8 (V <= 2048)
        __syncthreads();
        for (int j = 0; j < nk; ++j) { s_val[base + j] = kv[j]; s_idx[base + j] = ki[j]; }
        __syncthreads();
        if (wv == 0) {
            // total = sum of exp(v - m) over the survivors, 64 at a time
            float total = 0.f;
            for (int j0 = 0; j0 < n_keep; j0 += 64) total += (j0 + lane < n_keep) ? expf(s_val[j0 + lane] - m) : 0.f;
            total = wave_sum(total);
            const float u = uniform01(seed, draw_key, (uint32_t)pos) * total;
            float run = 0.f;
            int pick = n_keep - 1;
            bool found = false;
            for (int j0 = 0; j0 < n_keep && !found; j0 += 64) {
                const float e = (j0 + lane < n_keep) ? expf(s_val[j0 + lane] - m) : 0.f;
                float inc = e;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const float up = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += up;
                }
                const unsigned long long hit = __ballot(j0 + lane < n_keep && run + inc > u);
                if (hit) { pick = j0 + __ffsll((long long)hit) - 1; found = true; }
                run += __shfl(inc, 63, 64);
            }
            if (lane == 0) {
                s_sel[2] = s_idx[pick];
                s_red[4] = (s_val[pick] - m) - logf(total);
            }
        }
        __syncthreads();
        pick_tok = s_sel[2];
        pick_logprob = s_red[4];
    } else {
        // ---- general path: full descending sort, then top-k / top-p on the sorted scores -------------------
        for (int i = tid; i < npow2; i += 256) {
            s_val[i] = i < V && !(suppress_eos && i == eos) ? lr[i] * inv_temp : -INFINITY;
            s_idx[i] = i;
        }
        __syncthreads();
        for (int k = 2; k <= npow2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < npow2; i += 256) {
                    const int p = i ^ j;
                    if (p > i) {
                        const bool desc = (i & k) == 0;
                        const float a = s_val[i], c = s_val[p];
                        const int ia = s_idx[i], ic = s_idx[p];
                        const bool a_first = a > c || (a == c && ia < ic);   // a belongs before c
                        if (desc ? !a_first : a_first) {
                            s_val[i] = c; s_val[p] = a; s_idx[i] = ic; s_idx[p] = ia;
                        }
                    }
                }
                __syncthreads();
            }
        if (tid == 0) {
            int n_keep = V;
            if (top_k > 0) {
                const float kth = s_val[min(top_k, V) - 1];
                n_keep = min(top_k, V);
                while (n_keep < V && s_val[n_keep] >= kth) ++n_keep;         // ties kept
                if (greedy) n_keep = 1;                                      // (V == 1: the only row top_k == 1 brings here)
            }
            // a suppressed EOS sorts to the tail as -inf (top_k <= 0 or >= V keeps it in the array): out of the kept set,
            // so that neither the top-p walk nor the draw's last-entry fallback can return it
            while (suppress_eos && n_keep > 1 && s_val[n_keep - 1] == -INFINITY) --n_keep;
            const float m = s_val[0];
            float total = 0.f;
            for (int i = 0; i < n_keep; ++i) total += expf(s_val[i] - m);
            if (top_p >= 0.f && top_p <= 1.f) {                              // drop the low-probability tail
                const float limit = (1.0f - top_p) * total;
                float tail = 0.f;
                int n2 = n_keep;
                while (n2 > 1) {
                    tail += expf(s_val[n2 - 1] - m);
                    if (tail > limit) break;
                    --n2;
                }
                n_keep = n2;
                total = 0.f;
                for (int i = 0; i < n_keep; ++i) total += expf(s_val[i] - m);
            }
            const float u = uniform01(seed, draw_key, (uint32_t)pos) * total;
            float acc = 0.f;
            int pick = n_keep - 1;
            for (int i = 0; i < n_keep; ++i) {
                acc += expf(s_val[i] - m);
                if (acc > u) { pick = i; break; }
            }
            s_sel[2] = s_idx[pick];
            s_red[4] = (s_val[pick] - m) - logf(total);
        }
        __syncthreads();
        pick_tok = s_sel[2];
        pick_logprob = s_red[4];
    }
    if (greedy) pick_logprob = 0.f;
    const int64_t* hist = codes + (int64_t)b * codes_stride;
    if (ras_window != 0 && !greedy && !force_eos && hist[pos - 1] != (int64_t)eos) {
        const int lo = (int)max((int64_t)1, (int64_t)pos - (int64_t)ras_window);
        if ((uint32_t)block_count_eq<4>(hist, lo, pos, pick_tok, s_hist) > ras_max) {
            // the redraw: every scaled logit back into s_val in index order, their maximum, the block-parallel draw
            float vmax = -INFINITY;
            for (int i = tid; i < V; i += 256) {
                float x = lr[i] * inv_temp;
                if (suppress_eos && i == eos) x = -INFINITY;
                s_val[i] = x;
                vmax = fmaxf(vmax, x);
            }
            vmax = wave_max(vmax);
            if (lane == 0) s_red[4 + wv] = vmax;
            __syncthreads();
            const float m = fmaxf(fmaxf(s_red[4], s_red[5]), fmaxf(s_red[6], s_red[7]));
            wide_draw<4>(s_val, V, m, uniform01(seed, draw_key, (uint32_t)pos | RAS_STREAM), s_red, &s_sel[2], &s_red[4]);
            pick_tok = s_sel[2];
            // (the walk's last entry when rounding leaves none may be the suppressed EOS: its neighbour then; V >= 2.  Only a
            // row whose neighbour's logit is -inf as well could take a log-probability of -inf here: pathological logits)
            if (suppress_eos && pick_tok == eos) pick_tok = eos > 0 ? eos - 1 : 1;
            pick_logprob = (s_val[pick_tok] - m) - logf(s_red[4]);
        }
    }
    if (tid == 0) {
        int64_t* row = codes + (int64_t)b * codes_stride;
        int tok = pick_tok;
        const bool finished = row[pos - 1] == (int64_t)eos;
        if (sum_logprobs && !finished && !force_eos) sum_logprobs[b] += pick_logprob;   // valle_ar.py:167 (a forced EOS is not the model's choice)
        if (finished) tok = eos;                                             // valle_ar.py:168
        row[pos] = tok;
        if (tok == eos) atomicAdd(&eos_count[pos - (pos_base ? pos_base[b] : 0)], 1);
        s_tok = tok;
    }
    __syncthreads();
    const int tok = s_tok;
    const float* er = audio_emb + (int64_t)tok * d;
    const float* pr = pe + (int64_t)pos * d;
    for (int c = tid * 4; c < d; c += 1024) {
        const f32x4 e = ld4(er + c) + ld4(pr + c);
        st4(x_next + (int64_t)b * d + c, e);
    }
    if (tid == 0) {
        audio_pos[b] = pos + 1;
        cache_len[b] += 1;
    }
}

// vh_sample_step with the seed = seed + *seed_dev (seed_dev may be NULL), or with per-row records (rs != NULL: top_k, top_p,
// temperature, seed and seed_dev are not read; limits: the rows' length bounds beside them, or NULL): the decoder plan's form
// (plan.hip)
int vh_internal_sample_step(const float* logits, int ldl, int V, int eos, int top_k, float top_p,
                            float temperature, uint64_t seed, const uint64_t* seed_dev, const vh_row_sampling* rs,
                            const vh_row_limits* limits, int64_t* codes, int64_t codes_stride,
                            int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                            const float* audio_emb, const float* pe, int32_t* audio_pos,
                            int32_t* cache_len, float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(logits && codes && eos_count && audio_emb && pe && audio_pos && cache_len && x_next,
               VH_EINVAL, "vh_sample_step: null pointer");
    VH_REQUIRE(B > 0 && V > 0 && V <= SAMPLE_MAXV && ldl >= V && d > 0 && d % 4 == 0, VH_EINVAL,
               "vh_sample_step: bad dims B=%d V=%d (<= %d) ldl=%d d=%d", B, V, SAMPLE_MAXV, ldl, d);
    VH_REQUIRE(rs || temperature > 0.f, VH_EINVAL, "vh_sample_step: temperature must be positive");
    VH_REQUIRE(vh_aligned16(rs), VH_EALIGN, "vh_sample_step: the per-row sampling records must be 16-byte aligned");
    CHECK_ROW_LIMITS("vh_sample_step");
    VH_REQUIRE(vh_aligned16(audio_emb) && vh_aligned16(pe) && vh_aligned16(x_next), VH_EALIGN,
               "vh_sample_step: audio_emb/pe/x_next must be 16-byte aligned");
    int npow2 = 2;
    while (npow2 < V) npow2 <<= 1;
    const auto kernel = limits ? sample_step_kernel<true> : sample_step_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, logits, ldl, V,
                       eos, top_k, top_p, rs ? 1.0f : 1.0f / temperature, seed, codes, codes_stride, eos_count,
                       pos_base, sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, d, npow2, seed_dev, rs, limits);
    VH_CHECK_LAUNCH("vh_sample_step");
    return VH_OK;
}

extern "C" int vh_sample_step(const float* logits, int ldl, int V, int eos, int top_k, float top_p,
                              float temperature, uint64_t seed, int64_t* codes, int64_t codes_stride,
                              int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                              const float* audio_emb, const float* pe, int32_t* audio_pos,
                              int32_t* cache_len, float* x_next, int B, int d, void* stream) {
    return vh_internal_sample_step(logits, ldl, V, eos, top_k, top_p, temperature, seed, nullptr, nullptr, nullptr, codes, codes_stride,
                                   eos_count, pos_base, sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, B, d, stream);
}

extern "C" int vh_sample_step_rows(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs, int64_t* codes,
                                  int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                                  const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                                  float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(rs, VH_EINVAL, "vh_sample_step_rows: null sampling records (vh_sample_step takes one filter for every row)");
    return vh_internal_sample_step(logits, ldl, V, eos, 0, 1.f, 1.f, 0, nullptr, rs, nullptr, codes, codes_stride, eos_count, pos_base,
                                  sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, B, d, stream);
}

extern "C" int vh_sample_step_rows_bounded(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs,
                                          const vh_row_limits* limits, int64_t* codes, int64_t codes_stride, int32_t* eos_count,
                                          const int32_t* pos_base, float* sum_logprobs, const float* audio_emb, const float* pe,
                                          int32_t* audio_pos, int32_t* cache_len, float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(rs, VH_EINVAL, "vh_sample_step_rows_bounded: null sampling records (vh_sample_step takes one filter for every row)");
    return vh_internal_sample_step(logits, ldl, V, eos, 0, 1.f, 1.f, 0, nullptr, rs, limits, codes, codes_stride, eos_count, pos_base,
                                  sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, B, d, stream);
}

// ---------------------------------------------------------------------------------------------
// K12 (stochastic, wide vocabularies)  vh_sample_step's semantics for 1 <= V <= VH_SAMPLE_MAX_V (16384).
// One 1024-thread workgroup per row; the scores and their indices live in LDS (2 x 64 KiB at V = 16384; rows are far
// fewer than CUs, so one workgroup per CU costs nothing):
//   1. scores = logits / temperature into LDS, row maximum m;
//   2. 0 < top_k < V: the key of the k-th largest score by the narrow kernel's 4 x 8-bit radix select;
//   3. the survivors (score >= the k-th, ties kept; everything when top_k <= 0 or top_k >= V) are compacted in index
//      order: every wave owns 64 x ceil(V / 1024) consecutive indices, a ballot per 64 of them and a scan over the 16
//      wave counts give each survivor its slot — no per-thread cap;
//   fast path (0 < top_k < V, top_p == 1): the draw walks the survivors in index order, as the narrow kernel's does;
//   general path: bitonic sort of the survivors only, descending (ties: lower index first), then the top-p cut
//      (suffix sums from the smallest, block-parallel) and the draw over the kept prefix of the sorted order.
//   4. the draw: each thread sums exp(score - m) over a contiguous run, a block scan turns the run sums into CDF
//      intervals, and the one thread whose interval holds u = uniform01(seed, row, audio_pos[b]) * total walks its
//      run (the narrow kernel's general path does this on one thread over V entries).
// No per-row state outlives the launch, so a captured graph replays as the narrow kernel's does.
// ---------------------------------------------------------------------------------------------
#define WIDE_THREADS 1024
#define WIDE_WAVES (WIDE_THREADS / 64)
#define WIDE_PER (VH_SAMPLE_MAX_V / WIDE_THREADS)   // indices per lane and 64-wide round of the compaction, at most

template <bool BOUNDED>     // as sample_step_kernel's
__global__ __launch_bounds__(WIDE_THREADS) void sample_step_wide_kernel(
    const float* __restrict__ logits, int ldl, int V, int eos, int top_k, float top_p, float inv_temp,
    uint64_t seed, int64_t* __restrict__ codes, int64_t codes_stride, int32_t* __restrict__ eos_count,
    const int32_t* __restrict__ pos_base, float* __restrict__ sum_logprobs,
    const float* __restrict__ audio_emb, const float* __restrict__ pe, int32_t* __restrict__ audio_pos,
    int32_t* __restrict__ cache_len, float* __restrict__ x_next, int d, const uint64_t* __restrict__ seed_dev,
    const vh_row_sampling* __restrict__ rs, const vh_row_limits* __restrict__ limits) {
    uint32_t draw_key = blockIdx.x;
    uint32_t ras_window = 0, ras_max = 0;
    bool greedy = false, suppress_eos = false, force_eos = false;
    if (rs) {
        ROW_SAMPLING_LOAD(rs[blockIdx.x]);
    } else if (seed_dev) {
        seed += *seed_dev;
    }
    __shared__ float s_val[VH_SAMPLE_MAX_V];
    __shared__ int s_idx[VH_SAMPLE_MAX_V];
    __shared__ int s_hist[256];
    __shared__ float s_wf[WIDE_WAVES];
    __shared__ int s_wi[WIDE_WAVES];
    __shared__ float s_max[WIDE_WAVES];
    __shared__ int s_sel[3];          // [0] chosen bin, [1] rank still wanted inside it, [2] pick (slot)
    __shared__ float s_tot;
    __shared__ int s_tok;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* lr = logits + (int64_t)b * ldl;
    const int pos = audio_pos[b];
    if (BOUNDED) ROW_LIMITS_LOAD(limits[b], codes[(int64_t)b * codes_stride + pos - 1]);
    float m = 0.f;
    int pick_tok = eos;               // (what a forced row writes: nothing below runs for it)
    float pick_logprob = 0.f;

    if (!force_eos) {
        // 1. scores and their maximum (a suppressed EOS enters as -inf: outside the maximum, the select and the survivors)
        float vmax = -INFINITY;
        for (int i = tid; i < V; i += WIDE_THREADS) {
            float x = lr[i] * inv_temp;
            if (greedy) x += 0.0f;                          // -0.0 -> +0.0, as in the narrow kernel
            if (suppress_eos && i == eos) x = -INFINITY;
            s_val[i] = x;
            vmax = fmaxf(vmax, x);
        }
        vmax = wave_max(vmax);
        if (lane == 0) s_max[wv] = vmax;
        __syncthreads();
        m = s_max[0];
#pragma unroll
        for (int w = 1; w < WIDE_WAVES; ++w) m = fmaxf(m, s_max[w]);

        // 2. key of the k-th largest score (survivors: key >= prefix; prefix 0 keeps every score)
        uint32_t prefix = 0;
        if (top_k > 0 && top_k < V) {
            uint32_t mask = 0;
            int want = top_k;                               // rank (from the top) of the k-th value among candidates
            for (int shift = 24; shift >= 0; shift -= 8) {
                if (tid < 256) s_hist[tid] = 0;
                __syncthreads();
                for (int i = tid; i < V; i += WIDE_THREADS) {
                    const uint32_t key = okey(s_val[i]);
                    if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1);
                }
                __syncthreads();
                if (wv == 0) {                              // lane l owns bins 255-4l .. 252-4l (descending)
                    int c[4], tot = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) { c[j] = s_hist[255 - 4 * lane - j]; tot += c[j]; }
                    int incl = tot;
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int up = __shfl_up(incl, o, 64);
                        if (lane >= o) incl += up;
                    }
                    const int before = incl - tot;
                    if (before < want && incl >= want) {     // exactly one lane
                        int acc = before;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (acc < want && acc + c[j] >= want) { s_sel[0] = 255 - 4 * lane - j; s_sel[1] = want - acc; }
                            acc += c[j];
                        }
                    }
                }
                __syncthreads();
                prefix |= (uint32_t)s_sel[0] << shift;
                mask |= 255u << shift;
                want = s_sel[1];
            }
        }

        // 3. compact the survivors in index order: (score, index) pairs into s_val[0..n) / s_idx[0..n).  A suppressed EOS is
        // never one of them (prefix 0 would keep its -inf): no sort, top-p walk or last-entry fallback below can return it
        const int per = (V + WIDE_THREADS - 1) / WIDE_THREADS;       // 64-wide rounds per wave
        const int w0 = wv * 64 * per;
        float v[WIDE_PER];
        uint32_t keep = 0;
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < WIDE_PER; ++r) {
            const int i = w0 + r * 64 + lane;
            const bool in = r < per && i < V && !(suppress_eos && i == eos);
            v[r] = in ? s_val[i] : 0.f;
            const bool k = in && okey(v[r]) >= prefix;
            keep |= (uint32_t)k << r;
            cnt += __popcll(__ballot(k));
        }
        if (lane == 0) s_wi[wv] = cnt;
        __syncthreads();                                   // every read of s_val above precedes the writes below
        int at = 0, n = 0;
#pragma unroll
        for (int w = 0; w < WIDE_WAVES; ++w) {
            if (w == wv) at = n;
            n += s_wi[w];
        }
        const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
        for (int r = 0; r < WIDE_PER; ++r) {
            const bool k = (keep >> r) & 1u;
            const uint64_t bal = __ballot(k);
            if (k) {
                const int slot = at + __popcll(bal & below);
                s_val[slot] = v[r];
                s_idx[slot] = w0 + r * 64 + lane;
            }
            at += __popcll(bal);
        }
        __syncthreads();
        if (greedy) n = 1;                                 // slot 0: the lowest index of the ties for the maximum
        const float u01 = uniform01(seed, draw_key, (uint32_t)pos);

        if (top_k > 0 && top_k < V && top_p == 1.0f) {
            // fast path: the draw over the survivors in index order
            wide_draw<WIDE_WAVES>(s_val, n, m, u01, s_wf, &s_sel[2], &s_tot);
        } else {
            // general path: sort the survivors descending (ties: lower index first) over the next power of two
            int np2 = 1;
            while (np2 < n) np2 <<= 1;
            for (int i = n + tid; i < np2; i += WIDE_THREADS) { s_val[i] = -INFINITY; s_idx[i] = 0x7fffffff; }
            __syncthreads();
            for (int k = 2; k <= np2; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int q = tid; q < (np2 >> 1); q += WIDE_THREADS) {
                        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), p = i | j;   // the pair (i, i ^ j), i < p
                        const bool desc = (i & k) == 0;
                        const float a = s_val[i], c = s_val[p];
                        const int ia = s_idx[i], ic = s_idx[p];
                        const bool a_first = a > c || (a == c && ia < ic);   // a belongs before c
                        if (desc ? !a_first : a_first) {
                            s_val[i] = c; s_val[p] = a; s_idx[i] = ic; s_idx[p] = ia;
                        }
                    }
                    __syncthreads();
                }
            int n_keep = n;
            if (top_p >= 0.f && top_p <= 1.f) {
                // drop entries from the smallest up while the cumulative probability of the dropped ones is <= 1 - top_p,
                // always keeping the largest: n_keep = 1 + #{j >= 1 : sum_{i >= j} e_i > (1 - top_p) * total}.  Thread t
                // owns the run that ends at n - t * run, so its exclusive prefix is the suffix sum after its run.
                const int run = (n + WIDE_THREADS - 1) / WIDE_THREADS;
                const int j1 = max(0, n - tid * run), j0 = max(0, j1 - run);
                float s = 0.f;
                for (int j = j1 - 1; j >= j0; --j) s += expf(s_val[j] - m);
                float after, total;
                wide_block_scan<WIDE_WAVES>(s, s_wf, &after, &total);
                const float limit = (1.0f - top_p) * total;
                float tail = after;
                int over = 0;
                for (int j = j1 - 1; j >= j0; --j) {
                    tail += expf(s_val[j] - m);
                    over += j >= 1 && tail > limit;
                }
                int ex, n_over;
                wide_block_scan<WIDE_WAVES>(over, s_wi, &ex, &n_over);
                n_keep = 1 + n_over;
            }
            wide_draw<WIDE_WAVES>(s_val, n_keep, m, u01, s_wf, &s_sel[2], &s_tot);
        }
        const int slot = s_sel[2];
        pick_tok = s_idx[slot];
        pick_logprob = greedy ? 0.f : (s_val[slot] - m) - logf(s_tot);
    }
    const int64_t* hist = codes + (int64_t)b * codes_stride;
    if (ras_window != 0 && !greedy && !force_eos && hist[pos - 1] != (int64_t)eos) {
        const int lo = (int)max((int64_t)1, (int64_t)pos - (int64_t)ras_window);
        if ((uint32_t)block_count_eq<WIDE_WAVES>(hist, lo, pos, pick_tok, s_wi) > ras_max) {
            // the redraw: every scaled logit back into s_val in index order (m is their maximum already), then the draw
            for (int i = tid; i < V; i += WIDE_THREADS) s_val[i] = suppress_eos && i == eos ? -INFINITY : lr[i] * inv_temp;
            __syncthreads();
            wide_draw<WIDE_WAVES>(s_val, V, m, uniform01(seed, draw_key, (uint32_t)pos | RAS_STREAM), s_wf, &s_sel[2], &s_tot);
            pick_tok = s_sel[2];
            // (the walk's last entry when rounding leaves none may be the suppressed EOS: its neighbour then; V >= 2.  Only a
            // row whose neighbour's logit is -inf as well could take a log-probability of -inf here: pathological logits)
            if (suppress_eos && pick_tok == eos) pick_tok = eos > 0 ? eos - 1 : 1;
            pick_logprob = (s_val[pick_tok] - m) - logf(s_tot);
        }
    }

    if (tid == 0) {
        int64_t* row = codes + (int64_t)b * codes_stride;
        int tok = pick_tok;
        const bool finished = row[pos - 1] == (int64_t)eos;
        if (sum_logprobs && !finished && !force_eos) sum_logprobs[b] += pick_logprob;   // valle_ar.py:167 (a forced EOS is not the model's choice)
        if (finished) tok = eos;                                             // valle_ar.py:168
        row[pos] = tok;
        if (tok == eos) atomicAdd(&eos_count[pos - (pos_base ? pos_base[b] : 0)], 1);
        s_tok = tok;
    }
    __syncthreads();
    const int tok = s_tok;
    const float* er = audio_emb + (int64_t)tok * d;
    const float* pr = pe + (int64_t)pos * d;
    for (int c = tid * 4; c < d; c += 4 * WIDE_THREADS) {
        const f32x4 e = ld4(er + c) + ld4(pr + c);
        st4(x_next + (int64_t)b * d + c, e);
    }
    if (tid == 0) {
        audio_pos[b] = pos + 1;
        cache_len[b] += 1;
    }
}

// vh_sample_step_wide with the seed = seed + *seed_dev (seed_dev may be NULL), or with per-row records (rs != NULL: top_k, top_p,
// temperature, seed and seed_dev are not read; limits: the rows' length bounds beside them, or NULL): the decoder plan's form
// (plan.hip)
int vh_internal_sample_step_wide(const float* logits, int ldl, int V, int eos, int top_k, float top_p,
                                 float temperature, uint64_t seed, const uint64_t* seed_dev, const vh_row_sampling* rs,
                                 const vh_row_limits* limits, int64_t* codes, int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                                 const float* audio_emb, const float* pe, int32_t* audio_pos,
                                 int32_t* cache_len, float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(logits && codes && eos_count && audio_emb && pe && audio_pos && cache_len && x_next,
               VH_EINVAL, "vh_sample_step_wide: null pointer");
    VH_REQUIRE(B > 0 && V > 0 && V <= VH_SAMPLE_MAX_V && ldl >= V && d > 0 && d % 4 == 0, VH_EINVAL,
               "vh_sample_step_wide: bad dims B=%d V=%d (<= %d) ldl=%d d=%d", B, V, VH_SAMPLE_MAX_V, ldl, d);
    VH_REQUIRE(rs || temperature > 0.f, VH_EINVAL, "vh_sample_step_wide: temperature must be positive");
    VH_REQUIRE(vh_aligned16(rs), VH_EALIGN, "vh_sample_step_wide: the per-row sampling records must be 16-byte aligned");
    CHECK_ROW_LIMITS("vh_sample_step_wide");
    VH_REQUIRE(vh_aligned16(audio_emb) && vh_aligned16(pe) && vh_aligned16(x_next), VH_EALIGN,
               "vh_sample_step_wide: audio_emb/pe/x_next must be 16-byte aligned");
    const auto kernel = limits ? sample_step_wide_kernel<true> : sample_step_wide_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(WIDE_THREADS), 0, (hipStream_t)stream, logits, ldl, V,
                       eos, top_k, top_p, rs ? 1.0f : 1.0f / temperature, seed, codes, codes_stride, eos_count,
                       pos_base, sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, d, seed_dev, rs, limits);
    VH_CHECK_LAUNCH("vh_sample_step_wide");
    return VH_OK;
}

extern "C" int vh_sample_step_wide(const float* logits, int ldl, int V, int eos, int top_k, float top_p,
                                   float temperature, uint64_t seed, int64_t* codes, int64_t codes_stride,
                                   int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                                   const float* audio_emb, const float* pe, int32_t* audio_pos,
                                   int32_t* cache_len, float* x_next, int B, int d, void* stream) {
    return vh_internal_sample_step_wide(logits, ldl, V, eos, top_k, top_p, temperature, seed, nullptr, nullptr, nullptr, codes,
                                        codes_stride, eos_count, pos_base, sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next,
                                        B, d, stream);
}

extern "C" int vh_sample_step_wide_rows(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs, int64_t* codes,
                                       int64_t codes_stride, int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                                       const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                                       float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(rs, VH_EINVAL, "vh_sample_step_wide_rows: null sampling records (vh_sample_step_wide takes one filter for every row)");
    return vh_internal_sample_step_wide(logits, ldl, V, eos, 0, 1.f, 1.f, 0, nullptr, rs, nullptr, codes, codes_stride, eos_count, pos_base,
                                       sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, B, d, stream);
}

extern "C" int vh_sample_step_wide_rows_bounded(const float* logits, int ldl, int V, int eos, const vh_row_sampling* rs,
                                               const vh_row_limits* limits, int64_t* codes, int64_t codes_stride,
                                               int32_t* eos_count, const int32_t* pos_base, float* sum_logprobs,
                                               const float* audio_emb, const float* pe, int32_t* audio_pos, int32_t* cache_len,
                                               float* x_next, int B, int d, void* stream) {
    VH_REQUIRE(rs, VH_EINVAL,
               "vh_sample_step_wide_rows_bounded: null sampling records (vh_sample_step_wide takes one filter for every row)");
    return vh_internal_sample_step_wide(logits, ldl, V, eos, 0, 1.f, 1.f, 0, nullptr, rs, limits, codes, codes_stride, eos_count,
                                       pos_base, sum_logprobs, audio_emb, pe, audio_pos, cache_len, x_next, B, d, stream);
}


// ---------------------------------------------------------------------------------------------
// Categorical(logits / temperature).sample() per row — the NAR stage sampler (valle/models/valle_nar.py:160)
// — or the arg-max (lowest index on ties) when `greedy`.  One wave per row, 4 rows per workgroup:
//   lane l owns the contiguous index range [l*chunk, (l+1)*chunk): row maximum by wave reduction, the
//   lane's sum of exp(x - max), an inclusive scan over the 64 lane sums (DPP-free shuffles: 6 steps),
//   u = uniform(seed, row, stream_id) * total picks the lane whose range holds the draw, and that lane walks
//   its range (inverse CDF in index order).  Also returns log p(token) (tests; optional).
// ---------------------------------------------------------------------------------------------
// One row of either launch below, by its wave: `lr` the row's logits, u01 its uniform, `token` / `lp` (may be NULL) where
// lane 0 (greedy) or the owner lane stores.
__device__ __forceinline__ void categorical_row(const float* __restrict__ lr, int V, int lane, float inv_temp, bool greedy,
                                                float u01, int64_t* __restrict__ token, float* __restrict__ lp) {
    const int chunk = (V + 63) / 64;
    const int i0 = min(V, lane * chunk), i1 = min(V, i0 + chunk);
    float m = -INFINITY;
    int am = V;                                         // first index of the lane's maximum
    for (int i = i0; i < i1; ++i) {
        const float x = lr[i] * inv_temp;
        if (x > m) { m = x; am = i; }
    }
    const float wm = wave_max(m);
    if (greedy) {
        // lowest index among the lanes holding the row maximum (torch.argmax's tie rule)
        int cand = (m == wm) ? am : V;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) cand = min(cand, __shfl_xor(cand, o));
        if (lane == 0) {
            // a row of NaN / -inf only has no maximum: emit the last valid id, never V (outside every table)
            *token = min(cand, V - 1);
            if (lp) *lp = 0.f;
        }
        return;
    }
    float s = 0.f;
    for (int i = i0; i < i1; ++i) s += expf(lr[i] * inv_temp - wm);
    float incl = s;                                     // inclusive scan over lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    const float total = __shfl(incl, 63);
    const float u = u01 * total;
    // the first lane whose inclusive sum exceeds u holds the draw (a lane with an empty range never does
    // unless every later lane is empty too: the last non-empty lane is the fallback for u == total rounding)
    const unsigned long long hit = __ballot(incl > u && i1 > i0);
    const unsigned long long nonempty = __ballot(i1 > i0);
    const int owner = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)nonempty);
    if (lane == owner) {
        float acc = incl - s;
        int pick = i1 - 1;
        for (int i = i0; i < i1; ++i) {
            acc += expf(lr[i] * inv_temp - wm);
            if (acc > u) { pick = i; break; }
        }
        *token = pick;
        if (lp) *lp = (lr[pick] * inv_temp - wm) - logf(total);
    }
}

__global__ __launch_bounds__(256) void categorical_rows_kernel(
    const float* __restrict__ logits, int ld, int V, int rows, float inv_temp, int greedy, uint64_t seed,
    uint32_t stream_id, int64_t* __restrict__ tokens, int64_t tokens_stride, float* __restrict__ logprob) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    categorical_row(logits + (int64_t)row * ld, V, lane, inv_temp, greedy != 0, uniform01(seed, (uint32_t)row, stream_id),
                    tokens + (int64_t)row * tokens_stride, logprob ? logprob + row : nullptr);
}

extern "C" int vh_categorical_rows(const float* logits, int ld, int V, int rows, float temperature, int greedy,
                                   uint64_t seed, uint32_t stream_id, int64_t* tokens, int64_t tokens_stride,
                                   float* logprob, void* stream) {
    VH_REQUIRE(logits && tokens && V > 0 && ld >= V && rows >= 0 && tokens_stride >= 1, VH_EINVAL,
               "vh_categorical_rows: bad args rows=%d V=%d ld=%d", rows, V, ld);
    VH_REQUIRE(greedy || temperature > 0.f, VH_EINVAL, "vh_categorical_rows: temperature=%g must be > 0",
               temperature);
    if (rows == 0) return VH_OK;
    hipLaunchKernelGGL(categorical_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld,
                       V, rows, greedy ? 1.0f : 1.0f / temperature, greedy, seed, stream_id, tokens, tokens_stride,
                       logprob);
    VH_CHECK_LAUNCH("vh_categorical_rows");
    return VH_OK;
}

// The same draw keyed on the REQUEST: packed row r belongs to request g = row_request[r] and is its frame t = row_key[r];
// seed, temperature and greediness (top_k == 1) come from requests[g], the uniform is uniform01(seed, t, stream_id) and the
// token lands at tokens[g * request_stride + t * key_stride] — nothing of the row's place in the launch enters.  g and t are
// the same for every lane of the wave (read through the first lane, so the record is a wave-uniform load); a row whose g or
// t is out of range reads no record and stores nothing.  1 / temperature is the fp32 division of ROW_SAMPLING_LOAD.
__global__ __launch_bounds__(256) void categorical_rows_keyed_kernel(
    const float* __restrict__ logits, int ld, int V, int rows, const vh_row_sampling* __restrict__ requests, int n_requests,
    const int32_t* __restrict__ row_request, const int32_t* __restrict__ row_key, int n_keys, uint32_t stream_id,
    int64_t* __restrict__ tokens, int64_t request_stride, int64_t key_stride, float* __restrict__ logprob) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int g = __builtin_amdgcn_readfirstlane(row_request[row]);
    const int t = __builtin_amdgcn_readfirstlane(row_key[row]);
    if (g < 0 || g >= n_requests || t < 0 || t >= n_keys) return;
    const vh_row_sampling rq = requests[g];
    const bool greedy = rq.top_k == 1;
    categorical_row(logits + (int64_t)row * ld, V, lane, greedy ? 1.0f : 1.0f / rq.temperature, greedy,
                    uniform01(rq.seed, (uint32_t)t, stream_id), tokens + (int64_t)g * request_stride + (int64_t)t * key_stride,
                    logprob ? logprob + row : nullptr);
}

extern "C" int vh_categorical_rows_keyed(const float* logits, int ld, int V, int rows, const vh_row_sampling* requests,
                                         int n_requests, const int32_t* row_request, const int32_t* row_key, int n_keys,
                                         uint32_t stream_id, int64_t* tokens, int64_t request_stride, int64_t key_stride,
                                         float* logprob, void* stream) {
    VH_REQUIRE(logits, VH_EINVAL, "vh_categorical_rows_keyed: null logits");
    VH_REQUIRE(requests, VH_EINVAL, "vh_categorical_rows_keyed: null requests (vh_categorical_rows takes one seed for every row)");
    VH_REQUIRE(row_request && row_key, VH_EINVAL, "vh_categorical_rows_keyed: null row_request / row_key");
    VH_REQUIRE(tokens, VH_EINVAL, "vh_categorical_rows_keyed: null tokens");
    VH_REQUIRE(V > 0 && ld >= V && rows >= 0, VH_EINVAL, "vh_categorical_rows_keyed: bad dims rows=%d V=%d ld=%d", rows, V, ld);
    VH_REQUIRE(n_requests >= 1 && n_keys >= 1, VH_EINVAL, "vh_categorical_rows_keyed: n_requests=%d n_keys=%d must be >= 1",
               n_requests, n_keys);
    VH_REQUIRE(request_stride >= 1 && key_stride >= 1, VH_EINVAL,
               "vh_categorical_rows_keyed: request_stride=%lld key_stride=%lld must be >= 1", (long long)request_stride,
               (long long)key_stride);
    VH_REQUIRE(vh_aligned16(requests), VH_EALIGN, "vh_categorical_rows_keyed: requests must be 16-byte aligned");
    if (rows == 0) return VH_OK;
    hipLaunchKernelGGL(categorical_rows_keyed_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld,
                       V, rows, requests, n_requests, row_request, row_key, n_keys, stream_id, tokens, request_stride,
                       key_stride, logprob);
    VH_CHECK_LAUNCH("vh_categorical_rows_keyed");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// Queued decoding (ValleAR.generate_queued): the rows of a decode launch are G = B / beams groups, each group the beams of
// one utterance, and a group that has finished hands its rows to a waiting utterance while the others keep stepping.
//   decode_groups_poll_kernel   what the host needs to know at a poll, in one launch and one small read: per group whether it
//                               is done and how many tokens it has produced, and the largest cache_len / audio_pos — over
//                               all rows (the high-water marks) and over the rows of groups that are NOT done (the rows that
//                               step on from where they stand: what the host bounds before it replays).
//   decode_group_reset_kernel   re-arms the rows of one group for a new utterance, or parks them.
// Plain loads and stores, no atomics: the same state gives the same bits.
// ---------------------------------------------------------------------------------------------
#define POLL_NONE (-(1 << 30))     // a maximum over no rows

__device__ __forceinline__ int wave_max_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// One workgroup of four waves; wave w takes groups w, w + 4, ... (a group is never split over waves), its lanes the beams.
__global__ __launch_bounds__(256) void decode_groups_poll_kernel(
    const int64_t* __restrict__ codes, int64_t codes_stride, int codes_width, const int32_t* __restrict__ cache_len,
    const int32_t* __restrict__ audio_pos, const int32_t* __restrict__ pos_base, int eos, int n_groups, int beams,
    int max_new, int32_t* __restrict__ group_done, int32_t* __restrict__ group_steps, int32_t* __restrict__ maxima) {
    __shared__ int s_max[4][4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int m_cl = POLL_NONE, m_ap = POLL_NONE, live_cl = POLL_NONE, live_ap = POLL_NONE;
    for (int g = w; g < n_groups; g += 4) {                  // wave-uniform trip count
        int not_eos = 0, steps_min = 0x7fffffff, steps_max = POLL_NONE, cl = POLL_NONE, ap = POLL_NONE;
        for (int j = lane; j < beams; j += 64) {
            const int b = g * beams + j;
            const int pos = audio_pos[b], steps = pos - pos_base[b];
            // the latest token; a position outside the row reads nothing and counts as "not finished"
            const bool at_eos = pos >= 1 && pos <= codes_width && codes[(int64_t)b * codes_stride + pos - 1] == (int64_t)eos;
            not_eos |= at_eos ? 0 : 1;
            steps_min = min(steps_min, steps);
            steps_max = max(steps_max, steps);
            cl = max(cl, cache_len[b]);
            ap = max(ap, pos);
        }
        not_eos = wave_max_i32(not_eos);
        steps_min = -wave_max_i32(-steps_min);
        steps_max = wave_max_i32(steps_max);
        cl = wave_max_i32(cl);
        ap = wave_max_i32(ap);
        const int done = (!not_eos || steps_min >= max_new) ? 1 : 0;
        if (lane == 0) {
            group_done[g] = done;
            group_steps[g] = steps_max;
        }
        m_cl = max(m_cl, cl);
        m_ap = max(m_ap, ap);
        if (!done) {
            live_cl = max(live_cl, cl);
            live_ap = max(live_ap, ap);
        }
    }
    if (lane == 0) { s_max[w][0] = m_cl; s_max[w][1] = m_ap; s_max[w][2] = live_cl; s_max[w][3] = live_ap; }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int k = threadIdx.x;
        maxima[k] = max(max(s_max[0][k], s_max[1][k]), max(s_max[2][k], s_max[3][k]));
    }
}

extern "C" int vh_decode_groups_poll(const int64_t* codes, int64_t codes_stride, int codes_width, const int32_t* cache_len,
                                     const int32_t* audio_pos, const int32_t* pos_base, int eos, int B, int beams, int max_new,
                                     int32_t* group_done, int32_t* group_steps, int32_t* maxima, void* stream) {
    VH_REQUIRE(codes && cache_len && audio_pos && pos_base && group_done && group_steps && maxima, VH_EINVAL,
               "vh_decode_groups_poll: null pointer");
    VH_REQUIRE(B > 0 && codes_width > 0 && codes_stride >= codes_width && eos >= 0, VH_EINVAL,
               "vh_decode_groups_poll: bad dims B=%d codes_width=%d codes_stride=%lld eos=%d", B, codes_width,
               (long long)codes_stride, eos);
    VH_REQUIRE(beams >= 1 && B % beams == 0, VH_EINVAL,
               "vh_decode_groups_poll: B=%d is not a multiple of beams=%d (the rows of a group)", B, beams);
    VH_REQUIRE(max_new >= 0, VH_EINVAL, "vh_decode_groups_poll: max_new=%d", max_new);
    VH_REQUIRE((reinterpret_cast<uintptr_t>(codes) & 7u) == 0 &&
                   ((reinterpret_cast<uintptr_t>(cache_len) | reinterpret_cast<uintptr_t>(audio_pos) |
                     reinterpret_cast<uintptr_t>(pos_base) | reinterpret_cast<uintptr_t>(group_done) |
                     reinterpret_cast<uintptr_t>(group_steps) | reinterpret_cast<uintptr_t>(maxima)) & 3u) == 0,
               VH_EALIGN, "vh_decode_groups_poll: codes must be 8-byte aligned, the int32 arrays 4-byte aligned");
    hipLaunchKernelGGL(decode_groups_poll_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, codes, codes_stride, codes_width,
                       cache_len, audio_pos, pos_base, eos, B / beams, beams, max_new, group_done, group_steps, maxima);
    VH_CHECK_LAUNCH("vh_decode_groups_poll");
    return VH_OK;
}

// One workgroup per beam row of the group.  prompt_len >= 1: the row becomes BOS + the prompt's prompt_len - 1 ids + EOS to
// its end, the counters those of a row before its first sample.  prompt_len == 0: parked — see the header.
__global__ __launch_bounds__(256) void decode_group_reset_kernel(
    int64_t* __restrict__ codes, int64_t codes_stride, int codes_width, const int64_t* __restrict__ prompt, int prompt_len,
    int prefix_len, int bos, int eos, int group, int beams, int32_t* __restrict__ cache_len, int32_t* __restrict__ audio_pos,
    int32_t* __restrict__ pos_base, float* __restrict__ sum_logprobs, int32_t* __restrict__ prefix_lens) {
    const int b = group * beams + blockIdx.x, tid = threadIdx.x;
    int64_t* row = codes + (int64_t)b * codes_stride;
    if (prompt_len >= 1) {
        for (int c = tid; c < codes_width; c += 256)
            row[c] = c == 0 ? (int64_t)bos : (c < prompt_len ? prompt[c - 1] : (int64_t)eos);
        if (tid == 0) {
            cache_len[b] = 0;
            audio_pos[b] = prompt_len;
            pos_base[b] = prompt_len;
            sum_logprobs[b] = 0.f;
        }
    } else if (tid == 0) {
        // parked: EOS where the row's first generated token stood and the counters of a fresh row behind it — every further
        // step finds EOS at audio_pos - 1 and writes EOS at audio_pos, over and over the same few places between two rewinds
        const int p = min(max(pos_base[b], 1), codes_width - 2);      // (a base outside the row is pulled into it)
        row[p] = (int64_t)eos;
        pos_base[b] = p;
        audio_pos[b] = p + 1;
        cache_len[b] = 0;
    }
    if (blockIdx.x == 0 && tid == 0) prefix_lens[group] = prompt_len >= 1 ? prefix_len : 0;
}

extern "C" int vh_decode_group_reset(int64_t* codes, int64_t codes_stride, int codes_width, const int64_t* prompt,
                                     int prompt_len, int prefix_len, int bos, int eos, int group, int B, int beams,
                                     int32_t* cache_len, int32_t* audio_pos, int32_t* pos_base, float* sum_logprobs,
                                     int32_t* prefix_lens, void* stream) {
    VH_REQUIRE(codes && cache_len && audio_pos && pos_base && sum_logprobs && prefix_lens && (prompt || prompt_len <= 1),
               VH_EINVAL, "vh_decode_group_reset: null pointer");
    VH_REQUIRE(B > 0 && codes_width >= 3 && codes_stride >= codes_width && eos >= 0 && bos >= 0, VH_EINVAL,
               "vh_decode_group_reset: bad dims B=%d codes_width=%d codes_stride=%lld eos=%d bos=%d", B, codes_width,
               (long long)codes_stride, eos, bos);
    VH_REQUIRE(beams >= 1 && B % beams == 0, VH_EINVAL,
               "vh_decode_group_reset: B=%d is not a multiple of beams=%d (the rows of a group)", B, beams);
    VH_REQUIRE(group >= 0 && group < B / beams, VH_EINVAL, "vh_decode_group_reset: group=%d of %d", group, B / beams);
    VH_REQUIRE(prompt_len >= 0 && prompt_len < codes_width, VH_EINVAL,
               "vh_decode_group_reset: prompt_len=%d (BOS + prompt) must leave room in a row of %d", prompt_len, codes_width);
    VH_REQUIRE(prompt_len == 0 ? prefix_len == 0 : prefix_len >= prompt_len, VH_EINVAL,
               "vh_decode_group_reset: prefix_len=%d with prompt_len=%d (text + BOS + prompt keys; 0 parks the group)",
               prefix_len, prompt_len);
    VH_REQUIRE(((reinterpret_cast<uintptr_t>(codes) | reinterpret_cast<uintptr_t>(prompt)) & 7u) == 0 &&
                   ((reinterpret_cast<uintptr_t>(cache_len) | reinterpret_cast<uintptr_t>(audio_pos) |
                     reinterpret_cast<uintptr_t>(pos_base) | reinterpret_cast<uintptr_t>(sum_logprobs) |
                     reinterpret_cast<uintptr_t>(prefix_lens)) & 3u) == 0,
               VH_EALIGN, "vh_decode_group_reset: codes / prompt must be 8-byte aligned, the 32-bit arrays 4-byte aligned");
    hipLaunchKernelGGL(decode_group_reset_kernel, dim3(beams), dim3(256), 0, (hipStream_t)stream, codes, codes_stride,
                       codes_width, prompt, prompt_len, prefix_len, bos, eos, group, beams, cache_len, audio_pos, pos_base,
                       sum_logprobs, prefix_lens);
    VH_CHECK_LAUNCH("vh_decode_group_reset");
    return VH_OK;
}

// ---------------------------------------------------------------------------------------------
// vh_kv_unpack: the K/V rows a packed forward left in ONE (1, h, S_src, 64) stream per (layer, K|V) go to the per-row caches
// the decoder reads, all layers and both of K and V in one launch.  Segment s of a (stream, head) is one contiguous run of
// seg_len[s] x 256 bytes on both sides, so the whole kernel is n_streams x h x n_seg straight copies: workgroup (x = stream x
// head, y = segment, z) takes the 64-row pieces z, z + gridDim.z, ... of its run, a thread four 16-byte loads in flight and
// then their four stores (16 KiB per workgroup per trip, consecutive lanes on consecutive 16 bytes).  Plain loads and stores:
// the rows are read again by the first decode steps, and whether a non-temporal form helps has not been measured.
// Guards as in attn_rows_packed_kernel (workgroup-uniform): a segment that starts outside the stream or names a row outside
// [0, B_dst) copies nothing; one that reaches past S_src, or is longer than S_dst, is cut there.
// ---------------------------------------------------------------------------------------------
#define KVU_ROWS 64                  // fp32 rows per workgroup trip: 256 threads x 4 x 16 bytes = 64 rows of 64 floats (128 rows of 64 halves)
// One kernel for both element widths (T = float: vh_kv_unpack, T = uint16_t: vh_kv_unpack_bf16, a row is then 128 bytes): only
// the number of 16-byte units per row depends on T, the copy itself moves 16 bytes at a time whatever they hold.
template <typename T>
__global__ __launch_bounds__(256) void kv_unpack_kernel(const T* __restrict__ src, T* __restrict__ dst,
                                                        const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_len,
                                                        const int32_t* __restrict__ dst_row, int n_heads, int S_src, int B_dst,
                                                        int S_dst) {
    constexpr int E = 16 / (int)sizeof(T);                        // elements of a 16-byte unit
    const int sh = blockIdx.x, strm = sh / n_heads, head = sh - strm * n_heads;
    const int s = blockIdx.y;
    const int s0 = seg_start[s], row = dst_row[s];
    if (s0 < 0 || s0 >= S_src || row < 0 || row >= B_dst) return;
    const int len = min(min(seg_len[s], S_src - s0), S_dst);
    if (len <= 0) return;
    const T* from = src + ((int64_t)sh * S_src + s0) * VH_HEAD_DIM;
    T* to = dst + (((int64_t)strm * B_dst + row) * n_heads + head) * (int64_t)S_dst * VH_HEAD_DIM;
    const int n4 = len * (VH_HEAD_DIM / E);                       // 16-byte units of the run (S_dst x 16 < 2^31: checked by the host)
    for (int i0 = blockIdx.z * (KVU_ROWS * 16) + threadIdx.x; i0 < n4; i0 += gridDim.z * (KVU_ROWS * 16)) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + 256 * j < n4) v[j] = ld4(reinterpret_cast<const float*>(from + E * (int64_t)(i0 + 256 * j)));
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + 256 * j < n4) st4(reinterpret_cast<float*>(to + E * (int64_t)(i0 + 256 * j)), v[j]);
    }
}

// the checks and the launch of both entry points (`name`: the one the refusal is reported under)
template <typename T>
static int kv_unpack_launch(const char* name, const T* src, T* dst, int n_streams, int n_heads, int S_src, int B_dst, int S_dst,
                            const int32_t* seg_start, const int32_t* seg_len, const int32_t* dst_row, int n_seg, void* stream) {
    VH_REQUIRE(src && dst, VH_EINVAL, "%s: null pointer (src or dst)", name);
    VH_REQUIRE(seg_start && seg_len && dst_row, VH_EINVAL, "%s: null pointer (seg_start, seg_len or dst_row)", name);
    VH_REQUIRE(n_streams > 0 && n_heads > 0 && S_src > 0 && B_dst > 0 && S_dst > 0, VH_EINVAL,
               "%s: bad dims n_streams=%d n_heads=%d S_src=%d B_dst=%d S_dst=%d", name, n_streams, n_heads, S_src, B_dst, S_dst);
    VH_REQUIRE(n_seg > 0, VH_EINVAL, "%s: n_seg=%d", name, n_seg);
    VH_REQUIRE(vh_aligned16(src) && vh_aligned16(dst), VH_EALIGN, "%s: src and dst must be 16-byte aligned", name);
    VH_REQUIRE(((reinterpret_cast<uintptr_t>(seg_start) | reinterpret_cast<uintptr_t>(seg_len) | reinterpret_cast<uintptr_t>(dst_row)) & 3u) == 0,
               VH_EALIGN, "%s: seg_start, seg_len and dst_row must be 4-byte aligned", name);
    VH_REQUIRE((int64_t)n_streams * n_heads <= 0x7fffffffLL && n_seg <= 65535, VH_EUNSUPPORTED,
               "%s: n_streams=%d x n_heads=%d, n_seg=%d workgroups (x <= 2^31 - 1, y <= 65535)", name, n_streams, n_heads, n_seg);
    VH_REQUIRE(S_src <= (1 << 26) && S_dst <= (1 << 26), VH_EUNSUPPORTED, "%s: S_src=%d S_dst=%d (at most 2^26 rows per stream)", name,
               S_src, S_dst);
    // pieces of a run share the segment's workgroups over z until the launch has ~2048 workgroups (8 per CU) or a workgroup per
    // trip (64 fp32 rows, 128 16-bit rows) of the longest possible run
    const int64_t runs = (int64_t)n_streams * n_heads * n_seg;
    const int trip_rows = KVU_ROWS * 4 / (int)sizeof(T);
    const int trips = (min(S_src, S_dst) + trip_rows - 1) / trip_rows;
    const int gz = (int)max((int64_t)1, min((int64_t)min(trips, 64), (2048 + runs - 1) / runs));
    hipLaunchKernelGGL(kv_unpack_kernel<T>, dim3(n_streams * n_heads, n_seg, gz), dim3(256), 0, (hipStream_t)stream, src, dst, seg_start,
                       seg_len, dst_row, n_heads, S_src, B_dst, S_dst);
    VH_CHECK_LAUNCH(name);
    return VH_OK;
}

extern "C" int vh_kv_unpack(const float* src, float* dst, int n_streams, int n_heads, int S_src, int B_dst, int S_dst,
                            const int32_t* seg_start, const int32_t* seg_len, const int32_t* dst_row, int n_seg, void* stream) {
    return kv_unpack_launch<float>("vh_kv_unpack", src, dst, n_streams, n_heads, S_src, B_dst, S_dst, seg_start, seg_len, dst_row, n_seg,
                                   stream);
}

extern "C" int vh_kv_unpack_bf16(const uint16_t* src, uint16_t* dst, int n_streams, int n_heads, int S_src, int B_dst, int S_dst,
                                 const int32_t* seg_start, const int32_t* seg_len, const int32_t* dst_row, int n_seg, void* stream) {
    return kv_unpack_launch<uint16_t>("vh_kv_unpack_bf16", src, dst, n_streams, n_heads, S_src, B_dst, S_dst, seg_start, seg_len, dst_row,
                                      n_seg, stream);
}
