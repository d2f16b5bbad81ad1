// Single-query decode attention over an fp32 K/V cache (B, h, S_max, hd) for a head width hd other than 64
// (valle/models/modules.py:112 lets head_dim = d_model / n_heads be any divisor), and the prompt pass's K/V copy into
// that cache.  Width 64 keeps attention.hip's kernels; this file serves 16 <= hd <= 256, hd % 4 == 0.
//
//  attn_decode_hd_kernel : the structure of attn_decode_ring_kernel (attention.hip) with the lane map as a template:
//                          LK lanes per key (LK = min(16, next_pow2(hd / 4))), so 64 / LK keys per wave instruction;
//                          each lane holds NV 16-byte slots of its key (slot j = dimensions 4 (c + LK j) .. +3 with
//                          c = lane % LK); slots at or past hd / 4 are neither loaded nor multiplied, so the bytes
//                          fetched are exactly the cache's.  A register set holds LPS loads per operand and slot
//                          (LPS * NV ~ 8 16-byte loads per operand and lane, as at width 64), i.e. CK = LPS * 64 / LK
//                          keys; a wave owns a ring of D sets with D - 1 bursts outstanding while one is reduced, the
//                          first bursts issued before cache_len arrives (addresses clamped inside the allocation),
//                          non-temporal loads.  Dot products reduce over the LK lanes with DPP; online softmax in
//                          exp2 with q pre-scaled by scale * log2(e); keys past the row's length are selected away.
//                          Waves merge through LDS; key splits leave a record of round_up(hd + 2, 4) floats each.
//  attn_decode_hd_combine_kernel : the second launch of a key split: records added in split order (deterministic, no
//                          ticket words, no initialisation contract on the workspace).
//  kv_store_kernel       : the K and V column blocks of a (B T, 3 d) QKV projection into cache rows 0 .. T-1.
#include <hip/hip_ext.h>
#include "vh_common.h"

#define LOG2E_HD 1.44269504088896340736f
#define HD_MAX 256

// sums over the 8 lanes of a half DPP row (lanes 8j .. 8j+7) and over the 4 lanes of a quad: every lane gets the sum
__device__ __forceinline__ float hd_row8_sum(float v) {
    v += dpp_get<0xB1, 0xF>(v, 0.f);
    v += dpp_get<0x4E, 0xF>(v, 0.f);
    v += dpp_get<0x141, 0xF>(v, 0.f);     // row_half_mirror: lane i <-> 7 - i inside each half row
    return v;
}
__device__ __forceinline__ float hd_row4_sum(float v) {
    v += dpp_get<0xB1, 0xF>(v, 0.f);
    v += dpp_get<0x4E, 0xF>(v, 0.f);
    return v;
}
template <int LK>
__device__ __forceinline__ float lanes_sum(float v) {
    if constexpr (LK == 16) return row16_sum(v);
    else if constexpr (LK == 8) return hd_row8_sum(v);
    else return hd_row4_sum(v);
}

__host__ __device__ static inline int hd_record_floats(int hd) { return (hd + 2 + 3) & ~3; }

template <int NW, int D, int LK, int NV>
__global__ __launch_bounds__(NW * 64) void attn_decode_hd_kernel(
    const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc,
    float* __restrict__ out, int ldo, const int32_t* __restrict__ cache_len, int len_bias, int n_heads, int hd,
    int S_max, float scale, int n_split, float* __restrict__ partial) {
    constexpr int KPI = 64 / LK;                                   // keys per wave instruction
    constexpr int LPS = (8 + NV - 1) / NV;                         // loads per set, operand and slot
    constexpr int CK = LPS * KPI;                                  // keys per register set
    __shared__ float s_m[NW], s_l[NW];
    __shared__ __attribute__((aligned(16))) float s_o[NW][HD_MAX];
    const int bh = blockIdx.y, b = bh / n_heads, head = bh - b * n_heads;
    const int split = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c = lane % LK, g = lane / LK;
    const int hd4 = hd >> 2;
    bool sv[NV];                                                   // slot j of this lane lies inside the row
#pragma unroll
    for (int j = 0; j < NV; ++j) sv[j] = c + LK * j < hd4;
    const float* kb = kc + (int64_t)bh * S_max * hd + 4 * c;
    const float* vb = vc + (int64_t)bh * S_max * hd + 4 * c;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    f32x4 kf[D][LPS][NV], vf[D][LPS][NV];
    int key_limit = S_max - 1;                                     // before the length is known: stay inside the allocation
    auto load = [&](int ch, f32x4 (&kq)[LPS][NV], f32x4 (&vq)[LPS][NV]) {
        const int key0 = ch * CK + g;
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            const int64_t row = (int64_t)min(key0 + KPI * i, key_limit) * hd;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                kq[i][j] = sv[j] ? ld4_stream(kb + row + 4 * LK * j) : zero4;
                vq[i][j] = sv[j] ? ld4_stream(vb + row + 4 * LK * j) : zero4;
            }
        }
    };
    const bool spec = n_split == 1;
    if (spec) {
#pragma unroll
        for (int j = 0; j < D - 1; ++j) load(w + j * NW, kf[j], vf[j]);
    }
    const int len = cache_len[b] + len_bias;
    const int nchunks = (len + CK - 1) / CK;
    const int cps = (nchunks + n_split - 1) / n_split;
    const int c_begin = split * cps;
    const int c_end = min(nchunks, c_begin + cps);
    key_limit = len - 1;
    const float qscale = scale * LOG2E_HD;
    f32x4 q4[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j)
        q4[j] = sv[j] ? ld4(q + (int64_t)b * ldq + head * hd + 4 * (c + LK * j)) * qscale : zero4;
    if (!spec) {
#pragma unroll
        for (int j = 0; j < D - 1; ++j)
            if (c_begin + w + j * NW < c_end) load(c_begin + w + j * NW, kf[j], vf[j]);
    }

    float m = -INFINITY, l = 0.f;
    f32x4 o[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) o[j] = zero4;
    auto reduce = [&](int ch, const f32x4 (&kq)[LPS][NV], const f32x4 (&vq)[LPS][NV]) {
        const int key0 = ch * CK + g;
        const bool whole = ch * CK + CK <= len;                    // wave-uniform: no masking for interior sets
        float sc[LPS];
        float cmax = -INFINITY;
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const f32x4 t = kq[i][j] * q4[j];
                d += (t.x + t.y) + (t.z + t.w);
            }
            d = lanes_sum<LK>(d);
            sc[i] = (whole || key0 + KPI * i < len) ? d : -INFINITY;
            cmax = fmaxf(cmax, sc[i]);
        }
#pragma unroll
        for (int sh = LK; sh < 64; sh <<= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, sh, 64));
        const float m_new = fmaxf(m, cmax);                        // finite: set ch < nchunks holds >= 1 valid key
        const float alpha = vh_exp2(m - m_new);
        l *= alpha;
#pragma unroll
        for (int j = 0; j < NV; ++j) o[j] *= alpha;
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            const float p = vh_exp2(sc[i] - m_new);
            l += p;
            // rows beyond the length hold whatever the allocation held (possibly NaN): select, do not multiply by 0
            const bool in = whole || key0 + KPI * i < len;
#pragma unroll
            for (int j = 0; j < NV; ++j) o[j] += (in ? vq[i][j] : zero4) * p;
        }
        m = m_new;
    };
    for (int c0 = c_begin + w; c0 < c_end; c0 += D * NW) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int ch = c0 + j * NW;
            if (ch < c_end) {
                const int cn = ch + (D - 1) * NW;                  // the burst that keeps D - 1 outstanding
                if (cn < c_end) load(cn, kf[(j + D - 1) % D], vf[(j + D - 1) % D]);
                reduce(ch, kf[j], vf[j]);
            }
        }
    }
    // fold the key groups of the wave (lanes l, l ^ LK, l ^ 2 LK, ... hold the same dimensions)
#pragma unroll
    for (int sh = LK; sh < 64; sh <<= 1) {
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            o[j].x += __shfl_xor(o[j].x, sh, 64); o[j].y += __shfl_xor(o[j].y, sh, 64);
            o[j].z += __shfl_xor(o[j].z, sh, 64); o[j].w += __shfl_xor(o[j].w, sh, 64);
        }
        l += __shfl_xor(l, sh, 64);
    }
    if (lane < LK) {
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (sv[j]) st4(&s_o[w][4 * (c + LK * j)], o[j]);
    }
    if (lane == 0) { s_m[w] = m; s_l[w] = l; }
    __syncthreads();
    if (tid < hd) {
        float M = s_m[0];
#pragma unroll
        for (int k = 1; k < NW; ++k) M = fmaxf(M, s_m[k]);
        float L = 0.f, O = 0.f;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const float wgt = s_m[k] == -INFINITY ? 0.f : vh_exp2(s_m[k] - M);
            L += s_l[k] * wgt;
            O += s_o[k][tid] * wgt;
        }
        if (n_split == 1) {
            out[(int64_t)b * ldo + head * hd + tid] = O / L;
        } else {
            float* pr = partial + ((int64_t)bh * n_split + split) * hd_record_floats(hd);
            pr[tid] = O;
            if (tid == 0) { pr[hd] = M; pr[hd + 1] = L; }
        }
    }
}

// the split records of every (b, head), added in split order (a split without keys has M = -inf and weighs 0)
__global__ __launch_bounds__(HD_MAX) void attn_decode_hd_combine_kernel(
    const float* __restrict__ partial, float* __restrict__ out, int ldo, int n_heads, int hd, int n_split) {
    const int bh = blockIdx.x, b = bh / n_heads, head = bh - b * n_heads;
    const int tid = threadIdx.x;
    if (tid >= hd) return;
    const int ld = hd_record_floats(hd);
    const float* pr = partial + (int64_t)bh * n_split * ld;
    float M = -INFINITY;
    for (int s = 0; s < n_split; ++s) M = fmaxf(M, pr[s * ld + hd]);
    float L = 0.f, O = 0.f;
    for (int s = 0; s < n_split; ++s) {
        const float ms = pr[s * ld + hd];
        const float wgt = ms == -INFINITY ? 0.f : vh_exp2(ms - M);
        L += pr[s * ld + hd + 1] * wgt;
        O += pr[s * ld + tid] * wgt;
    }
    out[(int64_t)b * ldo + head * hd + tid] = O / L;
}

// ---- what attention.hip's check, plan and launcher (vh_attn_decode_hd is one of its entry points) need of this file ----
static_assert(HD_MAX == VH_HEAD_DIM_MAX, "the plan sizes the combine launch by VH_HEAD_DIM_MAX");
int vh_internal_attn_hd_record_floats(int hd) { return hd_record_floats(hd); }

// the planned kernel (events on its dispatch packet) and its combine launch; false: no such lane map is compiled
bool vh_internal_attn_decode_hd_launch(const vh_attn_decode_form_info& f, const DecodeAttnCall& c, hipEvent_t start, hipEvent_t stop) {
    hipStream_t s = (hipStream_t)c.stream;
    auto launch = [&](auto kernel) {
        hipExtLaunchKernelGGL(kernel, dim3(f.grid[0], f.grid[1], f.grid[2]), dim3(f.block), 0, s, start, stop, 0, c.q, c.ldq,
                              (const float*)c.k, (const float*)c.v, c.out, c.ldo, c.len, c.len_bias, c.n_heads, c.head_dim, c.S_max,
                              c.scale, c.n_split, (float*)c.ws);
        return true;
    };
    const bool compiled = f.nw != 8 || f.d != 2 ? false
                          : f.lk == 4 && f.nv == 1 ? launch(attn_decode_hd_kernel<8, 2, 4, 1>)
                          : f.lk == 8 && f.nv == 1 ? launch(attn_decode_hd_kernel<8, 2, 8, 1>)
                          : f.lk != 16 ? false
                          : f.nv == 1 ? launch(attn_decode_hd_kernel<8, 2, 16, 1>)
                          : f.nv == 2 ? launch(attn_decode_hd_kernel<8, 2, 16, 2>)
                          : f.nv == 3 ? launch(attn_decode_hd_kernel<8, 2, 16, 3>)
                          : f.nv == 4 ? launch(attn_decode_hd_kernel<8, 2, 16, 4>) : false;
    if (compiled && f.second == VH_ATTN_2ND_HD_COMBINE)
        hipLaunchKernelGGL(attn_decode_hd_combine_kernel, dim3(f.second_grid), dim3(f.second_block), 0, s, (const float*)c.ws, c.out,
                           c.ldo, c.n_heads, c.head_dim, c.n_split);
    return compiled;
}

// ---- prompt pass: K / V column blocks of the QKV projection into cache rows 0 .. T-1 ----
// one thread per 16 bytes of K or V: g4 indexes the (B T) x (d / 4) groups of one block; a group never crosses a head
// (hd % 4 == 0)
__global__ __launch_bounds__(256) void kv_store_kernel(const float* __restrict__ qkv, int ld, float* __restrict__ kc,
                                                       float* __restrict__ vc, int T, int n_heads, int hd, int S_max,
                                                       int64_t n4) {
    const int d4 = n_heads * hd / 4, hd4 = hd / 4;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < 2 * n4; i += (int64_t)gridDim.x * 256) {
        const int which = i >= n4;                                 // 0: K, 1: V
        const int64_t g4 = i - which * n4;
        const int64_t r = g4 / d4;                                 // row b T + t of the projection
        const int cg = (int)(g4 - r * d4), head = cg / hd4, e4 = cg - head * hd4;
        const int64_t b = r / T, t = r - b * T;
        const f32x4 v = ld4(qkv + r * ld + (int64_t)(1 + which) * n_heads * hd + 4 * cg);
        float* dst = which ? vc : kc;
        st4(dst + (((b * n_heads + head) * S_max) + t) * hd + 4 * e4, v);
    }
}

extern "C" int vh_kv_store(const float* qkv, int ld, float* kcache, float* vcache, int B, int T, int n_heads, int head_dim,
                           int S_max, void* stream) {
    VH_REQUIRE(qkv && kcache && vcache, VH_EINVAL, "vh_kv_store: null pointer");
    VH_REQUIRE(B >= 0 && T >= 0 && n_heads > 0 && head_dim > 0 && head_dim % 4 == 0 && T <= S_max, VH_EINVAL,
               "vh_kv_store: B=%d T=%d h=%d head_dim=%d S_max=%d (head_dim a multiple of 4, T <= S_max)", B, T, n_heads,
               head_dim, S_max);
    VH_REQUIRE(ld % 4 == 0 && ld >= 3 * n_heads * head_dim, VH_EINVAL, "vh_kv_store: ld=%d", ld);
    VH_REQUIRE(vh_aligned16(qkv) && vh_aligned16(kcache) && vh_aligned16(vcache), VH_EALIGN,
               "vh_kv_store: pointers must be 16-byte aligned");
    const int64_t n4 = (int64_t)B * T * n_heads * head_dim / 4;
    if (n4 == 0) return VH_OK;
    const int blocks = (int)min((int64_t)2048, (2 * n4 + 255) / 256);
    hipLaunchKernelGGL(kv_store_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, qkv, ld, kcache, vcache, T, n_heads,
                       head_dim, S_max, n4);
    VH_CHECK_LAUNCH("vh_kv_store");
    return VH_OK;
}
