// Self-attention kernels over the (B, h, S_max, 64) fp32 KV cache.
//
//  attn_rows_kernel   : many query rows (prefill, NAR stage, training forward). Flash-style online
//                       softmax, fp32 MFMA 32x32x2 for both products, computed TRANSPOSED
//                       (Sᵀ = K·Qᵀ, Oᵀ = Vᵀ·Pᵀ) so a query is a lane: row max/sum are in-lane
//                       plus one cross-half shuffle, the P accumulator registers ARE the next
//                       MFMA's B operand, and the O rescale is lane-local.  K/V tiles of 32 keys
//                       are register-staged into double-buffered LDS.  Masks are analytic
//                       (prefix-LM / full / key length), never materialised.   MFMA-bound.
//  attn_rows_packed_kernel : the same body (attn_rows_body.inc) over the SEGMENTS of one packed row
//                       stream under the full mask: a ragged NAR batch with no padding rows.
//  attn_rows_packed_lse_kernel, attn_bwd_packed_kernel : its training forms (packed AR training), at the end of the file.
//  attn_decode_kernel : one query row per (batch, head) against the whole cache — the dominant
//                       kernel of AR decoding.  Pure HBM streaming: every K/V byte is read once
//                       with 16-B loads, 1 KiB per wave-instruction, 16 KiB in flight per wave;
//                       dot products reduce over the 16 lanes of a DPP row; online softmax per
//                       32-key chunk; waves combine through LDS, key splits through a small
//                       workspace.   HBM-bound (algorithmic bytes = 2·len·64·4 per (b,head)).
#include <hip/hip_ext.h>
#include "vh_common.h"
#include <mutex>
#include <queue>
#include <type_traits>
#include <unordered_map>
#include <vector>

#define HD VH_HEAD_DIM
#define LOG2E 1.44269504088896340736f
#define NEG_INF (-INFINITY)

// =============================================================================================
// decode
// =============================================================================================
#define PART_LD 72  // floats per partial record: o[64], m, l, pad

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 ld16_stream(const uint16_t* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
}
// sum over the 8 lanes of a half DPP row (lanes 8j .. 8j+7)
__device__ __forceinline__ float row8_sum(float v) {
    v += dpp_get<0xB1, 0xF>(v, 0.f);
    v += dpp_get<0x4E, 0xF>(v, 0.f);
    v += dpp_get<0x141, 0xF>(v, 0.f);     // row_half_mirror: lane i <-> 7 - i inside each half row
    return v;
}
#define BF_LO(w) vh_h16_lo(w)
#define BF_HI(w) vh_h16_hi(w)

// ---- what every decode form ends with ----
// The NW waves of a workgroup left their (o, m, l) in LDS (a barrier lies between): thread tid < 64 merges column tid.  A wave
// without a chunk holds m = -inf and weighs nothing; M itself is -inf only for an empty key range.
// FMA_O: whether O += o_k * w_k rounds once (fma) or twice.  The compiler used to choose, differently from kernel to kernel
// (once where O is divided by L in place and in the 16-bit shared-prompt kernel, twice in the other record writers); the
// result bits are the contract, so each caller states what its kernel has always computed.  L rounds once everywhere.
template <int NW, bool FMA_O>
__device__ __forceinline__ void wave_merge(const float* s_m, const float* s_l, const float (*s_o)[HD], int tid, float& M,
                                           float& L, float& O) {
    M = s_m[0];
#pragma unroll
    for (int k = 1; k < NW; ++k) M = fmaxf(M, s_m[k]);
    L = 0.f;
    O = 0.f;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
        const float wgt = s_m[k] == NEG_INF ? 0.f : vh_exp2(s_m[k] - M);
        L = __builtin_fmaf(s_l[k], wgt, L);
        if constexpr (FMA_O) {
            O = __builtin_fmaf(s_o[k][tid], wgt, O);
        } else {
#pragma clang fp contract(off)
            const float t = s_o[k][tid] * wgt;
            O = O + t;
        }
    }
}
// column tid < 64 of one PART_LD record: O unnormalised, M in log2 units, L
__device__ __forceinline__ void write_record(float* pr, int tid, float O, float M, float L) {
    pr[tid] = O;
    if (tid == 0) { pr[HD] = M; pr[HD + 1] = L; }
}
// column tid of the n_split records at pr, added IN SPLIT ORDER and normalised; ldg is how a float is loaded
template <class Ld>
__device__ __forceinline__ float combine_splits(const float* pr, int n_split, int tid, Ld ldg) {
    float M = NEG_INF;
    for (int k = 0; k < n_split; ++k) M = fmaxf(M, ldg(pr + k * PART_LD + HD));
    float L = 0.f, O = 0.f;
    for (int k = 0; k < n_split; ++k) {
        const float ms = ldg(pr + k * PART_LD + HD);
        const float wgt = ms == NEG_INF ? 0.f : vh_exp2(ms - M);
        L += ldg(pr + k * PART_LD + HD + 1) * wgt;
        O += ldg(pr + k * PART_LD + tid) * wgt;
    }
    return O / L;
}

// Burst form (round 1): every wave requests a whole 32-key chunk with predicated loads, waits for it, reduces it and asks again.
// Serves key splits and more (b, head) pairs than CUs (vh_attn_decode).
template <int NW>
__global__ __launch_bounds__(NW * 64) void attn_decode_kernel(
    const float* __restrict__ q, int ldq, const float* __restrict__ kc,
    const float* __restrict__ vc, float* __restrict__ out, int ldo,
    const int32_t* __restrict__ cache_len, int len_bias, int n_heads, int S_max, int n_split,
    float* __restrict__ partial, unsigned* __restrict__ arrived) {
    __shared__ float s_m[NW], s_l[NW];
    __shared__ __attribute__((aligned(16))) float s_o[NW][HD];
    __shared__ int s_last;
    const int bh = blockIdx.y, b = bh / n_heads, head = bh - b * n_heads;
    const int split = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int c16 = lane & 15, g = lane >> 4;
    const int len = cache_len[b] + len_bias;
    const int nchunks = (len + 31) >> 5;
    const int cps = (nchunks + n_split - 1) / n_split;
    const int c_begin = split * cps;
    const int c_end = min(nchunks, c_begin + cps);

    const float qscale = 0.125f * LOG2E;  // 1/sqrt(64), folded with log2(e) for exp2
    const f32x4 q4 = ld4(q + (int64_t)b * ldq + head * HD + 4 * c16) * qscale;
    const float* kb = kc + (int64_t)bh * S_max * HD + 4 * c16;
    const float* vb = vc + (int64_t)bh * S_max * HD + 4 * c16;

    float m = NEG_INF, l = 0.f;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    for (int c = c_begin + w; c < c_end; c += NW) {
        const int key0 = c * 32 + g;
        f32x4 kf[8], vf[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int key = key0 + 4 * i;
            const bool in = key < len;
            kf[i] = in ? ld4_stream(kb + (int64_t)key * HD) : f32x4{0.f, 0.f, 0.f, 0.f};
            vf[i] = in ? ld4_stream(vb + (int64_t)key * HD) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float s[8];
        float cmax = NEG_INF;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4 t = kf[i] * q4;
            float d = row16_sum((t.x + t.y) + (t.z + t.w));
            s[i] = (key0 + 4 * i < len) ? d : NEG_INF;
            cmax = fmaxf(cmax, s[i]);
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
        const float m_new = fmaxf(m, cmax);  // finite: chunk c < nchunks holds >= 1 valid key
        const float alpha = vh_exp2(m - m_new);
        o *= alpha;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float p = vh_exp2(s[i] - m_new);
            l += p;
            o += vf[i] * p;
        }
        m = m_new;
    }
    // fold the 4 key groups of the wave (lanes l, l^16, l^32, l^48 hold the same dims)
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1) {
        o.x += __shfl_xor(o.x, sh, 64); o.y += __shfl_xor(o.y, sh, 64);
        o.z += __shfl_xor(o.z, sh, 64); o.w += __shfl_xor(o.w, sh, 64);
        l += __shfl_xor(l, sh, 64);
    }
    if (lane < 16) st4(&s_o[w][4 * c16], o);
    if (lane == 0) { s_m[w] = m; s_l[w] = l; }
    __syncthreads();
    if (tid < HD) {
        float M, L, O;
        wave_merge<NW, true>(s_m, s_l, s_o, tid, M, L, O);
        if (n_split == 1) {
            out[(int64_t)b * ldo + head * HD + tid] = O / L;
        } else if (arrived == nullptr) {                     // two-launch form: plain stores, the next launch reads them
            write_record(partial + ((int64_t)bh * n_split + split) * PART_LD, tid, O, M, L);
        } else {                                             // handed to another workgroup of THIS launch: write-through
            float* pr = partial + ((int64_t)bh * n_split + split) * PART_LD;
            __hip_atomic_store(pr + tid, O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tid == 0) {
                __hip_atomic_store(pr + HD, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(pr + HD + 1, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // Key splits, combined by the LAST workgroup of the (b, head) to arrive instead of by a second launch (opt-in,
    // VH_TUNE_DECODE_COMBINE = 1: measured slower than the launch it removes, see vh_attn_decode).  The 8 XCDs have
    // private L2s, so the record leaves as agent-scope (sc1, write-through) stores that the storing wave drains before
    // one lane takes a ticket with a relaxed agent-scope add — no release fence: an agent-scope release writes back the
    // whole L2 and made this form 240 us per step SLOWER than the second launch it replaces
    // (cdna_hip_programming.md Guideline 16, recipe R1).  The workgroup that draws the last ticket reads every record with
    // agent-scope loads (they bypass its L1: no acquire either) and adds them IN SPLIT ORDER — the result does not depend
    // on who came last — then re-arms the ticket word for the next launch of the stream (words start at zero:
    // vh_attn_decode_ws_bytes).
    if (arrived == nullptr) return;                          // (uniform: n_split == 1, or the two-launch form)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // every storing wave: its record has left
    __syncthreads();
    if (tid == 0) {
        const unsigned ticket = __hip_atomic_fetch_add(arrived + bh, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = ticket == (unsigned)(n_split - 1);
        if (s_last) __hip_atomic_store(arrived + bh, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the loads below the ticket)
    if (tid < HD)
        out[(int64_t)b * ldo + head * HD + tid] = combine_splits(
            partial + (int64_t)bh * n_split * PART_LD, n_split, tid,
            [](const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
}

__global__ __launch_bounds__(64) void attn_decode_combine_kernel(
    const float* __restrict__ partial, float* __restrict__ out, int ldo, int n_heads, int n_split) {
    const int bh = blockIdx.x, b = bh / n_heads, head = bh - b * n_heads;
    const int tid = threadIdx.x;
    out[(int64_t)b * ldo + head * HD + tid] =
        combine_splits(partial + (int64_t)bh * n_split * PART_LD, n_split, tid, [](const float* p) { return *p; });
}

// Ring form (round 2).  The burst kernel has its 256 KB per CU in flight only at the moment its 16 waves have
// all just issued; each wave then waits for its whole burst, reduces it, and only then asks again, and its very first
// request waits for a dependent load of cache_len[b].  Here a wave owns a ring of D register sets of 32 keys each:
// D-1 bursts are always outstanding while one is reduced, and with SPEC the first D-1 bursts are issued BEFORE the context
// length is known (addresses clamped inside the cache allocation; what lies beyond the row's length is masked once
// the length has arrived), so the stream starts with the kernel.  The read ceiling of this part is 6.3-6.5 TB/s
// for any read-only kernel (tools/probe_read_bw.hip, corrected: its first version dropped loop remainders and
// reported 8 TB/s); the 8 x 2 ring reaches 6.0-6.1 TB/s inside the decode step.
//
// One body serves the fp32 cache and the 16-bit cache of perf mode (half the bytes of the stream that bounds the decode step; q,
// the softmax and the accumulators stay fp32).  What differs is the lane map.  Either way a wave-instruction moves 1 KiB:
//   float     a key row is 256 B = 16 lanes x 16 B: lane l holds dimensions 4 (l & 15) .. +3 of key (l >> 4) of a group of 4 keys
//   uint16_t  a key row is 128 B =  8 lanes x 16 B: lane l holds dimensions 8 (l & 7) .. +7 of key (l >> 3) of a group of 8 keys
template <class T> struct KvLanes;
__device__ __forceinline__ f32x4 fma4(f32x4 a, float b, f32x4 c) { return __builtin_elementwise_fma(a, f32x4{b, b, b, b}, c); }
// o * alpha + v * p, the step of the online softmax that takes in a set's first key.  One of the two products is rounded before
// the fma; which one used to be the compiler's choice, and it chose differently for the fp32 shared-prompt suffix (o * alpha
// rounded: ALPHA_FMA = false) than for every other ring form (v * p rounded).  The result bits are the contract: pinned here.
template <bool ALPHA_FMA>
__device__ __forceinline__ f32x4 rescale_add(f32x4 o, float alpha, f32x4 v, float p) {
#pragma clang fp contract(off)
    if constexpr (ALPHA_FMA) {
        const f32x4 t = v * p;
        return fma4(o, alpha, t);
    } else {
        const f32x4 t = o * alpha;
        return fma4(v, p, t);
    }
}
template <> struct KvLanes<float> {
    typedef f32x4 Raw;                                             // what one lane loads of a key row
    static constexpr int LK = 16, NV = 1;                          // lanes per key; f32x4 per lane once widened
    static __device__ __forceinline__ Raw load(const float* p) { return ld4_stream(p); }
    static __device__ __forceinline__ Raw zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ float dot(const Raw& k, const f32x4 (&q)[NV]) {
        const f32x4 t = k * q[0];
        return row16_sum((t.x + t.y) + (t.z + t.w));
    }
    static __device__ __forceinline__ void widen(const Raw& v, f32x4 (&o)[NV]) { o[0] = v; }
};
template <> struct KvLanes<uint16_t> {
    typedef u32x4 Raw;
    static constexpr int LK = 8, NV = 2;
    static __device__ __forceinline__ Raw load(const uint16_t* p) { return ld16_stream(p); }
    static __device__ __forceinline__ Raw zero() { return u32x4{0u, 0u, 0u, 0u}; }
    static __device__ __forceinline__ float dot(const Raw& kk, const f32x4 (&q)[NV]) {
        float d = BF_LO(kk.x) * q[0].x + BF_HI(kk.x) * q[0].y + BF_LO(kk.y) * q[0].z + BF_HI(kk.y) * q[0].w;
        d += BF_LO(kk.z) * q[1].x + BF_HI(kk.z) * q[1].y + BF_LO(kk.w) * q[1].z + BF_HI(kk.w) * q[1].w;
        return row8_sum(d);
    }
    static __device__ __forceinline__ void widen(const Raw& v, f32x4 (&o)[NV]) {
        o[0] = f32x4{BF_LO(v.x), BF_HI(v.x), BF_LO(v.y), BF_HI(v.y)};
        o[1] = f32x4{BF_LO(v.z), BF_HI(v.z), BF_LO(v.w), BF_HI(v.w)};
    }
};

struct KeyRange { int len, c_begin, c_end; };   // the row's keys, and the 32-key chunks [c_begin, c_end) of them to reduce

// Chunks [c_begin, c_end) of ONE (row, head) stream, by the NW waves of a workgroup.  qrow: the head's 64 query values; kb / vb:
// the stream's first row.  `range` gives the row's length and the chunk range; it is evaluated AFTER the speculative bursts of
// SPEC (chunks w, w + NW, ... whatever the length is: c_begin must be 0, and until the length is there loads are clamped to row
// S_max - 1) and before anything else.  No load is predicated: loads are clamped to the row's last key and the keys past the
// length are SELECTED away (the rows behind them may hold NaN / Inf).  On return threads tid < 64 hold column tid of the
// workgroup's record: O (unnormalised), M (scores in log2 units; -inf for an empty range) and L.  Every thread of the workgroup
// must call it (one barrier inside).  ALPHA_FMA: see rescale_add; FMA_O: see wave_merge.
template <class T, int NW, int D, bool SPEC, bool ALPHA_FMA, bool FMA_O, class RangeFn>
__device__ __forceinline__ void ring_range(const float* __restrict__ qrow, const T* __restrict__ kb, const T* __restrict__ vb,
                                           int S_max, RangeFn range, float& M, float& L, float& O) {
    typedef KvLanes<T> KV;
    typedef typename KV::Raw Raw;
    constexpr int LK = KV::LK, NV = KV::NV;
    constexpr int KPI = 64 / LK, LPS = 32 / KPI, DPL = HD / LK;    // keys per wave-instruction; loads per set and operand; dims per lane
    __shared__ float s_m[NW], s_l[NW];
    __shared__ __attribute__((aligned(16))) float s_o[NW][HD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = lane & (LK - 1), kg = lane / LK;
    kb += DPL * col;
    vb += DPL * col;
    Raw kf[D][LPS], vf[D][LPS];
    int key_limit = S_max - 1;                                     // before the length is known: stay inside the allocation
    auto load = [&](int c, Raw (&kq)[LPS], Raw (&vq)[LPS]) {       // unconditional loads, clamped row index
        const int key0 = c * 32 + kg;
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            const int key = min(key0 + KPI * i, key_limit);
            kq[i] = KV::load(kb + (int64_t)key * HD);
            vq[i] = KV::load(vb + (int64_t)key * HD);
        }
    };
    if constexpr (SPEC) {
#pragma unroll
        for (int j = 0; j < D - 1; ++j) load(w + j * NW, kf[j], vf[j]);
    }
    const KeyRange kr = range();
    const int len = kr.len, c_begin = kr.c_begin, c_end = kr.c_end;
    key_limit = len - 1;                 // from here on the tail re-reads the row's last key instead of rows beyond it
    if constexpr (!SPEC) {
#pragma unroll
        for (int j = 0; j < D - 1; ++j)
            if (c_begin + w + j * NW < c_end) load(c_begin + w + j * NW, kf[j], vf[j]);
    }
    const float qscale = 0.125f * LOG2E;  // 1/sqrt(64), folded with log2(e) for exp2
    f32x4 qv[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) qv[n] = ld4(qrow + DPL * col + 4 * n) * qscale;

    float m = NEG_INF, l = 0.f;
    f32x4 o[NV];
#pragma unroll
    for (int n = 0; n < NV; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto reduce = [&](int c, const Raw (&kq)[LPS], const Raw (&vq)[LPS]) {
        const int key0 = c * 32 + kg;
        const bool whole = c * 32 + 32 <= len;                     // wave-uniform: no masking for interior chunks
        float sc[LPS];
        float cmax = NEG_INF;
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            const float d = KV::dot(kq[i], qv);
            sc[i] = (whole || key0 + KPI * i < len) ? d : NEG_INF;
            cmax = fmaxf(cmax, sc[i]);
        }
#pragma unroll
        for (int sh = LK; sh <= 32; sh <<= 1) cmax = fmaxf(cmax, __shfl_xor(cmax, sh, 64));
        const float m_new = fmaxf(m, cmax);                        // finite: chunk c < ceil(len / 32) holds >= 1 valid key
        const float alpha = vh_exp2(m - m_new);
        float p[LPS];
#pragma unroll
        for (int i = 0; i < LPS; ++i) p[i] = vh_exp2(sc[i] - m_new);
        l = __builtin_fmaf(l, alpha, p[0]);                        // l = l * alpha + sum p, o = o * alpha + sum v p: left to right
#pragma unroll
        for (int i = 1; i < LPS; ++i) l += p[i];
#pragma unroll
        for (int i = 0; i < LPS; ++i) {
            // rows beyond the length hold whatever the allocation held (possibly NaN): select, do not multiply by 0
            const Raw vv = (whole || key0 + KPI * i < len) ? vq[i] : KV::zero();
            f32x4 vw[NV];
            KV::widen(vv, vw);
#pragma unroll
            for (int n = 0; n < NV; ++n) o[n] = i == 0 ? rescale_add<ALPHA_FMA>(o[n], alpha, vw[n], p[0]) : fma4(vw[n], p[i], o[n]);
        }
        m = m_new;
    };
    for (int c0 = c_begin + w; c0 < c_end; c0 += D * NW) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const int c = c0 + j * NW;
            if (c < c_end) {
                const int cn = c + (D - 1) * NW;                   // the burst that keeps D - 1 outstanding
                if (cn < c_end) load(cn, kf[(j + D - 1) % D], vf[(j + D - 1) % D]);
                reduce(c, kf[j], vf[j]);
            }
        }
    }
    // fold the key groups of the wave (lanes l, l ^ LK, ..., l ^ 32 hold the same dimensions)
#pragma unroll
    for (int sh = LK; sh <= 32; sh <<= 1) {
#pragma unroll
        for (int n = 0; n < NV; ++n) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[n][j] += __shfl_xor(o[n][j], sh, 64);
        }
        l += __shfl_xor(l, sh, 64);
    }
    if (lane < LK) {
#pragma unroll
        for (int n = 0; n < NV; ++n) st4(&s_o[w][DPL * col + 4 * n], o[n]);
    }
    if (lane == 0) { s_m[w] = m; s_l[w] = l; }
    __syncthreads();
    M = NEG_INF;
    L = 0.f;
    O = 0.f;
    if (tid < HD) wave_merge<NW, FMA_O>(s_m, s_l, s_o, tid, M, L, O);
}

// whole row, speculative start: the default of vh_attn_decode (fp32 cache) and vh_attn_decode_kv16
template <class T, int NW, int D>
__device__ __forceinline__ void decode_ring_body(const float* __restrict__ q, int ldq, const T* __restrict__ kc,
                                                 const T* __restrict__ vc, float* __restrict__ out, int ldo,
                                                 const int32_t* __restrict__ cache_len, int len_bias, int n_heads, int S_max) {
    const int bh = blockIdx.y, b = bh / n_heads, head = bh - b * n_heads;
    float M, L, O;
    ring_range<T, NW, D, true, true, true>(q + (int64_t)b * ldq + head * HD, kc + (int64_t)bh * S_max * HD, vc + (int64_t)bh * S_max * HD,
                               S_max, [&] {
                                   const int len = cache_len[b] + len_bias;
                                   return KeyRange{len, 0, (len + 31) / 32};
                               }, M, L, O);
    const int tid = threadIdx.x;
    if (tid < HD) out[(int64_t)b * ldo + head * HD + tid] = O / L;
}
template <int NW, int D>
__global__ __launch_bounds__(NW * 64) void attn_decode_ring_kernel(
    const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc, float* __restrict__ out,
    int ldo, const int32_t* __restrict__ cache_len, int len_bias, int n_heads, int S_max) {
    decode_ring_body<float, NW, D>(q, ldq, kc, vc, out, ldo, cache_len, len_bias, n_heads, S_max);
}
template <int NW, int D>
__global__ __launch_bounds__(NW * 64) void attn_decode_ring16_kernel(
    const float* __restrict__ q, int ldq, const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
    float* __restrict__ out, int ldo, const int32_t* __restrict__ cache_len, int len_bias, int n_heads, int S_max) {
    decode_ring_body<uint16_t, NW, D>(q, ldq, kc, vc, out, ldo, cache_len, len_bias, n_heads, S_max);
}

// Key-split form of the ring16 kernel: grid (n_split, B h); split s of a (row, head) takes chunks [s cps, (s + 1) cps) of its
// ceil(len / 32) and writes one PART_LD record (o[64], m, l) — the layout attn_decode_combine_kernel reads.  A split without keys
// leaves m = -inf and weighs nothing.  No speculative bursts: a key split does not know its chunks before it knows the length.
template <int NW, int D>
__global__ __launch_bounds__(NW * 64) void attn_decode_ring16_split_kernel(
    const float* __restrict__ q, int ldq, const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
    const int32_t* __restrict__ cache_len, int len_bias, int n_heads, int S_max, int n_split, float* __restrict__ partial) {
    const int bh = blockIdx.y, b = bh / n_heads, head = bh - b * n_heads;
    const int split = blockIdx.x;
    float M, L, O;
    ring_range<uint16_t, NW, D, false, true, false>(q + (int64_t)b * ldq + head * HD, kc + (int64_t)bh * S_max * HD,
                                       vc + (int64_t)bh * S_max * HD, S_max, [&] {
                                           const int len = min(cache_len[b] + len_bias, S_max);   // (never a row beyond the allocation)
                                           const int nchunks = (len + 31) / 32;
                                           const int cps = (nchunks + n_split - 1) / n_split;
                                           const int c_begin = split * cps;
                                           return KeyRange{len, c_begin, min(nchunks, c_begin + cps)};
                                       }, M, L, O);
    const int tid = threadIdx.x;
    if (tid < HD) write_record(partial + ((int64_t)bh * n_split + split) * PART_LD, tid, O, M, L);
}

// fp32 cache rows -> bf16 cache rows (round to nearest even): the prompt pass runs in fp32, its K/V are narrowed once
__global__ __launch_bounds__(256) void kv_to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst,
                                                         int rows, int64_t src_stride, int64_t dst_stride) {
    const int stream = blockIdx.y;
    const float* s = src + (int64_t)stream * src_stride;
    uint16_t* d = dst + (int64_t)stream * dst_stride;
    const int64_t n8 = (int64_t)rows * HD / 8;
    for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const f32x4 a = ld4(s + 8 * i), c = ld4(s + 8 * i + 4);
        u32x4 o;
        o.x = vh_pack_h16(a.x, a.y); o.y = vh_pack_h16(a.z, a.w);
        o.z = vh_pack_h16(c.x, c.y); o.w = vh_pack_h16(c.z, c.w);
        *reinterpret_cast<u32x4*>(d + 8 * i) = o;
    }
}

extern "C" int vh_kv_to_bf16(const float* src, uint16_t* dst, int n_streams, int rows, int S_src, int S_dst, void* stream) {
    VH_REQUIRE(src && dst && n_streams > 0 && rows >= 0 && rows <= S_src && rows <= S_dst, VH_EINVAL,
               "vh_kv_to_bf16: n_streams=%d rows=%d S_src=%d S_dst=%d", n_streams, rows, S_src, S_dst);
    VH_REQUIRE(vh_aligned16(src) && vh_aligned16(dst), VH_EALIGN, "vh_kv_to_bf16: pointers must be 16-byte aligned");
    if (rows == 0) return VH_OK;
    const int bx = (int)min((int64_t)64, ((int64_t)rows * HD / 8 + 255) / 256);
    hipLaunchKernelGGL(kv_to_bf16_kernel, dim3(bx, n_streams), dim3(256), 0, (hipStream_t)stream, src, dst, rows,
                       (int64_t)S_src * HD, (int64_t)S_dst * HD);
    VH_CHECK_LAUNCH("vh_kv_to_bf16");
    return VH_OK;
}

// The single-query kernels above are instantiated here, in this order, and so lie in the code object where they always have:
// the launcher that names them (attn_launch) is at the end of the file, behind the backward kernels.  (Instantiated from there
// they moved behind attn_bwd_fused_kernel and bench.py read 0.35 % lower in three alternating runs, 49216 against 49388
// tokens/s; in this order the .text section is the same bytes as before the launcher moved and the runs agree.)
[[maybe_unused]] static const void* const ATTN_DECODE_KERNEL_ORDER[] = {
    (const void*)attn_decode_ring16_kernel<8, 2>, (const void*)attn_decode_ring16_split_kernel<8, 2>,
    (const void*)attn_decode_ring16_split_kernel<4, 2>, (const void*)attn_decode_ring_kernel<8, 2>,
    (const void*)attn_decode_kernel<16>, (const void*)attn_decode_kernel<8>, (const void*)attn_decode_kernel<4>};

// =============================================================================================
// many-row attention
// =============================================================================================
#define QB 128   // queries per block (4 waves x 32)
#define KT 32    // keys per tile
#define KLD 68   // LDS row stride (floats): 17 x 16-B slots → conflict-free ds_read_b128 by row

struct RowsArgs {
    const float* q; int ldq;
    const float* kc; const float* vc;
    float* out; int ldo;
    int n_heads, Tq, Tk, S_max, mode, x_len;
    const int32_t* x_len_dev; const int32_t* kv_len;
    const uint8_t* mask; const uint8_t* pad;
    int n_qblocks;
    float* lse2;   // optional (B, h, Tq): log2-sum-exp of the scaled scores, for the backward kernels
    int64_t mask_bstride;   // explicit mode: elements between the masks of consecutive batch rows (0: one (Tq,Tk) mask for all)
};

// The segments of vh_attn_rows_packed: utterance s owns rows seg_start[s] .. seg_start[s] + seg_len[s] - 1 of ONE (M, ·) q / out
// and of one (1, h, S_max, 64) K/V stream; blocks[2 i], blocks[2 i + 1] = (segment, first query inside it) of workgroup row i.
struct PackedSegs {
    const int32_t* seg_start; const int32_t* seg_len; const int32_t* blocks;
    int n_seg, n_rows;            // n_rows: the cache's S_max — no segment row at or beyond it is touched
};

#define ATTN_ROWS_PACKED 0
#include "attn_rows_body.inc"       // attn_rows_kernel(RowsArgs)
#undef ATTN_ROWS_PACKED
#define ATTN_ROWS_PACKED 1
#include "attn_rows_body.inc"       // attn_rows_packed_kernel(RowsArgs, PackedSegs)
#undef ATTN_ROWS_PACKED

static int attn_rows_launch(const float* q, int ldq, const float* kcache, const float* vcache,
                            float* out, int ldo, int B, int n_heads, int Tq, int Tk, int S_max,
                            int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len,
                            const uint8_t* mask, const uint8_t* pad, float* lse2, void* stream, int64_t mask_bstride = 0) {
    VH_REQUIRE(q && kcache && vcache && out, VH_EINVAL, "vh_attn_rows: null pointer");
    VH_REQUIRE(B >= 0 && n_heads > 0 && Tq >= 0 && Tk >= Tq && S_max >= Tk, VH_EINVAL,
               "vh_attn_rows: bad dims B=%d h=%d Tq=%d Tk=%d S_max=%d", B, n_heads, Tq, Tk, S_max);
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX || mode == VH_MASK_EXPLICIT, VH_EINVAL,
               "vh_attn_rows: mode=%d", mode);
    VH_REQUIRE(mode != VH_MASK_EXPLICIT || mask, VH_EINVAL, "vh_attn_rows: explicit mode needs mask");
    VH_REQUIRE(ldq % 4 == 0 && ldo % 4 == 0 && ldq >= n_heads * HD && ldo >= n_heads * HD, VH_EINVAL,
               "vh_attn_rows: ldq=%d ldo=%d", ldq, ldo);
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(kcache) && vh_aligned16(vcache) && vh_aligned16(out),
               VH_EALIGN, "vh_attn_rows: pointers must be 16-byte aligned");
    if (B == 0 || Tq == 0) return VH_OK;
    const int nqb = (Tq + QB - 1) / QB;
    RowsArgs a{q, ldq, kcache, vcache, out, ldo, n_heads, Tq, Tk, S_max, mode, x_len,
               x_len_dev, kv_len, mask, pad, nqb, lse2, mask_bstride};
    dim3 grid(nqb * B * n_heads);
    hipLaunchKernelGGL(attn_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    VH_CHECK_LAUNCH("vh_attn_rows");
    return VH_OK;
}

extern "C" int vh_attn_rows(const float* q, int ldq, const float* kcache, const float* vcache,
                            float* out, int ldo, int B, int n_heads, int Tq, int Tk, int S_max,
                            int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len,
                            const uint8_t* mask, const uint8_t* pad, void* stream) {
    return attn_rows_launch(q, ldq, kcache, vcache, out, ldo, B, n_heads, Tq, Tk, S_max, mode, x_len,
                            x_len_dev, kv_len, mask, pad, nullptr, stream);
}

extern "C" int vh_attn_rows_bmask(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo, int B,
                                  int n_heads, int Tq, int Tk, int S_max, const uint8_t* mask, int64_t mask_batch_stride,
                                  const uint8_t* pad, void* stream) {
    VH_REQUIRE(mask && (mask_batch_stride == 0 || mask_batch_stride >= (int64_t)Tq * Tk), VH_EINVAL,
               "vh_attn_rows_bmask: a (B,Tq,Tk) mask with batch stride >= Tq*Tk (or 0: one mask for every row), got %lld",
               (long long)mask_batch_stride);
    return attn_rows_launch(q, ldq, kcache, vcache, out, ldo, B, n_heads, Tq, Tk, S_max, VH_MASK_EXPLICIT, 0, nullptr, nullptr,
                            mask, pad, nullptr, stream, mask_batch_stride);
}

extern "C" int vh_attn_rows_lse(const float* q, int ldq, const float* kcache, const float* vcache,
                                float* out, int ldo, int B, int n_heads, int Tq, int Tk, int S_max,
                                int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len,
                                const uint8_t* mask, const uint8_t* pad, float* lse2, void* stream) {
    VH_REQUIRE(lse2, VH_EINVAL, "vh_attn_rows_lse: null lse2");
    return attn_rows_launch(q, ldq, kcache, vcache, out, ldo, B, n_heads, Tq, Tk, S_max, mode, x_len,
                            x_len_dev, kv_len, mask, pad, lse2, stream);
}

extern "C" int vh_attn_rows_packed(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                                   int n_heads, int S_max, const int32_t* seg_start, const int32_t* seg_len, int n_seg,
                                   const int32_t* blocks, int n_blocks, void* stream) {
    VH_REQUIRE(q && kcache && vcache && out, VH_EINVAL, "vh_attn_rows_packed: null pointer (q, kcache, vcache or out)");
    VH_REQUIRE(seg_start && seg_len && blocks, VH_EINVAL, "vh_attn_rows_packed: null pointer (seg_start, seg_len or blocks)");
    VH_REQUIRE(n_heads > 0 && S_max >= 1, VH_EINVAL, "vh_attn_rows_packed: bad dims n_heads=%d S_max=%d", n_heads, S_max);
    VH_TRY(vh_packed_attn_sizes("vh_attn_rows_packed", n_heads, n_seg, n_blocks, ldq, ldo, 4));
    VH_REQUIRE(vh_aligned16(q), VH_EALIGN, "vh_attn_rows_packed: q must be 16-byte aligned");
    VH_REQUIRE(vh_aligned16(out), VH_EALIGN, "vh_attn_rows_packed: out must be 16-byte aligned");
    VH_REQUIRE(vh_aligned16(kcache) && vh_aligned16(vcache), VH_EALIGN,
               "vh_attn_rows_packed: kcache and vcache must be 16-byte aligned");
    VH_TRY(vh_packed_workgroups("vh_attn_rows_packed", n_blocks, n_heads));
    RowsArgs a{q, ldq, kcache, vcache, out, ldo, n_heads, 0, 0, S_max, VH_MASK_FULL, 0,
               nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0};
    PackedSegs ps{seg_start, seg_len, blocks, n_seg, S_max};
    hipLaunchKernelGGL(attn_rows_packed_kernel, dim3(n_blocks * n_heads), dim3(256), 0, (hipStream_t)stream, a, ps);
    VH_CHECK_LAUNCH("vh_attn_rows_packed");
    return VH_OK;
}

// =============================================================================================
// many-row attention, backward (training: Tq == Tk).  Two launches, no atomics, P never materialised:
//   dq kernel : one workgroup per 128 queries of a (b,head), queries are lanes (the forward's layout);
//               per 32-key tile   Sᵀ = K·Qᵀ,  P = exp2(Sᵀ − lse),  dPᵀ = V·dOᵀ,  dSᵀ = P∘(dPᵀ − D),
//               dQᵀ += Kᵀ·dSᵀ   (D[q] = Σ_d dO[q][d]·O[q][d], lane-local, also written out for the next kernel)
//   dkv kernel: one workgroup per 128 keys, keys are lanes; per 32-query tile
//               S = Q·Kᵀ, P, dP = dO·Vᵀ, dS as above (lse, D per register now),  dVᵀ += dOᵀ·P,  dKᵀ += Qᵀ·dS
// In both, the accumulator of the first product IS the B operand of the last (no shuffle, no LDS trip).
// =============================================================================================
struct BwdArgs {
    const float* q; int ldq;          // (B*T, ldq), head h at columns h*64
    const float* kc; const float* vc; // (B, h, S_max, 64)
    const float* o; int ldo;          // forward output (B*T, ldo)
    const float* dout; int lddo;      // its gradient
    const float* lse2;                // (B, h, T) from vh_attn_rows_lse
    float* dsum;                      // (B, h, T): D, written by the dq kernel, read by the dkv kernel
    float* dq; float* dk; float* dv; int ldg;   // gradients, each (B*T, ldg) with head h at columns h*64
    int n_heads, T, S_max, mode, x_len;
    const int32_t* x_len_dev; const int32_t* kv_len;
    const uint8_t* mask; const uint8_t* pad;
    int n_blocks;
    float* slab;                      // fused form: dQ partial sums, (n_blocks, B*h, T, 64); null = one key chunk, dq written directly
    int chunk_keys;                   // fused form: keys per workgroup (a multiple of 32, <= 256)
};

__device__ __forceinline__ bool bwd_visible(const BwdArgs& a, int b, int qi, int key, int kvl, int xl) {
    if (a.mode == VH_MASK_EXPLICIT)
        return key < a.T && qi < a.T && !a.mask[(int64_t)qi * a.T + key] && !(a.pad && a.pad[(int64_t)b * a.T + key]);
    bool vis = key < kvl;
    if (a.mode == VH_MASK_PREFIX) vis = vis && (key < xl || (qi >= xl && key <= qi));
    return vis;
}

__global__ __launch_bounds__(256, 2) void attn_bwd_dq_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * KT * KLD];   // [buf][K|V][key][KLD]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int n_bh = gridDim.x / a.n_blocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int q0 = (a.n_blocks - 1 - (int)(blockIdx.x / n_bh)) * QB;      // heaviest query blocks first
    const int kvl = a.kv_len ? min(a.kv_len[b], a.T) : a.T;
    const int xl = a.x_len_dev ? a.x_len_dev[b] : a.x_len;
    const int last_pos = min(q0 + QB, a.T) - 1;
    int kmax = kvl;
    if (a.mode == VH_MASK_PREFIX) kmax = min(kvl, max(xl, last_pos >= xl ? last_pos + 1 : 0));
    if (a.mode == VH_MASK_EXPLICIT) kmax = a.T;
    const int n_tiles = (kmax + KT - 1) / KT;

    const int qi = q0 + w * 32 + r;
    const bool qin = qi < a.T;
    const float qscale = 0.125f * LOG2E;
    f32x4 qf[8], df[8];
    float dsum = 0.f;
    {
        const int64_t row = (int64_t)b * a.T + min(qi, a.T - 1);
        const float* qp = a.q + row * a.ldq + head * HD + 4 * h;
        const float* dp = a.dout + row * a.lddo + head * HD + 4 * h;
        const float* op = a.o + row * a.ldo + head * HD + 4 * h;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            qf[t] = ld4(qp + 8 * t) * qscale;
            df[t] = ld4(dp + 8 * t);
            const f32x4 ov = ld4(op + 8 * t);
            dsum += (df[t].x * ov.x + df[t].y * ov.y) + (df[t].z * ov.z + df[t].w * ov.w);
        }
    }
    dsum += __shfl_xor(dsum, 32, 64);
    const float lse = a.lse2[(int64_t)bh * a.T + min(qi, a.T - 1)];
    if (h == 0 && qin) a.dsum[(int64_t)bh * a.T + qi] = dsum;

    const float* kb = a.kc + (int64_t)bh * a.S_max * HD;
    const float* vb = a.vc + (int64_t)bh * a.S_max * HD;
    const int skey = tid >> 4, squad = (tid & 15) * 4;
    f32x4 rk[2], rv[2];
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {                          // keys clamped (masked anyway); uniform base + 32-bit lane offset
            const uint32_t off = (uint32_t)(min(k0 + skey + 16 * i, a.T - 1) * HD + squad) * 4u;
            rk[i] = ld4((const float*)((const char*)kb + off));
            rv[i] = ld4((const float*)((const char*)vb + off));
        }
    };
    auto lstore = [&](int buf) {
        float* kd = lds + buf * (2 * KT * KLD);
        float* vd = kd + KT * KLD;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            st4(kd + (skey + 16 * i) * KLD + squad, rk[i]);
            st4(vd + (skey + 16 * i) * KLD + squad, rv[i]);
        }
    };
    f32x16 G0, G1;                      // dQᵀ halves: d = r and r + 32
#pragma unroll
    for (int e = 0; e < 16; ++e) { G0[e] = 0.f; G1[e] = 0.f; }
    const int wpos_min = q0 + w * 32, wpos_max = wpos_min + 31;
    if (n_tiles > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    for (int kt = 0; kt < n_tiles; ++kt) {
        const int cur = kt & 1, k0 = kt * KT;
        if (kt + 1 < n_tiles) gload(k0 + KT);
        bool any = k0 < kvl;
        if (a.mode == VH_MASK_PREFIX) any = any && (k0 < xl || (wpos_max >= xl && k0 <= wpos_max));
        else if (a.mode == VH_MASK_EXPLICIT) any = true;
        if (any) {
            const float* ks = lds + cur * (2 * KT * KLD);
            const float* vs = ks + KT * KLD;
            f32x16 S, P;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const f32x4 kf = ld4(ks + r * KLD + 8 * t + 4 * h);
                const f32x4 vf = ld4(vs + r * KLD + 8 * t + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {      // the first products start from the constant-zero C operand
                    S = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[t][j], (t | j) ? S : f32x16{}, 0, 0, 0);   // Sᵀ[key][q]
                    P = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[j], df[t][j], (t | j) ? P : f32x16{}, 0, 0, 0);   // dPᵀ[key][q]
                }
            }
            // whole tile visible to every query of this wave: no per-element mask (vector compares and selects
            // are MFMA issue slots)
            bool all = wpos_max < a.T && k0 + KT <= kvl;
            if (a.mode == VH_MASK_PREFIX) all = all && (k0 + KT <= xl || (wpos_min >= xl && k0 + KT - 1 <= wpos_min));
            else if (a.mode == VH_MASK_EXPLICIT) all = false;
            if (all) {
#pragma unroll
                for (int e = 0; e < 16; ++e) S[e] = vh_exp2(S[e] - lse) * (P[e] - dsum);   // dSᵀ[key][q]
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    const bool vis = qin && bwd_visible(a, b, qi, key, kvl, xl);
                    const float p = vis ? vh_exp2(S[e] - lse) : 0.f;
                    S[e] = p * (P[e] - dsum);
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float* krow = ks + ((e & 3) + 8 * (e >> 2) + 4 * h) * KLD + r;
                G0 = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[0], S[e], G0, 0, 0, 0);
                G1 = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[32], S[e], G1, 0, 0, 0);
            }
        }
        if (kt + 1 < n_tiles) lstore(cur ^ 1);
        __syncthreads();
    }
    float* ob = lds;                // [128][KLD] transpose buffer
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        f32x4 v0 = {G0[4 * g4], G0[4 * g4 + 1], G0[4 * g4 + 2], G0[4 * g4 + 3]};
        f32x4 v1 = {G1[4 * g4], G1[4 * g4 + 1], G1[4 * g4 + 2], G1[4 * g4 + 3]};
        st4(ob + (w * 32 + r) * KLD + 8 * g4 + 4 * h, v0 * 0.125f);
        st4(ob + (w * 32 + r) * KLD + 32 + 8 * g4 + 4 * h, v1 * 0.125f);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = skey + 16 * i;
        if (q0 + row < a.T)
            st4(a.dq + ((int64_t)b * a.T + q0 + row) * a.ldg + head * HD + squad, ld4(ob + row * KLD + squad));
    }
}

__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_kernel(BwdArgs a) {
    // [buf][Q|dO][query][KLD] + [buf][lse|D][32]
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * KT * KLD];
    __shared__ __attribute__((aligned(16))) float stat[2][2][KT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int n_bh = gridDim.x / a.n_blocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int kb0 = (int)(blockIdx.x / n_bh) * QB;                          // first key of this block
    const int kvl = a.kv_len ? min(a.kv_len[b], a.T) : a.T;
    const int xl = a.x_len_dev ? a.x_len_dev[b] : a.x_len;
    // queries that can see a key of this block: all of them for keys < xl (or FULL / EXPLICIT), else q >= key
    int qmin = 0;
    if (a.mode == VH_MASK_PREFIX && kb0 >= xl) qmin = kb0;
    const int t_first = qmin / KT, n_tiles = (a.T + KT - 1) / KT;

    const int kj = kb0 + w * 32 + r;            // this lane's key
    const bool kin = kj < a.T;
    const float qscale = 0.125f * LOG2E;
    f32x4 kf[8], vf[8];
    {
        const float* kp = a.kc + ((int64_t)bh * a.S_max + min(kj, a.T - 1)) * HD + 4 * h;
        const float* vp = a.vc + ((int64_t)bh * a.S_max + min(kj, a.T - 1)) * HD + 4 * h;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            kf[t] = ld4(kp + 8 * t);
            vf[t] = ld4(vp + 8 * t);
        }
    }
    const int sq = tid >> 4, squad = (tid & 15) * 4;   // staging: 2 query rows per thread per operand
    f32x4 rq[2], rd[2];
    float rstat = 0.f;
    const float* qbase = a.q + (int64_t)b * a.T * a.ldq + head * HD;
    const float* dbase = a.dout + (int64_t)b * a.T * a.lddo + head * HD;
    auto gload = [&](int q0t) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {                          // uniform (batch row, head) base + 32-bit lane offset
            const int qrow = min(q0t + sq + 16 * i, a.T - 1);
            rq[i] = ld4((const float*)((const char*)qbase + (uint32_t)(qrow * a.ldq + squad) * 4u));
            rd[i] = ld4((const float*)((const char*)dbase + (uint32_t)(qrow * a.lddo + squad) * 4u));
        }
        if (tid < 2 * KT) {
            const int qq = min(q0t + (tid & 31), a.T - 1);
            rstat = (tid < KT ? a.lse2 : a.dsum)[(int64_t)bh * a.T + qq];
        }
    };
    auto lstore = [&](int buf) {
        float* qd = lds + buf * (2 * KT * KLD);
        float* dd = qd + KT * KLD;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            // Q is staged PRE-SCALED, as the forward holds it: S = (c Q) K^T then has the forward's bits (same products, same
            // order), so P = exp2(S - lse2) is the forward's own P.  With c folded into K instead S differs from the forward's
            // by an ulp — 3e-5 at |S| = 290 —, independently per key, and the row sum of dS no longer cancels.
            st4(qd + (sq + 16 * i) * KLD + squad, rq[i] * qscale);
            st4(dd + (sq + 16 * i) * KLD + squad, rd[i]);
        }
        if (tid < 2 * KT) stat[buf][tid >> 5][tid & 31] = rstat;
    };
    f32x16 GK0, GK1, GV0, GV1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { GK0[e] = 0.f; GK1[e] = 0.f; GV0[e] = 0.f; GV1[e] = 0.f; }
    const int wk_min = kb0 + w * 32;
    if (t_first < n_tiles) {
        gload(t_first * KT);
        lstore(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): K / V fragments landed on every path (see attn_bwd_fused_kernel)
    __syncthreads();
    for (int qt = t_first; qt < n_tiles; ++qt) {
        const int cur = (qt - t_first) & 1, q0t = qt * KT;
        if (qt + 1 < n_tiles) gload(q0t + KT);
        bool any = wk_min < kvl;
        if (a.mode == VH_MASK_PREFIX) any = any && (wk_min < xl || q0t + KT - 1 >= wk_min);
        else if (a.mode == VH_MASK_EXPLICIT) any = true;
        if (any) {
            const float* qs = lds + cur * (2 * KT * KLD);
            const float* ds = qs + KT * KLD;
            f32x16 S, P;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const f32x4 qv = ld4(qs + r * KLD + 8 * t + 4 * h);
                const f32x4 dv = ld4(ds + r * KLD + 8 * t + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    S = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[j], kf[t][j], (t | j) ? S : f32x16{}, 0, 0, 0);   // S[q][key]
                    P = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[j], vf[t][j], (t | j) ? P : f32x16{}, 0, 0, 0);   // dP[q][key]
                }
            }
            // every (query of the tile, key of this wave) pair visible: no per-element mask
            const int wk_max = wk_min + 31;
            bool all = wk_max < kvl && q0t + KT <= a.T;
            if (a.mode == VH_MASK_PREFIX) all = all && (wk_max < xl || (q0t >= xl && wk_max <= q0t));
            else if (a.mode == VH_MASK_EXPLICIT) all = false;
            if (all) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4 lse4 = ld4(&stat[cur][0][8 * g4 + 4 * h]);
                    const f32x4 d4 = ld4(&stat[cur][1][8 * g4 + 4 * h]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int e = 4 * g4 + j;
                        const float p = vh_exp2(S[e] - lse4[j]);
                        S[e] = p;                                   // P[q][key]
                        P[e] = p * (P[e] - d4[j]);                  // dS[q][key]
                    }
                }
            } else {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4 lse4 = ld4(&stat[cur][0][8 * g4 + 4 * h]);
                    const f32x4 d4 = ld4(&stat[cur][1][8 * g4 + 4 * h]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int e = 4 * g4 + j;
                        const int qi = q0t + 8 * g4 + 4 * h + j;
                        const bool vis = kin && qi < a.T && bwd_visible(a, b, qi, kj, kvl, xl);
                        const float p = vis ? vh_exp2(S[e] - lse4[j]) : 0.f;
                        S[e] = p;
                        P[e] = p * (P[e] - d4[j]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int qrow = (e & 3) + 8 * (e >> 2) + 4 * h;
                const float* dorow = ds + qrow * KLD + r;
                const float* qrowp = qs + qrow * KLD + r;
                GV0 = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow[0], S[e], GV0, 0, 0, 0);    // dVᵀ[d][key]
                GV1 = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow[32], S[e], GV1, 0, 0, 0);
                GK0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qrowp[0], P[e], GK0, 0, 0, 0);    // dKᵀ[d][key]
                GK1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qrowp[32], P[e], GK1, 0, 0, 0);
            }
        }
        if (qt + 1 < n_tiles) lstore(cur ^ 1);
        __syncthreads();
    }
    float* ob = lds;
    for (int which = 0; which < 2; ++which) {
        const f32x16& A0 = which ? GV0 : GK0;
        const f32x16& A1 = which ? GV1 : GK1;
        const float sc = which ? 1.0f : 0.125f / qscale;       // dK was added up over the pre-scaled Q rows
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            f32x4 v0 = {A0[4 * g4], A0[4 * g4 + 1], A0[4 * g4 + 2], A0[4 * g4 + 3]};
            f32x4 v1 = {A1[4 * g4], A1[4 * g4 + 1], A1[4 * g4 + 2], A1[4 * g4 + 3]};
            st4(ob + (w * 32 + r) * KLD + 8 * g4 + 4 * h, v0 * sc);
            st4(ob + (w * 32 + r) * KLD + 32 + 8 * g4 + 4 * h, v1 * sc);
        }
        __syncthreads();
        float* dst = which ? a.dv : a.dk;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = sq + 16 * i;
            if (kb0 + row < a.T)
                st4(dst + ((int64_t)b * a.T + kb0 + row) * a.ldg + head * HD + squad, ld4(ob + row * KLD + squad));
        }
        __syncthreads();
    }
}

// =============================================================================================
// many-row attention, backward, FIVE products in one kernel (round 4).  The keys-as-lanes kernel above already holds
// dS[q][key] in registers; dQ = dS·K contracts over the key, which is the LANE index of those registers, so the
// two-kernel form recomputes S and dP in a second kernel with queries as lanes (7 products).  Here dS makes one trip
// through LDS instead: a workgroup of 8 waves owns a chunk of up to 256 keys (K transposed into LDS once per
// workgroup), every wave writes its 32 x 32 block of dS into a shared [32 q][256 keys] tile, and after a barrier each
// wave computes ONE 16 x 16 block of the tile's dQ (4 d-blocks x 2 q-blocks = 8 waves) over ALL the chunk's keys on
// mfma_f32_16x16x4 — no cross-wave reduction.  Both operands are read with ds_read_b128: four consecutive keys per
// lane (the contraction index of four consecutive MFMAs is permuted accordingly: key(u, g, j) = 16u + 4g + j), rows
// XOR-swizzled by (row & 15) in 16-byte slots, which is conflict-free for the instruction's four 16-lane groups.
// The dQ partial of a (query tile, key chunk) pair goes to slab `chunk` — (n_chunks, B*h, T, 64), T/256 = 4 slabs at the
// training shape — and attn_dq_reduce_kernel adds the slabs in chunk order: bitwise reproducible, no atomics.
// D = rowsum(dO∘O) is computed while the dO / O rows are staged (the dq kernel used to do it).
// =============================================================================================
#define FKMAX 256       // keys per workgroup at most (8 waves x 32)

// FW waves per workgroup = FW x 32 keys per chunk at most.  FW = 8: one workgroup per CU (113 KB of LDS); FW = 4: two per
// CU (65 KB each) — the same eight waves per CU in half-size work items.  The Q / dO tile is single-buffered: every read
// of tile i happens before the tile's first barrier and the staged rows of tile i + 1 are stored after it, so the two
// barriers the dS hand-over needs anyway also order the tile buffer.
#define ATTN_BWD_PACKED 0
#include "attn_bwd_fused_body.inc"   // attn_bwd_fused_kernel<FW>(BwdArgs)
#undef ATTN_BWD_PACKED

// dq[row][head*64 + d] = 1/8 · Σ_chunks slab[chunk][b,head][q][d], chunks in index order; a chunk contributes to a query
// exactly when the fused kernel visited the pair (same rule, so no slab element is read that was not written).
__global__ __launch_bounds__(256) void attn_dq_reduce_kernel(BwdArgs a, int64_t n4) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n4) return;
    const int d4 = (int)(idx & 15);
    const int64_t rh = idx >> 4;
    const int head = (int)(rh % a.n_heads);
    const int64_t row = rh / a.n_heads;
    const int b = (int)(row / a.T), q = (int)(row - (int64_t)b * a.T);
    const int kvl = a.kv_len ? min(a.kv_len[b], a.T) : a.T;
    const int xl = a.x_len_dev ? a.x_len_dev[b] : a.x_len;
    const int64_t n_bh = (int64_t)(n4 / 16 / a.T / a.n_heads) * a.n_heads;   // B * h
    const int bh = b * a.n_heads + head;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < a.n_blocks; ++c) {
        const int kb0 = c * a.chunk_keys;
        if (a.mode != VH_MASK_EXPLICIT && kb0 >= kvl) break;
        if (a.mode == VH_MASK_PREFIX && kb0 >= xl && q < kb0) break;
        acc = acc + ld4(a.slab + (((int64_t)c * n_bh + bh) * a.T + q) * HD + 4 * d4);
    }
    st4(a.dq + row * a.ldg + head * HD + 4 * d4, acc * 0.125f);
}

extern "C" int vh_attn_rows_bwd(const float* q, int ldq, const float* kcache, const float* vcache,
                                const float* out, int ldo, const float* dout, int lddo, const float* lse2,
                                float* dsum, float* dq, float* dk, float* dv, int ldg, int B, int n_heads,
                                int T, int S_max, int mode, int x_len, const int32_t* x_len_dev,
                                const int32_t* kv_len, const uint8_t* mask, const uint8_t* pad, void* stream) {
    VH_REQUIRE(q && kcache && vcache && out && dout && lse2 && dsum && dq && dk && dv, VH_EINVAL,
               "vh_attn_rows_bwd: null pointer");
    VH_REQUIRE(B >= 0 && n_heads > 0 && T >= 0 && S_max >= T, VH_EINVAL,
               "vh_attn_rows_bwd: bad dims B=%d h=%d T=%d S_max=%d", B, n_heads, T, S_max);
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX || (mode == VH_MASK_EXPLICIT && mask), VH_EINVAL,
               "vh_attn_rows_bwd: mode=%d", mode);
    const int wd = n_heads * HD;
    VH_REQUIRE(ldq % 4 == 0 && ldo % 4 == 0 && lddo % 4 == 0 && ldg % 4 == 0 && ldq >= wd && ldo >= wd &&
                   lddo >= wd && ldg >= wd,
               VH_EINVAL, "vh_attn_rows_bwd: leading dimensions");
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(kcache) && vh_aligned16(vcache) && vh_aligned16(out) &&
                   vh_aligned16(dout) && vh_aligned16(dq) && vh_aligned16(dk) && vh_aligned16(dv),
               VH_EALIGN, "vh_attn_rows_bwd: pointers must be 16-byte aligned");
    if (B == 0 || T == 0) return VH_OK;
    const int nb = (T + QB - 1) / QB;
    BwdArgs a{q, ldq, kcache, vcache, out, ldo, dout, lddo, lse2, dsum, dq, dk, dv, ldg,
              n_heads, T, S_max, mode, x_len, x_len_dev, kv_len, mask, pad, nb, nullptr, 0};
    dim3 grid(nb * B * n_heads);
    hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    VH_CHECK_LAUNCH("vh_attn_rows_bwd");
    return VH_OK;
}

// ---- the same gradients with a caller-provided workspace: the five-product kernel + slab reduce (default), or the
// two-kernel form above with its D scratch inside the workspace (VH_TUNE_ATTN_BWD = 1)
// Key chunks per (batch row, head): at least ceil(T / 256) (a workgroup holds 256 keys), more when that evens out the
// launch.  Model, calibrated with tools/sweep_attn_bwd_chunks.py (profiles/r4_sweep_attn_bwd_chunks.log): workgroups are
// dealt one per CU in index order (chunk 0 first) to whichever CU frees up; a workgroup's time is its query tiles x
// 1.0 with 5..8 active 32-key waves (two per SIMD) or x 0.6 with <= 4 (one per SIMD: 10.7 vs 6.5 us per tile); under the
// prefix mask chunk c only sees the query tiles from its first key on; every chunk adds a slab of dQ partials
// (B*h*T*512 bytes written and read at ~5 TB/s).  The launch is simulated for every admissible count (chunks of 97..256
// keys) and the cheapest taken; results are cached per shape.
static int bwd_chunks_model(int bh, int T, bool causal) {
    const int nc_min = (T + FKMAX - 1) / FKMAX, nc_max = max(nc_min, (T + 127) / 128);
    int best = nc_min;
    double best_cost = 1e300;
    const int n_tiles = (T + KT - 1) / KT;
    for (int nc = nc_min; nc <= nc_max; ++nc) {
        const int keys = ((T + nc - 1) / nc + 31) / 32 * 32;
        if ((int64_t)keys * (nc - 1) >= T) continue;                     // the last chunk would be empty
        const double unit = keys > 128 ? 1.0 : (causal ? 0.6 : 0.55);   // <= 128 keys: four active waves (full / explicit masks: the 4-wave kernel, two per CU)
        std::priority_queue<double, std::vector<double>, std::greater<double>> cu;
        for (int i = 0; i < 256; ++i) cu.push(0.0);
        double end = 0.0;
        for (int c = 0; c < nc; ++c) {
            const double work = unit * (causal ? n_tiles - c * keys / KT : n_tiles);
            for (int j = 0; j < bh; ++j) {
                const double t = cu.top() + work;
                cu.pop();
                cu.push(t);
                end = t > end ? t : end;
            }
        }
        const double cost = end + (nc > 1 ? 1e-5 * nc * bh * (double)T : 0.0);
        if (cost < best_cost * (1.0 - 1e-9)) { best_cost = cost; best = nc; }
    }
    return best;
}

static int bwd_chunks(int B, int n_heads, int T, bool causal) {
    const int nc_min = (T + FKMAX - 1) / FKMAX;
    const int forced = vh_tuning(VH_TUNE_ATTN_BWD_CHUNKS);
    if (forced > 0) {
        int nc = max(nc_min, min(forced, (T + 31) / 32));
        while (nc > nc_min && (int64_t)(((T + nc - 1) / nc + 31) / 32 * 32) * (nc - 1) >= T) --nc;   // no empty last chunk
        return nc;
    }
    static std::mutex mu;
    static std::unordered_map<uint64_t, int> cache;
    const uint64_t key = ((uint64_t)(B * n_heads) << 33) | ((uint64_t)T << 1) | (causal ? 1u : 0u);
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    if (cache.size() > 4096) cache.clear();
    return cache[key] = bwd_chunks_model(B * n_heads, T, causal);
}

extern "C" int vh_attn_rows_bwd_chunks(int B, int n_heads, int T, int mode) {
    if (B <= 0 || n_heads <= 0 || T <= 0) return 0;
    return bwd_chunks(B, n_heads, T, mode == VH_MASK_PREFIX);
}

extern "C" size_t vh_attn_rows_bwd_ws_bytes(int B, int n_heads, int T) {
    if (B <= 0 || n_heads <= 0 || T <= 0) return 0;
    const int nc = max(bwd_chunks(B, n_heads, T, false), bwd_chunks(B, n_heads, T, true));   // either mask family fits
    const size_t slabs = nc > 1 ? (size_t)nc * B * n_heads * T * HD * sizeof(float) : 0;
    const size_t dsum = ((size_t)B * n_heads * T * sizeof(float) + 15) & ~(size_t)15;
    return slabs > dsum ? slabs : dsum;
}

extern "C" int vh_attn_rows_bwd_ws(const float* q, int ldq, const float* kcache, const float* vcache,
                                   const float* out, int ldo, const float* dout, int lddo, const float* lse2,
                                   float* dq, float* dk, float* dv, int ldg, int B, int n_heads, int T, int S_max,
                                   int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len,
                                   const uint8_t* mask, const uint8_t* pad, void* ws, size_t ws_bytes, void* stream) {
    VH_REQUIRE(B < 0 || T < 0 || n_heads <= 0 || ws_bytes >= vh_attn_rows_bwd_ws_bytes(B, n_heads, T), VH_EINVAL,
               "vh_attn_rows_bwd_ws: workspace of %zu bytes, need %zu", ws_bytes, vh_attn_rows_bwd_ws_bytes(B, n_heads, T));
    VH_REQUIRE(ws && vh_aligned16(ws), VH_EALIGN, "vh_attn_rows_bwd_ws: workspace must be a 16-byte aligned device pointer");
    if (vh_tuning(VH_TUNE_ATTN_BWD) == 1)
        return vh_attn_rows_bwd(q, ldq, kcache, vcache, out, ldo, dout, lddo, lse2, (float*)ws, dq, dk, dv, ldg, B,
                                n_heads, T, S_max, mode, x_len, x_len_dev, kv_len, mask, pad, stream);
    VH_REQUIRE(q && kcache && vcache && out && dout && lse2 && dq && dk && dv, VH_EINVAL,
               "vh_attn_rows_bwd_ws: null pointer");
    VH_REQUIRE(B >= 0 && n_heads > 0 && T >= 0 && S_max >= T, VH_EINVAL,
               "vh_attn_rows_bwd_ws: bad dims B=%d h=%d T=%d S_max=%d", B, n_heads, T, S_max);
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX || (mode == VH_MASK_EXPLICIT && mask), VH_EINVAL,
               "vh_attn_rows_bwd_ws: mode=%d", mode);
    const int wd = n_heads * HD;
    VH_REQUIRE(ldq % 4 == 0 && ldo % 4 == 0 && lddo % 4 == 0 && ldg % 4 == 0 && ldq >= wd && ldo >= wd &&
                   lddo >= wd && ldg >= wd,
               VH_EINVAL, "vh_attn_rows_bwd_ws: leading dimensions");
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(kcache) && vh_aligned16(vcache) && vh_aligned16(out) &&
                   vh_aligned16(dout) && vh_aligned16(dq) && vh_aligned16(dk) && vh_aligned16(dv),
               VH_EALIGN, "vh_attn_rows_bwd_ws: pointers must be 16-byte aligned");
    if (B == 0 || T == 0) return VH_OK;
    const int nc = bwd_chunks(B, n_heads, T, mode == VH_MASK_PREFIX);
    const int chunk_keys = ((T + nc - 1) / nc + 31) / 32 * 32;       // equal chunks of whole 32-key wave blocks
    BwdArgs a{q, ldq, kcache, vcache, out, ldo, dout, lddo, lse2, nullptr, dq, dk, dv, ldg,
              n_heads, T, S_max, mode, x_len, x_len_dev, kv_len, mask, pad, nc, nc > 1 ? (float*)ws : nullptr, chunk_keys};
    // chunks of <= 128 keys under a uniform mask: the four-wave kernel, two workgroups per CU (NAR step 391 -> 375 us per
    // layer).  Not under the prefix mask: both slots of every CU are filled at once in index order, which pairs the heavy
    // low chunks with each other's neighbours instead of with the light high ones (B = 8: 269 -> 305 us).
    if (chunk_keys <= 128 && mode != VH_MASK_PREFIX)
        hipLaunchKernelGGL(attn_bwd_fused_kernel<4>, dim3(nc * B * n_heads), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(attn_bwd_fused_kernel<8>, dim3(nc * B * n_heads), dim3(512), 0, (hipStream_t)stream, a);
    if (nc > 1) {
        const int64_t n4 = (int64_t)B * T * n_heads * 16;
        hipLaunchKernelGGL(attn_dq_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, n4);
    }
    VH_CHECK_LAUNCH("vh_attn_rows_bwd_ws");
    return VH_OK;
}

// =============================================================================================
// Decode attention over a SHARED PROMPT (round 5): the reference's own generate() replicates ONE utterance over
// num_beams rows (valle/models/valle_ar.py:135-138), so every beam's prompt K/V is the same bits.  Here the prompt K/V
// ("prefix": (1, h, prefix_S, 64) per layer, written once by a one-row prompt pass) is read ONCE per step for all beams
// and every beam keeps only its own generated rows ("suffix": (B, h, S_suf, 64)).  Bytes per step and layer:
// 2 (S0 + B t) d instead of 2 B (S0 + t) d.  Two launches:
//   attn_shared_kernel   workgroups of 4 waves in two roles.  PREFIX role (blocks of 4 x 32 prompt keys, per head): a wave
//                        takes one 32-key block and computes S^T = K Q^T for ALL beams at once — beams are the 32 lanes of a
//                        32x32x2 MFMA tile (a second pass for beams 32..63) — the block's softmax statistics and unnormalised
//                        O^T = V^T P^T, one split record per (beam, head, key block).  SUFFIX role ((beam, head), key split):
//                        the burst kernel over the beam's own rows, one record per split.  The roles share nothing and run
//                        side by side.
//   attn_records_merge_kernel   per (beam, head): all records merged — weights by one parallel pass over the (m, l) pairs,
//                        the o vectors summed by four thread groups over interleaved records, partials added in group
//                        order (deterministic).  (The serial loop of attn_decode_combine_kernel is fine for <= 16 splits;
//                        here there are up to 157 + 64 records, each load a trip beyond the L1.)
// Record format and units as the key-split decode kernels' (PART_LD floats: o[64], m, l; scores scaled by log2 e / 8).
// =============================================================================================
// T: float, or uint16_t for the 16-bit caches of perf mode (vh_attn_decode_shared_kv16) — the prompt's K / V tiles are loaded ONCE
// as 16-bit and widened to fp32 in registers, then go through the same fp32 MFMA score and output products with the beams as lanes
// (q is not rounded: fp32 arithmetic on the rounded cache; a bf16 MFMA would round q: not built); records, merge launch and
// workspace are the fp32 form's.
template <class T>
struct SharedArgs {
    const float* q; int ldq;
    const T* kp; const T* vp;                    // prefix (1, h, prefix_S, 64)
    int prefix_len, prefix_S;
    const T* ks; const T* vs;                    // suffix (B, h, S_suf, 64)
    const int32_t* suffix_len; int len_bias;
    int S_suf, n_split;
    float* partial;
    int n_heads, B, n_pb, n_tot, prefix_wgs;     // n_pb: 32-key blocks of the prefix; prefix_wgs = ceil(n_pb / 4) * n_heads
    // grouped form (vh_attn_decode_shared_groups) only: kp / vp are (n_groups, h, prefix_S, 64), group g's prompt holds
    // group_len[g] keys (device array), rows g * beams .. g * beams + beams - 1 are its beams; n_pb counts the blocks of the
    // prefix CAPACITY and prefix_wgs = ceil(n_pb / 4) * n_heads * n_groups.  The other forms: nullptr, 1, B.
    const int32_t* group_len; int n_groups, beams;
};

// what the prefix role fetches differently per cache type: the 32 values kr[0 .. 31] of a key row as the K fragment (16-bit: 64
// bytes = four 16-byte loads, widened), and one V element (16-bit: half the bytes of the fp32 form at the SAME 32 load instructions
// per lane, while K went from eight loads to four — the first thing to look at in a kernel trace of this role)
__device__ __forceinline__ void prefix_k_fragment(const float* kr, f32x4 (&kf)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) kf[j] = ld4(kr + 4 * j);
}
__device__ __forceinline__ void prefix_k_fragment(const uint16_t* kr, f32x4 (&kf)[8]) {
    u32x4 kw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) kw[j] = *reinterpret_cast<const u32x4*>(kr + 8 * j);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        kf[2 * j] = f32x4{BF_LO(kw[j].x), BF_HI(kw[j].x), BF_LO(kw[j].y), BF_HI(kw[j].y)};
        kf[2 * j + 1] = f32x4{BF_LO(kw[j].z), BF_HI(kw[j].z), BF_LO(kw[j].w), BF_HI(kw[j].w)};
    }
}
__device__ __forceinline__ float prefix_v(const float* p) { return *p; }
__device__ __forceinline__ float prefix_v(const uint16_t* p) { return BF_LO((uint32_t)*p); }

// GROUPS = false: the one shared prompt of SharedArgs::prefix_len keys, columns = all B rows.  GROUPS = true: workgroup
// (group, head, four blocks); the prompt, its length and the columns are the group's own.
template <bool GROUPS, class T>
__device__ __forceinline__ void shared_prefix_role(const SharedArgs<T>& a, int wg, int lane, int w) {
    const int head = wg % a.n_heads;
    int blk, grp = 0, plen = a.prefix_len, nb = a.B;
    if constexpr (GROUPS) {
        const int t = wg / a.n_heads;
        grp = t % a.n_groups;
        blk = (t / a.n_groups) * 4 + w;
        plen = min(a.group_len[grp], a.prefix_len);          // (prefix_len holds the capacity; a length beyond it is cut there)
        nb = a.beams;
        // a block wholly beyond the group's own prompt: no load, no record — the merge never reads this group's slots
        // from ceil(plen / 32) on
        if (blk * 32 >= plen) return;
    } else {
        blk = (wg / a.n_heads) * 4 + w;
    }
    if (blk >= a.n_pb) return;                               // (wave-uniform; no barrier in this role)
    const int r = lane & 31, hh = lane >> 5;
    const int row0 = grp * nb;                               // the first of the nb rows that attend this prompt
    const T* kb = a.kp + ((int64_t)grp * a.n_heads + head) * a.prefix_S * HD;
    const T* vb = a.vp + ((int64_t)grp * a.n_heads + head) * a.prefix_S * HD;
    const int k0 = blk * 32;
    const float qscale = 0.125f * LOG2E;
    // K fragment (A operand): key k0 + r, d = 32 hh + j; rows beyond the prompt repeat its last row (masked below).  The k
    // index of the product is only summed over, so both operands simply use the same d per (hh, j).
    f32x4 kf[8];
    prefix_k_fragment(kb + (int64_t)min(k0 + r, plen - 1) * HD + 32 * hh, kf);
    // V^T operand values: product x pairs key base(x) (lanes hh = 0) with base(x) + 4 (lanes hh = 1), base(x) = (x & 3) +
    // 8 (x >> 2) — exactly the keys whose weights sit in accumulator register x of the two lane halves
    float vf[2][16];
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        const int key = min(k0 + (x & 3) + 8 * (x >> 2) + 4 * hh, plen - 1);
        vf[0][x] = prefix_v(vb + (int64_t)key * HD + r);
        vf[1][x] = prefix_v(vb + (int64_t)key * HD + 32 + r);
    }
    const bool whole = k0 + 32 <= plen;                      // wave-uniform
    for (int qb = 0; qb * 32 < nb; ++qb) {
        const int b = row0 + min(qb * 32 + r, nb - 1);       // lanes beyond the beams repeat the last one (never stored)
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
        {
            const float* qr = a.q + (int64_t)b * a.ldq + head * HD + 32 * hh;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 qf = ld4(qr + 4 * j) * qscale;
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j].x, qf.x, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j].y, qf.y, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j].z, qf.z, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j].w, qf.w, s, 0, 0, 0);
            }
        }
        // D reg x of lane (r = beam, hh): key k0 + (x & 3) + 8 (x >> 2) + 4 hh
        float m = NEG_INF;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            if (!whole && k0 + (x & 3) + 8 * (x >> 2) + 4 * hh >= plen) s[x] = NEG_INF;
            m = fmaxf(m, s[x]);
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));                 // the beam's other key half; finite: key k0 < prefix_len
        float l = 0.f;
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            s[x] = vh_exp2(s[x] - m);
            l += s[x];
        }
        l += __shfl_xor(l, 32, 64);
        f32x16 o0, o1;
#pragma unroll
        for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
#pragma unroll
        for (int x = 0; x < 16; ++x) {                       // O^T += V^T P^T: P^T is the B operand as it lies
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[0][x], s[x], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[1][x], s[x], o1, 0, 0, 0);
        }
        if (qb * 32 + r < nb) {
            float* pr = a.partial + (((int64_t)b * a.n_heads + head) * a.n_tot + blk) * PART_LD;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                st4(pr + 8 * g4 + 4 * hh, f32x4{o0[4 * g4], o0[4 * g4 + 1], o0[4 * g4 + 2], o0[4 * g4 + 3]});
                st4(pr + 32 + 8 * g4 + 4 * hh, f32x4{o1[4 * g4], o1[4 * g4 + 1], o1[4 * g4 + 2], o1[4 * g4 + 3]});
            }
            if (hh == 0) { pr[HD] = m; pr[HD + 1] = l; }
        }
    }
}

template <bool GROUPS, class T>
__device__ __forceinline__ void attn_shared_body(const SharedArgs<T>& a) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if ((int)blockIdx.x < a.prefix_wgs) {                    // workgroup-uniform
        shared_prefix_role<GROUPS>(a, blockIdx.x, lane, w);
        return;
    }
    // ---- suffix role: (beam, head) x key split over the beam's own rows: a 4 x 2 ring without speculative bursts (non-temporal
    // loads: the beams' rows must not evict the weights)
    const int unit = blockIdx.x - a.prefix_wgs;
    const int split = unit % a.n_split, bh = unit / a.n_split;
    const int b = bh / a.n_heads, head = bh - b * a.n_heads;
    // a parked group (prefix length <= 0): its rows attend nothing — no load of q, K or V, no record (workgroup-uniform,
    // before the barrier below; the merge writes the rows' zeros without reading a slot)
    if constexpr (GROUPS) {
        if (a.group_len[b / a.beams] <= 0) return;
    }
    constexpr bool is16 = std::is_same<T, uint16_t>::value;   // (the roundings the two forms have always had: ring_range)
    float M, L, O;
    ring_range<T, 4, 2, false, is16, is16>(a.q + (int64_t)b * a.ldq + head * HD, a.ks + (int64_t)bh * a.S_suf * HD,
                               a.vs + (int64_t)bh * a.S_suf * HD, a.S_suf, [&] {
                                   int len = a.suffix_len[b] + a.len_bias;
                                   // (the 16-bit form alone cuts the length at the allocation; kept as each form had it)
                                   if constexpr (!std::is_same<T, float>::value) len = min(len, a.S_suf);
                                   const int nchunks = (len + 31) >> 5;
                                   const int cps = (nchunks + a.n_split - 1) / a.n_split;
                                   const int c_begin = split * cps;
                                   return KeyRange{len, c_begin, min(nchunks, c_begin + cps)};
                               }, M, L, O);
    if (tid < HD) write_record(a.partial + ((int64_t)bh * a.n_tot + a.n_pb + split) * PART_LD, tid, O, M, L);
}

__global__ __launch_bounds__(256) void attn_shared_kernel(SharedArgs<float> a) { attn_shared_body<false>(a); }
// several utterances' beams, each group over its own prompt (vh_attn_decode_shared_groups)
__global__ __launch_bounds__(256) void attn_shared_groups_kernel(SharedArgs<float> a) { attn_shared_body<true>(a); }
// 16-bit caches (vh_attn_decode_shared_kv16)
__global__ __launch_bounds__(256) void attn_shared16_kernel(SharedArgs<uint16_t> a) { attn_shared_body<false>(a); }

// out[b, head] = merge of the n_tot records of (b, head).  256 threads: one parallel pass over the (m, l) pairs gives the
// weights and the denominator; thread group g = tid >> 6 then sums records g, g + 4, ... of column tid & 63 (independent
// loads, issued back to back) and the four partial sums are added in group order.
//
// The grouped form keeps n_slots = n_pb + n_split slots per (b, head), n_pb the blocks of the prefix CAPACITY, of which row
// b's group wrote only its own n_first = ceil(group_len / 32) prefix records and the n_split suffix records.  The merge runs
// over those n_tot = n_first + n_split records alone — record k lives in slot k, or from the first suffix record on in slot
// k + (unwritten slots) — so an unwritten slot is never loaded (the workspace is not initialised, and a zero weight would
// not stop a NaN).  The other forms: n_slots = n_first = n_tot, slot k is record k.
__device__ __forceinline__ void records_merge_body(const float* __restrict__ partial, float* __restrict__ out, int ldo,
                                                   int n_heads, int n_tot, int n_slots, int n_first) {
    __shared__ float s_w[256], s_red[8], s_part[4][HD];
    const int bh = blockIdx.x, b = bh / n_heads, head = bh - b * n_heads;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* pr = partial + (int64_t)bh * n_slots * PART_LD;
    const int skip = n_slots - n_tot;
    auto slot = [&](int k) { return k < n_first ? k : k + skip; };
    // ONE memory round trip: the (m, l) pair of record tid and the first eight o values of this thread's column (records
    // w, w + 4, ..., w + 28) are requested together — the o values do not depend on the weights
    const bool have = tid < n_tot;
    const float mk = have ? pr[slot(tid) * PART_LD + HD] : NEG_INF;
    const float lk = have ? pr[slot(tid) * PART_LD + HD + 1] : 0.f;
    float a8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) a8[j] = pr[slot(min(w + 4 * j, n_tot - 1)) * PART_LD + lane];
    const float wm = wave_max(mk);
    if (lane == 0) s_red[w] = wm;
    __syncthreads();
    const float M = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));   // finite: the prefix holds >= 1 key
    const float wk = mk == NEG_INF ? 0.f : vh_exp2(mk - M);
    s_w[tid] = wk;                                           // (0 beyond n_tot: the clamped loads above weigh nothing)
    const float ws = wave_sum(lk * wk);
    if (lane == 0) s_red[4 + w] = ws;
    __syncthreads();
    const float L = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += a8[j] * s_w[w + 4 * j];
    for (int k = w + 32; k < n_tot; k += 16) {               // longer prompts: four more independent loads per pass
        const float a0 = pr[slot(k) * PART_LD + lane], a1 = pr[slot(min(k + 4, n_tot - 1)) * PART_LD + lane];
        const float a2 = pr[slot(min(k + 8, n_tot - 1)) * PART_LD + lane], a3 = pr[slot(min(k + 12, n_tot - 1)) * PART_LD + lane];
        acc += a0 * s_w[k];
        acc += a1 * s_w[min(k + 4, 255)];
        acc += a2 * s_w[min(k + 8, 255)];
        acc += a3 * s_w[min(k + 12, 255)];
    }
    s_part[w][lane] = acc;
    __syncthreads();
    if (tid < HD) out[(int64_t)b * ldo + head * HD + tid] = ((s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid])) / L;
}

__global__ __launch_bounds__(256) void attn_records_merge_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                 int ldo, int n_heads, int n_tot) {
    records_merge_body(partial, out, ldo, n_heads, n_tot, n_tot, n_tot);
}

__global__ __launch_bounds__(256) void attn_records_merge_groups_kernel(const float* __restrict__ partial, float* __restrict__ out,
                                                                        int ldo, int n_heads, int n_pb, int n_split,
                                                                        const int32_t* __restrict__ group_len, int beams) {
    const int b = blockIdx.x / n_heads;
    const int glen = group_len[b / beams];
    if (glen <= 0) {
        // a parked group wrote no record at all: exactly 0.0 for its rows and no slot read (records_merge_body would divide
        // by a denominator built from slots nobody wrote)
        if (threadIdx.x < HD) out[(int64_t)b * ldo + (blockIdx.x - b * n_heads) * HD + threadIdx.x] = 0.f;
        return;
    }
    const int n_first = min((glen + 31) >> 5, n_pb);         // the prefix records this row's group wrote (cut at the capacity
                                                             // as the prefix role cuts)
    records_merge_body(partial, out, ldo, n_heads, n_first + n_split, n_pb + n_split, n_first);
}

// =============================================================================================
// decode attention, host side: one call record (vh_common.h), one check, one plan, one launcher.  The seven vh_attn_decode*
// entry points and the decoder (plan.hip) fill a DecodeAttnCall; vh_attn_decode_form asks the same check and plan and
// launches nothing (tests/golden/attn_decode_forms.txt pins what they answer).
// =============================================================================================
#define ATTN_MAX_RECORDS 256   // records of a (row, head) one merge launch serves (records_merge_body: one thread per record)

typedef vh_attn_decode_form_info AttnForm;
struct AttnKnobs { int variant, waves, combine; };   // VH_TUNE_DECODE_VARIANT, _WAVES, _COMBINE

int vh_internal_attn_hd_record_floats(int hd);                                                          // attention_hd.hip
bool vh_internal_attn_decode_hd_launch(const AttnForm& f, const DecodeAttnCall& c, hipEvent_t start, hipEvent_t stop);   // attention_hd.hip

// start / stop events attached to the first kernel's own dispatch packet (hipExtLaunchKernelGGL), i.e. the kernel's begin /
// end timestamps rather than a marker bracket; set only by vh_ar_decoder_profile_attn
static thread_local hipEvent_t g_attn_ev[2] = {nullptr, nullptr};
void vh_internal_attn_decode_events(hipEvent_t start, hipEvent_t stop) { g_attn_ev[0] = start; g_attn_ev[1] = stop; }

// split records per (row, head): a shared prompt leaves one per 32-key block of the prefix (of the prefix CAPACITY with groups)
// and one per suffix split; without one a key split leaves one per split, and an unsplit call none
static int attn_records(const DecodeAttnCall& c) {
    return c.prefix_kind ? (c.prefix + 31) / 32 + c.n_split : c.n_split > 1 ? c.n_split : 0;
}
static int attn_record_floats(const DecodeAttnCall& c) { return c.any_width ? vh_internal_attn_hd_record_floats(c.head_dim) : PART_LD; }
// workspace: [B h][records] records; the width-64 key splits then keep B h ticket words (one per (b, head), padded to 16 B),
// whichever way this call combines its records
static size_t attn_records_bytes(const DecodeAttnCall& c) {
    return (size_t)c.B * c.n_heads * attn_records(c) * attn_record_floats(c) * sizeof(float);
}
static size_t attn_ws_bytes(const DecodeAttnCall& c) {
    const size_t rec = attn_records_bytes(c);
    const bool tickets = rec && !c.prefix_kind && !c.any_width;
    return rec + (tickets ? ((size_t)c.B * c.n_heads * sizeof(unsigned) + 15) / 16 * 16 : 0);
}

int vh_internal_attn_decode_check(const DecodeAttnCall& c, bool pointers) {
    const bool prefix = c.prefix_kind != ATTN_PREFIX_NONE, groups = c.prefix_kind == ATTN_PREFIX_GROUPS;
    VH_REQUIRE(!c.any_width || (c.head_dim % 4 == 0 && c.head_dim >= 16 && c.head_dim <= VH_HEAD_DIM_MAX), VH_EUNSUPPORTED,
               "%s: head_dim=%d (served: multiples of 4 from 16 to %d)", c.name, c.head_dim, VH_HEAD_DIM_MAX);
    // a shared prompt always leaves records: its workspace is one of the pointers
    VH_REQUIRE(!pointers || (c.q && c.k && c.v && c.out && c.len && (!prefix || (c.kprefix && c.vprefix && c.ws)) &&
                             (!groups || c.group_len)), VH_EINVAL, "%s: null pointer", c.name);
    VH_REQUIRE(c.B > 0 && c.n_heads > 0 && c.S_max > 0, VH_EINVAL, "%s: bad dims B=%d h=%d S_max=%d", c.name, c.B, c.n_heads, c.S_max);
    // the rows of a shared prompt are the columns of one score tile (two passes of 32)
    VH_REQUIRE(!prefix || (c.B <= 64 && c.prefix > 0 && c.prefix <= c.prefix_S), VH_EINVAL,
               "%s: bad dims B=%d (1..64 rows over a shared prompt) %s=%d/%d", c.name, c.B, groups ? "prefix_cap" : "prefix", c.prefix,
               c.prefix_S);
    const int max_split = c.kv16 ? 16 : 64;
    VH_REQUIRE(c.n_split >= 1 && c.n_split <= max_split, VH_EINVAL, "%s: n_split=%d (1..%d)", c.name, c.n_split, max_split);
    VH_REQUIRE(!groups || (c.beams >= 1 && c.B % c.beams == 0), VH_EINVAL,
               "%s: B=%d is not a multiple of beams=%d (the rows of a group)", c.name, c.B, c.beams);
    VH_REQUIRE(!prefix || attn_records(c) <= ATTN_MAX_RECORDS, VH_EUNSUPPORTED,
               "%s: %d prefix blocks + %d splits exceed the %d records one merge serves", c.name, attn_records(c) - c.n_split,
               c.n_split, ATTN_MAX_RECORDS);
    VH_REQUIRE(c.len_bias == 0 || c.len_bias == 1, VH_EINVAL, "%s: len_bias=%d", c.name, c.len_bias);
    const int width = c.n_heads * c.head_dim;
    VH_REQUIRE(c.ldq % 4 == 0 && c.ldq >= width && c.ldo >= width, VH_EINVAL, "%s: ldq=%d ldo=%d", c.name, c.ldq, c.ldo);
    // (the fp32 forms without a shared prompt have never looked at the workspace's alignment)
    VH_REQUIRE(!pointers || (vh_aligned16(c.q) && vh_aligned16(c.k) && vh_aligned16(c.v) && vh_aligned16(c.kprefix) &&
                             vh_aligned16(c.vprefix) && (vh_aligned16(c.ws) || !(prefix || c.kv16))), VH_EALIGN,
               "%s: pointers must be 16-byte aligned", c.name);
    const size_t need = attn_ws_bytes(c);
    VH_REQUIRE(need == 0 || (c.ws && (c.ws_bytes == ATTN_WS_SIZE_NOT_GIVEN || c.ws_bytes >= need)), VH_EINVAL,
               "%s: n_split=%d needs a workspace (%s) of %zu bytes (got %zu)", c.name, c.n_split, c.ws_name, need,
               c.ws && c.ws_bytes != ATTN_WS_SIZE_NOT_GIVEN ? c.ws_bytes : (size_t)0);
    return VH_OK;
}

// Which kernels a checked call launches: pure (no launch, no device memory), the shape part of the record and the knobs only.
static int attn_plan(const DecodeAttnCall& c, const AttnKnobs& knobs, AttnForm& f) {
    f = AttnForm{};
    const unsigned bh = (unsigned)(c.B * c.n_heads);
    f.records = attn_records(c);
    f.record_floats = f.records ? attn_record_floats(c) : 0;
    f.ws_bytes = attn_ws_bytes(c);
    f.grid[0] = (unsigned)c.n_split, f.grid[1] = bh, f.grid[2] = 1;           // (split, (row, head)) unless said otherwise
    // few workgroups -> many waves each (one (b, head) can own a whole CU); many -> 4 waves each, several per CU
    const bool few = (int64_t)c.B * c.n_heads * c.n_split < 1024;
    if (c.prefix_kind) {
        VH_REQUIRE(!(c.kv16 && c.prefix_kind == ATTN_PREFIX_GROUPS) && !c.any_width, VH_EUNSUPPORTED,
                   "%s: a shared prompt is served at width 64, groups over fp32 caches only", c.name);
        // one launch whose workgroups take either four 32-key blocks of a prefix for all its beams or one (row, head, split) of the
        // suffixes, and the merge of every (row, head)'s records
        const unsigned n_groups = c.prefix_kind == ATTN_PREFIX_GROUPS ? c.B / c.beams : 1;
        const unsigned prefix_wgs = ((unsigned)(c.prefix + 31) / 32 + 3) / 4 * c.n_heads * n_groups;
        f.kernel = c.kv16 ? VH_ATTN_K_SHARED16 : c.prefix_kind == ATTN_PREFIX_GROUPS ? VH_ATTN_K_SHARED_GROUPS : VH_ATTN_K_SHARED;
        f.grid[0] = prefix_wgs + c.n_split * bh, f.grid[1] = 1, f.block = 256;
        f.second = c.prefix_kind == ATTN_PREFIX_GROUPS ? VH_ATTN_2ND_MERGE_GROUPS : VH_ATTN_2ND_MERGE;
        f.second_grid = bh, f.second_block = 256;
    } else if (c.any_width) {
        // lane map: LK = min(16, next_pow2(hd / 4)) lanes per key, NV = ceil(hd / (4 LK)) 16-byte slots per lane
        const int hd = c.head_dim;
        f.kernel = VH_ATTN_K_HD, f.nw = 8, f.d = 2, f.block = 8 * 64;
        f.lk = hd == 16 ? 4 : hd <= 32 ? 8 : 16;
        f.nv = (hd + 4 * f.lk - 1) / (4 * f.lk);
        if (c.n_split > 1) f.second = VH_ATTN_2ND_HD_COMBINE, f.second_grid = bh, f.second_block = VH_HEAD_DIM_MAX;
    } else if (c.kv16 && c.n_split == 1) {
        // ring shape (waves x register sets of 32 keys): 8 x 2 as the fp32 kernel; 16 x 1, 16 x 2, 8 x 3, 8 x 4 and 4 x 4
        // measured within 3 % of it (461-477 us per decode step, profiles/r3_ab_decode_perf_mode.log)
        f.kernel = VH_ATTN_K_RING16, f.nw = 8, f.d = 2, f.block = 8 * 64;
    } else if (c.kv16) {
        // few workgroups -> 8 waves each (the ring16 shape: a (row, head, split) may own a CU); many -> 4 waves, several per CU.
        // The threshold is the fp32 launch's rule (`few`), taken over as it stands: NOT measured for the 16-bit stream.
        f.kernel = VH_ATTN_K_RING16_SPLIT, f.nw = few ? 8 : 4, f.d = 2, f.block = f.nw * 64;
        // records added in split order by the combine launch of the fp32 form: deterministic
        f.second = VH_ATTN_2ND_COMBINE, f.second_grid = bh, f.second_block = 64;
    } else if (knobs.variant != 1 && few && c.n_split == 1 && knobs.waves == 0) {
        // default: one (b, head) per CU and no key split -> the ring kernel (8 waves x 2 register sets of 32 keys, speculative
        // start: 605.9 vs 615.2 us per decode step, profiles/r2_ab_decode_ring.log); otherwise — key splits, more (b, head)
        // pairs than CUs — the burst kernel.  VH_TUNE_DECODE_VARIANT = 1 forces the burst kernel (A/B); the other ring
        // shapes round 2 measured (8x3, 16x1, 12x2, 16x2x16-key, 8x4x16-key; profiles/r2_attn_ab.log) were slower and are gone.
        f.kernel = VH_ATTN_K_RING, f.nw = 8, f.d = 2, f.block = 8 * 64;
    } else {
        const int waves = knobs.waves ? knobs.waves : few ? 16 : 4;
        f.kernel = VH_ATTN_K_BURST, f.nw = waves == 16 || waves == 8 ? waves : 4, f.block = f.nw * 64;
        // key splits: combined by a second launch or by the last workgroup of a (row, head) to arrive (VH_TUNE_DECODE_COMBINE = 1).
        // Measured on generate() at the reference defaults (4 beams, 8 splits, 12L/512d; profiles/r4_ab_default_generate_combine.log):
        // second launch 364.6 us per step; in-launch with an agent-scope release + acquire 609.7 (the release writes back the
        // L2); in-launch with write-through stores and agent-scope loads, no fences, 377.6 — the hand-off (drain, ticket,
        // dependent loads from beyond the L2) still costs 1 us per layer more than the 1.75 us dependent-launch floor it saves.
        // Knob 1: inside this launch; knob 2: the second launch; default: inside at TWO splits (configs[4], 8 rows x 16 heads:
        // 1483.5 vs 1496.6 us per step at context 2.7 k, 1027.2 vs 1028.3 at 0.6 k, profiles/r6_ab_config5_combine.log), the
        // second launch at more (4 beams x 8 heads, 8 splits: DESIGN 3.1)
        f.fused_combine = c.n_split > 1 && (knobs.combine == 1 || (knobs.combine == 0 && c.n_split == 2));
        if (f.fused_combine) f.ticket_offset = attn_records_bytes(c);
        else if (c.n_split > 1) f.second = VH_ATTN_2ND_COMBINE, f.second_grid = bh, f.second_block = 64;
    }
    return VH_OK;
}

// the compiled first kernels: (kernel, NW, D, LK, NV) as attn_launch's switch (and attention_hd.hip's) instantiates them
static const int ATTN_FORMS[][5] = {
    {VH_ATTN_K_BURST, 4, 0, 0, 0},  {VH_ATTN_K_BURST, 8, 0, 0, 0},  {VH_ATTN_K_BURST, 16, 0, 0, 0}, {VH_ATTN_K_RING, 8, 2, 0, 0},
    {VH_ATTN_K_RING16, 8, 2, 0, 0}, {VH_ATTN_K_RING16_SPLIT, 8, 2, 0, 0}, {VH_ATTN_K_RING16_SPLIT, 4, 2, 0, 0},
    {VH_ATTN_K_HD, 8, 2, 4, 1},     {VH_ATTN_K_HD, 8, 2, 8, 1},     {VH_ATTN_K_HD, 8, 2, 16, 1},    {VH_ATTN_K_HD, 8, 2, 16, 2},
    {VH_ATTN_K_HD, 8, 2, 16, 3},    {VH_ATTN_K_HD, 8, 2, 16, 4},    {VH_ATTN_K_SHARED, 0, 0, 0, 0}, {VH_ATTN_K_SHARED_GROUPS, 0, 0, 0, 0},
    {VH_ATTN_K_SHARED16, 0, 0, 0, 0}};

template <class T>
static SharedArgs<T> shared_args(const AttnForm& f, const DecodeAttnCall& c) {
    const bool groups = c.prefix_kind == ATTN_PREFIX_GROUPS;
    const int n_pb = f.records - c.n_split;
    return SharedArgs<T>{c.q, c.ldq, (const T*)c.kprefix, (const T*)c.vprefix, c.prefix, c.prefix_S, (const T*)c.k, (const T*)c.v,
                         c.len, c.len_bias, c.S_max, c.n_split, (float*)c.ws, c.n_heads, c.B, n_pb, f.records,
                         (int)f.grid[0] - c.n_split * c.B * c.n_heads, groups ? c.group_len : nullptr, groups ? c.B / c.beams : 1,
                         groups ? c.beams : c.B};
}

// the first kernel with the profiling events on its dispatch packet, then the second launch: every template instantiation
// of the decode attention is in this switch (the any-width kernels: in vh_internal_attn_decode_hd_launch's)
static int attn_launch(const AttnForm& f, const DecodeAttnCall& c) {
    hipStream_t s = (hipStream_t)c.stream;
    const dim3 grid(f.grid[0], f.grid[1], f.grid[2]), block(f.block);
    auto first = [&](auto kernel, auto... args) {
        hipExtLaunchKernelGGL(kernel, grid, block, 0, s, g_attn_ev[0], g_attn_ev[1], 0, args...);
        return true;
    };
    auto burst = [&](auto kernel) {
        return first(kernel, c.q, c.ldq, (const float*)c.k, (const float*)c.v, c.out, c.ldo, c.len, c.len_bias, c.n_heads, c.S_max,
                     c.n_split, (float*)c.ws, f.fused_combine ? (unsigned*)((char*)c.ws + f.ticket_offset) : (unsigned*)nullptr);
    };
    auto ring16_split = [&](auto kernel) {
        return first(kernel, c.q, c.ldq, (const uint16_t*)c.k, (const uint16_t*)c.v, c.len, c.len_bias, c.n_heads, c.S_max, c.n_split,
                     (float*)c.ws);
    };
    bool compiled = false;
    switch (f.kernel) {
    case VH_ATTN_K_BURST:
        compiled = f.nw == 16 ? burst(attn_decode_kernel<16>) : f.nw == 8 ? burst(attn_decode_kernel<8>)
                   : f.nw == 4 ? burst(attn_decode_kernel<4>) : false;
        break;
    case VH_ATTN_K_RING:
        compiled = f.nw == 8 && f.d == 2 && first(attn_decode_ring_kernel<8, 2>, c.q, c.ldq, (const float*)c.k, (const float*)c.v, c.out,
                                                  c.ldo, c.len, c.len_bias, c.n_heads, c.S_max);
        break;
    case VH_ATTN_K_RING16:
        compiled = f.nw == 8 && f.d == 2 && first(attn_decode_ring16_kernel<8, 2>, c.q, c.ldq, (const uint16_t*)c.k, (const uint16_t*)c.v,
                                                  c.out, c.ldo, c.len, c.len_bias, c.n_heads, c.S_max);
        break;
    case VH_ATTN_K_RING16_SPLIT:
        compiled = f.d != 2 ? false : f.nw == 8 ? ring16_split(attn_decode_ring16_split_kernel<8, 2>)
                   : f.nw == 4 ? ring16_split(attn_decode_ring16_split_kernel<4, 2>) : false;
        break;
    case VH_ATTN_K_HD: compiled = vh_internal_attn_decode_hd_launch(f, c, g_attn_ev[0], g_attn_ev[1]); break;
    case VH_ATTN_K_SHARED: compiled = first(attn_shared_kernel, shared_args<float>(f, c)); break;
    case VH_ATTN_K_SHARED_GROUPS: compiled = first(attn_shared_groups_kernel, shared_args<float>(f, c)); break;
    case VH_ATTN_K_SHARED16: compiled = first(attn_shared16_kernel, shared_args<uint16_t>(f, c)); break;
    }
    VH_REQUIRE(compiled, VH_EUNSUPPORTED, "%s: internal: no compiled kernel %d <NW %d, D %d, LK %d, NV %d>", c.name, f.kernel, f.nw, f.d,
               f.lk, f.nv);
    const dim3 grid2(f.second_grid), block2(f.second_block);
    switch (f.second) {
    case VH_ATTN_2ND_COMBINE:
        hipLaunchKernelGGL(attn_decode_combine_kernel, grid2, block2, 0, s, (const float*)c.ws, c.out, c.ldo, c.n_heads, c.n_split);
        break;
    case VH_ATTN_2ND_MERGE:
        hipLaunchKernelGGL(attn_records_merge_kernel, grid2, block2, 0, s, (const float*)c.ws, c.out, c.ldo, c.n_heads, f.records);
        break;
    case VH_ATTN_2ND_MERGE_GROUPS:
        hipLaunchKernelGGL(attn_records_merge_groups_kernel, grid2, block2, 0, s, (const float*)c.ws, c.out, c.ldo, c.n_heads,
                           f.records - c.n_split, c.n_split, c.group_len, c.beams);
        break;
    default: break;                                      // none, or the any-width combine (launched with its kernel)
    }
    VH_CHECK_LAUNCH(c.name);
    return VH_OK;
}

// vh_attn_decode_form: the entry points run as they are, and the form is handed over instead of launched
static thread_local AttnForm* t_attn_form_query = nullptr;

int vh_internal_attn_decode(const DecodeAttnCall& c) {
    const int rc = vh_internal_attn_decode_check(c, true);
    if (rc != VH_OK) return rc;
    AttnForm f;
    const int prc = attn_plan(c, AttnKnobs{vh_tuning(VH_TUNE_DECODE_VARIANT), vh_tuning(VH_TUNE_DECODE_WAVES), vh_tuning(VH_TUNE_DECODE_COMBINE)}, f);
    if (prc != VH_OK) return prc;
    if (t_attn_form_query) {
        *t_attn_form_query = f;
        return VH_OK;
    }
    return attn_launch(f, c);
}

// the record of a width-64 call without a shared prompt; the entry points below fill in what they have beyond it
static DecodeAttnCall attn_call(const char* name, const float* q, int ldq, const void* k, const void* v, float* out, int ldo,
                                const int32_t* len, int len_bias, int B, int n_heads, int S_max, bool kv16, int n_split, void* ws,
                                size_t ws_bytes, void* stream) {
    return DecodeAttnCall{name, "partial", q, ldq, out, ldo, len, len_bias, B, n_heads, false, HD, 0.f, kv16, k, v, S_max,
                          ATTN_PREFIX_NONE, nullptr, nullptr, 0, 0, nullptr, 1, n_split, ws, ws_bytes, stream};
}
static DecodeAttnCall attn_call_shared(DecodeAttnCall c, int kind, const void* kprefix, const void* vprefix, int prefix, int prefix_S,
                                       const int32_t* group_len, int beams) {
    c.prefix_kind = kind, c.kprefix = kprefix, c.vprefix = vprefix, c.prefix = prefix, c.prefix_S = prefix_S;
    c.group_len = group_len, c.beams = beams;
    return c;
}

extern "C" size_t vh_attn_decode_ws_bytes(int B, int n_heads, int n_split) {
    return attn_ws_bytes(attn_call("", nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, B, n_heads, 0, false, n_split, nullptr, 0, nullptr));
}
extern "C" size_t vh_attn_decode_shared_ws_bytes(int B, int n_heads, int prefix_len, int n_split_suffix) {
    if (B <= 0 || n_heads <= 0 || prefix_len <= 0 || n_split_suffix < 1) return 0;
    DecodeAttnCall c = attn_call("", nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, B, n_heads, 0, false, n_split_suffix, nullptr, 0, nullptr);
    return attn_ws_bytes(attn_call_shared(c, ATTN_PREFIX_ONE, nullptr, nullptr, prefix_len, prefix_len, nullptr, 1));
}
// several utterances at once: the records of the prefix CAPACITY
extern "C" size_t vh_attn_decode_shared_groups_ws_bytes(int B, int n_heads, int prefix_cap, int n_split_suffix) {
    return vh_attn_decode_shared_ws_bytes(B, n_heads, prefix_cap, n_split_suffix);
}
static DecodeAttnCall attn_call_any_width(DecodeAttnCall c, int head_dim, float scale) {
    c.any_width = true, c.head_dim = head_dim, c.scale = scale;
    return c;
}
extern "C" size_t vh_attn_decode_hd_ws_bytes(int B, int n_heads, int head_dim, int n_split) {
    if (n_split <= 1 || B <= 0 || n_heads <= 0 || head_dim <= 0) return 0;
    DecodeAttnCall c = attn_call("", nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, B, n_heads, 0, false, n_split, nullptr, 0, nullptr);
    return attn_ws_bytes(attn_call_any_width(c, head_dim, 0.f));
}

// a head width other than 64 (attention_hd.hip's kernels; 64 itself is served, for comparisons)
extern "C" int vh_attn_decode_hd(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                                 const int32_t* cache_len, int len_bias, int B, int n_heads, int head_dim, int S_max, float scale,
                                 int n_split, void* partial, size_t partial_bytes, void* stream) {
    const DecodeAttnCall c = attn_call("vh_attn_decode_hd", q, ldq, kcache, vcache, out, ldo, cache_len, len_bias, B, n_heads, S_max, false,
                                       n_split, partial, partial_bytes, stream);
    return vh_internal_attn_decode(attn_call_any_width(c, head_dim, scale));
}

extern "C" int vh_attn_decode(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                              const int32_t* cache_len, int len_bias, int B, int n_heads, int S_max, int n_split, void* partial,
                              void* stream) {
    return vh_internal_attn_decode(attn_call("vh_attn_decode", q, ldq, kcache, vcache, out, ldo, cache_len, len_bias, B, n_heads, S_max,
                                             false, n_split, partial, ATTN_WS_SIZE_NOT_GIVEN, stream));
}

extern "C" int vh_attn_decode_kv16(const float* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, float* out, int ldo,
                                   const int32_t* cache_len, int len_bias, int B, int n_heads, int S_max, void* stream) {
    return vh_internal_attn_decode(attn_call("vh_attn_decode_kv16", q, ldq, kcache16, vcache16, out, ldo, cache_len, len_bias, B, n_heads,
                                             S_max, true, 1, nullptr, 0, stream));
}

// (n_split == 1 is the record of vh_attn_decode_kv16 but for the name: its launch, bit for bit)
extern "C" int vh_attn_decode_kv16_split(const float* q, int ldq, const uint16_t* kcache16, const uint16_t* vcache16, float* out,
                                         int ldo, const int32_t* cache_len, int len_bias, int B, int n_heads, int S_max, int n_split,
                                         void* partial, size_t partial_bytes, void* stream) {
    return vh_internal_attn_decode(attn_call("vh_attn_decode_kv16_split", q, ldq, kcache16, vcache16, out, ldo, cache_len, len_bias, B,
                                             n_heads, S_max, true, n_split, partial, partial_bytes, stream));
}

extern "C" int vh_attn_decode_shared(const float* q, int ldq, const float* kprefix, const float* vprefix, int prefix_len,
                                     int prefix_S, const float* ksuffix, const float* vsuffix, float* out, int ldo,
                                     const int32_t* suffix_len, int len_bias, int B, int n_heads, int S_suf, int n_split_suffix,
                                     void* partial, size_t partial_bytes, void* stream) {
    const DecodeAttnCall c = attn_call("vh_attn_decode_shared", q, ldq, ksuffix, vsuffix, out, ldo, suffix_len, len_bias, B, n_heads, S_suf,
                                       false, n_split_suffix, partial, partial_bytes, stream);
    return vh_internal_attn_decode(attn_call_shared(c, ATTN_PREFIX_ONE, kprefix, vprefix, prefix_len, prefix_S, nullptr, 1));
}

// several utterances at once: B = n_groups * beams rows, rows g * beams .. g * beams + beams - 1 over group g's prompt
extern "C" int vh_attn_decode_shared_groups(const float* q, int ldq, const float* kprefix, const float* vprefix,
                                            const int32_t* prefix_len, int prefix_cap, int prefix_S, const float* ksuffix,
                                            const float* vsuffix, float* out, int ldo, const int32_t* suffix_len, int len_bias,
                                            int B, int beams, int n_heads, int S_suf, int n_split_suffix, void* partial,
                                            size_t partial_bytes, void* stream) {
    const DecodeAttnCall c = attn_call("vh_attn_decode_shared_groups", q, ldq, ksuffix, vsuffix, out, ldo, suffix_len, len_bias, B, n_heads,
                                       S_suf, false, n_split_suffix, partial, partial_bytes, stream);
    return vh_internal_attn_decode(attn_call_shared(c, ATTN_PREFIX_GROUPS, kprefix, vprefix, prefix_cap, prefix_S, prefix_len, beams));
}

extern "C" int vh_attn_decode_shared_kv16(const float* q, int ldq, const uint16_t* kprefix16, const uint16_t* vprefix16,
                                          int prefix_len, int prefix_S, const uint16_t* ksuffix16, const uint16_t* vsuffix16,
                                          float* out, int ldo, const int32_t* suffix_len, int len_bias, int B, int n_heads,
                                          int S_suf, int n_split_suffix, void* partial, size_t partial_bytes, void* stream) {
    const DecodeAttnCall c = attn_call("vh_attn_decode_shared_kv16", q, ldq, ksuffix16, vsuffix16, out, ldo, suffix_len, len_bias, B,
                                       n_heads, S_suf, true, n_split_suffix, partial, partial_bytes, stream);
    return vh_internal_attn_decode(attn_call_shared(c, ATTN_PREFIX_ONE, kprefix16, vprefix16, prefix_len, prefix_S, nullptr, 1));
}

// ---- which kernels a call launches: the entry point itself runs, on operands that are never touched, up to its launch ----
extern "C" int vh_attn_decode_form(int entry, int B, int n_heads, int head_dim, int S_max, int n_split, int prefix, int prefix_S,
                                   int beams, size_t ws_bytes, vh_attn_decode_form_info* out) {
    VH_REQUIRE(out, VH_EINVAL, "vh_attn_decode_form: null pointer");
    *out = AttnForm{};
    VH_REQUIRE(entry >= VH_ATTN_ENTRY_DECODE && entry <= VH_ATTN_ENTRY_HD, VH_EINVAL, "vh_attn_decode_form: entry=%d", entry);
    alignas(16) static float operand[4];          // every pointer argument: non-null, 16-byte aligned, never dereferenced
    float* const P = operand;
    const uint16_t* const H = reinterpret_cast<const uint16_t*>(operand);
    const int32_t* const I = reinterpret_cast<const int32_t*>(operand);
    const int ld = n_heads * (entry == VH_ATTN_ENTRY_HD ? head_dim : HD);
    AttnForm f{};
    t_attn_form_query = &f;
    int rc;
    switch (entry) {
    case VH_ATTN_ENTRY_DECODE: rc = vh_attn_decode(P, ld, P, P, P, ld, I, 1, B, n_heads, S_max, n_split, P, nullptr); break;
    case VH_ATTN_ENTRY_KV16: rc = vh_attn_decode_kv16(P, ld, H, H, P, ld, I, 1, B, n_heads, S_max, nullptr); break;
    case VH_ATTN_ENTRY_KV16_SPLIT:
        rc = vh_attn_decode_kv16_split(P, ld, H, H, P, ld, I, 1, B, n_heads, S_max, n_split, P, ws_bytes, nullptr);
        break;
    case VH_ATTN_ENTRY_SHARED:
        rc = vh_attn_decode_shared(P, ld, P, P, prefix, prefix_S, P, P, P, ld, I, 1, B, n_heads, S_max, n_split, P, ws_bytes, nullptr);
        break;
    case VH_ATTN_ENTRY_SHARED_GROUPS:
        rc = vh_attn_decode_shared_groups(P, ld, P, P, I, prefix, prefix_S, P, P, P, ld, I, 1, B, beams, n_heads, S_max, n_split, P,
                                          ws_bytes, nullptr);
        break;
    case VH_ATTN_ENTRY_SHARED_KV16:
        rc = vh_attn_decode_shared_kv16(P, ld, H, H, prefix, prefix_S, H, H, P, ld, I, 1, B, n_heads, S_max, n_split, P, ws_bytes, nullptr);
        break;
    default:
        rc = vh_attn_decode_hd(P, ld, P, P, P, ld, I, 1, B, n_heads, head_dim, S_max, 1.f, n_split, P, ws_bytes, nullptr);
        break;
    }
    t_attn_form_query = nullptr;
    if (rc == VH_OK) *out = f;
    return rc;
}

// the compiled first kernels, i = 0, 1, ...: kernel and template arguments in *out; VH_EINVAL past the last row
extern "C" int vh_attn_decode_form_row(int i, vh_attn_decode_form_info* out) {
    const int rows = (int)(sizeof(ATTN_FORMS) / sizeof(ATTN_FORMS[0]));
    VH_REQUIRE(out && i >= 0 && i < rows, VH_EINVAL, "vh_attn_decode_form_row: row %d of %d", i, rows);
    *out = AttnForm{};
    out->kernel = ATTN_FORMS[i][0], out->nw = ATTN_FORMS[i][1], out->d = ATTN_FORMS[i][2], out->lk = ATTN_FORMS[i][3], out->nv = ATTN_FORMS[i][4];
    return VH_OK;
}


// =============================================================================================
// many-row attention over packed rows, TRAINING forms (packed AR training: a ragged batch without padding rows).  The
// kernels are stamped out here, behind everything else, so every earlier kernel lies in the code object where it did.
//   attn_rows_packed_lse_kernel  attn_rows_packed_kernel with the launch's mask mode (full / prefix per segment) and lse2
//   attn_bwd_packed_kernel<8>    attn_bwd_fused_kernel<8> with the sequence taken from the segment table; work items
//                                (segment, key chunk) x head from a host-built table, heaviest first
//   attn_dq_reduce_packed_kernel the dQ slabs (max_chunks, n_heads, M, 64) added in chunk order, per 128-query block of the
//                                forward's block table: every row of dq once, no atomics
// =============================================================================================
#define ATTN_ROWS_PACKED 2
#include "attn_rows_body.inc"       // attn_rows_packed_lse_kernel(RowsArgs, PackedSegs, seg_x_len)
#undef ATTN_ROWS_PACKED

// The segments of vh_attn_rows_bwd_packed: PackedSegs' arrays plus the text lengths, and items[2 i], items[2 i + 1] =
// (segment, key chunk) of work item i.  n_rows = M: lse2 and the slabs are (·, M) and no row at or beyond M is touched.
struct PackedBwdSegs {
    const int32_t* seg_start; const int32_t* seg_len; const int32_t* seg_x_len; const int32_t* items; const int32_t* blocks;
    int n_seg, n_rows;
};

#define ATTN_BWD_PACKED 1
#include "attn_bwd_fused_body.inc"   // attn_bwd_packed_kernel<FW>(BwdArgs, PackedBwdSegs)
#undef ATTN_BWD_PACKED

// dq[seg_start + q][head*64 + d] = 1/8 · Σ_chunks slab[chunk][head][seg_start + q][d] for the 128 queries of one block of
// the forward's table, chunks in index order under attn_dq_reduce_kernel's rule (a chunk contributes to a query exactly
// when the packed kernel visited the pair).  A segment of one chunk goes through here as well: one slab read.
__global__ __launch_bounds__(256) void attn_dq_reduce_packed_kernel(BwdArgs a, PackedBwdSegs ps) {
    const int blk = blockIdx.x / a.n_heads;
    const int head = blockIdx.x - blk * a.n_heads;
    const int seg = ps.blocks[2 * blk], q0 = ps.blocks[2 * blk + 1];
    if ((unsigned)seg >= (unsigned)ps.n_seg) return;
    const int s0 = ps.seg_start[seg], len = ps.seg_len[seg];
    if (s0 < 0 || len < 1 || (int64_t)s0 + len > ps.n_rows || q0 < 0 || q0 >= len) return;
    const int xl = a.mode == VH_MASK_PREFIX ? min(max(ps.seg_x_len[seg], 0), len) : len;   // full mask: every chunk sees every query
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = threadIdx.x + 256 * i;
        const int q = q0 + (idx >> 4), d4 = idx & 15;
        if (q >= len) break;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < a.n_blocks; ++c) {
            const int kb0 = c * a.chunk_keys;
            if (kb0 >= len) break;
            if (kb0 >= xl && q < kb0) break;
            acc = acc + ld4(a.slab + ((((int64_t)c * a.n_heads + head) * ps.n_rows + s0 + q) * HD + 4 * d4));
        }
        st4(a.dq + ((int64_t)s0 + q) * a.ldg + head * HD + 4 * d4, acc * 0.125f);
    }
}

extern "C" int vh_attn_rows_packed_lse(const float* q, int ldq, const float* kcache, const float* vcache, float* out, int ldo,
                                       int n_heads, int M, int S_max, int mode, const int32_t* seg_start, const int32_t* seg_len,
                                       const int32_t* seg_x_len, int n_seg, const int32_t* blocks, int n_blocks, float* lse2,
                                       void* stream) {
    VH_REQUIRE(q && kcache && vcache && out && lse2, VH_EINVAL, "vh_attn_rows_packed_lse: null pointer (q, kcache, vcache, out or lse2)");
    VH_REQUIRE(seg_start && seg_len && blocks, VH_EINVAL, "vh_attn_rows_packed_lse: null pointer (seg_start, seg_len or blocks)");
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX, VH_EINVAL, "vh_attn_rows_packed_lse: mode=%d (full or prefix)", mode);
    VH_REQUIRE(mode != VH_MASK_PREFIX || seg_x_len, VH_EINVAL, "vh_attn_rows_packed_lse: the prefix mask needs seg_x_len");
    VH_REQUIRE(n_heads > 0 && M >= 1 && S_max >= M, VH_EINVAL, "vh_attn_rows_packed_lse: bad dims n_heads=%d M=%d S_max=%d", n_heads, M, S_max);
    VH_TRY(vh_packed_attn_sizes("vh_attn_rows_packed_lse", n_heads, n_seg, n_blocks, ldq, ldo, 4));
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(out), VH_EALIGN, "vh_attn_rows_packed_lse: q and out must be 16-byte aligned");
    VH_REQUIRE(vh_aligned16(kcache) && vh_aligned16(vcache), VH_EALIGN,
               "vh_attn_rows_packed_lse: kcache and vcache must be 16-byte aligned");
    VH_REQUIRE(((uintptr_t)lse2 & 3) == 0, VH_EALIGN, "vh_attn_rows_packed_lse: lse2 must be 4-byte aligned");
    VH_TRY(vh_packed_workgroups("vh_attn_rows_packed_lse", n_blocks, n_heads));
    RowsArgs a{q, ldq, kcache, vcache, out, ldo, n_heads, M, 0, S_max, mode, 0,
               nullptr, nullptr, nullptr, nullptr, 0, lse2, 0};
    PackedSegs ps{seg_start, seg_len, blocks, n_seg, M};        // n_rows = M: a segment reaching past it is cut (lse2 has M rows)
    hipLaunchKernelGGL(attn_rows_packed_lse_kernel, dim3(n_blocks * n_heads), dim3(256), 0, (hipStream_t)stream, a, ps, seg_x_len);
    VH_CHECK_LAUNCH("vh_attn_rows_packed_lse");
    return VH_OK;
}

extern "C" size_t vh_attn_rows_bwd_packed_ws_bytes(int n_heads, int M, int max_chunks) {
    if (n_heads <= 0 || M <= 0 || max_chunks <= 1) return 0;
    return (size_t)max_chunks * n_heads * M * HD * sizeof(float);
}

extern "C" int vh_attn_rows_bwd_packed(const float* q, int ldq, const float* kcache, const float* vcache, const float* out,
                                       int ldo, const float* dout, int lddo, const float* lse2, float* dq, float* dk, float* dv,
                                       int ldg, int n_heads, int M, int S_max, int mode, const int32_t* seg_start,
                                       const int32_t* seg_len, const int32_t* seg_x_len, int n_seg, const int32_t* items,
                                       int n_items, int chunk_keys, int max_chunks, const int32_t* blocks, int n_blocks,
                                       void* ws, size_t ws_bytes, void* stream) {
    VH_REQUIRE(q && kcache && vcache && out && dout && lse2 && dq && dk && dv, VH_EINVAL, "vh_attn_rows_bwd_packed: null pointer");
    VH_REQUIRE(seg_start && seg_len && items && blocks, VH_EINVAL,
               "vh_attn_rows_bwd_packed: null pointer (seg_start, seg_len, items or blocks)");
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX, VH_EINVAL, "vh_attn_rows_bwd_packed: mode=%d (full or prefix)", mode);
    VH_REQUIRE(mode != VH_MASK_PREFIX || seg_x_len, VH_EINVAL, "vh_attn_rows_bwd_packed: the prefix mask needs seg_x_len");
    VH_REQUIRE(n_heads > 0 && M >= 1 && S_max >= M, VH_EINVAL, "vh_attn_rows_bwd_packed: bad dims n_heads=%d M=%d S_max=%d", n_heads, M, S_max);
    VH_REQUIRE(n_seg >= 1, VH_EINVAL, "vh_attn_rows_bwd_packed: n_seg=%d", n_seg);
    VH_REQUIRE(n_items >= 1 && n_blocks >= 1, VH_EINVAL, "vh_attn_rows_bwd_packed: n_items=%d n_blocks=%d", n_items, n_blocks);
    VH_REQUIRE(chunk_keys >= 32 && chunk_keys <= FKMAX && chunk_keys % 32 == 0, VH_EINVAL,
               "vh_attn_rows_bwd_packed: chunk_keys=%d (a multiple of 32, at most %d)", chunk_keys, FKMAX);
    VH_REQUIRE(max_chunks >= 1 && (int64_t)max_chunks * chunk_keys <= 0x7fffffffLL, VH_EINVAL,
               "vh_attn_rows_bwd_packed: max_chunks=%d", max_chunks);
    const int wd = n_heads * HD;
    VH_REQUIRE(ldq % 4 == 0 && ldo % 4 == 0 && lddo % 4 == 0 && ldg % 4 == 0 && ldq >= wd && ldo >= wd && lddo >= wd && ldg >= wd,
               VH_EINVAL, "vh_attn_rows_bwd_packed: leading dimensions");
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(kcache) && vh_aligned16(vcache) && vh_aligned16(out) && vh_aligned16(dout) &&
                   vh_aligned16(dq) && vh_aligned16(dk) && vh_aligned16(dv),
               VH_EALIGN, "vh_attn_rows_bwd_packed: pointers must be 16-byte aligned");
    const size_t need = vh_attn_rows_bwd_packed_ws_bytes(n_heads, M, max_chunks);
    VH_REQUIRE(ws_bytes >= need, VH_EINVAL, "vh_attn_rows_bwd_packed: workspace of %zu bytes, need %zu", ws_bytes, need);
    VH_REQUIRE(need == 0 || (ws && vh_aligned16(ws)), VH_EALIGN,
               "vh_attn_rows_bwd_packed: workspace must be a 16-byte aligned device pointer");
    VH_REQUIRE((int64_t)n_items * n_heads <= 0x7fffffffLL && (int64_t)n_blocks * n_heads <= 0x7fffffffLL, VH_EUNSUPPORTED,
               "vh_attn_rows_bwd_packed: n_items=%d, n_blocks=%d x n_heads=%d workgroups", n_items, n_blocks, n_heads);
    // max_chunks == 1: every segment fits one chunk and the kernel writes dq itself (no slab, no reduce launch)
    BwdArgs a{q, ldq, kcache, vcache, out, ldo, dout, lddo, lse2, nullptr, dq, dk, dv, ldg,
              n_heads, 0, S_max, mode, 0, nullptr, nullptr, nullptr, nullptr, max_chunks, need ? (float*)ws : nullptr, chunk_keys};
    PackedBwdSegs ps{seg_start, seg_len, seg_x_len, items, blocks, n_seg, M};
    hipLaunchKernelGGL(attn_bwd_packed_kernel<8>, dim3(n_items * n_heads), dim3(512), 0, (hipStream_t)stream, a, ps);
    if (need)
        hipLaunchKernelGGL(attn_dq_reduce_packed_kernel, dim3(n_blocks * n_heads), dim3(256), 0, (hipStream_t)stream, a, ps);
    VH_CHECK_LAUNCH("vh_attn_rows_bwd_packed");
    return VH_OK;
}
