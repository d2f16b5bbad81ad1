// Many-row (prompt pass / NAR stage / recompute) flash attention, forward, for a head width hd other than 64: fp32 q, k, v
// read IN PLACE as the per-head column blocks of a (rows, 3 d) QKV projection — strided (B, h, T, hd) views with unit stride
// in the last dimension, no cache layout, no transposition pass, no staging copy — and out written as the per-head columns of
// a (rows, d) buffer.  Width 64 keeps attention.hip's kernels over the cache layout; this file serves hd % 4 == 0,
// 16 <= hd <= 128 (64 included, for comparisons).  Wider heads and explicit masks stay on the materialised route
// (kernels.attn_generic).
//
//  attn_rows_hd_kernel<NB> : the structure of attn_rows_kernel (attn_rows_body.inc) with the head width as NB = ceil(hd / 32)
//                          blocks of 32 columns.  One workgroup = 128 queries of one (batch row, head) over that row's keys in
//                          32-key tiles, K and V double-buffered in LDS ([buf][K|V][key][32 NB + 4]); key tiles wholly outside
//                          the block's mask are skipped; the heaviest query blocks (the last ones under the prefix mask) get
//                          the lowest workgroup ids.  Both products on v_mfma_f32_32x32x2_f32: S^T = K Q^T with the Q fragment
//                          in registers (4 NB x 4 floats per lane, pre-scaled by scale * log2(e)), O^T += V^T P with NB
//                          accumulators of 16 registers; exp2 online softmax, fp32 throughout; the score tile lives in 16
//                          registers per lane and nowhere else.  Columns hd .. 32 NB - 1 are ZERO-FILLED in LDS and in the Q
//                          fragment and never loaded (every 16-byte load starts at a column < hd and hd % 4 == 0, so the last
//                          head of the last row reads nothing past its own columns); output columns >= hd are never stored.
#include "vh_common.h"

#define RH_LOG2E 1.44269504088896340736f
#define RH_NEG_INF (-INFINITY)
#define RH_QB 128   // queries per block (4 waves x 32)
#define RH_KT 32    // keys per tile

struct RowsHdArgs {
    const float* q; const float* k; const float* v; float* out;
    int64_t q_sb, q_sh, q_sr;      // elements between batch rows, heads and rows of each operand
    int64_t k_sb, k_sh, k_sr;
    int64_t v_sb, v_sh, v_sr;
    int64_t o_sb, o_sh, o_sr;
    int n_heads, hd, Tq, Tk, mode, x_len;
    const int32_t* x_len_dev; const int32_t* kv_len;
    int n_qblocks;
    float qscale;                  // softmax scale * log2(e)
};

template <int NB>
__global__ __launch_bounds__(256, 2) void attn_rows_hd_kernel(RowsHdArgs a) {
    constexpr int KLD = 32 * NB + 4;   // LDS row stride (floats): 8 NB + 1 16-B slots, odd → conflict-free ds_read_b128 by row
    // [buf][K|V][key][KLD]; reused at the end as the [128][KLD] output transpose buffer (2 * 2 * 32 = 128 rows either way)
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * RH_KT * KLD];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // (w in an SGPR)
    const int r = lane & 31, h = lane >> 5;
    const int hd = a.hd;
    // 1-D grid, heaviest query blocks first; id % (B*h) is the (b, head) — attn_rows_kernel's order and its reasons
    const int n_bh = gridDim.x / a.n_qblocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int q0 = (a.n_qblocks - 1 - (int)(blockIdx.x / n_bh)) * RH_QB;
    const int q_off = a.Tk - a.Tq;
    const int kvl = a.kv_len ? min(a.kv_len[b], a.Tk) : a.Tk;
    // the full mask is the prefix mask whose prefix never ends: one body, no mode branches
    const int xl = a.mode == VH_MASK_PREFIX ? (a.x_len_dev ? a.x_len_dev[b] : a.x_len) : INT32_MAX;

    // number of key tiles this block has to visit
    const int last_pos = q_off + min(q0 + RH_QB, a.Tq) - 1;
    const int kmax = min(kvl, max(xl, last_pos >= xl ? last_pos + 1 : 0));
    const int n_tiles = (kmax + RH_KT - 1) / RH_KT;

    // Q fragment (B operand of Sᵀ = K·Qᵀ): lane holds Q[qi][8t+4h+j], pre-scaled; zero at and beyond column hd
    const int qi = q0 + w * 32 + r;            // this lane's query row
    const int qpos = q_off + qi;               // its key position
    const int vis_end = min(kvl, max(xl, qpos >= xl ? qpos + 1 : 0));   // key j visible to this query iff j < vis_end
    f32x4 qf[4 * NB];
    {
        // branch-free: a row at or beyond Tq and a column at or beyond hd load a valid element instead and are selected away
        const float* qp = a.q + b * a.q_sb + head * a.q_sh + (int64_t)min(qi, a.Tq - 1) * a.q_sr;
#pragma unroll
        for (int t = 0; t < 4 * NB; ++t) {
            const int c = 8 * t + 4 * h;
            const f32x4 x = ld4(qp + min(c, hd - 4)) * a.qscale;
            qf[t] = (qi < a.Tq && c < hd) ? x : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }

    const float* kb = a.k + b * a.k_sb + head * a.k_sh;
    const float* vb = a.v + b * a.v_sb + head * a.v_sh;
    const int skey = tid >> 3, scol = (tid & 7) * 4;    // staging: one key, NB 16-byte slots (columns scol + 32 i) per operand
    f32x4 rk[NB], rv[NB];
    // Keys beyond Tk are clamped to the last row of the view: their scores are masked to -inf, so their (finite) values
    // meet p = 0.  Columns at or beyond hd are not loaded (branch-free: such a slot loads the head's last four columns
    // instead and is selected away): the LDS image holds zeros there.
    // Address = workgroup-uniform head base + one 32-bit per-lane byte offset (the entry point checks that a view's last
    // row lies within 4 GB of its first): no 64-bit vector arithmetic in the loop.
    auto gload = [&](f32x4 (&rs)[NB], const float* base, uint32_t stride, int k0) {
        const uint32_t row = (uint32_t)min(k0 + skey, a.Tk - 1) * stride;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int c = scol + 32 * i;
            const f32x4 x = ld4((const float*)((const char*)base + (row + (uint32_t)min(c, hd - 4)) * 4u));
            rs[i] = c < hd ? x : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    const uint32_t k_sr = (uint32_t)a.k_sr, v_sr = (uint32_t)a.v_sr;
    auto lstore = [&](const f32x4 (&rs)[NB], int buf, int is_v) {
        float* d = lds + (2 * buf + is_v) * (RH_KT * KLD) + skey * KLD + scol;
#pragma unroll
        for (int i = 0; i < NB; ++i) st4(d + 32 * i, rs[i]);
    };
    f32x16 O[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) O[n][e] = 0.f;
    float m = RH_NEG_INF, l = 0.f;

    // positions covered by this wave's 32 queries (for tile skipping / fast path)
    const int wpos_min = q_off + q0 + w * 32, wpos_max = wpos_min + 31;

    if (n_tiles > 0) {
        gload(rk, kb, k_sr, 0);
        gload(rv, vb, v_sr, 0);
        lstore(rk, 0, 0);
        lstore(rv, 0, 1);
    }
    __syncthreads();
    for (int kt = 0; kt < n_tiles; ++kt) {
        const int cur = kt & 1, k0 = kt * RH_KT;
        const bool more = kt + 1 < n_tiles;
        if (more) {                                    // the next tile's K and V in flight across this tile's products
            gload(rk, kb, k_sr, k0 + RH_KT);
            gload(rv, vb, v_sr, k0 + RH_KT);
        }

        const bool any = k0 < kvl && (k0 < xl || (wpos_max >= xl && k0 <= wpos_max));
        const bool all = k0 + RH_KT <= kvl && (k0 + RH_KT <= xl || (wpos_min >= xl && k0 + RH_KT - 1 <= wpos_min));
        if (any) {
            const float* ks = lds + cur * (2 * RH_KT * KLD);
            const float* vs = ks + RH_KT * KLD;
            // ---- Sᵀ[key][q] = sum_d K[key][d] Q[q][d]
            f32x16 S;
#pragma unroll
            for (int t = 0; t < 4 * NB; ++t) {
                const f32x4 kf = ld4(ks + r * KLD + 8 * t + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j)            // the first product starts from the constant-zero C operand
                    S = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[t][j], (t | j) ? S : f32x16{}, 0, 0, 0);
            }
            // ---- mask: reg e ↔ key k0 + (e&3) + 8(e>>2) + 4h ; lane ↔ query qi
            if (!all) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (key >= vis_end) S[e] = RH_NEG_INF;
                }
            }
            // ---- online softmax (per lane = per query; the other 16 keys sit in lane^32)
            float tmax = S[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) tmax = fmaxf(tmax, S[e]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m, tmax);
            const float m_use = m_new == RH_NEG_INF ? 0.f : m_new;  // fully masked so far: p = 0
            const float alpha = vh_exp2(m - m_use);
            float psum = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                S[e] = vh_exp2(S[e] - m_use);
                psum += S[e];
            }
            l = l * alpha + psum;
            m = m_new;
            if (__any(alpha != 1.0f)) {                // no query of this wave raised its maximum: nothing to rescale
#pragma unroll
                for (int n = 0; n < NB; ++n)
#pragma unroll
                    for (int e = 0; e < 16; ++e) O[n][e] *= alpha;
            }
            // ---- Oᵀ[d][q] += sum_key V[key][d] P[key][q]; k-step e covers keys (e,h=0),(e,h=1)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float* vrow = vs + ((e & 3) + 8 * (e >> 2) + 4 * h) * KLD + r;
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    O[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * n], S[e], O[n], 0, 0, 0);
            }
        }
        if (more) {
            lstore(rk, cur ^ 1, 0);
            lstore(rv, cur ^ 1, 1);
        }
        __syncthreads();
    }

    // ---- normalise, transpose through LDS, store coalesced rows
    const float ltot = l + __shfl_xor(l, 32, 64);
    const float inv = 1.0f / ltot;  // fully masked row (kv_len <= 0 included) → 0/0 = NaN, as attn_rows_kernel and SDPA give
    float* ob = lds;                // [128][KLD]; all K/V reads finished at the last barrier
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            // regs 4g4..4g4+3 of O[n] ↔ d = 32n + 8*g4 + 4h + {0..3}
            const f32x4 v0 = {O[n][4 * g4], O[n][4 * g4 + 1], O[n][4 * g4 + 2], O[n][4 * g4 + 3]};
            st4(ob + (w * 32 + r) * KLD + 32 * n + 8 * g4 + 4 * h, v0 * inv);
        }
    __syncthreads();
    float* outb = a.out + b * a.o_sb + head * a.o_sh + scol;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = skey + 32 * i;
        if (q0 + row < a.Tq) {
            float* op = outb + (int64_t)(q0 + row) * a.o_sr;
#pragma unroll
            for (int n = 0; n < NB; ++n)
                if (scol + 32 * n < hd) st4(op + 32 * n, ld4(ob + row * KLD + scol + 32 * n));
        }
    }
}

extern "C" int vh_attn_rows_hd(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                               const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                               const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                               float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                               int B, int n_heads, int head_dim, int Tq, int Tk, float scale,
                               int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len, void* stream) {
    VH_REQUIRE(q && k && v && out, VH_EINVAL, "vh_attn_rows_hd: null pointer (q=%p k=%p v=%p out=%p)", (const void*)q,
               (const void*)k, (const void*)v, (const void*)out);
    VH_REQUIRE(mode != VH_MASK_EXPLICIT, VH_EUNSUPPORTED,
               "vh_attn_rows_hd: mode=%d (VH_MASK_EXPLICIT): caller-supplied masks take the materialised route", mode);
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX, VH_EINVAL, "vh_attn_rows_hd: mode=%d", mode);
    VH_REQUIRE(B > 0 && n_heads > 0 && Tq > 0 && Tk >= Tq, VH_EINVAL, "vh_attn_rows_hd: bad dims B=%d h=%d Tq=%d Tk=%d", B,
               n_heads, Tq, Tk);
    VH_REQUIRE(head_dim % 4 == 0 && head_dim >= 16 && head_dim <= 128, VH_EUNSUPPORTED,
               "vh_attn_rows_hd: head_dim=%d (a multiple of 4 from 16 to 128)", head_dim);
    const int64_t strides[12] = {q_sb, q_sh, q_sr, k_sb, k_sh, k_sr, v_sb, v_sh, v_sr, o_sb, o_sh, o_sr};
    static const char* const stride_names[12] = {"q batch", "q head", "q row", "k batch", "k head", "k row",
                                                 "v batch", "v head", "v row", "out batch", "out head", "out row"};
    for (int i = 0; i < 12; ++i)
        VH_REQUIRE(strides[i] % 4 == 0, VH_EINVAL, "vh_attn_rows_hd: %s stride=%lld (a multiple of 4 floats: rows stay 16-byte aligned)",
                   stride_names[i], (long long)strides[i]);
    // the kernel addresses a key row by a 32-bit byte offset from its (batch row, head) base
    const int64_t reach = ((1LL << 30) - head_dim) / (Tk > 1 ? Tk - 1 : 1);      // (no product that could overflow)
    VH_REQUIRE(k_sr >= 0 && v_sr >= 0 && k_sr <= reach && v_sr <= reach,
               VH_EUNSUPPORTED, "vh_attn_rows_hd: k row stride=%lld v row stride=%lld with Tk=%d (the last key row must lie within 4 GB of the first)",
               (long long)k_sr, (long long)v_sr, Tk);
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(k) && vh_aligned16(v) && vh_aligned16(out), VH_EALIGN,
               "vh_attn_rows_hd: q=%p k=%p v=%p out=%p must be 16-byte aligned", (const void*)q, (const void*)k, (const void*)v,
               (const void*)out);
    const int nqb = (Tq + RH_QB - 1) / RH_QB;
    VH_REQUIRE((int64_t)B * n_heads <= 0x7fffffffLL / nqb, VH_EINVAL,
               "vh_attn_rows_hd: B=%d h=%d Tq=%d: %d x %lld workgroups exceed one grid", B, n_heads, Tq, nqb, (long long)B * n_heads);
    RowsHdArgs a{q, k, v, out, q_sb, q_sh, q_sr, k_sb, k_sh, k_sr, v_sb, v_sh, v_sr, o_sb, o_sh, o_sr,
                 n_heads, head_dim, Tq, Tk, mode, x_len, x_len_dev, kv_len, nqb, scale * RH_LOG2E};
    const dim3 grid(nqb * B * n_heads), block(256);
    switch ((head_dim + 31) / 32) {
    case 1: hipLaunchKernelGGL(attn_rows_hd_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL(attn_rows_hd_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
    case 3: hipLaunchKernelGGL(attn_rows_hd_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL(attn_rows_hd_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
    }
    VH_CHECK_LAUNCH("vh_attn_rows_hd");
    return VH_OK;
}
