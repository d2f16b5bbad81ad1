// Many-row flash attention, BACKWARD, for a head width hd other than 64 (training: Tq == Tk == T): the gradients of
// vh_attn_rows_hd_lse (attention_rows_hd.hip) over the same operands — fp32 strided (B, h, T, hd) views with unit stride in
// the last dimension, read and written IN PLACE: q / k / v the per-head column blocks of a (rows, 3 d) projection, dq / dk /
// dv the same blocks of its gradient buffer, out / dout those of (rows, d) buffers.  hd % 4 == 0, 16 <= hd <= 128, the
// analytic masks.  Two launches, no atomics, P never in memory: attention.hip's two-kernel form (attn_bwd_dq_kernel /
// attn_bwd_dkv_kernel) with the head width as NB = ceil(hd / 32) blocks of 32 columns.
//
//  attn_rows_hd_bwd_dq_kernel<NB>  : one workgroup = 128 queries of one (b, head), queries are lanes; 32-key tiles of K and V
//                                  double-buffered in LDS ([buf][K|V][key][32 NB + 4]).  Per tile  S^T = K Q^T (Q pre-scaled by
//                                  scale * log2(e): the forward's bits),  P = exp2(S^T - lse2),  dP^T = V dO^T,
//                                  dS^T = P o (dP^T - D),  dQ^T += K^T dS^T.  D[q] = sum_d dO O is lane-local and also goes to
//                                  the workspace for the second kernel.  Tiles outside the block's mask are skipped, the
//                                  heaviest blocks get the lowest workgroup ids.
//  attn_rows_hd_bwd_dkv_kernel<NB> : one workgroup = 128 keys, keys are lanes; 32-query tiles of Q (pre-scaled) and dO, with
//                                  their lse2 and D, double-buffered in LDS.  S = Q K^T, P, dP = dO V^T, dS;
//                                  dV^T += dO^T P,  dK^T += Q^T dS.
// All products on v_mfma_f32_32x32x2_f32, fp32 throughout; the accumulator of the first product IS the B operand of the
// last.  The final factor `scale` is applied once to dQ and once to dK (dK was summed over the pre-scaled Q: x scale / qscale).
// Columns hd .. 32 NB - 1 are ZERO in every fragment and LDS image and never loaded (every 16-byte load starts at a column
// < hd, hd % 4 == 0); the four padding floats of an LDS row are never read (4 NB d-steps of 8 columns); gradient columns >= hd
// are never stored.  Every element of dq / dk / dv inside (B, h, T, hd) is written exactly once, zeros included: a workgroup
// that visits no tile (kv_len = 0, keys at or beyond kv_len) stores its zero accumulators.  A masked pair gets P = 0 and
// dS = 0 by selection, never by arithmetic: a fully masked query has lse2 = -inf and D = NaN (its forward output is 0 / 0).
//
// Registers: the dq kernel holds Q, dO and dQ (3 x 16 NB), the dkv kernel K, V, dK and dV (4 x 16 NB), plus two 16-register
// tiles and the staging rows.  The 512-entry file gives 256 per wave at two waves per SIMD: NB 1, 2 (and the dq kernel at
// NB 3) fit and keep __launch_bounds__(256, 2); the others are compiled for ONE workgroup per CU (256, 1) rather than
// spilled or sent through LDS a second time — no scratch at any NB (DESIGN.md section 3.17 has the numbers).
#include "vh_common.h"

#define RB_LOG2E 1.44269504088896340736f
#define RB_QB 128   // rows (queries or keys) per block: 4 waves x 32
#define RB_KT 32    // rows per LDS tile

struct RowsHdBwdArgs {
    const float* q; const float* k; const float* v; const float* o; const float* dout;
    const float* lse2;             // (B, h, T) from vh_attn_rows_hd_lse
    float* dsum;                   // (B, h, T): D, written by the dq kernel, read by the dkv kernel
    float* dq; float* dk; float* dv;
    int64_t q_sb, q_sh, q_sr;      // elements between batch rows, heads and rows of each operand
    int64_t k_sb, k_sh, k_sr;
    int64_t v_sb, v_sh, v_sr;
    int64_t o_sb, o_sh, o_sr;
    int64_t d_sb, d_sh, d_sr;      // dout
    int64_t g_sb, g_sh, g_sr;      // dq, dk, dv: blocks of one buffer, one stride set
    int n_heads, hd, T, mode, x_len;
    const int32_t* x_len_dev; const int32_t* kv_len;
    int n_blocks;
    float qscale;                  // softmax scale * log2(e)
    float scale;                   // softmax scale
};

// key visible to query qi: the header's rule with the full mask as the prefix that never ends (xl = INT32_MAX)
__device__ __forceinline__ bool rb_visible(int qi, int key, int kvl, int xl) {
    return key < kvl && (key < xl || (qi >= xl && key <= qi));
}

// 32 rows x NB 16-byte slots per thread-row: thread (srow = tid >> 3, scol = (tid & 7) * 4) loads columns scol + 32 i of row
// r0 + srow (clamped to the view's last row) — a slot at or beyond hd loads the head's last four columns instead and is
// selected away: zeros.  Address = workgroup-uniform head base + one 32-bit per-lane byte offset (the entry checks the reach).
template <int NB>
__device__ __forceinline__ void rb_gload(f32x4 (&rs)[NB], const float* base, uint32_t stride, int r0, int srow, int scol, int T,
                                         int hd) {
    const uint32_t row = (uint32_t)min(r0 + srow, T - 1) * stride;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int c = scol + 32 * i;
        const f32x4 x = ld4((const float*)((const char*)base + (row + (uint32_t)min(c, hd - 4)) * 4u));
        rs[i] = c < hd ? x : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// The accumulators acc[NB] (reg 4 g4 + j of block n <-> column 32 n + 8 g4 + 4 h + j, lane <-> row w * 32 + r) times sc,
// transposed through `ob` ([128][KLD]) and stored as coalesced rows of a (T, hd) view; rows >= T and columns >= hd are not
// stored.  Ends with a barrier: `ob` may be reused at once.
template <int NB>
__device__ __forceinline__ void rb_store_rows(float* ob, const f32x16 (&acc)[NB], float sc, float* dst, int64_t sr, int row0,
                                              int T, int hd, int w, int r, int h, int srow, int scol) {
    constexpr int KLD = 32 * NB + 4;
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 v0 = {acc[n][4 * g4], acc[n][4 * g4 + 1], acc[n][4 * g4 + 2], acc[n][4 * g4 + 3]};
            st4(ob + (w * 32 + r) * KLD + 32 * n + 8 * g4 + 4 * h, v0 * sc);
        }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = srow + 32 * i;
        if (row0 + row < T) {
            float* op = dst + (int64_t)(row0 + row) * sr + scol;
#pragma unroll
            for (int n = 0; n < NB; ++n)
                if (scol + 32 * n < hd) st4(op + 32 * n, ld4(ob + row * KLD + scol + 32 * n));
        }
    }
    __syncthreads();
}

// workgroups per CU the kernels are compiled for (see the register note above)
constexpr int rb_dq_occupancy(int NB) { return NB <= 3 ? 2 : 1; }
constexpr int rb_dkv_occupancy(int NB) { return NB <= 2 ? 2 : 1; }

template <int NB>
__global__ __launch_bounds__(256, rb_dq_occupancy(NB)) void attn_rows_hd_bwd_dq_kernel(RowsHdBwdArgs a) {
    constexpr int KLD = 32 * NB + 4;   // LDS row stride (floats): odd number of 16-byte slots, conflict-free ds_read_b128 by row
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * RB_KT * KLD];   // [buf][K|V][key][KLD]; at the end [128][KLD]
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int hd = a.hd, T = a.T;
    const int n_bh = gridDim.x / a.n_blocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int q0 = (a.n_blocks - 1 - (int)(blockIdx.x / n_bh)) * RB_QB;      // heaviest query blocks first
    const int kvl = a.kv_len ? min(a.kv_len[b], T) : T;
    const int xl = a.mode == VH_MASK_PREFIX ? (a.x_len_dev ? a.x_len_dev[b] : a.x_len) : INT32_MAX;
    const int last_pos = min(q0 + RB_QB, T) - 1;
    const int kmax = min(kvl, max(xl, last_pos >= xl ? last_pos + 1 : 0));
    const int n_tiles = (kmax + RB_KT - 1) / RB_KT;

    const int qi = q0 + w * 32 + r;
    const bool qin = qi < T;
    // Q (pre-scaled) and dO fragments: lane holds row qi, columns 8 t + 4 h + j; zero at and beyond column hd
    f32x4 qf[4 * NB], df[4 * NB];
    float dsum = 0.f;
    {
        const int64_t row = min(qi, T - 1);
        const float* qp = a.q + b * a.q_sb + head * a.q_sh + row * a.q_sr;
        const float* dp = a.dout + b * a.d_sb + head * a.d_sh + row * a.d_sr;
        const float* op = a.o + b * a.o_sb + head * a.o_sh + row * a.o_sr;
#pragma unroll
        for (int t = 0; t < 4 * NB; ++t) {
            const int c = 8 * t + 4 * h, cc = min(c, hd - 4);
            const bool in = c < hd;
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const f32x4 ov = in ? ld4(op + cc) : z;
            qf[t] = in ? ld4(qp + cc) * a.qscale : z;
            df[t] = in ? ld4(dp + cc) : z;
            dsum += (df[t].x * ov.x + df[t].y * ov.y) + (df[t].z * ov.z + df[t].w * ov.w);
        }
    }
    dsum += __shfl_xor(dsum, 32, 64);
    const float lse = a.lse2[(int64_t)bh * T + min(qi, T - 1)];
    if (h == 0 && qin) a.dsum[(int64_t)bh * T + qi] = dsum;

    const float* kb = a.k + b * a.k_sb + head * a.k_sh;
    const float* vb = a.v + b * a.v_sb + head * a.v_sh;
    const int skey = tid >> 3, scol = (tid & 7) * 4;
    const uint32_t k_sr = (uint32_t)a.k_sr, v_sr = (uint32_t)a.v_sr;
    f32x4 rk[NB], rv[NB];
    auto lstore = [&](const f32x4 (&rs)[NB], int buf, int is_v) {
        float* d = lds + (2 * buf + is_v) * (RB_KT * KLD) + skey * KLD + scol;
#pragma unroll
        for (int i = 0; i < NB; ++i) st4(d + 32 * i, rs[i]);
    };
    f32x16 G[NB];                       // dQ^T: block n <-> d = 32 n + r
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) G[n][e] = 0.f;
    const int wpos_min = q0 + w * 32, wpos_max = wpos_min + 31;
    if (n_tiles > 0) {
        rb_gload<NB>(rk, kb, k_sr, 0, skey, scol, T, hd);
        rb_gload<NB>(rv, vb, v_sr, 0, skey, scol, T, hd);
        lstore(rk, 0, 0);
        lstore(rv, 0, 1);
    }
    __syncthreads();
    for (int kt = 0; kt < n_tiles; ++kt) {
        const int cur = kt & 1, k0 = kt * RB_KT;
        const bool more = kt + 1 < n_tiles;
        if (more) {
            rb_gload<NB>(rk, kb, k_sr, k0 + RB_KT, skey, scol, T, hd);
            rb_gload<NB>(rv, vb, v_sr, k0 + RB_KT, skey, scol, T, hd);
        }
        const bool any = k0 < kvl && (k0 < xl || (wpos_max >= xl && k0 <= wpos_max));
        if (any) {
            const float* ks = lds + cur * (2 * RB_KT * KLD);
            const float* vs = ks + RB_KT * KLD;
            f32x16 S, P;
#pragma unroll
            for (int t = 0; t < 4 * NB; ++t) {
                const f32x4 kf = ld4(ks + r * KLD + 8 * t + 4 * h);
                const f32x4 vf = ld4(vs + r * KLD + 8 * t + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {      // the first products start from the constant-zero C operand
                    S = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[t][j], (t | j) ? S : f32x16{}, 0, 0, 0);   // S^T[key][q]
                    P = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[j], df[t][j], (t | j) ? P : f32x16{}, 0, 0, 0);   // dP^T[key][q]
                }
            }
            // whole tile visible to every query of this wave (all of them rows of the view): no per-element mask
            const bool all = wpos_max < T && k0 + RB_KT <= kvl &&
                             (k0 + RB_KT <= xl || (wpos_min >= xl && k0 + RB_KT - 1 <= wpos_min));
            if (all) {
#pragma unroll
                for (int e = 0; e < 16; ++e) S[e] = vh_exp2(S[e] - lse) * (P[e] - dsum);   // dS^T[key][q]
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    const bool vis = qin && rb_visible(qi, key, kvl, xl);
                    S[e] = vis ? vh_exp2(S[e] - lse) * (P[e] - dsum) : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float* krow = ks + ((e & 3) + 8 * (e >> 2) + 4 * h) * KLD + r;
#pragma unroll
                for (int n = 0; n < NB; ++n)
                    G[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(krow[32 * n], S[e], G[n], 0, 0, 0);
            }
        }
        if (more) {
            lstore(rk, cur ^ 1, 0);
            lstore(rv, cur ^ 1, 1);
        }
        __syncthreads();
    }
    rb_store_rows<NB>(lds, G, a.scale, a.dq + b * a.g_sb + head * a.g_sh, a.g_sr, q0, T, hd, w, r, h, skey, scol);
}

template <int NB>
__global__ __launch_bounds__(256, rb_dkv_occupancy(NB)) void attn_rows_hd_bwd_dkv_kernel(RowsHdBwdArgs a) {
    constexpr int KLD = 32 * NB + 4;
    // [buf][Q|dO][query][KLD] + [buf][lse|D][32]; lds reused at the end as the [128][KLD] transpose buffer
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * RB_KT * KLD];
    __shared__ __attribute__((aligned(16))) float stat[2][2][RB_KT];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int hd = a.hd, T = a.T;
    const int n_bh = gridDim.x / a.n_blocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int kb0 = (int)(blockIdx.x / n_bh) * RB_QB;                          // first key of this block
    const int kvl = a.kv_len ? min(a.kv_len[b], T) : T;
    const int xl = a.mode == VH_MASK_PREFIX ? (a.x_len_dev ? a.x_len_dev[b] : a.x_len) : INT32_MAX;
    // queries that can see a key of this block: all of them for keys < xl (the full mask: every key), else q >= key
    const int qmin = kb0 >= xl ? kb0 : 0;
    const int t_first = qmin / RB_KT, n_tiles = (T + RB_KT - 1) / RB_KT;

    const int kj = kb0 + w * 32 + r;            // this lane's key
    const bool kin = kj < T;
    f32x4 kf[4 * NB], vf[4 * NB];               // K and V fragments: row kj, columns 8 t + 4 h + j; zero at and beyond hd
    {
        const int64_t row = min(kj, T - 1);
        const float* kp = a.k + b * a.k_sb + head * a.k_sh + row * a.k_sr;
        const float* vp = a.v + b * a.v_sb + head * a.v_sh + row * a.v_sr;
#pragma unroll
        for (int t = 0; t < 4 * NB; ++t) {
            const int c = 8 * t + 4 * h, cc = min(c, hd - 4);
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            kf[t] = c < hd ? ld4(kp + cc) : z;
            vf[t] = c < hd ? ld4(vp + cc) : z;
        }
    }
    const int sq = tid >> 3, scol = (tid & 7) * 4;   // staging: one query row, NB slots per operand
    const uint32_t q_sr = (uint32_t)a.q_sr, d_sr = (uint32_t)a.d_sr;
    const float* qbase = a.q + b * a.q_sb + head * a.q_sh;
    const float* dbase = a.dout + b * a.d_sb + head * a.d_sh;
    f32x4 rq[NB], rd[NB];
    float rstat = 0.f;
    auto gload = [&](int q0t) {
        rb_gload<NB>(rq, qbase, q_sr, q0t, sq, scol, T, hd);
        rb_gload<NB>(rd, dbase, d_sr, q0t, sq, scol, T, hd);
        if (tid < 2 * RB_KT) {
            const int qq = min(q0t + (tid & 31), T - 1);
            rstat = (tid < RB_KT ? a.lse2 : (const float*)a.dsum)[(int64_t)bh * T + qq];
        }
    };
    auto lstore = [&](int buf) {
        float* qd = lds + buf * (2 * RB_KT * KLD) + sq * KLD + scol;
        float* dd = qd + RB_KT * KLD;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            // Q is staged PRE-SCALED, as the forward holds it: S = (c Q) K^T then has the forward's bits, and
            // P = exp2(S - lse2) is the forward's own P (attention.hip, attn_bwd_dkv_kernel, says what goes wrong otherwise)
            st4(qd + 32 * i, rq[i] * a.qscale);
            st4(dd + 32 * i, rd[i]);
        }
        if (tid < 2 * RB_KT) stat[buf][tid >> 5][tid & 31] = rstat;
    };
    f32x16 GK[NB], GV[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) { GK[n][e] = 0.f; GV[n][e] = 0.f; }
    const int wk_min = kb0 + w * 32, wk_max = wk_min + 31;
    if (t_first < n_tiles) {
        gload(t_first * RB_KT);
        lstore(0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): K / V fragments landed on every path (attention.hip, attn_bwd_dkv_kernel)
    __syncthreads();
    for (int qt = t_first; qt < n_tiles; ++qt) {
        const int cur = (qt - t_first) & 1, q0t = qt * RB_KT;
        const bool more = qt + 1 < n_tiles;
        if (more) gload(q0t + RB_KT);
        const bool any = wk_min < kvl && (wk_min < xl || q0t + RB_KT - 1 >= wk_min);
        if (any) {
            const float* qs = lds + cur * (2 * RB_KT * KLD);
            const float* ds = qs + RB_KT * KLD;
            f32x16 S, P;
#pragma unroll
            for (int t = 0; t < 4 * NB; ++t) {
                const f32x4 qv = ld4(qs + r * KLD + 8 * t + 4 * h);
                const f32x4 dv = ld4(ds + r * KLD + 8 * t + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    S = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[j], kf[t][j], (t | j) ? S : f32x16{}, 0, 0, 0);   // S[q][key]
                    P = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[j], vf[t][j], (t | j) ? P : f32x16{}, 0, 0, 0);   // dP[q][key]
                }
            }
            // every (query of the tile, key of this wave) pair visible: no per-element mask
            const bool all = wk_max < kvl && q0t + RB_KT <= T && (wk_max < xl || (q0t >= xl && wk_max <= q0t));
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 lse4 = ld4(&stat[cur][0][8 * g4 + 4 * h]);
                const f32x4 d4 = ld4(&stat[cur][1][8 * g4 + 4 * h]);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int e = 4 * g4 + j;
                    const int qi = q0t + 8 * g4 + 4 * h + j;
                    const bool vis = all || (kin && qi < T && rb_visible(qi, kj, kvl, xl));
                    const float p = vis ? vh_exp2(S[e] - lse4[j]) : 0.f;
                    S[e] = p;                                       // P[q][key]
                    P[e] = vis ? p * (P[e] - d4[j]) : 0.f;          // dS[q][key]
                }
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int qrow = (e & 3) + 8 * (e >> 2) + 4 * h;
                const float* dorow = ds + qrow * KLD + r;
                const float* qrowp = qs + qrow * KLD + r;
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    GV[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(dorow[32 * n], S[e], GV[n], 0, 0, 0);    // dV^T[d][key]
                    GK[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(qrowp[32 * n], P[e], GK[n], 0, 0, 0);    // dK^T[d][key]
                }
            }
        }
        if (more) lstore(cur ^ 1);
        __syncthreads();
    }
    const int64_t goff = b * a.g_sb + head * a.g_sh;
    rb_store_rows<NB>(lds, GK, a.scale / a.qscale, a.dk + goff, a.g_sr, kb0, T, hd, w, r, h, sq, scol);   // summed over c Q
    rb_store_rows<NB>(lds, GV, 1.0f, a.dv + goff, a.g_sr, kb0, T, hd, w, r, h, sq, scol);
}

extern "C" size_t vh_attn_rows_hd_bwd_ws_bytes(int B, int n_heads, int T) {
    if (B <= 0 || n_heads <= 0 || T <= 0) return 0;
    return ((size_t)B * (size_t)n_heads * (size_t)T * sizeof(float) + 15) / 16 * 16;
}

extern "C" int vh_attn_rows_hd_bwd(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                                   const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                                   const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                                   const float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                                   const float* dout, int64_t d_sb, int64_t d_sh, int64_t d_sr,
                                   const float* lse2, float* dq, float* dk, float* dv, int64_t g_sb, int64_t g_sh, int64_t g_sr,
                                   int B, int n_heads, int head_dim, int T, float scale, int mode, int x_len,
                                   const int32_t* x_len_dev, const int32_t* kv_len, void* ws, size_t ws_bytes, void* stream) {
    VH_REQUIRE(q && k && v && out && dout && lse2 && dq && dk && dv && ws, VH_EINVAL,
               "vh_attn_rows_hd_bwd: null pointer (q=%p k=%p v=%p out=%p dout=%p lse2=%p dq=%p dk=%p dv=%p ws=%p)", (const void*)q,
               (const void*)k, (const void*)v, (const void*)out, (const void*)dout, (const void*)lse2, (const void*)dq,
               (const void*)dk, (const void*)dv, (const void*)ws);
    VH_REQUIRE(mode != VH_MASK_EXPLICIT, VH_EUNSUPPORTED,
               "vh_attn_rows_hd_bwd: mode=%d (VH_MASK_EXPLICIT): caller-supplied masks take the materialised route", mode);
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX, VH_EINVAL, "vh_attn_rows_hd_bwd: mode=%d", mode);
    VH_REQUIRE(B > 0 && n_heads > 0 && T > 0, VH_EINVAL, "vh_attn_rows_hd_bwd: bad dims B=%d h=%d T=%d", B, n_heads, T);
    VH_REQUIRE(head_dim % 4 == 0 && head_dim >= 16 && head_dim <= 128, VH_EUNSUPPORTED,
               "vh_attn_rows_hd_bwd: head_dim=%d (a multiple of 4 from 16 to 128)", head_dim);
    const int64_t strides[18] = {q_sb, q_sh, q_sr, k_sb, k_sh, k_sr, v_sb, v_sh, v_sr,
                                 o_sb, o_sh, o_sr, d_sb, d_sh, d_sr, g_sb, g_sh, g_sr};
    static const char* const stride_names[18] = {"q batch", "q head", "q row", "k batch", "k head", "k row",
                                                 "v batch", "v head", "v row", "out batch", "out head", "out row",
                                                 "dout batch", "dout head", "dout row", "grad batch", "grad head", "grad row"};
    for (int i = 0; i < 18; ++i)
        VH_REQUIRE(strides[i] % 4 == 0, VH_EINVAL,
                   "vh_attn_rows_hd_bwd: %s stride=%lld (a multiple of 4 floats: rows stay 16-byte aligned)", stride_names[i],
                   (long long)strides[i]);
    // the kernels address the rows they stage through LDS (k, v; q, dout) by a 32-bit byte offset from the (batch row, head) base
    const int64_t reach = ((1LL << 30) - head_dim) / (T > 1 ? T - 1 : 1);        // (no product that could overflow)
    VH_REQUIRE(q_sr >= 0 && k_sr >= 0 && v_sr >= 0 && d_sr >= 0 && q_sr <= reach && k_sr <= reach && v_sr <= reach && d_sr <= reach,
               VH_EUNSUPPORTED,
               "vh_attn_rows_hd_bwd: q row stride=%lld k row stride=%lld v row stride=%lld dout row stride=%lld with T=%d (the last "
               "row must lie within 4 GB of the first)", (long long)q_sr, (long long)k_sr, (long long)v_sr, (long long)d_sr, T);
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(k) && vh_aligned16(v) && vh_aligned16(out) && vh_aligned16(dout) &&
                   vh_aligned16(lse2) && vh_aligned16(dq) && vh_aligned16(dk) && vh_aligned16(dv) && vh_aligned16(ws),
               VH_EALIGN,
               "vh_attn_rows_hd_bwd: q=%p k=%p v=%p out=%p dout=%p lse2=%p dq=%p dk=%p dv=%p ws=%p must be 16-byte aligned",
               (const void*)q, (const void*)k, (const void*)v, (const void*)out, (const void*)dout, (const void*)lse2,
               (const void*)dq, (const void*)dk, (const void*)dv, (const void*)ws);
    const int nb = (int)(((int64_t)T + RB_QB - 1) / RB_QB);
    VH_REQUIRE((int64_t)B * n_heads <= 0x7fffffffLL / nb, VH_EINVAL,
               "vh_attn_rows_hd_bwd: B=%d h=%d T=%d: %d x %lld workgroups exceed one grid", B, n_heads, T, nb, (long long)B * n_heads);
    const size_t need = vh_attn_rows_hd_bwd_ws_bytes(B, n_heads, T);             // (after the grid check: B h T < 2^38)
    VH_REQUIRE(ws_bytes >= need, VH_EINVAL, "vh_attn_rows_hd_bwd: workspace of %zu bytes, need %zu", ws_bytes, need);
    RowsHdBwdArgs a{q, k, v, out, dout, lse2, (float*)ws, dq, dk, dv,
                    q_sb, q_sh, q_sr, k_sb, k_sh, k_sr, v_sb, v_sh, v_sr, o_sb, o_sh, o_sr, d_sb, d_sh, d_sr, g_sb, g_sh, g_sr,
                    n_heads, head_dim, T, mode, x_len, x_len_dev, kv_len, nb, scale * RB_LOG2E, scale};
    const dim3 grid(nb * B * n_heads), block(256);
    const hipStream_t st = (hipStream_t)stream;
    switch ((head_dim + 31) / 32) {
    case 1:
        hipLaunchKernelGGL(attn_rows_hd_bwd_dq_kernel<1>, grid, block, 0, st, a);
        hipLaunchKernelGGL(attn_rows_hd_bwd_dkv_kernel<1>, grid, block, 0, st, a);
        break;
    case 2:
        hipLaunchKernelGGL(attn_rows_hd_bwd_dq_kernel<2>, grid, block, 0, st, a);
        hipLaunchKernelGGL(attn_rows_hd_bwd_dkv_kernel<2>, grid, block, 0, st, a);
        break;
    case 3:
        hipLaunchKernelGGL(attn_rows_hd_bwd_dq_kernel<3>, grid, block, 0, st, a);
        hipLaunchKernelGGL(attn_rows_hd_bwd_dkv_kernel<3>, grid, block, 0, st, a);
        break;
    default:
        hipLaunchKernelGGL(attn_rows_hd_bwd_dq_kernel<4>, grid, block, 0, st, a);
        hipLaunchKernelGGL(attn_rows_hd_bwd_dkv_kernel<4>, grid, block, 0, st, a);
        break;
    }
    VH_CHECK_LAUNCH("vh_attn_rows_hd_bwd");
    return VH_OK;
}
