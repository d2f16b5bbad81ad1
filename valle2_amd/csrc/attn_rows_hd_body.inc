// The body of attention_rows_hd.hip's two kernels, included once per value of ATTN_ROWS_HD_LSE:
//   0: attn_rows_hd_kernel<NB>(RowsHdArgs)              — the inference forward; compiles to what it was before the other existed
//   1: attn_rows_hd_lse_kernel<NB>(RowsHdArgs, lse2)    — the training forward: also stores lse2[(b h + head) Tq + qi] =
//      m + log2(l), the base-2 log-sum-exp of the row's scaled scores (vh_attn_rows_lse's units), which the backward
//      (attention_rows_hd_bwd.hip) recomputes P from
template <int NB>
#if ATTN_ROWS_HD_LSE
__global__ __launch_bounds__(256, 2) void attn_rows_hd_lse_kernel(RowsHdArgs a, float* lse2) {
#else
__global__ __launch_bounds__(256, 2) void attn_rows_hd_kernel(RowsHdArgs a) {
#endif
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
#if ATTN_ROWS_HD_LSE
    if (h == 0 && qi < a.Tq) lse2[(int64_t)bh * a.Tq + qi] = m + log2f(ltot);   // fully masked row: -inf
#endif
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
