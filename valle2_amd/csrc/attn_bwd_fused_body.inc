// The body of the five-product backward kernels, included by attention.hip once per kernel (ATTN_BWD_PACKED 0:
// attn_bwd_fused_kernel<FW>(BwdArgs), 1: attn_bwd_packed_kernel<FW>(BwdArgs, PackedBwdSegs)).  An include for the reason
// attn_rows_body.inc is one: attn_bwd_fused_kernel sits at the register limit, and stamped out as the kernel itself, with the
// BW_* macros below expanding to its own expressions, it compiles to the instructions it had before the packed kernel existed.
//
// One workgroup = one chunk of up to FW x 32 keys of one (sequence, head) against that sequence's queries in 32-query tiles.
// The sequence is batch row b of a padded (B, T, ·) layout (every mask mode, key padding) or one segment of a packed row
// stream (full or prefix mask per segment, no padding key): there T = kvl = the segment's length, row 0 of the sequence is row
// seg_start of q / out / dout / dq / dk / dv and of the head's K/V stream, lse2 and the slabs are laid out (n_heads, M), and
// the (segment, chunk) pair comes from a host-built table.  The segment's first row goes into the 64-bit bases; every
// per-lane byte offset stays relative to it (32 bits), so M x ld x 4 may exceed 2^32.
template <int FW>
#if ATTN_BWD_PACKED
__global__ __launch_bounds__(FW * 64, FW == 8 ? 1 : 2) void attn_bwd_packed_kernel(BwdArgs a, PackedBwdSegs ps) {
#else
__global__ __launch_bounds__(FW * 64, FW == 8 ? 1 : 2) void attn_bwd_fused_kernel(BwdArgs a) {
#endif
    constexpr int KEYS = FW * 32;                    // row length of Kt and dS
    constexpr int RPT = 8 / FW;                      // staged tile rows per thread (32 rows x 16 threads over FW x 64 threads)
    constexpr int QB_W = 8 / FW;                     // 16-query blocks of the dQ tile per wave (FW = 4: both, one d-block per wave)
    // [Q|dO][query][KLD] | [lse|D][32] | Kt [64 d][KEYS] | dS [32 q][KEYS]
    __shared__ __attribute__((aligned(16))) float lds[2 * KT * KLD + 2 * KT + HD * KEYS + KT * KEYS];
    float* const stat = lds + 2 * KT * KLD;
    float* const kt = stat + 2 * KT;
    float* const dsb = kt + HD * KEYS;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
#if ATTN_BWD_PACKED
    // work item = blockIdx.x / n_heads of the host's table, heaviest first; id % n_heads is the head.  An entry out of range
    // (workgroup-uniform) returns before it touches memory: a.n_blocks is the number of slabs the workspace holds.
    const int item = blockIdx.x / a.n_heads;
    const int head = blockIdx.x - item * a.n_heads;
    const int seg = ps.items[2 * item], chunk = ps.items[2 * item + 1];
    if ((unsigned)seg >= (unsigned)ps.n_seg || (unsigned)chunk >= (unsigned)a.n_blocks) return;
    const int s0 = ps.seg_start[seg], len = ps.seg_len[seg];
    if (s0 < 0 || len < 1 || (int64_t)s0 + len > ps.n_rows) return;
    const int kb0 = chunk * a.chunk_keys;
    if (kb0 >= len) return;
    const int kend = min(kb0 + a.chunk_keys, len);              // keys [kb0, kend) belong to this workgroup
    const int pmode = a.mode == VH_MASK_PREFIX ? VH_MASK_PREFIX : VH_MASK_FULL;
    const int kvl = len;                                        // no key of a segment is padding
    const int xl = pmode == VH_MASK_PREFIX ? min(max(ps.seg_x_len[seg], 0), len) : 0;
    const int sq = tid >> 4, squad = (tid & 15) * 4;
#define BW_T len                                               /* queries = keys = the segment's rows */
#define BW_MODE pmode
#define BW_ROW0 (int64_t)s0                                    /* row of q / o / dout / dq / dk / dv that holds the sequence's row 0 */
#define BW_KVROW(k) ((int64_t)head * a.S_max + s0 + (k))       /* key k of the sequence in the head's K / V stream */
#define BW_STAT(p, i) (p)[(int64_t)head * ps.n_rows + s0 + (i)]
#define BW_SLAB (a.slab + (((int64_t)chunk * a.n_heads + head) * ps.n_rows + s0) * HD)
#define BW_VISIBLE(qi, key) ((key) < kvl && (pmode != VH_MASK_PREFIX || (key) < xl || ((qi) >= xl && (key) <= (qi))))
#else
#define BW_T a.T
#define BW_MODE a.mode
#define BW_ROW0 (int64_t)b * a.T
#define BW_KVROW(k) ((int64_t)bh * a.S_max + (k))
#define BW_STAT(p, i) (p)[(int64_t)bh * a.T + (i)]
#define BW_SLAB (a.slab + ((int64_t)chunk * n_bh + bh) * a.T * HD)
#define BW_VISIBLE(qi, key) bwd_visible(a, b, qi, key, kvl, xl)
    const int n_bh = gridDim.x / a.n_blocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int chunk = (int)(blockIdx.x / n_bh);                 // chunk 0 first: under the prefix mask it sees every query
    const int kb0 = chunk * a.chunk_keys;
    const int kend = min(kb0 + a.chunk_keys, a.T);              // keys [kb0, kend) belong to this workgroup
    const int kvl = a.kv_len ? min(a.kv_len[b], a.T) : a.T;
    const int xl = a.x_len_dev ? a.x_len_dev[b] : a.x_len;
    const int sq = tid >> 4, squad = (tid & 15) * 4;            // staging: row sq (+ 16 with four waves), one 16-byte chunk

    if (a.mode != VH_MASK_EXPLICIT && kb0 >= kvl) {
        // every key of the chunk is padding: dK = dV = 0, no dQ contribution (the reduce kernel skips this chunk too)
        for (int row = kb0 + sq; row < kend; row += FW * 4) {
            const int64_t o = ((int64_t)b * a.T + row) * a.ldg + head * HD + squad;
            st4(a.dk + o, f32x4{0.f, 0.f, 0.f, 0.f});
            st4(a.dv + o, f32x4{0.f, 0.f, 0.f, 0.f});
        }
        // a single chunk writes dQ itself (no slab, no reduce launch): a row without any valid key (kv_len = 0, T <= 256)
        // must leave zeros there, not the caller's uninitialised buffer (round-4 advisor finding)
        if (a.slab == nullptr)
            for (int row = sq; row < a.T; row += FW * 4)
                st4(a.dq + ((int64_t)b * a.T + row) * a.ldg + head * HD + squad, f32x4{0.f, 0.f, 0.f, 0.f});
        return;
    }
#endif
    int qmin = 0;
    if (BW_MODE == VH_MASK_PREFIX && kb0 >= xl) qmin = kb0;
    const int t_first = qmin / KT, n_tiles = (BW_T + KT - 1) / KT;

    const int wk_min = kb0 + w * 32, wk_max = wk_min + 31;
    const int kj = wk_min + r;                   // this lane's key
    const bool kin = kj < kend;
    const float qscale = 0.125f * LOG2E;
    f32x4 kf[8], vf[8];
    {
        const int64_t krow = BW_KVROW(min(kj, BW_T - 1));
        const float* kp = a.kc + krow * HD + 4 * h;
        const float* vp = a.vc + krow * HD + 4 * h;
        const int kl = w * 32 + r;               // key inside the chunk
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            kf[t] = ld4(kp + 8 * t);
            vf[t] = ld4(vp + 8 * t);
#pragma unroll
            for (int j = 0; j < 4; ++j) {        // Kt[d][key], 16-byte slot (key >> 2) XOR-swizzled by d & 15
                const int d = 8 * t + 4 * h + j;
                kt[d * KEYS + ((((kl >> 2) ^ (d & 15)) << 2) | (kl & 3))] = kf[t][j];
            }
        }
    }
    f32x4 rq[RPT], rd[RPT], ro[RPT];
    float rlse = 0.f;
    const float* qbase = a.q + BW_ROW0 * a.ldq + head * HD;
    const float* dbase = a.dout + BW_ROW0 * a.lddo + head * HD;
    const float* obase = a.o + BW_ROW0 * a.ldo + head * HD;
    // loads only: nothing here may wait for them.  Q and dO rows are requested at the top of a tile and land under its
    // MFMAs; the O row (needed only for D) and lse are requested after the tile's first barrier, when the S / dP
    // registers are dead (the kernel sits at the register limit), and land under the dQ product.
    // (four waves stage two rows per thread: the second row's Q / dO are requested late as well — eight registers less
    // across the S / dP / dV / dK phase, where the count peaks)
    auto gload = [&](int q0t) {
        const int qrow = min(q0t + sq, BW_T - 1);
        rq[0] = ld4((const float*)((const char*)qbase + (uint32_t)(qrow * a.ldq + squad) * 4u));
        rd[0] = ld4((const float*)((const char*)dbase + (uint32_t)(qrow * a.lddo + squad) * 4u));
    };
    auto gload_late = [&](int q0t) {
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            const int qrow = min(q0t + sq + 16 * i, BW_T - 1);
            if (i > 0) {
                rq[i] = ld4((const float*)((const char*)qbase + (uint32_t)(qrow * a.ldq + squad) * 4u));
                rd[i] = ld4((const float*)((const char*)dbase + (uint32_t)(qrow * a.lddo + squad) * 4u));
            }
            ro[i] = ld4((const float*)((const char*)obase + (uint32_t)(qrow * a.ldo + squad) * 4u));
        }
        if (tid < KT) rlse = BW_STAT(a.lse2, min(q0t + tid, BW_T - 1));
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            st4(lds + (sq + 16 * i) * KLD + squad, rq[i] * qscale);     // pre-scaled, as the forward holds Q (attn_bwd_dkv_kernel)
            st4(lds + KT * KLD + (sq + 16 * i) * KLD + squad, rd[i]);
            const float dsum = row16_sum((rd[i].x * ro[i].x + rd[i].y * ro[i].y) + (rd[i].z * ro[i].z + rd[i].w * ro[i].w));
            if ((tid & 15) == 0) stat[KT + sq + 16 * i] = dsum;                  // D of the staged row
        }
        if (tid < KT) stat[tid] = rlse;
    };
    f32x16 GK0, GK1, GV0, GV1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { GK0[e] = 0.f; GK1[e] = 0.f; GV0[e] = 0.f; GV1[e] = 0.f; }
    // the dQ block(s) of this wave: d0 = 16 (w & 3); q0 = 16 (w >> 2) with eight waves, both q-blocks with four;
    // lane (i, g) reads row i of both operands
    const int mi = lane & 15, mg = lane >> 4;
    const float* ap = kt + (16 * (w & 3) + mi) * KEYS;
    const float* bp = dsb + (FW == 8 ? 16 * (w >> 2) + mi : mi) * KEYS;
    const int n_waves_keys = (kend - kb0 + 31) >> 5;            // waves that own at least one key of the chunk
    if (t_first < n_tiles) {
        gload(t_first * KT);
        gload_late(t_first * KT);
        lstore();
    }
    // vmcnt(0), unconditionally: the K / V fragments are first USED inside the loop and are still outstanding on the path
    // around the conditional above — without this the wait insertion puts vmcnt(3..0) in front of the first score MFMAs
    // of EVERY tile, which makes the tile wait for its own prefetch of the next Q / dO rows (seen in the ISA, round 6)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    for (int qt = t_first; qt < n_tiles; ++qt) {
        const int q0t = qt * KT;
        if (qt + 1 < n_tiles) gload(q0t + KT);
        // waves of this workgroup that see a query of the tile: a prefix of the waves (every term falls with the key index)
        int n_act = n_waves_keys;
        if (BW_MODE != VH_MASK_EXPLICIT) {
            n_act = min(n_act, (kvl - kb0 + 31) >> 5);
            if (BW_MODE == VH_MASK_PREFIX) {
                // wave v is active iff kb0 + 32 v < xl  or  kb0 + 32 v <= q0t + 31
                const int lim = max(xl - 1, q0t + KT - 1) - kb0;   // largest admissible 32 v
                n_act = min(n_act, lim < 0 ? 0 : (lim >> 5) + 1);
            }
        }
        const bool any = w < n_act;
        const float* qs = lds;
        const float* ds = qs + KT * KLD;
        const float* st = stat;
        if (any) {
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
            bool all = wk_max < min(kvl, kend) && q0t + KT <= BW_T;
            if (BW_MODE == VH_MASK_PREFIX) all = all && (wk_max < xl || (q0t >= xl && wk_max <= q0t));
            else if (BW_MODE == VH_MASK_EXPLICIT) all = false;
            if (all) {
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4) {
                    const f32x4 lse4 = ld4(st + 8 * g4 + 4 * h);
                    const f32x4 d4 = ld4(st + KT + 8 * g4 + 4 * h);
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
                    const f32x4 lse4 = ld4(st + 8 * g4 + 4 * h);
                    const f32x4 d4 = ld4(st + KT + 8 * g4 + 4 * h);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int e = 4 * g4 + j;
                        const int qi = q0t + 8 * g4 + 4 * h + j;
                        const bool vis = kin && qi < BW_T && BW_VISIBLE(qi, kj);
                        const float p = vis ? vh_exp2(S[e] - lse4[j]) : 0.f;
                        S[e] = p;
                        P[e] = p * (P[e] - d4[j]);
                    }
                }
            }
            // dS → the shared tile, [q][key] with the slot swizzle: one ds_write_b32 per register, 32 consecutive keys per half-wave
            {
                const int kl = w * 32 + r;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int qrow = (e & 3) + 8 * (e >> 2) + 4 * h;
                    dsb[qrow * KEYS + ((((kl >> 2) ^ (qrow & 15)) << 2) | (kl & 3))] = P[e];
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
        __syncthreads();                     // the dS blocks of the n_act active waves are in LDS; the Q / dO tile is free
        if (qt + 1 < n_tiles) gload_late(q0t + KT);
        {
            // dQ[q][d] block = Σ_key dS[q][key]·K[key][d] over the active waves' keys: A = Kᵀ rows (d), B = dS rows (q)
            f32x4 c[QB_W][4];
#pragma unroll
            for (int qb = 0; qb < QB_W; ++qb)
#pragma unroll
                for (int j = 0; j < 4; ++j) c[qb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int nu = 2 * n_act;                    // 16-key groups of the active waves (n_act >= 1 on every visited tile)
            f32x4 a4 = ld4(ap + ((mg ^ mi) << 2)), b4[QB_W];
#pragma unroll
            for (int qb = 0; qb < QB_W; ++qb) b4[qb] = ld4(bp + qb * 16 * KEYS + ((mg ^ mi) << 2));
            for (int u = 0; u < nu; ++u) {               // operands of group u + 1 requested BEFORE group u's MFMAs
                const int slot = ((4 * min(u + 1, nu - 1) + mg) ^ mi) << 2;
                const f32x4 an = ld4(ap + slot);
                f32x4 bn[QB_W];
#pragma unroll
                for (int qb = 0; qb < QB_W; ++qb) bn[qb] = ld4(bp + qb * 16 * KEYS + slot);
                __builtin_amdgcn_sched_barrier(0);       // (left alone the compiler sinks the reads below the MFMAs)
#pragma unroll
                for (int qb = 0; qb < QB_W; ++qb)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        c[qb][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b4[qb][j], c[qb][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                a4 = an;
#pragma unroll
                for (int qb = 0; qb < QB_W; ++qb) b4[qb] = bn[qb];
            }
            const uint32_t dcol = 16 * (w & 3) + 4 * mg;
#pragma unroll
            for (int qb = 0; qb < QB_W; ++qb) {
                const f32x4 cc = (c[qb][0] + c[qb][1]) + (c[qb][2] + c[qb][3]);   // lane (q = mi, d = 4 mg + e)
                const int qi = q0t + (FW == 8 ? 16 * (w >> 2) : 16 * qb) + mi;
                if (qi < BW_T) {                         // wave-uniform 64-bit base + one 32-bit lane offset
                    if (a.slab) st4((float*)((char*)BW_SLAB + (uint32_t)(qi * HD + dcol) * 4u), cc);
                    else st4((float*)((char*)(a.dq + BW_ROW0 * a.ldg + head * HD) + (uint32_t)(qi * a.ldg + dcol) * 4u), cc * 0.125f);
                }
            }
        }
        if (qt + 1 < n_tiles) lstore();
        __syncthreads();                     // next tile staged; every wave is done with this tile's dS
    }
    // ---- dK, dV: transposed through LDS (everything above is dead), whole rows out
    float* ob = lds;                         // [KEYS][KLD]
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
            const int row = sq + FW * 4 * i;
            if (kb0 + row < kend)
                st4(dst + (BW_ROW0 + kb0 + row) * a.ldg + head * HD + squad, ld4(ob + row * KLD + squad));
        }
        __syncthreads();
    }
#undef BW_T
#undef BW_MODE
#undef BW_ROW0
#undef BW_KVROW
#undef BW_STAT
#undef BW_SLAB
#undef BW_VISIBLE
}
