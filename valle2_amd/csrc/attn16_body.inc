// The body of the 16-bit many-row attention kernels, included by bf16.hip once per kernel (ATTN16_PACKED 0: attn16_kernel,
// 1: attn16_packed_kernel, 2: attn16_packed_lm_kernel), as attn_rows_body.inc is by attention.hip and for its reason: stamped
// out as the kernel itself the text compiles for attn16_kernel to the instructions it had before the packed kernels existed.
// What differs between them — the sequence's lengths, its first row, its K/V base and the workgroup's first query — is spelt
// by the A16_* macros below, which expand to attn16_kernel's own expressions.
//
// One workgroup = 128 queries (4 waves x 32) of one (sequence, head) over that sequence's keys in 64-key tiles.  The sequence
// is batch row b of a padded (B, Tq, ·) layout (attn16_kernel, FULL / PREFIX mask) or one segment of a packed row stream
// (attn16_packed_kernel, full mask; attn16_packed_lm_kernel, the prefix-LM mask of the segment's own text length
// seg_x_len[seg]): there Tq = Tk = kvl = the segment's length, row 0 of the sequence is row seg_start of
// q / out / the one K/V stream, and everything below — the ring of three images, the clamp of a tail tile to the
// sequence's own last row, the waits, the arithmetic and the epilogue — is the same code.
#if ATTN16_PACKED == 2
__global__ __launch_bounds__(256, 2) void attn16_packed_lm_kernel(Attn16Args a, Packed16LmSegs ps) {
#elif ATTN16_PACKED
__global__ __launch_bounds__(256, 2) void attn16_packed_kernel(Attn16Args a, Packed16Segs ps) {
#else
__global__ __launch_bounds__(256, 2) void attn16_kernel(Attn16Args a) {
#endif
    __shared__ __attribute__((aligned(16))) char lds[A16_RING * 2 * A16_KT * 128];   // ring of [K | V][64 keys][128 B] = 48 KB
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
#if ATTN16_PACKED
    // table row = blockIdx.x / n_heads, longest segment first (its blocks visit the most tiles); id % n_heads is the head.  With
    // n_heads % 8 == 0 every query block of one (segment, head) lands on the same XCD: its K / V is fetched into one L2.
    const int blk = blockIdx.x / a.n_heads;
    const int head = blockIdx.x - blk * a.n_heads;
    const int seg = ps.blocks[2 * blk], bq0 = ps.blocks[2 * blk + 1];
    if ((unsigned)seg >= (unsigned)ps.n_seg) return;          // (workgroup-uniform: a table the caller got wrong reads nothing)
    const int s0 = ps.seg_start[seg];
    if (s0 < 0 || s0 >= a.S_max) return;
    const int len = min(ps.seg_len[seg], a.S_max - s0);       // never a cache row at or beyond S_max, whatever the table says
    if (bq0 < 0 || bq0 >= len) return;                        // (all of these before the first DMA and the first barrier)
#if ATTN16_PACKED == 2
    // the segment's text length, clamped to 0 .. len (a text length beyond the segment is full visibility, as in attn16_kernel)
    const int q_off = 0, kvl = len, xl = min(max(ps.seg_x_len[seg], 0), len);
    const bool prefix = true;
#else
    const int q_off = 0, kvl = len, xl = 0;
    const bool prefix = false;
#endif
#define A16_TQ len                                            /* queries = keys = the segment's rows */
#define A16_TK len
#define A16_QBLK0 bq0                                         /* the workgroup's first query inside the sequence */
#define A16_ROW0 ((int64_t)s0)                                /* row of q / out that holds the sequence's query 0 */
#define A16_KV(p) ((p) + ((int64_t)head * a.S_max + s0) * VH_HEAD_DIM)   /* the sequence's key 0 in the head's K / V stream */
#else
    // Workgroup ids go round-robin over the 8 XCDs, each with its own L2; the grid is padded to 8 x ceil(n_bh / 8) (batch row,
    // head) pairs x n_qb query blocks.  FULL mask (every block of a pair costs the same): XCD x takes the pairs x, x + 8, ... and
    // runs the query blocks of ONE pair back to back, so the pair's K / V (2 x Tk x 128 B) is fetched once into that L2 and
    // re-read from there by the other blocks (NAR-stage shape: 0.93x the time of the order below).  PREFIX mask: the last
    // query block of a pair sees up to 4x the keys of the first, and the launch wants the heaviest blocks of ALL pairs
    // first (grouped by pair it took 1.4x the time at the prompt-pass shape); a pair's blocks still share an XCD.
    const int n_bh8 = (a.B * a.n_heads + 7) & ~7;
    int bh, qb;
    // (grouped only when the pairs deal evenly over the 8 XCDs, or are many: 4 pairs would leave half the chip without work)
    if (a.mode == VH_MASK_FULL && (a.B * a.n_heads == n_bh8 || a.B * a.n_heads >= 64)) {
        bh = (int)(blockIdx.x & 7) + 8 * (int)((blockIdx.x >> 3) / a.n_qb);
        qb = (int)((blockIdx.x >> 3) % a.n_qb);
    } else {
        bh = (int)(blockIdx.x % n_bh8);
        qb = a.n_qb - 1 - (int)(blockIdx.x / n_bh8);
    }
    if (bh >= a.B * a.n_heads) return;                       // (the whole workgroup)
    const int b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int q_off = a.Tk - a.Tq;
    const int kvl = a.kv_len ? min(a.kv_len[b], a.Tk) : a.Tk;
    const int xl = a.mode == VH_MASK_PREFIX ? (a.x_len_dev ? a.x_len_dev[b] : a.x_len) : 0;
    const bool prefix = a.mode == VH_MASK_PREFIX;
#define A16_TQ a.Tq
#define A16_TK a.Tk
#define A16_QBLK0 (qb * A16_QB)
#define A16_ROW0 ((int64_t)b * a.Tq)
#define A16_KV(p) ((p) + ((int64_t)b * a.n_heads + head) * a.S_max * VH_HEAD_DIM)
#endif

    const int q0 = A16_QBLK0 + 32 * w;                       // this wave's first query
    const int qi = min(q0 + r, A16_TQ - 1);                  // this lane's query (clamped: rows beyond Tq are never stored)
    const int qpos = q_off + qi;
    // this lane's query sees exactly the keys [0, klim): key < kv_len and (key < x_len or (qpos >= x_len and key <= qpos))
    const int klim = prefix ? min(kvl, qpos >= xl ? qpos + 1 : xl) : kvl;
    // keys any query of the WORKGROUP can see: [0, kend)
    const int wg_qlast = q_off + min(A16_QBLK0 + A16_QB, A16_TQ) - 1;
    int kend = kvl;
    if (prefix) kend = min(kvl, wg_qlast >= xl ? max(xl, wg_qlast + 1) : xl);
    const int n_tiles = (kend + A16_KT - 1) / A16_KT;
    // ... and of this WAVE (wave-uniform): tiles from wave_kend on are skipped by the wave (it still stages and syncs)
    const int wv_qfirst = q_off + min(q0, A16_TQ - 1), wv_qlast = q_off + min(q0 + 31, A16_TQ - 1);
    int wave_kend = kvl;
    if (prefix) wave_kend = min(kvl, wv_qlast >= xl ? max(xl, wv_qlast + 1) : xl);

    // staging by LDS-DMA (global_load_lds_dwordx4: one 1-KiB piece = 8 key rows x 128 B per wave-instruction, no staging
    // registers, no ds_write): a tile is 8 pieces of K + 8 of V; waves 0 / 1 bring the K rows 0..31 / 32..63, waves 2 / 3
    // the V rows.  Lane L fills slot (row L >> 3 of the piece, 16-byte chunk L & 7) of the lane-linear image, so it FETCHES
    // chunk (L & 7) ^ swz(row): the swizzle lives in the source address.  Keys beyond Tk re-read the last written row
    // (a masked weight is 0, but 0 x the NaN an unwritten cache row may hold is NaN).  Three images in a ring: tile t + 2 is
    // requested at the top of tile t (two tiles of flight time); the barrier at the end of tile t orders tile t + 1.
    const bool stage_v = w >= 2;
    const char* sbase = (const char*)A16_KV(stage_v ? a.vc : a.kc);
    const uint32_t lds0 = (uint32_t)(uintptr_t)lds + (stage_v ? A16_KT * 128 : 0) + (w & 1) * 4096;
    int srow[4];
    uint32_t schunk[4], soff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        srow[i] = 32 * (w & 1) + 8 * i + (lane >> 3);
        const int swz = stage_v ? ((srow[i] >> 1) & 1) << 2 : (srow[i] >> 1) & 7;
        schunk[i] = (uint32_t)(((lane & 7) ^ swz) << 4);
        soff[i] = (uint32_t)srow[i] * 128u + schunk[i];      // byte offset inside a tile that lies wholly below Tk
    }
    auto dma_tile = [&](int k0, int buf) {
        const bool whole = k0 + A16_KT <= A16_TK;             // (wave-uniform) no row of the tile needs the clamp
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t voff = whole ? soff[i] + (uint32_t)k0 * 128u : (uint32_t)min(k0 + srow[i], A16_TK - 1) * 128u + schunk[i];
            const uint32_t dst = lds0 + buf * (2 * A16_KT * 128) + i * 1024;
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(dst), "v"(voff), "s"(sbase) : "memory");
        }
    };
    if (n_tiles > 0) dma_tile(0, 0);
    if (n_tiles > 1) dma_tile(A16_KT, 1);

    // Q^T fragments (B operand of S^T = K Q^T): lane (r, h) holds Q'[query r][d = 16 s + 8 h + j].  Q' = c Q with
    // c = 1 / sqrt(64) * log2(e) comes PRE-SCALED from the producer (vh_linear_qkv_bf16 scales in fp32 before the one
    // narrowing: no second rounding), so the score accumulators are base-2 exponents.
    bf16x8 qf[4];
    {
        const uint16_t* qr = a.q + (A16_ROW0 + qi) * a.ldq + head * VH_HEAD_DIM + 8 * h;
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = __builtin_bit_cast(bf16x8, ldq(qr + 16 * s));
    }
    // Softmax without a per-element subtraction or sum (the kernel is bound by vector ISSUE slots, ~200 per 32 x 64 scores
    // before this; profiles/r6_pmc_attn16.md): the reference point m_ref of a row moves only when a tile's maximum exceeds it
    // by more than A16_LAZY (weights then reach at most 2^A16_LAZY: exact in the 16-bit formats, fp32 sums), and -m_ref sits
    // in sixteen registers that are the INITIAL ACCUMULATOR of the score MFMAs — the chain delivers c S - m_ref, the weight
    // is one v_exp_f32 of that.  The row sum comes out of the matrix pipe as well: a third accumulator block whose A operand
    // is 1 on rows 0 and 4 (lacc[0] of every lane = its query's sum over both key halves, taken from the ROUNDED weights
    // the products see).  Moving m_ref rescales O, the sums and the pending scores by 2^-delta, all of them (tile 0 always moves).
    f32x16 oacc[2], lacc, minit;
#pragma unroll
    for (int e = 0; e < 16; ++e) { oacc[0][e] = 0.f; oacc[1][e] = 0.f; lacc[e] = 0.f; minit[e] = 0.f; }
    float m_ref = 0.f;
    bf16x8 ones;
    {
        const uint32_t one2 = vh_pack_h16(1.f, 1.f), w1 = (r == 0 || r == 4) ? one2 : 0u;
        ones = __builtin_bit_cast(bf16x8, u32x4{w1, w1, w1, w1});
    }

    // K fragment addresses (A operand of S^T): key row 32 u + r, chunk (2 s + h) ^ ((r >> 1) & 7)
    const int kswz = (r >> 1) & 7;
    // V^T fragment addresses: group g = lane >> 4 (h = g >> 1), lane 4 q4 + p of the group supplies key row kb + q4,
    // columns d = 32 db + 16 (g & 1) + 4 p .. + 3 -> chunk 4 db + 2 (g & 1) + (p >> 1), byte 8 (p & 1) in it
    const int g = lane >> 4, q4 = (lane >> 2) & 3, p = lane & 3;

    // vmcnt(0), unconditionally and BEFORE the loop: the first two tiles and the Q fragments have landed.  (The Q fragments
    // are first used inside the loop; left to the compiler's wait insertion, vmcnt(3..0) lands in front of the first four
    // score MFMAs of EVERY tile — a wait for the tile's own prefetches.  Seen in the ISA in round 6.)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int buf = 0;
    for (int it = 0; it < n_tiles; ++it) {
        const int k0 = it * A16_KT;
        const bool ahead = it + 2 < n_tiles;                 // (wave-uniform)
        if (ahead) dma_tile(k0 + 2 * A16_KT, buf >= 1 ? buf - 1 : 2);      // into image (it + 2) % 3, free since the last barrier
        if (k0 < wave_kend) {
            const char* kl = lds + buf * 2 * A16_KT * 128;
            const char* vl = kl + A16_KT * 128;
            // ---- c S^T - m_ref = K (c Q)^T + (-m_ref) for the two 32-key sub-tiles
            f32x16 sacc[2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bf16x8 kf = __builtin_bit_cast(bf16x8, ldq(kl + (32 * u + r) * 128 + (((2 * s + h) ^ kswz) << 4)));
                    sacc[u] = VH_MFMA16(kf, qf[s], s ? sacc[u] : minit);
                }
            // ---- mask (only on tiles that need it: wave-uniform test): register x of sub-tile u holds key
            // k0 + 32 u + (x & 3) + 8 (x >> 2) + 4 h, visible iff it is below the lane's bound — one compare + select each
            const bool need_mask = k0 + A16_KT > kvl || (prefix && k0 + A16_KT > xl && (wv_qfirst < xl || k0 + A16_KT - 1 > wv_qfirst));
            if (need_mask) {
                const int t = klim - k0 - 4 * h;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int x = 0; x < 16; ++x) sacc[u][x] = 32 * u + (x & 3) + 8 * (x >> 2) < t ? sacc[u][x] : A16_NEG;
            }
            // ---- the tile's row maximum relative to m_ref (the query's other key half sits in lane ^ 32)
            float mx = A16_NEG;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int x = 0; x < 16; ++x) mx = fmaxf(mx, sacc[u][x]);
            {
                const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, mx), __builtin_bit_cast(uint32_t, mx), false, false);
                mx = fmaxf(__builtin_bit_cast(float, sw[0]), __builtin_bit_cast(float, sw[1]));
            }
            if (it == 0 || __builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(mx > A16_LAZY) != 0)) {
                // move the reference point: to the row's maximum on the first tile, up to it (never down) later
                // (a row without any visible key in tile 0 — none under the analytic masks while kv_len >= 1 — stays at 0)
                const float delta = it == 0 ? (mx > 0.5f * A16_NEG ? mx : 0.f) : fmaxf(mx, 0.f);
                m_ref += delta;
                const float alpha = vh_exp2(-delta);
#pragma unroll
                for (int e = 0; e < 16; ++e) { minit[e] = -m_ref; sacc[0][e] -= delta; sacc[1][e] -= delta; }
                if (it) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) { oacc[0][e] *= alpha; oacc[1][e] *= alpha; }
                    lacc[0] *= alpha;
                }
            }
            // ---- P^T = 2^(c S - m_ref) narrowed into the B operands (keys of a k-step in accumulator order)
            bf16x8 pf[2][2];
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    u32x4 pk;
#pragma unroll
                    for (int j = 0; j < 4; ++j) pk[j] = vh_pack_h16_unit(vh_exp2(sacc[u][8 * s + 2 * j]), vh_exp2(sacc[u][8 * s + 2 * j + 1]));
                    pf[u][s] = __builtin_bit_cast(bf16x8, pk);
                }
            // ---- O^T += V^T P^T: A operand element j of lane half h = V[key 32 u + 16 s + 8 (j >> 2) + 4 h + (j & 3)][d = 32 db + r];
            // and the row sums, l += 1^T P^T
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int db = 0; db < 2; ++db) {
                        u32x2 lo, hi;
                        {
                            const int key = 32 * u + 16 * s + 4 * (g >> 1) + q4;
                            const int c = 4 * db + 2 * (g & 1) + (p >> 1);
                            const char* ad = vl + key * 128 + ((c ^ (((key >> 1) & 1) << 2)) << 4) + 8 * (p & 1);
                            lo = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                                               (s16x4 __attribute__((address_space(3)))*)ad));
                            const int key2 = key + 8;
                            const char* ad2 = vl + key2 * 128 + ((c ^ (((key2 >> 1) & 1) << 2)) << 4) + 8 * (p & 1);
                            hi = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                                               (s16x4 __attribute__((address_space(3)))*)ad2));
                        }
                        const bf16x8 vf = __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
                        oacc[db] = VH_MFMA16(vf, pf[u][s], oacc[db]);
                    }
                    lacc = VH_MFMA16(ones, pf[u][s], lacc);
                }
        }
        // tile it + 1 (this wave's pieces of it: the four requests BEFORE the ones issued above) has landed; after the barrier
        // every wave's pieces have, and nobody reads image `buf` any more
        if (ahead) __builtin_amdgcn_s_waitcnt(0x0F74);       // vmcnt(4)
        else __builtin_amdgcn_s_waitcnt(0x0F70);             // vmcnt(0)
        __syncthreads();
        buf = buf == 2 ? 0 : buf + 1;
    }
    // ---- epilogue: O / l, narrowed, transposed through LDS (per wave: 32 queries x 64 d) and stored as whole 128-B rows
    const float l_tot = lacc[0];
    const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
    char* ow = lds + w * 32 * 144;                           // 144-B rows (128 + 16 of padding)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const u32x2 pk = {pack_bf16(oacc[db][4 * g4] * inv, oacc[db][4 * g4 + 1] * inv),
                              pack_bf16(oacc[db][4 * g4 + 2] * inv, oacc[db][4 * g4 + 3] * inv)};
            *reinterpret_cast<u32x2*>(ow + r * 144 + (32 * db + 8 * g4 + 4 * h) * 2) = pk;
        }
    __builtin_amdgcn_s_waitcnt(0xC07F);                       // lgkmcnt(0): the wave's own writes are in LDS (wave-private region)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = lane + 64 * i, row = id >> 3, c = id & 7;
        const int qrow = q0 + row;
        if (qrow < A16_TQ && qrow < A16_QBLK0 + A16_QB)
            stq(a.out + (A16_ROW0 + qrow) * a.ldo + head * VH_HEAD_DIM + 8 * c, ldq(ow + row * 144 + 16 * c));
    }
#undef A16_TQ
#undef A16_TK
#undef A16_QBLK0
#undef A16_ROW0
#undef A16_KV
}
