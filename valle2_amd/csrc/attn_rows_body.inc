// The body of the many-row attention kernels, included by attention.hip once per kernel (ATTN_ROWS_PACKED 0: attn_rows_kernel,
// 1: attn_rows_packed_kernel).  An include and not a __device__ template: inlined into a wrapper kernel the same text compiles
// to 133 VGPRs instead of 128 (the V-row address hoisting out of the tile loop comes out differently), which costs
// attn_rows_kernel its fourth workgroup per CU; stamped out as the kernel itself it compiles as it always did.  For the same
// reason what differs between the two — the sequence's lengths, mask mode, first row and K/V base — is spelt by the AR_*
// macros below, which expand to attn_rows_kernel's own expressions (a.Tq read where it is used, not copied to a local): its
// instructions are the ones it had before the packed kernel existed.
//
// One workgroup = 128 queries of one (sequence, head) over that sequence's keys in 32-key tiles.  The sequence is batch row
// b of a padded (B, Tq, ·) layout (attn_rows_kernel, every mask mode) or one segment of a packed row stream
// (attn_rows_packed_kernel, full mask): there Tq = Tk = kvl = the segment's length, row 0 of the sequence is row seg_start
// of q / out / the cache, and everything below — tile order, clamps, arithmetic — is the same code.
//
// ATTN_ROWS_PACKED 2: attn_rows_packed_lse_kernel, the packed kernel as the TRAINING forward — the mask mode (full or prefix)
// is the launch's, a prefix segment's text length comes from seg_x_len, and the log2-sum-exp of every row goes to
// lse2 (n_heads, M), M = a.Tq.  The first two kernels compile to what they were before it existed.
#if ATTN_ROWS_PACKED == 2
__global__ __launch_bounds__(256, 2) void attn_rows_packed_lse_kernel(RowsArgs a, PackedSegs ps, const int32_t* seg_x_len) {
#elif ATTN_ROWS_PACKED
__global__ __launch_bounds__(256, 2) void attn_rows_packed_kernel(RowsArgs a, PackedSegs ps) {
#else
__global__ __launch_bounds__(256, 2) void attn_rows_kernel(RowsArgs a) {
#endif
    // [buf][K|V][key][KLD]; reused at the end as the [128][KLD] output transpose buffer
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * KT * KLD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
#if ATTN_ROWS_PACKED
    // table row = blockIdx.x / n_heads, longest segment first (its blocks visit the most tiles); id % n_heads is the head
    const int blk = blockIdx.x / a.n_heads;
    const int head = blockIdx.x - blk * a.n_heads, bh = head, b = 0;
    const int seg = ps.blocks[2 * blk], q0 = ps.blocks[2 * blk + 1];
    if ((unsigned)seg >= (unsigned)ps.n_seg) return;          // (workgroup-uniform: a table the caller got wrong reads nothing)
    const int s0 = ps.seg_start[seg];
    if (s0 < 0 || s0 >= ps.n_rows) return;
    const int len = min(ps.seg_len[seg], ps.n_rows - s0);      // never a cache row at or beyond S_max, whatever the table says
    if (q0 < 0 || q0 >= len) return;
#if ATTN_ROWS_PACKED == 2
    const int pmode = a.mode == VH_MASK_PREFIX ? VH_MASK_PREFIX : VH_MASK_FULL;
    const int kvl = len, xl = pmode == VH_MASK_PREFIX ? min(max(seg_x_len[seg], 0), len) : 0, q_off = 0;
#define AR_MODE pmode
#else
    const int kvl = len, xl = 0, q_off = 0;
#define AR_MODE VH_MASK_FULL
#endif
#define AR_TQ len                                              /* queries = keys = the segment's rows */
#define AR_TK len
#define AR_ROW0 (int64_t)s0                                    /* row of q / out that holds the sequence's query 0 */
#define AR_KV(p) ((p) + ((int64_t)bh * a.S_max + s0) * HD)     /* the sequence's key 0 in the head's K / V stream */
#else
    // 1-D grid, heaviest query blocks first: under the causal/prefix mask the last query block of
    // a head visits up to 4x the key tiles of the first, and with only ~4 workgroups per CU slot a
    // heavy block dispatched late becomes the tail.  id % (B*h) is the (b,head), so workgroups that
    // share an XCD (ids b, b+8, ...) still see every query block: no XCD gets only heavy ones.
    const int n_bh = gridDim.x / a.n_qblocks;
    const int bh = blockIdx.x % n_bh, b = bh / a.n_heads, head = bh - b * a.n_heads;
    const int q0 = (a.n_qblocks - 1 - (int)(blockIdx.x / n_bh)) * QB;
    const int q_off = a.Tk - a.Tq;
    const int kvl = a.kv_len ? min(a.kv_len[b], a.Tk) : a.Tk;
    const int xl = a.x_len_dev ? a.x_len_dev[b] : a.x_len;
#define AR_TQ a.Tq
#define AR_TK a.Tk
#define AR_MODE a.mode
#define AR_ROW0 (int64_t)b * a.Tq
#define AR_KV(p) ((p) + (int64_t)bh * a.S_max * HD)
#endif

    // number of key tiles this block has to visit
    const int last_pos = q_off + min(q0 + QB, AR_TQ) - 1;
    int kmax = kvl;
    if (AR_MODE == VH_MASK_PREFIX) kmax = min(kvl, max(xl, last_pos >= xl ? last_pos + 1 : 0));
    if (AR_MODE == VH_MASK_EXPLICIT) kmax = AR_TK;
    const int n_tiles = (kmax + KT - 1) / KT;

    // Q fragment (B operand of Sᵀ = K·Qᵀ): lane holds Q[qi][8t+4h+j], pre-scaled
    const int qi = q0 + w * 32 + r;            // this lane's query row
    const int qpos = q_off + qi;               // its key position
    const float qscale = 0.125f * LOG2E;
    f32x4 qf[8];
    {
        const float* qp = a.q + (AR_ROW0 + qi) * a.ldq + head * HD + 4 * h;
#pragma unroll
        for (int t = 0; t < 8; ++t)
            qf[t] = qi < AR_TQ ? ld4(qp + 8 * t) * qscale : f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const float* kb = AR_KV(a.kc);
    const float* vb = AR_KV(a.vc);
    const int skey = tid >> 4, squad = (tid & 15) * 4;  // staging: 2 keys per thread per operand
    f32x4 rk[2], rv[2];
    // Keys beyond Tk are clamped to the last written row (rows < Tk were all written by this forward's QKV GEMM):
    // their scores are masked to -inf, so their (finite) values meet p = 0.  Address = wave-uniform head base +
    // one 32-bit per-lane byte offset: no 64-bit vector arithmetic in the loop (VALU slots are MFMA slots).
    auto gload = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint32_t off = (uint32_t)(min(k0 + skey + 16 * i, AR_TK - 1) * HD + squad) * 4u;
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

    f32x16 O0, O1;
#pragma unroll
    for (int e = 0; e < 16; ++e) { O0[e] = 0.f; O1[e] = 0.f; }
    float m = NEG_INF, l = 0.f;

    // positions covered by this wave's 32 queries (for tile skipping / fast path)
    const int wpos_min = q_off + q0 + w * 32, wpos_max = wpos_min + 31;

    if (n_tiles > 0) {
        gload(0);
        lstore(0);
    }
    __syncthreads();
    for (int kt = 0; kt < n_tiles; ++kt) {
        const int cur = kt & 1, k0 = kt * KT;
        if (kt + 1 < n_tiles) gload(k0 + KT);

        bool any = k0 < kvl, all = k0 + KT <= kvl;
        if (AR_MODE == VH_MASK_PREFIX) {
            any = any && (k0 < xl || (wpos_max >= xl && k0 <= wpos_max));
            all = all && (k0 + KT <= xl || (wpos_min >= xl && k0 + KT - 1 <= wpos_min));
        } else if (AR_MODE == VH_MASK_EXPLICIT) {
            any = true; all = false;
        }
        if (any) {
            const float* ks = lds + cur * (2 * KT * KLD);
            const float* vs = ks + KT * KLD;
            // ---- Sᵀ[key][q] = sum_d K[key][d] Q[q][d]
            f32x16 S;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const f32x4 kf = ld4(ks + r * KLD + 8 * t + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j)        // the first product starts from the constant-zero C operand
                    S = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[j], qf[t][j], (t | j) ? S : f32x16{}, 0, 0, 0);
            }
            // ---- mask: reg e ↔ key k0 + (e&3) + 8(e>>2) + 4h ; lane ↔ query qi
            if (!all) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
                    bool vis;
                    if (AR_MODE == VH_MASK_EXPLICIT) {
                        vis = key < AR_TK && qi < AR_TQ && !a.mask[b * a.mask_bstride + (int64_t)qi * AR_TK + key] &&
                              !(a.pad && a.pad[(int64_t)b * AR_TK + key]);
                    } else {
                        vis = key < kvl;
                        if (AR_MODE == VH_MASK_PREFIX) vis = vis && (key < xl || (qpos >= xl && key <= qpos));
                    }
                    if (!vis) S[e] = NEG_INF;
                }
            }
            // ---- online softmax (per lane = per query; the other 16 keys sit in lane^32)
            float tmax = S[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) tmax = fmaxf(tmax, S[e]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float m_new = fmaxf(m, tmax);
            const float m_use = m_new == NEG_INF ? 0.f : m_new;  // fully masked so far: p = 0
            const float alpha = vh_exp2(m - m_use);
            // subtract and sum two scores per instruction (v_pk_add_f32); the exponentials stay scalar
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            f32x2 psum2 = {0.f, 0.f};
            const f32x2 nm2 = {-m_use, -m_use};
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                f32x2 d = f32x2{S[e], S[e + 1]} + nm2;
                d.x = vh_exp2(d.x);
                d.y = vh_exp2(d.y);
                psum2 += d;
                S[e] = d.x;
                S[e + 1] = d.y;
            }
            const float psum = psum2.x + psum2.y;
            l = l * alpha + psum;
            m = m_new;
            if (__any(alpha != 1.0f)) {                // no query of this wave raised its maximum: nothing to rescale
#pragma unroll
                for (int e = 0; e < 16; ++e) { O0[e] *= alpha; O1[e] *= alpha; }
            }
            // ---- Oᵀ[d][q] += sum_key V[key][d] P[key][q]; k-step e covers keys (e,h=0),(e,h=1)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float* vrow = vs + ((e & 3) + 8 * (e >> 2) + 4 * h) * KLD + r;
                O0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], S[e], O0, 0, 0, 0);
                O1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32], S[e], O1, 0, 0, 0);
            }
        }
        if (kt + 1 < n_tiles) lstore(cur ^ 1);
        __syncthreads();
    }

    // ---- normalise, transpose through LDS, store coalesced rows
    const float ltot = l + __shfl_xor(l, 32, 64);
    const float inv = 1.0f / ltot;  // fully masked row → 0/0 = NaN, as SDPA gives
#if ATTN_ROWS_PACKED == 2
    if (h == 0 && qi < AR_TQ) a.lse2[(int64_t)head * a.Tq + s0 + qi] = m + log2f(ltot);
#else
    if (!ATTN_ROWS_PACKED && a.lse2 && h == 0 && qi < AR_TQ) a.lse2[(int64_t)bh * AR_TQ + qi] = m + log2f(ltot);
#endif
    float* ob = lds;                // [128][KLD]; all K/V reads finished at the last barrier
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
        // regs 4g4..4g4+3 ↔ d = 8*g4 + 4h + {0..3} (+32 for O1)
        f32x4 v0 = {O0[4 * g4], O0[4 * g4 + 1], O0[4 * g4 + 2], O0[4 * g4 + 3]};
        f32x4 v1 = {O1[4 * g4], O1[4 * g4 + 1], O1[4 * g4 + 2], O1[4 * g4 + 3]};
        st4(ob + (w * 32 + r) * KLD + 8 * g4 + 4 * h, v0 * inv);
        st4(ob + (w * 32 + r) * KLD + 32 + 8 * g4 + 4 * h, v1 * inv);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int row = skey + 16 * i;
        if (q0 + row < AR_TQ)
            st4(a.out + (AR_ROW0 + q0 + row) * a.ldo + head * HD + squad,
                ld4(ob + row * KLD + squad));
    }
#undef AR_TQ
#undef AR_TK
#undef AR_MODE
#undef AR_ROW0
#undef AR_KV
}
