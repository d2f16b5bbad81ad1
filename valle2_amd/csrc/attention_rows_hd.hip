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
//  attn_rows_hd_lse_kernel<NB> : the same body (attn_rows_hd_body.inc, compiled once per kernel) that also stores every row's
//                          base-2 log-sum-exp: the training forward, whose backward is attention_rows_hd_bwd.hip.
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

#define ATTN_ROWS_HD_LSE 0
#include "attn_rows_hd_body.inc"   // attn_rows_hd_kernel<NB>(RowsHdArgs)
#undef ATTN_ROWS_HD_LSE
#define ATTN_ROWS_HD_LSE 1
#include "attn_rows_hd_body.inc"   // attn_rows_hd_lse_kernel<NB>(RowsHdArgs, float* lse2): the training forward
#undef ATTN_ROWS_HD_LSE

// The checks and the launch behind vh_attn_rows_hd (lse2 null) and vh_attn_rows_hd_lse; `nm` names the entry in messages.
static int rows_hd_launch(const char* nm, const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                          const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                          const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                          float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                          int B, int n_heads, int head_dim, int Tq, int Tk, float scale,
                          int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len, float* lse2, void* stream) {
    VH_REQUIRE(q && k && v && out, VH_EINVAL, "%s: null pointer (q=%p k=%p v=%p out=%p)", nm, (const void*)q,
               (const void*)k, (const void*)v, (const void*)out);
    VH_REQUIRE(mode != VH_MASK_EXPLICIT, VH_EUNSUPPORTED,
               "%s: mode=%d (VH_MASK_EXPLICIT): caller-supplied masks take the materialised route", nm, mode);
    VH_REQUIRE(mode == VH_MASK_FULL || mode == VH_MASK_PREFIX, VH_EINVAL, "%s: mode=%d", nm, mode);
    VH_REQUIRE(B > 0 && n_heads > 0 && Tq > 0 && Tk >= Tq, VH_EINVAL, "%s: bad dims B=%d h=%d Tq=%d Tk=%d", nm, B,
               n_heads, Tq, Tk);
    VH_REQUIRE(head_dim % 4 == 0 && head_dim >= 16 && head_dim <= 128, VH_EUNSUPPORTED,
               "%s: head_dim=%d (a multiple of 4 from 16 to 128)", nm, head_dim);
    const int64_t strides[12] = {q_sb, q_sh, q_sr, k_sb, k_sh, k_sr, v_sb, v_sh, v_sr, o_sb, o_sh, o_sr};
    static const char* const stride_names[12] = {"q batch", "q head", "q row", "k batch", "k head", "k row",
                                                 "v batch", "v head", "v row", "out batch", "out head", "out row"};
    for (int i = 0; i < 12; ++i)
        VH_REQUIRE(strides[i] % 4 == 0, VH_EINVAL, "%s: %s stride=%lld (a multiple of 4 floats: rows stay 16-byte aligned)",
                   nm, stride_names[i], (long long)strides[i]);
    // the kernel addresses a key row by a 32-bit byte offset from its (batch row, head) base
    const int64_t reach = ((1LL << 30) - head_dim) / (Tk > 1 ? Tk - 1 : 1);      // (no product that could overflow)
    VH_REQUIRE(k_sr >= 0 && v_sr >= 0 && k_sr <= reach && v_sr <= reach,
               VH_EUNSUPPORTED, "%s: k row stride=%lld v row stride=%lld with Tk=%d (the last key row must lie within 4 GB of the first)",
               nm, (long long)k_sr, (long long)v_sr, Tk);
    VH_REQUIRE(vh_aligned16(q) && vh_aligned16(k) && vh_aligned16(v) && vh_aligned16(out), VH_EALIGN,
               "%s: q=%p k=%p v=%p out=%p must be 16-byte aligned", nm, (const void*)q, (const void*)k, (const void*)v,
               (const void*)out);
    const int nqb = (Tq + RH_QB - 1) / RH_QB;
    VH_REQUIRE((int64_t)B * n_heads <= 0x7fffffffLL / nqb, VH_EINVAL,
               "%s: B=%d h=%d Tq=%d: %d x %lld workgroups exceed one grid", nm, B, n_heads, Tq, nqb, (long long)B * n_heads);
    RowsHdArgs a{q, k, v, out, q_sb, q_sh, q_sr, k_sb, k_sh, k_sr, v_sb, v_sh, v_sr, o_sb, o_sh, o_sr,
                 n_heads, head_dim, Tq, Tk, mode, x_len, x_len_dev, kv_len, nqb, scale * RH_LOG2E};
    const dim3 grid(nqb * B * n_heads), block(256);
    const int nb = (head_dim + 31) / 32;
    if (lse2) {
        switch (nb) {
        case 1: hipLaunchKernelGGL(attn_rows_hd_lse_kernel<1>, grid, block, 0, (hipStream_t)stream, a, lse2); break;
        case 2: hipLaunchKernelGGL(attn_rows_hd_lse_kernel<2>, grid, block, 0, (hipStream_t)stream, a, lse2); break;
        case 3: hipLaunchKernelGGL(attn_rows_hd_lse_kernel<3>, grid, block, 0, (hipStream_t)stream, a, lse2); break;
        default: hipLaunchKernelGGL(attn_rows_hd_lse_kernel<4>, grid, block, 0, (hipStream_t)stream, a, lse2); break;
        }
    } else {
        switch (nb) {
        case 1: hipLaunchKernelGGL(attn_rows_hd_kernel<1>, grid, block, 0, (hipStream_t)stream, a); break;
        case 2: hipLaunchKernelGGL(attn_rows_hd_kernel<2>, grid, block, 0, (hipStream_t)stream, a); break;
        case 3: hipLaunchKernelGGL(attn_rows_hd_kernel<3>, grid, block, 0, (hipStream_t)stream, a); break;
        default: hipLaunchKernelGGL(attn_rows_hd_kernel<4>, grid, block, 0, (hipStream_t)stream, a); break;
        }
    }
    VH_CHECK_LAUNCH(nm);
    return VH_OK;
}

extern "C" int vh_attn_rows_hd(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                               const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                               const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                               float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                               int B, int n_heads, int head_dim, int Tq, int Tk, float scale,
                               int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len, void* stream) {
    return rows_hd_launch("vh_attn_rows_hd", q, q_sb, q_sh, q_sr, k, k_sb, k_sh, k_sr, v, v_sb, v_sh, v_sr, out, o_sb, o_sh, o_sr,
                          B, n_heads, head_dim, Tq, Tk, scale, mode, x_len, x_len_dev, kv_len, nullptr, stream);
}

// vh_attn_rows_hd that also writes lse2 (B, n_heads, Tq), contiguous: the training forward of the flash route
extern "C" int vh_attn_rows_hd_lse(const float* q, int64_t q_sb, int64_t q_sh, int64_t q_sr,
                                   const float* k, int64_t k_sb, int64_t k_sh, int64_t k_sr,
                                   const float* v, int64_t v_sb, int64_t v_sh, int64_t v_sr,
                                   float* out, int64_t o_sb, int64_t o_sh, int64_t o_sr,
                                   int B, int n_heads, int head_dim, int Tq, int Tk, float scale,
                                   int mode, int x_len, const int32_t* x_len_dev, const int32_t* kv_len, float* lse2,
                                   void* stream) {
    VH_REQUIRE(lse2, VH_EINVAL, "vh_attn_rows_hd_lse: null pointer (lse2=%p)", (const void*)lse2);
    VH_REQUIRE(vh_aligned16(lse2), VH_EALIGN, "vh_attn_rows_hd_lse: lse2=%p must be 16-byte aligned", (const void*)lse2);
    return rows_hd_launch("vh_attn_rows_hd_lse", q, q_sb, q_sh, q_sr, k, k_sb, k_sh, k_sr, v, v_sb, v_sh, v_sr, out, o_sb, o_sh,
                          o_sr, B, n_heads, head_dim, Tq, Tk, scale, mode, x_len, x_len_dev, kv_len, lse2, stream);
}
