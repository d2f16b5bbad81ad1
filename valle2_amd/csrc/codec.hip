// The decoder half of the 24 kHz EnCodec family (SEANet decoder + residual vector quantiser), fp32: codes -> waveform on the
// device.  Activations are CHANNELS-LAST (B, T, C): a time step is a row, every convolution is a GEMM over rows.
//
//  rvq_decode_kernel        : out[b, t, :] = sum_{q < Q} codebooks[q][codes[b, q, t]], added in codebook order 0 .. Q-1 from 0.0f
//                             (the order of the reference's residual quantiser: fp32 torch adding in that order is bit-equal).
//                             One lane per 4 columns.  An id outside [0, K) is never read: it raises VH_DEVERR_EMBED_ID.
//  conv1d_causal_kernel<NT> : the windowed GEMM  out[m, n] = bias[n] + sum_k sum_ci act(xpad[b, t + k dil, ci]) w[n, k, ci]
//                             (+ residual[m, n]), m = b T + t, on v_mfma_f32_32x32x2_f32.  One workgroup = 128 rows x 32 NT
//                             columns, 4 waves of 32 rows; per (tap, 32 input channels) the activation rows of the window
//                             and the weight rows are staged through LDS ([row][32 + 4]) — the window, the left padding
//                             (reflect or zero, per batch row: row b's window never reads row b-1) and the ELU are applied on
//                             the way in — and every lane reads its fragments as 16-byte LDS loads: lane half h of k-step s
//                             takes channels 8 s + 4 h .. + 3 of BOTH operands, so one load feeds 4 MFMAs.  An output element's
//                             sum order depends on (taps, C_in) only, never on B, T or the row's place in a tile: a row of a
//                             padded batch has the bits of the same row computed alone — given lens: the reflection at the
//                             start of a batch row reads FORWARD (xpad[i] = x[pad - i]), so a row shorter than the padding
//                             must not see the batch's padding frames; beyond lens[b] * len_scale rows it reads zero, which
//                             is what the small-input branch gives that utterance alone.  Columns >= N and channels >= C_in
//                             are zero-filled in LDS and never loaded; rows >= M are neither loaded nor stored.
//  lstm_step_kernel<NI>     : ONE time step of one LSTM layer, one launch per step (nothing inside a launch waits for another
//                             workgroup).  A wave owns one hidden unit j: its four rows of W_hh (gates i, f, g, o) stay in
//                             registers over the B batch rows; per row the four dot products with h_{t-1} are wave sums in a
//                             fixed order (bits independent of B), lane 0 adds the input projection, updates c[b, j] in place
//                             (no other wave touches it) and stores h_t — and h_t + skip for the layer whose output the
//                             decoder adds its input to.
//
// And the encoder half, waveform -> codes, over the same stride-1 convolution and LSTM (documented at each kernel below):
//  conv1d_wave_kernel        : the first convolution, one input channel: a lane = 4 output channels of a row, 16-byte stores.
//  conv1d_causal_kernel<NT, true> : the strided, downsampling form of the windowed GEMM (vh_conv1d_down): the same tiles and
//                             sum order; a tile row is an output frame and the window is indexed through EncodecConv1d's
//                             causal padding (left reflection, the right-hand "extra" reflection, the small-input rule).
//  rvq_encode_kernel<NS>     : the residual quantiser's encode, every stage in one launch: the residual in registers, the
//                             codebook through LDS, scores 2 r.e - |e|^2 on the MFMA, a running arg-max (lowest index of a tie).
#include "vh_common.h"

// ---------------------------------------------------------------------------------------------------------------- RVQ decode
__global__ __launch_bounds__(256) void rvq_decode_kernel(const int64_t* __restrict__ codes, const float* __restrict__ books,
                                                         float* __restrict__ out, int Q, int T, int K, int D, int64_t n_items,
                                                         int32_t* __restrict__ err_flag) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_items) return;
    const int d4 = D >> 2;
    const int64_t row = idx / d4;
    const int c = (int)(idx - row * d4) * 4;
    const int64_t b = row / T;
    const int t = (int)(row - b * T);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bool bad = false;
    for (int q = 0; q < Q; ++q) {
        const int64_t id = codes[(b * Q + q) * T + t];
        if (id < 0 || id >= K) { bad = true; continue; }
        acc += ld4(books + ((int64_t)q * K + id) * D + c);
    }
    st4(out + row * D + c, acc);
    if (bad && err_flag && c == 0) atomicOr(err_flag, VH_DEVERR_EMBED_ID);
}

extern "C" int vh_rvq_decode(const int64_t* codes, const float* codebooks, float* out, int B, int Q, int T, int n_books, int K,
                             int D, int32_t* err_flag, void* stream) {
    VH_REQUIRE(codes && codebooks && out, VH_EINVAL, "vh_rvq_decode: null pointer (codes=%p codebooks=%p out=%p)",
               (const void*)codes, (const void*)codebooks, (const void*)out);
    VH_REQUIRE(B > 0 && Q > 0 && T > 0 && K > 0 && n_books > 0, VH_EINVAL, "vh_rvq_decode: bad dims B=%d Q=%d T=%d n_books=%d K=%d",
               B, Q, T, n_books, K);
    VH_REQUIRE(Q <= n_books, VH_EINVAL, "vh_rvq_decode: Q=%d codebooks asked of n_books=%d", Q, n_books);
    VH_REQUIRE(D > 0 && D % 4 == 0, VH_EUNSUPPORTED, "vh_rvq_decode: D=%d (a multiple of 4: rows stay 16-byte aligned)", D);
    VH_REQUIRE(vh_aligned16(codebooks) && vh_aligned16(out) && (reinterpret_cast<uintptr_t>(codes) & 7u) == 0, VH_EALIGN,
               "vh_rvq_decode: codebooks=%p out=%p must be 16-byte aligned, codes=%p 8-byte", (const void*)codebooks,
               (const void*)out, (const void*)codes);
    VH_REQUIRE((int64_t)B * T <= 0x7fffffffLL * 256 / (D / 4), VH_EINVAL, "vh_rvq_decode: B=%d T=%d D=%d exceed one grid", B, T, D);
    const int64_t n_items = (int64_t)B * T * (D / 4);
    hipLaunchKernelGGL(rvq_decode_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, codes,
                       codebooks, out, Q, T, K, D, n_items, err_flag);
    VH_CHECK_LAUNCH("vh_rvq_decode");
    return VH_OK;
}

// ------------------------------------------------------------------------------------------------------ causal windowed GEMM
#define CV_BM 128      // rows per workgroup (4 waves x 32)
#define CV_KC 32       // input channels per LDS chunk
#define CV_LD 36       // LDS row stride in floats (32 + 4: 16-byte aligned rows, staggered banks)

struct ConvArgs {
    const float* x; const float* w; const float* bias; const float* res; float* out;
    int64_t M;                       // B T rows
    int T, Cin, N, taps, dil, reflect, elu;
    const int32_t* lens; int len_scale;   // batch row b holds lens[b] * len_scale valid rows (null: T)
    int stride, Tout;                     // the strided form only: M = B Tout output rows over T input rows per batch row
};

__device__ __forceinline__ float cv_elu(float v) { return v > 0.f ? v : expm1f(v); }

// The strided form's padded row p of a batch row of `len` valid rows -> its x row, or -1 for a zero: EncodecConv1d's causal
// padding, `left` rows of reflection in front and, behind, the reflection that fills the last window; `ext` is the length the
// reflections see — len, or max(left, right) + 1 under the small-input rule (zero-extend, reflect, trim).
__device__ __forceinline__ int cv_down_src(int p, int left, int len, int ext) {
    const int j = p - left;
    if (j >= 0 && j < len) return j;
    if (j >= len && j < ext) return -1;
    const int s = j < 0 ? -j : 2 * ext - 2 - j;
    return s >= 0 && s < len ? s : -1;
}

__device__ __forceinline__ int cv_down_ext(int left, int len, int stride) {
    const int right = (len + stride - 1) / stride * stride - len;
    const int mx = left > right ? left : right;
    return len <= mx ? mx + 1 : len;
}

// DOWN: out[b, t', n] = bias[n] + sum_k sum_ci act(xpad_b[t' stride + k, ci]) w[n, k, ci] over Tout = ceil(T / stride) rows per
// batch row (vh_conv1d_down); the tile loop, the fragment order and so the sum order are the stride-1 form's.
template <int NT, bool DOWN>
__global__ __launch_bounds__(256) void conv1d_causal_kernel(ConvArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[(CV_BM + 32 * NT) * CV_LD];
    float* As = lds;
    float* Ws = lds + CV_BM * CV_LD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * CV_BM;
    const int n0 = blockIdx.y * (32 * NT);
    const int pad = DOWN ? a.taps - a.stride : (a.taps - 1) * a.dil;
    const int srow = tid >> 3, c4 = (tid & 7) * 4;     // staging: rows srow + 32 i of the tile, 4 channels from c4

    int64_t xrow0[4];        // first row of the batch row that tile row srow + 32 i belongs to; -1: a row >= M
    int xt[4];               // its time step
    int xlen[4];             // the valid rows of that batch row: the reflection reads zero beyond them
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + srow + 32 * i;
        if (DOWN && m < a.M) {
            const int64_t b = m / a.Tout;
            xrow0[i] = b * a.T;
            xt[i] = (int)(m - b * a.Tout) * a.stride;        // the window's first padded row
            xlen[i] = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
        } else if (m < a.M) {
            const int64_t b = m / a.T;
            xrow0[i] = b * a.T;
            xt[i] = (int)(m - b * a.T);
            xlen[i] = a.lens ? (int)min((int64_t)max(a.lens[b], 0) * a.len_scale, (int64_t)a.T) : a.T;
        } else {
            xrow0[i] = -1;
            xt[i] = 0;
            xlen[i] = 0;
        }
    }

    int xext[4];             // DOWN: the length the reflections of that batch row see
#pragma unroll
    for (int i = 0; i < 4; ++i) xext[i] = DOWN ? cv_down_ext(pad, xlen[i], a.stride) : 0;

    // NA independent accumulator sets, added at the end: channel e of every 4-channel fragment goes to set e % NA, so a set
    // sums 1 / NA of the terms — the rounding of a long k-ordered chain grows with its length and its partial sums
    constexpr int NA = NT == 4 ? 2 : 4;
    f32x16 acc[NA][NT];
#pragma unroll
    for (int q = 0; q < NA; ++q)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][j][r] = 0.f;

    for (int tap = 0; tap < a.taps; ++tap) {
        int src[4];          // the window's row for this tap: -1 reads as zero
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (DOWN) {
                src[i] = xrow0[i] < 0 ? -1 : cv_down_src(xt[i] + tap, pad, xlen[i], xext[i]);
                continue;
            }
            int s = xt[i] + tap * a.dil - pad;
            if (s < 0) s = a.reflect ? -s : -1;         // xpad[i] = x[pad - i] for i < pad
            // a FORWARD read (only the reflection makes one) beyond the valid rows: the zero extension of the small-input
            // reflect (length <= pad)
            if (s >= xlen[i] && s > xt[i]) s = -1;
            if (xrow0[i] < 0) s = -1;
            src[i] = s;
        }
        for (int c0 = 0; c0 < a.Cin; c0 += CV_KC) {
            const bool cin_ok = c0 + c4 < a.Cin;
            f32x4 av[4], wv[NT];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                av[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (cin_ok && src[i] >= 0) {
                    av[i] = ld4(a.x + (xrow0[i] + src[i]) * a.Cin + c0 + c4);
                    if (a.elu) av[i] = f32x4{cv_elu(av[i].x), cv_elu(av[i].y), cv_elu(av[i].z), cv_elu(av[i].w)};
                }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = n0 + srow + 32 * j;
                wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (cin_ok && n < a.N) wv[j] = ld4(a.w + ((int64_t)n * a.taps + tap) * a.Cin + c0 + c4);
            }
            __syncthreads();                             // the chunk before has been read
#pragma unroll
            for (int i = 0; i < 4; ++i) st4(As + (srow + 32 * i) * CV_LD + c4, av[i]);
#pragma unroll
            for (int j = 0; j < NT; ++j) st4(Ws + (srow + 32 * j) * CV_LD + c4, wv[j]);
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (c0 + 8 * s >= a.Cin) break;          // the rest of the chunk is zero fill
                const f32x4 af = ld4(As + (wave * 32 + l31) * CV_LD + 8 * s + 4 * h);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const f32x4 bf = ld4(Ws + (j * 32 + l31) * CV_LD + 8 * s + 4 * h);
                    acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc[1][j], 0, 0, 0);
                    acc[2 % NA][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc[2 % NA][j], 0, 0, 0);
                    acc[3 % NA][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc[3 % NA][j], 0, 0, 0);
                }
            }
        }
    }

    // accumulator register r of lane (l31, h): row (r & 3) + 8 (r >> 2) + 4 h of the wave's 32, column l31
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + j * 32 + l31;
        if (n >= a.N) continue;
        const float bn = a.bias ? a.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (m >= a.M) continue;
            float v = NA == 4 ? (acc[0][j][r] + acc[1][j][r]) + (acc[2][j][r] + acc[3][j][r]) : acc[0][j][r] + acc[1][j][r];
            v += bn;
            if (DOWN) {                                  // rows past the batch row's own ceil(len / stride) frames: zeros
                const int64_t b = m / a.Tout;
                const int len = a.lens ? min(max(a.lens[b], 0), a.T) : a.T;
                if ((m - b * a.Tout) * a.stride >= len) v = 0.f;
            }
            if (a.res) v += a.res[m * a.N + n];
            a.out[m * a.N + n] = v;
        }
    }
}

extern "C" int vh_conv1d_causal(const float* x, const float* w, const float* bias, const float* residual, float* out, int B, int T,
                                int C_in, int C_out, int taps, int dilation, int pad_mode, int elu, const int32_t* lens,
                                int len_scale, void* stream) {
    VH_REQUIRE(x && w && out, VH_EINVAL, "vh_conv1d_causal: null pointer (x=%p w=%p out=%p)", (const void*)x, (const void*)w,
               (const void*)out);
    VH_REQUIRE(B > 0 && T > 0, VH_EINVAL, "vh_conv1d_causal: bad dims B=%d T=%d", B, T);
    VH_REQUIRE(taps >= 1 && taps <= 64 && dilation >= 1 && dilation <= 4096, VH_EINVAL,
               "vh_conv1d_causal: taps=%d dilation=%d (1 .. 64 taps, dilation 1 .. 4096)", taps, dilation);
    VH_REQUIRE(pad_mode == VH_PAD_ZERO || pad_mode == VH_PAD_REFLECT, VH_EINVAL, "vh_conv1d_causal: pad_mode=%d", pad_mode);
    VH_REQUIRE(elu == 0 || elu == 1, VH_EINVAL, "vh_conv1d_causal: elu=%d (0 or 1)", elu);
    VH_REQUIRE(C_in > 0 && C_in % 4 == 0, VH_EUNSUPPORTED,
               "vh_conv1d_causal: C_in=%d (a multiple of 4: rows stay 16-byte aligned)", C_in);
    VH_REQUIRE(C_out == 1 || (C_out > 0 && C_out % 4 == 0), VH_EUNSUPPORTED,
               "vh_conv1d_causal: C_out=%d (a multiple of 4, or 1 for the waveform)", C_out);
    VH_REQUIRE(vh_aligned16(x) && vh_aligned16(w) && vh_aligned16(out) && vh_aligned16(residual), VH_EALIGN,
               "vh_conv1d_causal: x=%p w=%p residual=%p out=%p must be 16-byte aligned", (const void*)x, (const void*)w,
               (const void*)residual, (const void*)out);
    VH_REQUIRE((reinterpret_cast<uintptr_t>(bias) & 3u) == 0, VH_EALIGN, "vh_conv1d_causal: bias=%p must be 4-byte aligned",
               (const void*)bias);
    VH_REQUIRE(!lens || (len_scale >= 1 && len_scale <= (1 << 20)), VH_EINVAL, "vh_conv1d_causal: len_scale=%d (1 .. 2^20)",
               len_scale);
    VH_REQUIRE((reinterpret_cast<uintptr_t>(lens) & 3u) == 0, VH_EALIGN, "vh_conv1d_causal: lens=%p must be 4-byte aligned",
               (const void*)lens);
    const int64_t M = (int64_t)B * T;
    VH_REQUIRE((M + CV_BM - 1) / CV_BM <= 0x7fffffffLL, VH_EINVAL, "vh_conv1d_causal: B=%d T=%d rows exceed one grid", B, T);
    VH_REQUIRE(M <= (1LL << 40) / (C_in > C_out ? C_in : C_out), VH_EINVAL,
               "vh_conv1d_causal: B=%d T=%d C_in=%d C_out=%d: a tensor beyond 2^40 elements", B, T, C_in, C_out);
    ConvArgs a{x, w, bias, residual, out, M, T, C_in, C_out, taps, dilation, pad_mode == VH_PAD_REFLECT, elu, lens, len_scale,
               1, T};
    const int nt = C_out > 64 ? 4 : C_out > 32 ? 2 : 1;
    const int64_t n_tiles = ((int64_t)C_out + 32 * nt - 1) / (32 * nt);
    VH_REQUIRE(n_tiles <= 65535, VH_EINVAL, "vh_conv1d_causal: C_out=%d exceeds one grid", C_out);
    const dim3 grid((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)n_tiles), block(256);
    switch (nt) {
    case 4: hipLaunchKernelGGL((conv1d_causal_kernel<4, false>), grid, block, 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((conv1d_causal_kernel<2, false>), grid, block, 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL((conv1d_causal_kernel<1, false>), grid, block, 0, (hipStream_t)stream, a); break;
    }
    VH_CHECK_LAUNCH("vh_conv1d_causal");
    return VH_OK;
}

// ------------------------------------------------------------------------------------------------------------------- LSTM
#define LSTM_H_MAX 1024

__device__ __forceinline__ float lstm_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <int NI>
__global__ __launch_bounds__(256) void lstm_step_kernel(const float* __restrict__ xproj, const float* __restrict__ whh,
                                                        float* __restrict__ hseq, float* __restrict__ c,
                                                        const float* __restrict__ skip, float* __restrict__ y, int B, int T, int H,
                                                        int t) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);          // this wave's hidden unit
    if (j >= H) return;                                          // (no barrier in this kernel)
    f32x4 w[4][NI];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int k = lane * 4 + 256 * i;
            w[g][i] = k < H ? ld4(whh + ((int64_t)g * H + j) * H + k) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    for (int b = 0; b < B; ++b) {
        const int64_t row = (int64_t)b * T + t;
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int k = lane * 4 + 256 * i;
                if (k < H) {
                    const f32x4 hv = ld4(hseq + (row - 1) * H + k);
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        s[g] = fmaf(w[g][i].w, hv.w, fmaf(w[g][i].z, hv.z, fmaf(w[g][i].y, hv.y, fmaf(w[g][i].x, hv.x, s[g]))));
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) s[g] = wave_sum(s[g]);
        }
        if (lane == 0) {
            const float* xp = xproj + row * 4 * H + j;
            const float gi = lstm_sigmoid(xp[0] + s[0]);
            const float gf = lstm_sigmoid(xp[H] + s[1]);
            const float gg = tanhf(xp[2 * (int64_t)H] + s[2]);
            const float go = lstm_sigmoid(xp[3 * (int64_t)H] + s[3]);
            const float cp = t > 0 ? c[(int64_t)b * H + j] : 0.f;
            const float cn = gf * cp + gi * gg;
            c[(int64_t)b * H + j] = cn;
            const float hn = go * tanhf(cn);
            hseq[row * H + j] = hn;
            if (y) y[row * H + j] = hn + skip[row * H + j];
        }
    }
}

extern "C" int vh_lstm_layer(const float* xproj, const float* w_hh, float* h_seq, float* c, const float* skip, float* y, int B,
                             int T, int H, void* stream) {
    VH_REQUIRE(xproj && w_hh && h_seq && c, VH_EINVAL, "vh_lstm_layer: null pointer (xproj=%p w_hh=%p h_seq=%p c=%p)",
               (const void*)xproj, (const void*)w_hh, (const void*)h_seq, (const void*)c);
    VH_REQUIRE((skip == nullptr) == (y == nullptr), VH_EINVAL, "vh_lstm_layer: skip=%p and y=%p go together", (const void*)skip,
               (const void*)y);
    VH_REQUIRE(B > 0 && T > 0 && T <= (1 << 20), VH_EINVAL, "vh_lstm_layer: bad dims B=%d T=%d (T up to 2^20 steps)", B, T);
    VH_REQUIRE(H > 0 && H % 4 == 0 && H <= LSTM_H_MAX, VH_EUNSUPPORTED, "vh_lstm_layer: H=%d (a multiple of 4 up to %d)", H,
               LSTM_H_MAX);
    VH_REQUIRE((int64_t)B * T <= (1LL << 40) / (4 * (int64_t)H), VH_EINVAL, "vh_lstm_layer: B=%d T=%d H=%d: a tensor beyond 2^40 elements",
               B, T, H);
    VH_REQUIRE(vh_aligned16(xproj) && vh_aligned16(w_hh) && vh_aligned16(h_seq) && vh_aligned16(c) && vh_aligned16(skip) &&
                   vh_aligned16(y), VH_EALIGN,
               "vh_lstm_layer: xproj=%p w_hh=%p h_seq=%p c=%p skip=%p y=%p must be 16-byte aligned", (const void*)xproj,
               (const void*)w_hh, (const void*)h_seq, (const void*)c, (const void*)skip, (const void*)y);
    const dim3 grid((unsigned)((H + 3) / 4)), block(256);
    const int ni = (H + 255) / 256;
    for (int t = 0; t < T; ++t) {
        switch (ni) {
        case 1: hipLaunchKernelGGL(lstm_step_kernel<1>, grid, block, 0, (hipStream_t)stream, xproj, w_hh, h_seq, c, skip, y, B, T, H, t); break;
        case 2: hipLaunchKernelGGL(lstm_step_kernel<2>, grid, block, 0, (hipStream_t)stream, xproj, w_hh, h_seq, c, skip, y, B, T, H, t); break;
        case 3: hipLaunchKernelGGL(lstm_step_kernel<3>, grid, block, 0, (hipStream_t)stream, xproj, w_hh, h_seq, c, skip, y, B, T, H, t); break;
        default: hipLaunchKernelGGL(lstm_step_kernel<4>, grid, block, 0, (hipStream_t)stream, xproj, w_hh, h_seq, c, skip, y, B, T, H, t); break;
        }
    }
    VH_CHECK_LAUNCH("vh_lstm_layer");
    return VH_OK;
}

// ================================================================================================ the encoder's three kernels
// ------------------------------------------------------------------------------------------- the convolution over the waveform
// One lane = one output row's 4 channels: acc = 0, then fma over the taps in order, then + bias (a sum order of `taps` alone).
// The lanes of a row read the same samples (one cache line, broadcast); the store is 16 bytes.
__global__ __launch_bounds__(256) void conv1d_wave_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ out, int L, int N,
                                                          int taps, int64_t n_items, const int32_t* __restrict__ lens) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_items) return;
    const int n4 = N >> 2;
    const int64_t row = idx / n4;
    const int c = (int)(idx - row * n4) * 4;
    const int64_t b = row / L;
    const int t = (int)(row - b * L);
    const int len = lens ? min(max(lens[b], 0), L) : L;
    const int pad = taps - 1;
    const float* xb = x + b * L;
    const float* w0 = w + (int64_t)c * taps;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < taps; ++k) {
        int s = t + k - pad;
        if (s < 0) s = -s;                                   // xpad[i] = x[pad - i] for i < pad
        // a forward read beyond the valid samples is the zero extension of the small-input reflect; s <= t < L otherwise
        const float v = (s >= len && s > t) ? 0.f : xb[s];
        acc.x = fmaf(v, w0[k], acc.x);
        acc.y = fmaf(v, w0[taps + k], acc.y);
        acc.z = fmaf(v, w0[2 * taps + k], acc.z);
        acc.w = fmaf(v, w0[3 * taps + k], acc.w);
    }
    if (bias) acc += f32x4{bias[c], bias[c + 1], bias[c + 2], bias[c + 3]};
    st4(out + row * N + c, acc);
}

extern "C" int vh_conv1d_wave(const float* x, const float* w, const float* bias, float* out, int B, int L, int C_out, int taps,
                              const int32_t* lens, void* stream) {
    VH_REQUIRE(x && w && out, VH_EINVAL, "vh_conv1d_wave: null pointer (x=%p w=%p out=%p)", (const void*)x, (const void*)w,
               (const void*)out);
    VH_REQUIRE(B > 0 && L > 0, VH_EINVAL, "vh_conv1d_wave: bad dims B=%d L=%d", B, L);
    VH_REQUIRE(taps >= 1 && taps <= 64, VH_EINVAL, "vh_conv1d_wave: taps=%d (1 .. 64)", taps);
    VH_REQUIRE(C_out > 0 && C_out % 4 == 0, VH_EUNSUPPORTED,
               "vh_conv1d_wave: C_out=%d (a multiple of 4: rows stay 16-byte aligned)", C_out);
    VH_REQUIRE(vh_aligned16(out), VH_EALIGN, "vh_conv1d_wave: out=%p must be 16-byte aligned", (const void*)out);
    VH_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(bias) |
                 reinterpret_cast<uintptr_t>(lens)) & 3u) == 0, VH_EALIGN,
               "vh_conv1d_wave: x=%p w=%p bias=%p lens=%p must be 4-byte aligned", (const void*)x, (const void*)w,
               (const void*)bias, (const void*)lens);
    const int64_t M = (int64_t)B * L;
    VH_REQUIRE(M <= (1LL << 40) / C_out, VH_EINVAL, "vh_conv1d_wave: B=%d L=%d C_out=%d: a tensor beyond 2^40 elements", B, L,
               C_out);
    const int64_t n_items = M * (C_out / 4);
    VH_REQUIRE((n_items + 255) / 256 <= 0x7fffffffLL, VH_EINVAL, "vh_conv1d_wave: B=%d L=%d C_out=%d exceed one grid", B, L, C_out);
    hipLaunchKernelGGL(conv1d_wave_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, w, bias,
                       out, L, C_out, taps, n_items, lens);
    VH_CHECK_LAUNCH("vh_conv1d_wave");
    return VH_OK;
}

// ------------------------------------------------------------------------------------------ the strided, downsampling convolution
extern "C" int vh_conv1d_down(const float* x, const float* w, const float* bias, float* out, int B, int T, int C_in, int C_out,
                              int taps, int stride, int elu, const int32_t* lens, void* stream) {
    VH_REQUIRE(x && w && out, VH_EINVAL, "vh_conv1d_down: null pointer (x=%p w=%p out=%p)", (const void*)x, (const void*)w,
               (const void*)out);
    VH_REQUIRE(B > 0 && T > 0, VH_EINVAL, "vh_conv1d_down: bad dims B=%d T=%d", B, T);
    VH_REQUIRE(stride >= 1 && taps >= stride && taps <= 64, VH_EINVAL, "vh_conv1d_down: taps=%d stride=%d (1 <= stride <= taps <= 64)",
               taps, stride);
    VH_REQUIRE(elu == 0 || elu == 1, VH_EINVAL, "vh_conv1d_down: elu=%d (0 or 1)", elu);
    VH_REQUIRE(C_in > 0 && C_in % 4 == 0, VH_EUNSUPPORTED, "vh_conv1d_down: C_in=%d (a multiple of 4: rows stay 16-byte aligned)",
               C_in);
    VH_REQUIRE(C_out > 0 && C_out % 4 == 0, VH_EUNSUPPORTED, "vh_conv1d_down: C_out=%d (a multiple of 4)", C_out);
    VH_REQUIRE(vh_aligned16(x) && vh_aligned16(w) && vh_aligned16(out), VH_EALIGN,
               "vh_conv1d_down: x=%p w=%p out=%p must be 16-byte aligned", (const void*)x, (const void*)w, (const void*)out);
    VH_REQUIRE(((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(lens)) & 3u) == 0, VH_EALIGN,
               "vh_conv1d_down: bias=%p lens=%p must be 4-byte aligned", (const void*)bias, (const void*)lens);
    const int Tout = (int)(((int64_t)T + stride - 1) / stride);
    const int64_t M = (int64_t)B * Tout;
    VH_REQUIRE((M + CV_BM - 1) / CV_BM <= 0x7fffffffLL, VH_EINVAL, "vh_conv1d_down: B=%d T=%d rows exceed one grid", B, T);
    VH_REQUIRE((int64_t)B * T <= (1LL << 40) / C_in && M <= (1LL << 40) / C_out, VH_EINVAL,
               "vh_conv1d_down: B=%d T=%d C_in=%d C_out=%d: a tensor beyond 2^40 elements", B, T, C_in, C_out);
    ConvArgs a{x, w, bias, nullptr, out, M, T, C_in, C_out, taps, 1, 1, elu, lens, 1, stride, Tout};
    const int nt = C_out > 64 ? 4 : C_out > 32 ? 2 : 1;
    const int64_t n_tiles = ((int64_t)C_out + 32 * nt - 1) / (32 * nt);
    VH_REQUIRE(n_tiles <= 65535, VH_EINVAL, "vh_conv1d_down: C_out=%d exceeds one grid", C_out);
    const dim3 grid((unsigned)((M + CV_BM - 1) / CV_BM), (unsigned)n_tiles), block(256);
    switch (nt) {
    case 4: hipLaunchKernelGGL((conv1d_causal_kernel<4, true>), grid, block, 0, (hipStream_t)stream, a); break;
    case 2: hipLaunchKernelGGL((conv1d_causal_kernel<2, true>), grid, block, 0, (hipStream_t)stream, a); break;
    default: hipLaunchKernelGGL((conv1d_causal_kernel<1, true>), grid, block, 0, (hipStream_t)stream, a); break;
    }
    VH_CHECK_LAUNCH("vh_conv1d_down");
    return VH_OK;
}

// --------------------------------------------------------------------------------------------------------------- RVQ encode
// One launch for all Q stages.  A workgroup owns 128 rows, a wave 32 of them; the residual never leaves the registers: lane
// (l31, h) holds channels 8 s + 4 h .. + 3 of row l31 — exactly its A fragments of v_mfma_f32_32x32x2_f32.  Per stage the
// codebook streams through LDS in chunks of 32 entries ([entry][D + 4]); the MFMA forms r.e for 32 rows x 32 entries (two
// accumulator sets, channels e % 2), the score is 2 r.e - |e|^2 and every lane keeps, for its 16 rows, the best score of the
// entries of its column (k = l31 mod 32, ascending: a strict > keeps the lowest index).  A butterfly over the 32 columns then
// settles each row (larger score, or the lower index of equal scores; the index starts at 0 and a NaN score never wins, so a
// non-finite row still ends inside [0, K)), the ids go through LDS to the lanes that hold the rows, and r -= E[q][id] in
// plain fp32.  Nothing a row computes depends on another row.
#define RQ_BM 128
#define RQ_KC 32
#define RQ_D_MAX 128
#define RQ_K_MAX 16384

template <int NS>     // 8-channel steps: D <= 8 NS
__global__ __launch_bounds__(256) void rvq_encode_kernel(const float* __restrict__ x, const float* __restrict__ books,
                                                         const float* __restrict__ esq, int64_t* __restrict__ codes, int64_t M, int T,
                                                         int D, int Q, int K) {
    constexpr int LD = 8 * NS + 4;
    constexpr int NV = NS / 4;                             // 32-channel staging vectors per lane
    __shared__ __attribute__((aligned(16))) float Es[RQ_KC * LD];
    __shared__ int ids[RQ_BM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int srow = tid >> 3, c4 = (tid & 7) * 4;
    const int64_t m = (int64_t)blockIdx.x * RQ_BM + wave * 32 + l31;      // the row whose residual this lane holds half of
    const bool live = m < M;

    f32x4 r[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = 8 * s + 4 * h;
        r[s] = live && c < D ? ld4(x + m * D + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t b = live ? m / T : 0;
    const int t = live ? (int)(m - b * T) : 0;

    for (int q = 0; q < Q; ++q) {
        const float* Eq = books + (int64_t)q * K * D;
        const float* nq = esq + (int64_t)q * K;
        float best[16];
        int bidx[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = -INFINITY;
            bidx[i] = 0;
        }
        for (int k0 = 0; k0 < K; k0 += RQ_KC) {
            f32x4 ev[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = 32 * i + c4;
                ev[i] = k0 + srow < K && c < D ? ld4(Eq + (int64_t)(k0 + srow) * D + c) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            __syncthreads();                                 // the chunk before has been read
#pragma unroll
            for (int i = 0; i < NV; ++i) st4(Es + srow * LD + 32 * i + c4, ev[i]);
            __syncthreads();
            f32x16 acc0, acc1;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (8 * s >= D) break;                       // the rest is zero fill
                const f32x4 bf = ld4(Es + l31 * LD + 8 * s + 4 * h);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(r[s].x, bf.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(r[s].y, bf.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(r[s].z, bf.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(r[s].w, bf.w, acc1, 0, 0, 0);
            }
            // accumulator register i of lane (l31, h): row (i & 3) + 8 (i >> 2) + 4 h of the wave's 32, entry k0 + l31
            const int k = k0 + l31;
            if (k < K) {
                const float en = nq[k];
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float sc = 2.f * (acc0[i] + acc1[i]) - en;
                    if (sc > best[i]) {
                        best[i] = sc;
                        bidx[i] = k;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) {        // stays inside the 32-lane half: the columns of one row
                const float so = __shfl_xor(best[i], off);
                const int io = __shfl_xor(bidx[i], off);
                if (so > best[i] || (so == best[i] && io < bidx[i])) {
                    best[i] = so;
                    bidx[i] = io;
                }
            }
            if (l31 == 0) ids[wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] = bidx[i];
        }
        __syncthreads();          // ids is written again only after the next stage's chunk barriers
        const int id = ids[wave * 32 + l31];
        if (live) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 8 * s + 4 * h;
                if (c < D) r[s] -= ld4(Eq + (int64_t)id * D + c);
            }
            if (h == 0) codes[(b * Q + q) * T + t] = id;
        }
    }
}

extern "C" int vh_rvq_encode(const float* x, const float* codebooks, const float* e_sq, int64_t* codes, int B, int T, int D, int Q,
                             int n_books, int K, void* stream) {
    VH_REQUIRE(x && codebooks && e_sq && codes, VH_EINVAL, "vh_rvq_encode: null pointer (x=%p codebooks=%p e_sq=%p codes=%p)",
               (const void*)x, (const void*)codebooks, (const void*)e_sq, (const void*)codes);
    VH_REQUIRE(B > 0 && T > 0 && Q > 0 && n_books > 0 && K > 0, VH_EINVAL, "vh_rvq_encode: bad dims B=%d T=%d Q=%d n_books=%d K=%d",
               B, T, Q, n_books, K);
    VH_REQUIRE(Q <= n_books, VH_EINVAL, "vh_rvq_encode: Q=%d codebooks asked of n_books=%d", Q, n_books);
    VH_REQUIRE(D > 0 && D % 4 == 0 && D <= RQ_D_MAX, VH_EUNSUPPORTED, "vh_rvq_encode: D=%d (a multiple of 4 up to %d)", D, RQ_D_MAX);
    VH_REQUIRE(K <= RQ_K_MAX, VH_EUNSUPPORTED, "vh_rvq_encode: K=%d (codebooks of up to %d entries)", K, RQ_K_MAX);
    VH_REQUIRE(vh_aligned16(x) && vh_aligned16(codebooks), VH_EALIGN, "vh_rvq_encode: x=%p codebooks=%p must be 16-byte aligned",
               (const void*)x, (const void*)codebooks);
    VH_REQUIRE((reinterpret_cast<uintptr_t>(e_sq) & 3u) == 0 && (reinterpret_cast<uintptr_t>(codes) & 7u) == 0, VH_EALIGN,
               "vh_rvq_encode: e_sq=%p must be 4-byte aligned, codes=%p 8-byte", (const void*)e_sq, (const void*)codes);
    const int64_t M = (int64_t)B * T;
    VH_REQUIRE((M + RQ_BM - 1) / RQ_BM <= 0x7fffffffLL, VH_EINVAL, "vh_rvq_encode: B=%d T=%d rows exceed one grid", B, T);
    VH_REQUIRE(M <= (1LL << 40) / (D > Q ? D : Q), VH_EINVAL, "vh_rvq_encode: B=%d T=%d D=%d Q=%d: a tensor beyond 2^40 elements", B,
               T, D, Q);
    const dim3 grid((unsigned)((M + RQ_BM - 1) / RQ_BM)), block(256);
    if (D <= 32)
        hipLaunchKernelGGL(rvq_encode_kernel<4>, grid, block, 0, (hipStream_t)stream, x, codebooks, e_sq, codes, M, T, D, Q, K);
    else if (D <= 64)
        hipLaunchKernelGGL(rvq_encode_kernel<8>, grid, block, 0, (hipStream_t)stream, x, codebooks, e_sq, codes, M, T, D, Q, K);
    else
        hipLaunchKernelGGL(rvq_encode_kernel<16>, grid, block, 0, (hipStream_t)stream, x, codebooks, e_sq, codes, M, T, D, Q, K);
    VH_CHECK_LAUNCH("vh_rvq_encode");
    return VH_OK;
}
