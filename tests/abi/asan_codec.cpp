// The host-side argument checks of the EnCodec decoder's entries (vh_rvq_decode, vh_conv1d_causal, vh_lstm_layer) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only, as tests/abi/asan_attn_rows_hd.cpp does for the many-row attention:
// the library's HOST code is compiled with -fsanitize=address,undefined and -fno-gpu-sanitize (device code untouched) and this
// stand-alone driver hands each entry one bad argument at a time.  Every "device pointer" points into a FREED block, so a
// host-side read or write through one is a use-after-free report.  Every call must be refused with the documented code before
// any launch (no device is needed).
// Exit code 0 and "asan_codec: N checks passed" = clean; a sanitizer report aborts the process.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "valle_hip.h"

static int n_checks = 0;
#define EXPECT(cond, ...)                                         \
    do {                                                          \
        ++n_checks;                                               \
        if (!(cond)) {                                            \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);  \
            fprintf(stderr, __VA_ARGS__);                         \
            fprintf(stderr, " (last error: '%s')\n", vh_last_error()); \
            exit(1);                                              \
        }                                                         \
    } while (0)
// refused with `code`, and the message names the entry
#define REFUSED(entry, code, call)                                                                               \
    do {                                                                                                         \
        int rc_ = (call);                                                                                        \
        EXPECT(rc_ == (code) && strstr(vh_last_error(), entry), "%s must return %d, rc=%d", #call, (code), rc_); \
    } while (0)

static char* poisoned() {
    char* block = (char*)aligned_alloc(64, 1 << 16);
    free(block);                           // any host read or write through it from now on is a use-after-free report
    return block;
}

struct Rvq {
    const int64_t* codes; const float* books; float* out; int B, Q, T, n_books, K, D; int32_t* flag;
};
static int run(const Rvq& c) { return vh_rvq_decode(c.codes, c.books, c.out, c.B, c.Q, c.T, c.n_books, c.K, c.D, c.flag, nullptr); }

struct Conv {
    const float *x, *w, *bias, *res; float* out; int B, T, Cin, Cout, taps, dil, pad_mode, elu; const int32_t* lens; int scale;
};
static int run(const Conv& c) {
    return vh_conv1d_causal(c.x, c.w, c.bias, c.res, c.out, c.B, c.T, c.Cin, c.Cout, c.taps, c.dil, c.pad_mode, c.elu, c.lens,
                            c.scale, nullptr);
}

struct Lstm {
    const float *xproj, *whh; float *h, *c; const float* skip; float* y; int B, T, H;
};
static int run(const Lstm& c) { return vh_lstm_layer(c.xproj, c.whh, c.h, c.c, c.skip, c.y, c.B, c.T, c.H, nullptr); }

int main() {
    char* base = poisoned();
    float* P = (float*)base;
    float* MIS = (float*)(base + 4);                       // misaligned for the 16-byte rule
    int32_t* I32 = (int32_t*)(base + 8192);
    const int bad[] = {0, -1, INT32_MIN};

    {   // ---- vh_rvq_decode
        const char* E = "vh_rvq_decode";
        const Rvq good = {(const int64_t*)(base + 4096), P, P + 2048, 2, 4, 9, 8, 64, 32, I32};
        Rvq c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(E, code, run(c)); } while (0)
        WITH(c.codes = nullptr, VH_EINVAL);
        WITH(c.books = nullptr, VH_EINVAL);
        WITH(c.out = nullptr, VH_EINVAL);
        WITH(c.codes = (const int64_t*)(base + 4), VH_EALIGN);
        WITH(c.books = MIS, VH_EALIGN);
        WITH(c.out = MIS, VH_EALIGN);
        for (int v : bad) {
            WITH(c.B = v, VH_EINVAL);
            WITH(c.Q = v, VH_EINVAL);
            WITH(c.T = v, VH_EINVAL);
            WITH(c.n_books = v, VH_EINVAL);
            WITH(c.K = v, VH_EINVAL);
            WITH(c.D = v, VH_EUNSUPPORTED);
        }
        WITH(c.Q = 9, VH_EINVAL);
        const int widths[] = {1, 2, 3, 30, 33, INT32_MAX};
        for (int d : widths) WITH(c.D = d, VH_EUNSUPPORTED);
        WITH((c.B = INT32_MAX, c.T = INT32_MAX, c.D = INT32_MAX - 3), VH_EINVAL);   // the grid size is computed without overflow
#undef WITH
    }
    {   // ---- vh_conv1d_causal
        const char* E = "vh_conv1d_causal";
        const Conv good = {P, P + 1024, P + 2048, P + 3072, P + 4096, 2, 9, 32, 16, 3, 2, VH_PAD_REFLECT, 1, I32, 4};
        Conv c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(E, code, run(c)); } while (0)
        WITH(c.x = nullptr, VH_EINVAL);
        WITH(c.w = nullptr, VH_EINVAL);
        WITH(c.out = nullptr, VH_EINVAL);
        WITH(c.x = MIS, VH_EALIGN);
        WITH(c.w = MIS, VH_EALIGN);
        WITH(c.res = MIS, VH_EALIGN);
        WITH(c.out = MIS, VH_EALIGN);
        WITH(c.bias = (const float*)(base + 2), VH_EALIGN);
        WITH(c.lens = (const int32_t*)(base + 2), VH_EALIGN);
        for (int v : bad) {
            WITH(c.B = v, VH_EINVAL);
            WITH(c.T = v, VH_EINVAL);
            WITH(c.taps = v, VH_EINVAL);
            WITH(c.dil = v, VH_EINVAL);
            WITH(c.scale = v, VH_EINVAL);
            WITH(c.Cin = v, VH_EUNSUPPORTED);
            WITH(c.Cout = v, VH_EUNSUPPORTED);
        }
        WITH(c.taps = 65, VH_EINVAL);
        WITH(c.taps = INT32_MAX, VH_EINVAL);
        WITH(c.dil = 4097, VH_EINVAL);
        WITH(c.dil = INT32_MAX, VH_EINVAL);
        WITH(c.scale = INT32_MAX, VH_EINVAL);
        const int chans[] = {1, 2, 3, 6, 30, INT32_MAX};
        for (int v : chans) WITH(c.Cin = v, VH_EUNSUPPORTED);
        const int outs[] = {2, 3, 6, 30, INT32_MAX};
        for (int v : outs) WITH(c.Cout = v, VH_EUNSUPPORTED);
        const int modes[] = {-1, 2, INT32_MAX};
        for (int v : modes) { WITH(c.pad_mode = v, VH_EINVAL); WITH(c.elu = v, VH_EINVAL); }
        WITH((c.B = INT32_MAX, c.T = INT32_MAX), VH_EINVAL);                    // rows beyond one grid, no overflow on the way
        WITH((c.B = 1 << 15, c.T = 1 << 20, c.Cin = 64), VH_EINVAL);            // a tensor beyond 2^40 elements
        WITH((c.Cout = INT32_MAX - 3, c.B = 1, c.T = 1), VH_EINVAL);            // columns beyond one grid
        // null bias, residual and lens are allowed: the next check in line refuses
        WITH((c.bias = nullptr, c.res = nullptr, c.lens = nullptr, c.scale = 0, c.Cout = 5), VH_EUNSUPPORTED);
#undef WITH
    }
    {   // ---- vh_lstm_layer
        const char* E = "vh_lstm_layer";
        const Lstm good = {P, P + 1024, P + 2048, P + 3072, P + 4096, P + 5120, 2, 9, 32};
        Lstm c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(E, code, run(c)); } while (0)
        WITH(c.xproj = nullptr, VH_EINVAL);
        WITH(c.whh = nullptr, VH_EINVAL);
        WITH(c.h = nullptr, VH_EINVAL);
        WITH(c.c = nullptr, VH_EINVAL);
        WITH(c.skip = nullptr, VH_EINVAL);
        WITH(c.y = nullptr, VH_EINVAL);
        WITH(c.xproj = MIS, VH_EALIGN);
        WITH(c.whh = MIS, VH_EALIGN);
        WITH(c.h = MIS, VH_EALIGN);
        WITH(c.c = MIS, VH_EALIGN);
        WITH(c.skip = MIS, VH_EALIGN);
        WITH(c.y = MIS, VH_EALIGN);
        for (int v : bad) {
            WITH(c.B = v, VH_EINVAL);
            WITH(c.T = v, VH_EINVAL);
            WITH(c.H = v, VH_EUNSUPPORTED);
        }
        WITH(c.T = (1 << 20) + 1, VH_EINVAL);
        const int hs[] = {2, 30, 1028, 2048, INT32_MAX};
        for (int v : hs) WITH(c.H = v, VH_EUNSUPPORTED);
        WITH((c.B = INT32_MAX, c.T = 1 << 20, c.H = 1024), VH_EINVAL);          // a tensor beyond 2^40 elements, no overflow
#undef WITH
    }

    printf("asan_codec: %d checks passed\n", n_checks);
    return 0;
}
