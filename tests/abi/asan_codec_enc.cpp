// The host-side argument checks of the EnCodec encoder's entries (vh_conv1d_wave, vh_conv1d_down, vh_rvq_encode) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only, as tests/abi/asan_codec.cpp does for the decoder's: the library's
// HOST code is compiled with -fsanitize=address,undefined and -fno-gpu-sanitize (device code untouched) and this stand-alone
// driver hands each entry one bad argument at a time.  Every "device pointer" points into a FREED block, so a host-side read
// or write through one is a use-after-free report.  Every call must be refused with the documented code before any launch
// (no device is needed).
// Exit code 0 and "asan_codec_enc: N checks passed" = clean; a sanitizer report aborts the process.
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

struct Wave {
    const float *x, *w, *bias; float* out; int B, L, Cout, taps; const int32_t* lens;
};
static int run(const Wave& c) { return vh_conv1d_wave(c.x, c.w, c.bias, c.out, c.B, c.L, c.Cout, c.taps, c.lens, nullptr); }

struct Down {
    const float *x, *w, *bias; float* out; int B, T, Cin, Cout, taps, stride, elu; const int32_t* lens;
};
static int run(const Down& c) {
    return vh_conv1d_down(c.x, c.w, c.bias, c.out, c.B, c.T, c.Cin, c.Cout, c.taps, c.stride, c.elu, c.lens, nullptr);
}

struct Rvq {
    const float *x, *books, *esq; int64_t* codes; int B, T, D, Q, n_books, K;
};
static int run(const Rvq& c) { return vh_rvq_encode(c.x, c.books, c.esq, c.codes, c.B, c.T, c.D, c.Q, c.n_books, c.K, nullptr); }

int main() {
    char* base = poisoned();
    float* P = (float*)base;
    float* MIS = (float*)(base + 4);                       // misaligned for the 16-byte rule
    float* ODD = (float*)(base + 2);                       // misaligned for the 4-byte rule
    int32_t* I32 = (int32_t*)(base + 8192);
    const int bad[] = {0, -1, INT32_MIN};

    {   // ---- vh_conv1d_wave
        const char* E = "vh_conv1d_wave";
        const Wave good = {P, P + 1024, P + 2048, P + 3072, 2, 9, 8, 7, I32};
        Wave c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(E, code, run(c)); } while (0)
        WITH(c.x = nullptr, VH_EINVAL);
        WITH(c.w = nullptr, VH_EINVAL);
        WITH(c.out = nullptr, VH_EINVAL);
        WITH(c.out = MIS, VH_EALIGN);
        WITH(c.x = ODD, VH_EALIGN);
        WITH(c.w = ODD, VH_EALIGN);
        WITH(c.bias = ODD, VH_EALIGN);
        WITH(c.lens = (const int32_t*)(base + 2), VH_EALIGN);
        for (int v : bad) {
            WITH(c.B = v, VH_EINVAL);
            WITH(c.L = v, VH_EINVAL);
            WITH(c.taps = v, VH_EINVAL);
            WITH(c.Cout = v, VH_EUNSUPPORTED);
        }
        WITH(c.taps = 65, VH_EINVAL);
        WITH(c.taps = INT32_MAX, VH_EINVAL);
        const int outs[] = {1, 2, 3, 6, 30, INT32_MAX};
        for (int v : outs) WITH(c.Cout = v, VH_EUNSUPPORTED);
        WITH((c.B = 1 << 15, c.L = 1 << 20, c.Cout = 64), VH_EINVAL);            // a tensor beyond 2^40 elements
        WITH((c.B = INT32_MAX, c.L = INT32_MAX, c.Cout = INT32_MAX - 3), VH_EINVAL);   // no overflow on the way
        // null bias and lens are allowed: the next check in line refuses
        WITH((c.bias = nullptr, c.lens = nullptr, c.Cout = 5), VH_EUNSUPPORTED);
#undef WITH
    }
    {   // ---- vh_conv1d_down
        const char* E = "vh_conv1d_down";
        const Down good = {P, P + 1024, P + 2048, P + 3072, 2, 9, 32, 64, 4, 2, 1, I32};
        Down c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(E, code, run(c)); } while (0)
        WITH(c.x = nullptr, VH_EINVAL);
        WITH(c.w = nullptr, VH_EINVAL);
        WITH(c.out = nullptr, VH_EINVAL);
        WITH(c.x = MIS, VH_EALIGN);
        WITH(c.w = MIS, VH_EALIGN);
        WITH(c.out = MIS, VH_EALIGN);
        WITH(c.bias = ODD, VH_EALIGN);
        WITH(c.lens = (const int32_t*)(base + 2), VH_EALIGN);
        for (int v : bad) {
            WITH(c.B = v, VH_EINVAL);
            WITH(c.T = v, VH_EINVAL);
            WITH(c.taps = v, VH_EINVAL);
            WITH(c.stride = v, VH_EINVAL);
            WITH(c.Cin = v, VH_EUNSUPPORTED);
            WITH(c.Cout = v, VH_EUNSUPPORTED);
        }
        WITH(c.taps = 1, VH_EINVAL);                                            // fewer taps than the stride
        WITH(c.taps = 65, VH_EINVAL);
        WITH(c.taps = INT32_MAX, VH_EINVAL);
        WITH(c.stride = 5, VH_EINVAL);
        WITH(c.stride = INT32_MAX, VH_EINVAL);
        const int chans[] = {1, 2, 3, 6, 30, INT32_MAX};
        for (int v : chans) { WITH(c.Cin = v, VH_EUNSUPPORTED); WITH(c.Cout = v, VH_EUNSUPPORTED); }
        const int flags[] = {-1, 2, INT32_MAX};
        for (int v : flags) WITH(c.elu = v, VH_EINVAL);
        WITH((c.B = INT32_MAX, c.T = INT32_MAX, c.taps = 1, c.stride = 1), VH_EINVAL);   // rows beyond one grid, no overflow
        WITH((c.B = INT32_MAX, c.T = INT32_MAX), VH_EINVAL);
        WITH((c.B = 1 << 15, c.T = 1 << 20, c.Cin = 64), VH_EINVAL);            // a tensor beyond 2^40 elements
        WITH((c.Cout = INT32_MAX - 3, c.B = 1, c.T = 1), VH_EINVAL);            // columns beyond one grid
        WITH((c.bias = nullptr, c.lens = nullptr, c.Cout = 5), VH_EUNSUPPORTED);
#undef WITH
    }
    {   // ---- vh_rvq_encode
        const char* E = "vh_rvq_encode";
        const Rvq good = {P, P + 2048, P + 4096, (int64_t*)(base + 32768), 2, 9, 32, 4, 8, 64};
        Rvq c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(E, code, run(c)); } while (0)
        WITH(c.x = nullptr, VH_EINVAL);
        WITH(c.books = nullptr, VH_EINVAL);
        WITH(c.esq = nullptr, VH_EINVAL);
        WITH(c.codes = nullptr, VH_EINVAL);
        WITH(c.x = MIS, VH_EALIGN);
        WITH(c.books = MIS, VH_EALIGN);
        WITH(c.esq = ODD, VH_EALIGN);
        WITH(c.codes = (int64_t*)(base + 4), VH_EALIGN);
        for (int v : bad) {
            WITH(c.B = v, VH_EINVAL);
            WITH(c.T = v, VH_EINVAL);
            WITH(c.Q = v, VH_EINVAL);
            WITH(c.n_books = v, VH_EINVAL);
            WITH(c.K = v, VH_EINVAL);
            WITH(c.D = v, VH_EUNSUPPORTED);
        }
        WITH(c.Q = 9, VH_EINVAL);
        const int widths[] = {1, 2, 3, 30, 33, 132, 256, INT32_MAX};
        for (int d : widths) WITH(c.D = d, VH_EUNSUPPORTED);
        WITH(c.K = 16385, VH_EUNSUPPORTED);
        WITH(c.K = INT32_MAX, VH_EUNSUPPORTED);
        WITH((c.B = INT32_MAX, c.T = INT32_MAX), VH_EINVAL);                    // rows beyond one grid, no overflow on the way
        WITH((c.B = 1 << 15, c.T = 1 << 20, c.D = 128), VH_EINVAL);             // a tensor beyond 2^40 elements
        WITH((c.B = 1 << 15, c.T = 1 << 20, c.D = 4, c.Q = INT32_MAX, c.n_books = INT32_MAX), VH_EINVAL);   // ... of codes
#undef WITH
    }

    printf("asan_codec_enc: %d checks passed\n", n_checks);
    return 0;
}
