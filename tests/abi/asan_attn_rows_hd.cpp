// The host-side argument checks of vh_attn_rows_hd (many-row flash attention at a head width other than 64) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only, as tests/abi/asan_prompt_packed.cpp does for the packed prompt
// pass: the library's HOST code is compiled with -fsanitize=address,undefined and -fno-gpu-sanitize (device code untouched)
// and this stand-alone driver hands the entry one bad argument at a time.  Every "device pointer" points into a FREED
// block, so a host-side read or write through one is a use-after-free report.  Every call must be refused with the
// documented code before any launch (no device is needed).
// Exit code 0 and "asan_attn_rows_hd: N checks passed" = clean; a sanitizer report aborts the process.
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
#define REFUSED(code, call)                                                                                          \
    do {                                                                                                             \
        int rc_ = (call);                                                                                            \
        EXPECT(rc_ == (code) && strstr(vh_last_error(), "vh_attn_rows_hd"), "%s must return %d, rc=%d", #call, (code), rc_); \
    } while (0)

static char* poisoned() {
    char* block = (char*)aligned_alloc(64, 1 << 16);
    free(block);                           // any host read or write through it from now on is a use-after-free report
    return block;
}

struct Call {
    const float *q, *k, *v; float* out;
    int64_t qs[3], ks[3], vs[3], os[3];    // batch, head, row strides
    int B, h, hd, Tq, Tk; float scale; int mode, x_len;
    const int32_t *x_len_dev, *kv_len;
};
static int run(const Call& c) {
    return vh_attn_rows_hd(c.q, c.qs[0], c.qs[1], c.qs[2], c.k, c.ks[0], c.ks[1], c.ks[2], c.v, c.vs[0], c.vs[1], c.vs[2],
                           c.out, c.os[0], c.os[1], c.os[2], c.B, c.h, c.hd, c.Tq, c.Tk, c.scale, c.mode, c.x_len,
                           c.x_len_dev, c.kv_len, nullptr);
}

int main() {
    char* base = poisoned();
    float* P = (float*)base;
    float* MIS = (float*)(base + 4);                       // misaligned for the 16-byte rule
    int32_t* I32 = (int32_t*)(base + 8192);

    // q / k / v: the column blocks of a (B T, 3 h hd) projection; out: those of a (B T, h hd) buffer; B 2, h 3, hd 32, T 70
    const int B = 2, h = 3, hd = 32, T = 70;
    const int64_t ld = 3 * h * hd, ldo = h * hd;
    Call good = {P, P + h * hd, P + 2 * h * hd, P + 4096, {T * ld, hd, ld}, {T * ld, hd, ld}, {T * ld, hd, ld},
                 {T * ldo, hd, ldo}, B, h, hd, T, T, 0.17677669f, VH_MASK_PREFIX, 33, I32, I32};
    Call c;
#define WITH(stmt, code) do { c = good; stmt; REFUSED(code, run(c)); } while (0)
    // null operands
    WITH(c.q = nullptr, VH_EINVAL);
    WITH(c.k = nullptr, VH_EINVAL);
    WITH(c.v = nullptr, VH_EINVAL);
    WITH(c.out = nullptr, VH_EINVAL);
    // misaligned operands
    WITH(c.q = MIS, VH_EALIGN);
    WITH(c.k = MIS, VH_EALIGN);
    WITH(c.v = MIS, VH_EALIGN);
    WITH(c.out = MIS, VH_EALIGN);
    // strides that would leave a row off the 16-byte grid: every one of the twelve
    for (int i = 0; i < 3; ++i) {
        WITH(c.qs[i] += 2, VH_EINVAL);
        WITH(c.ks[i] += 1, VH_EINVAL);
        WITH(c.vs[i] += 3, VH_EINVAL);
        WITH(c.os[i] -= 2, VH_EINVAL);
    }
    // key rows the kernel's 32-bit offsets cannot reach, or a negative key stride
    WITH(c.ks[2] = -ld, VH_EUNSUPPORTED);
    WITH(c.vs[2] = -ld, VH_EUNSUPPORTED);
    WITH(c.ks[2] = INT64_MAX / 4 * 4, VH_EUNSUPPORTED);
    WITH(c.vs[2] = (int64_t)1 << 40, VH_EUNSUPPORTED);
    // dims
    const int bad[] = {0, -1, INT32_MIN};
    for (int v : bad) {
        WITH(c.B = v, VH_EINVAL);
        WITH(c.h = v, VH_EINVAL);
        WITH(c.Tq = v, VH_EINVAL);
        WITH(c.Tk = v, VH_EINVAL);                         // Tq > Tk
    }
    WITH(c.Tq = T + 1, VH_EINVAL);
    WITH((c.B = INT32_MAX, c.h = INT32_MAX), VH_EINVAL);   // the grid size is computed without overflow on the way to the refusal
    // widths
    const int widths[] = {0, -4, 4, 12, 18, 30, 130, 132, 192, 256, INT32_MAX, INT32_MIN};
    for (int w : widths) WITH(c.hd = w, VH_EUNSUPPORTED);
    // masks
    WITH(c.mode = VH_MASK_EXPLICIT, VH_EUNSUPPORTED);
    WITH(c.mode = 3, VH_EINVAL);
    WITH(c.mode = -1, VH_EINVAL);

    printf("asan_attn_rows_hd: %d checks passed\n", n_checks);
    return 0;
}
