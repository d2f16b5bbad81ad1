// The host-side argument checks of vh_attn_rows_hd_lse and vh_attn_rows_hd_bwd (training on flash attention at a head width
// other than 64) and vh_attn_rows_hd_bwd_ws_bytes under AddressSanitizer + UndefinedBehaviorSanitizer, CPU only, as
// tests/abi/asan_attn_rows_hd.cpp does for the forward: the library's HOST code is compiled with -fsanitize=address,undefined
// and -fno-gpu-sanitize (device code untouched) and this stand-alone driver hands the entries one bad argument at a time.
// Every "device pointer" points into a FREED block, so a host-side read or write through one is a use-after-free report.
// Every call must be refused with the documented code before any launch (no device is needed).
// Exit code 0 and "asan_attn_rows_hd_bwd: N checks passed" = clean; a sanitizer report aborts the process.
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
#define REFUSED(entry, code, call)                                                                             \
    do {                                                                                                       \
        int rc_ = (call);                                                                                      \
        EXPECT(rc_ == (code) && strstr(vh_last_error(), entry ":"), "%s must return %d, rc=%d", #call, (code), rc_); \
    } while (0)

static char* poisoned() {
    char* block = (char*)aligned_alloc(64, 1 << 16);
    free(block);                           // any host read or write through it from now on is a use-after-free report
    return block;
}

struct Call {
    const float *q, *k, *v, *out, *dout, *lse2; float *dq, *dk, *dv;
    int64_t qs[3], ks[3], vs[3], os[3], ds[3], gs[3];    // batch, head, row strides
    int B, h, hd, T; float scale; int mode, x_len;
    const int32_t *x_len_dev, *kv_len;
    void* ws; size_t ws_bytes;
};
static int bwd(const Call& c) {
    return vh_attn_rows_hd_bwd(c.q, c.qs[0], c.qs[1], c.qs[2], c.k, c.ks[0], c.ks[1], c.ks[2], c.v, c.vs[0], c.vs[1], c.vs[2],
                               c.out, c.os[0], c.os[1], c.os[2], c.dout, c.ds[0], c.ds[1], c.ds[2], c.lse2, c.dq, c.dk, c.dv,
                               c.gs[0], c.gs[1], c.gs[2], c.B, c.h, c.hd, c.T, c.scale, c.mode, c.x_len, c.x_len_dev, c.kv_len,
                               c.ws, c.ws_bytes, nullptr);
}
static int lse(const Call& c) {
    return vh_attn_rows_hd_lse(c.q, c.qs[0], c.qs[1], c.qs[2], c.k, c.ks[0], c.ks[1], c.ks[2], c.v, c.vs[0], c.vs[1], c.vs[2],
                               (float*)c.out, c.os[0], c.os[1], c.os[2], c.B, c.h, c.hd, c.T, c.T, c.scale, c.mode, c.x_len,
                               c.x_len_dev, c.kv_len, (float*)c.lse2, nullptr);
}

int main() {
    char* base = poisoned();
    float* P = (float*)base;
    float* MIS = (float*)(base + 4);                       // misaligned for the 16-byte rule
    int32_t* I32 = (int32_t*)(base + 8192);

    // q / k / v and dq / dk / dv: the column blocks of (B T, 3 h hd) buffers; out / dout: those of (B T, h hd) buffers
    const int B = 2, h = 3, hd = 32, T = 70;
    const int64_t ld = 3 * h * hd, ldo = h * hd;
    const size_t need = vh_attn_rows_hd_bwd_ws_bytes(B, h, T);
    EXPECT(need >= (size_t)B * h * T * sizeof(float) && need % 16 == 0, "ws bytes %zu", need);
    EXPECT(vh_attn_rows_hd_bwd_ws_bytes(1, 1, 1) >= 4, "ws bytes of one element");
    EXPECT(vh_attn_rows_hd_bwd_ws_bytes(INT32_MAX, 1, 1) >= (size_t)INT32_MAX * 4, "ws bytes: no 32-bit product");
    EXPECT(vh_attn_rows_hd_bwd_ws_bytes(1 << 15, 1 << 10, 1 << 10) >= ((size_t)1 << 37), "ws bytes: no 32-bit product");
    EXPECT(vh_attn_rows_hd_bwd_ws_bytes(0, h, T) == 0 && vh_attn_rows_hd_bwd_ws_bytes(B, -1, T) == 0 &&
               vh_attn_rows_hd_bwd_ws_bytes(B, h, INT32_MIN) == 0, "ws bytes of an empty problem");

    Call good = {P, P + h * hd, P + 2 * h * hd, P + 2048, P + 3072, P + 4096, P + 5120, P + 5120 + h * hd, P + 5120 + 2 * h * hd,
                 {T * ld, hd, ld}, {T * ld, hd, ld}, {T * ld, hd, ld}, {T * ldo, hd, ldo}, {T * ldo, hd, ldo}, {T * ld, hd, ld},
                 B, h, hd, T, 0.17677669f, VH_MASK_PREFIX, 33, I32, I32, P + 8192, need};
    Call c;
#define BWD(stmt, code) do { c = good; stmt; REFUSED("vh_attn_rows_hd_bwd", code, bwd(c)); } while (0)
#define LSE(stmt, code) do { c = good; stmt; REFUSED("vh_attn_rows_hd_lse", code, lse(c)); } while (0)
    // null operands
    BWD(c.q = nullptr, VH_EINVAL);
    BWD(c.k = nullptr, VH_EINVAL);
    BWD(c.v = nullptr, VH_EINVAL);
    BWD(c.out = nullptr, VH_EINVAL);
    BWD(c.dout = nullptr, VH_EINVAL);
    BWD(c.lse2 = nullptr, VH_EINVAL);
    BWD(c.dq = nullptr, VH_EINVAL);
    BWD(c.dk = nullptr, VH_EINVAL);
    BWD(c.dv = nullptr, VH_EINVAL);
    BWD(c.ws = nullptr, VH_EINVAL);
    // misaligned operands
    BWD(c.q = MIS, VH_EALIGN);
    BWD(c.k = MIS, VH_EALIGN);
    BWD(c.v = MIS, VH_EALIGN);
    BWD(c.out = MIS, VH_EALIGN);
    BWD(c.dout = MIS, VH_EALIGN);
    BWD(c.lse2 = MIS, VH_EALIGN);
    BWD(c.dq = MIS, VH_EALIGN);
    BWD(c.dk = MIS, VH_EALIGN);
    BWD(c.dv = MIS, VH_EALIGN);
    BWD(c.ws = MIS, VH_EALIGN);
    // strides that would leave a row off the 16-byte grid: every one of the eighteen
    for (int i = 0; i < 3; ++i) {
        BWD(c.qs[i] += 2, VH_EINVAL);
        BWD(c.ks[i] += 1, VH_EINVAL);
        BWD(c.vs[i] += 3, VH_EINVAL);
        BWD(c.os[i] -= 2, VH_EINVAL);
        BWD(c.ds[i] -= 1, VH_EINVAL);
        BWD(c.gs[i] += 6, VH_EINVAL);
    }
    // rows the kernels' 32-bit offsets cannot reach, or a negative stride of a staged operand
    BWD(c.qs[2] = -ld, VH_EUNSUPPORTED);
    BWD(c.ks[2] = -ld, VH_EUNSUPPORTED);
    BWD(c.vs[2] = -ld, VH_EUNSUPPORTED);
    BWD(c.ds[2] = -ldo, VH_EUNSUPPORTED);
    BWD(c.qs[2] = INT64_MAX / 4 * 4, VH_EUNSUPPORTED);
    BWD(c.ks[2] = (int64_t)1 << 40, VH_EUNSUPPORTED);
    BWD(c.vs[2] = INT64_MAX / 4 * 4, VH_EUNSUPPORTED);
    BWD(c.ds[2] = (int64_t)1 << 40, VH_EUNSUPPORTED);
    // dims
    const int bad[] = {0, -1, INT32_MIN};
    for (int v : bad) {
        BWD(c.B = v, VH_EINVAL);
        BWD(c.h = v, VH_EINVAL);
        BWD(c.T = v, VH_EINVAL);
    }
    BWD((c.B = INT32_MAX, c.h = INT32_MAX, c.ws_bytes = SIZE_MAX), VH_EINVAL);   // the grid size is computed without overflow
    BWD((c.B = INT32_MAX, c.h = INT32_MAX, c.T = 129, c.ws_bytes = SIZE_MAX), VH_EINVAL);
    // widths
    const int widths[] = {0, -4, 4, 12, 18, 30, 130, 132, 192, 256, INT32_MAX, INT32_MIN};
    for (int w : widths) BWD(c.hd = w, VH_EUNSUPPORTED);
    // masks
    BWD(c.mode = VH_MASK_EXPLICIT, VH_EUNSUPPORTED);
    BWD(c.mode = 3, VH_EINVAL);
    BWD(c.mode = -1, VH_EINVAL);
    // workspace
    BWD(c.ws_bytes = need - 1, VH_EINVAL);
    BWD(c.ws_bytes = 0, VH_EINVAL);

    // the forward with lse: its own two checks and the forward's under its name
    LSE(c.lse2 = nullptr, VH_EINVAL);
    LSE(c.lse2 = MIS, VH_EALIGN);
    LSE(c.q = nullptr, VH_EINVAL);
    LSE(c.out = nullptr, VH_EINVAL);
    LSE(c.k = MIS, VH_EALIGN);
    LSE(c.v = MIS, VH_EALIGN);
    for (int i = 0; i < 3; ++i) {
        LSE(c.qs[i] += 2, VH_EINVAL);
        LSE(c.os[i] -= 2, VH_EINVAL);
    }
    LSE(c.ks[2] = -ld, VH_EUNSUPPORTED);
    LSE(c.vs[2] = (int64_t)1 << 40, VH_EUNSUPPORTED);
    for (int v : bad) {
        LSE(c.B = v, VH_EINVAL);
        LSE(c.h = v, VH_EINVAL);
        LSE(c.T = v, VH_EINVAL);
    }
    LSE((c.B = INT32_MAX, c.h = INT32_MAX), VH_EINVAL);
    for (int w : widths) LSE(c.hd = w, VH_EUNSUPPORTED);
    LSE(c.mode = VH_MASK_EXPLICIT, VH_EUNSUPPORTED);
    LSE(c.mode = 3, VH_EINVAL);

    printf("asan_attn_rows_hd_bwd: %d checks passed\n", n_checks);
    return 0;
}
