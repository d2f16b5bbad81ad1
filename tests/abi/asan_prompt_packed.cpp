// The host-side argument checks of the packed AR prompt pass (vh_kv_unpack, vh_transformer_forward_packed_lm) under
// AddressSanitizer + UndefinedBehaviorSanitizer, CPU only, as tests/abi/asan_host.cpp does for the older entry points: the
// library's HOST code is compiled with -fsanitize=address,undefined and -fno-gpu-sanitize (device code untouched) and this
// stand-alone driver calls both entries with one fault at a time.  Every "device pointer" points into a FREED block, so a
// host-side read or write through one is a use-after-free report; the descriptor and its layer table are real host memory,
// which the checks may read.  Every call must be refused before any launch (no device is needed).
// Exit code 0 and "asan_prompt_packed: N checks passed" = clean; a sanitizer report aborts the process.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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
#define REFUSED(code, call) do { int rc_ = (call); EXPECT(rc_ == (code) && vh_last_error()[0], "%s must return %d, rc=%d", #call, (code), rc_); } while (0)

static char* poisoned() {
    char* block = (char*)aligned_alloc(64, 1 << 16);
    free(block);                           // any host read or write through it from now on is a use-after-free report
    return block;
}

int main() {
    char* base = poisoned();
    float* P = (float*)base;
    float* P2 = (float*)(base + 4096);
    float* MIS = (float*)(base + 4);                       // misaligned for the 16-byte rule
    int32_t* I32 = (int32_t*)(base + 8192);
    int32_t* I32_MIS = (int32_t*)(base + 8194);            // misaligned for the 4-byte rule
    void* S = nullptr;

    // ---- vh_kv_unpack: src, dst, n_streams, n_heads, S_src, B_dst, S_dst, seg_start, seg_len, dst_row, n_seg ------------
    REFUSED(VH_EINVAL, vh_kv_unpack(nullptr, P2, 4, 2, 700, 8, 320, I32, I32, I32, 8, S));
    REFUSED(VH_EINVAL, vh_kv_unpack(P, nullptr, 4, 2, 700, 8, 320, I32, I32, I32, 8, S));
    REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, nullptr, I32, I32, 8, S));
    REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, I32, nullptr, I32, 8, S));
    REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, I32, I32, nullptr, 8, S));
    REFUSED(VH_EALIGN, vh_kv_unpack(MIS, P2, 4, 2, 700, 8, 320, I32, I32, I32, 8, S));
    REFUSED(VH_EALIGN, vh_kv_unpack(P, MIS, 4, 2, 700, 8, 320, I32, I32, I32, 8, S));
    REFUSED(VH_EALIGN, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, I32_MIS, I32, I32, 8, S));
    REFUSED(VH_EALIGN, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, I32, I32, I32_MIS, 8, S));
    const int bad[] = {0, -1, INT32_MIN};
    for (int v : bad) {
        REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, v, 2, 700, 8, 320, I32, I32, I32, 8, S));
        REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, v, 700, 8, 320, I32, I32, I32, 8, S));
        REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, v, 8, 320, I32, I32, I32, 8, S));
        REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, 700, v, 320, I32, I32, I32, 8, S));
        REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, 700, 8, v, I32, I32, I32, 8, S));
        REFUSED(VH_EINVAL, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, I32, I32, I32, v, S));
    }
    // the products and bounds the launch geometry is computed from: no overflow on the way to the refusal
    REFUSED(VH_EUNSUPPORTED, vh_kv_unpack(P, P2, INT32_MAX, INT32_MAX, 700, 8, 320, I32, I32, I32, 8, S));
    REFUSED(VH_EUNSUPPORTED, vh_kv_unpack(P, P2, 4, 2, 700, 8, 320, I32, I32, I32, 65536, S));
    REFUSED(VH_EUNSUPPORTED, vh_kv_unpack(P, P2, 4, 2, INT32_MAX, 8, 320, I32, I32, I32, 8, S));
    REFUSED(VH_EUNSUPPORTED, vh_kv_unpack(P, P2, 4, 2, 700, INT32_MAX, INT32_MAX, I32, I32, I32, 8, S));

    // ---- vh_transformer_forward_packed_lm -----------------------------------------------------------------------------
    vh_layer layers[2] = {};
    for (vh_layer& l : layers) { l.kcache = P; l.vcache = P2; }
    vh_forward_desc good = {};
    good.B = 1; good.T = 300; good.d_model = 128; good.n_heads = 2; good.dff = 256; good.n_layers = 2; good.S_max = 320;
    good.mode = VH_MASK_PREFIX; good.ln_eps = 1e-5f; good.layers = layers;
    good.x = P; good.xn = P; good.q = P; good.attn = P; good.hidden = P;
#define LM(desc, ...) vh_transformer_forward_packed_lm(desc, __VA_ARGS__, S)
    REFUSED(VH_EINVAL, LM(nullptr, I32, I32, I32, 3, I32, 4, P));
    REFUSED(VH_EINVAL, LM(&good, nullptr, I32, I32, 3, I32, 4, P));
    REFUSED(VH_EINVAL, LM(&good, I32, nullptr, I32, 3, I32, 4, P));
    REFUSED(VH_EINVAL, LM(&good, I32, I32, nullptr, 3, I32, 4, P));
    REFUSED(VH_EINVAL, LM(&good, I32, I32, I32, 3, nullptr, 4, P));
    REFUSED(VH_EINVAL, LM(&good, I32, I32, I32, 3, I32, 4, nullptr));
    REFUSED(VH_EALIGN, LM(&good, I32, I32, I32, 3, I32, 4, (float*)(base + 2)));
    REFUSED(VH_EINVAL, LM(&good, I32, I32, I32, 0, I32, 4, P));
    REFUSED(VH_EINVAL, LM(&good, I32, I32, I32, -1, I32, 4, P));
    REFUSED(VH_EINVAL, LM(&good, I32, I32, I32, 3, I32, 0, P));
    REFUSED(VH_EUNSUPPORTED, LM(&good, I32, I32, I32, 3, I32, INT32_MAX, P));      // n_blocks x n_heads workgroups
    vh_forward_desc f;
#define WITH(stmt, code) do { f = good; stmt; REFUSED(code, LM(&f, I32, I32, I32, 3, I32, 4, P)); } while (0)
    WITH(f.mode = VH_MASK_FULL, VH_EUNSUPPORTED);
    WITH(f.mode = VH_MASK_EXPLICIT, VH_EUNSUPPORTED);
    WITH(f.mode = 77, VH_EUNSUPPORTED);
    WITH(f.B = 2, VH_EINVAL);
    WITH(f.B = 0, VH_EINVAL);
    WITH(f.T = 0, VH_EINVAL);
    WITH(f.T = -5, VH_EINVAL);
    WITH(f.n_layers = 0, VH_EINVAL);
    WITH(f.S_max = 299, VH_EINVAL);
    WITH(f.kv_len = I32, VH_EUNSUPPORTED);
    WITH(f.x_len_dev = I32, VH_EUNSUPPORTED);
    WITH(f.mask = (const uint8_t*)P, VH_EUNSUPPORTED);
    WITH(f.pad = (const uint8_t*)P, VH_EUNSUPPORTED);
    WITH(f.ada = P, VH_EUNSUPPORTED);
    WITH(f.n_heads = 4, VH_EUNSUPPORTED);
    WITH(f.d_model = INT32_MAX, VH_EUNSUPPORTED);
    WITH(f.layers = nullptr, VH_EINVAL);
    WITH(f.x = nullptr, VH_EINVAL);
    WITH(f.xn = nullptr, VH_EINVAL);
    WITH(f.q = nullptr, VH_EINVAL);
    WITH(f.attn = nullptr, VH_EINVAL);
    WITH(f.hidden = nullptr, VH_EINVAL);
    WITH(f.q = MIS, VH_EALIGN);
    WITH(f.attn = MIS, VH_EALIGN);
    vh_layer broken[2] = {layers[0], layers[1]};
    broken[1].kcache = MIS;
    WITH(f.layers = broken, VH_EALIGN);
    broken[1].kcache = P;
    broken[1].vcache = nullptr;
    WITH(f.layers = broken, VH_EINVAL);
    // the full-mask composite still refuses the prefix mask: the new entry is no new mode of the old one
    f = good;
    EXPECT(vh_transformer_forward_packed(&f, I32, I32, 3, I32, 4, S) == VH_EUNSUPPORTED, "vh_transformer_forward_packed takes the full mask only");

    printf("asan_prompt_packed: %d checks passed\n", n_checks);
    return 0;
}
