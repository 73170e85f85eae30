// attn_l0_asan_driver.cpp — bounds audit of the level-0 self-attention form 27 (csrc/attention.hip) on the CPU: a stand-alone
// program (its own main, no Python) that drives sdmi_attention_vt_ex of an AddressSanitizer build of the host-emulated library with q | k
// and V^T in heap allocations of exactly the size a launch addresses.  Form 27 addresses a full KV tile without a clamp, so what is
// audited is that only full tiles go that way: key counts with a ragged last tile (1064 = 16 full tiles + 40 keys, prefetched from a
// steady-state iteration; 104 = one full tile; 40 = none), the stacked q | k layout whose last K row ends at the end of the allocation, and
// a dense K of exactly M rows, and two images of eight heads stacked as the engine lays them out.  A read past the last key row or past V^T's last column is an ASan report and a non-zero exit; form 27 must
// also give the bits of form 17 on the same (pre-scaled) operands.  A clean run prints "attn_l0_asan_driver: ok".
//
//   L=$(SDMI_HOSTEMU_ASAN=1 python tests/hostemu/build.py)
//   clang++ -std=c++17 -O1 -g1 -fsanitize=address -shared-libasan -Iinclude tools/micro/attn_l0_asan_driver.cpp $L \
//       -Wl,-rpath,$(dirname $L) -Wl,-rpath,$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so)) -o attn_l0_asan_driver
//   ASAN_OPTIONS=detect_leaks=0 ./attn_l0_asan_driver
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sdmi.h"
extern "C" void emu_set_threaded(int);
typedef _Float16 half_t;
static float rnd() { return (float)(rand() & 0xFFFF) / 65536.0f - 0.5f; }

static int attn(int B, int H, int N, int M, bool stacked) {
    const int D = 40, C = H * D, vt_ld = (M + 63) / 64 * 64;
    const float rs = std::sqrt((1.0f / std::sqrt((float)D)) * 1.4426950408889634f);
    const int ld = stacked ? 2 * C : C;
    // exact sizes (malloc: ASan sees the first byte past them); stacked: one [B, N, 2C] block, K = block + C
    const size_t qn = (size_t)B * N * ld, kn = (size_t)B * M * ld, vn = (size_t)B * C * vt_ld, on = (size_t)B * N * C;
    if (stacked && N != M) return 1;
    int bad = 0;
    half_t* qb = (half_t*)malloc(qn * 2);
    half_t* kb = stacked ? qb : (half_t*)malloc(kn * 2);
    half_t* vt = (half_t*)malloc(vn * 2);
    half_t* o17 = (half_t*)malloc(on * 2);
    half_t* o = (half_t*)malloc(on * 2);
    srand(7);
    for (size_t i = 0; i < qn; ++i) qb[i] = (half_t)(2.f * rnd() * rs);            // q (| k), pre-scaled
    if (!stacked) for (size_t i = 0; i < kn; ++i) kb[i] = (half_t)(2.f * rnd() * rs);
    for (size_t i = 0; i < vn; ++i) vt[i] = (i % vt_ld) < (size_t)M ? (half_t)rnd() : (half_t)0;
    const half_t* q = qb;
    const half_t* k = stacked ? qb + C : kb;
    const float scale = 1.0f / std::sqrt((float)D);
    int rc = sdmi_attention_vt_ex(q, k, vt, o, B, H, N, M, D, ld, ld, vt_ld, C, scale, 1, 27, 0, nullptr);
    if (rc) { printf("  form 27 rc=%d %s\n", rc, sdmi_last_error()); bad = 1; }
    rc = sdmi_attention_vt_ex(q, k, vt, o17, B, H, N, M, D, ld, ld, vt_ld, C, scale, 1, 17, 0, nullptr);
    if (rc) { printf("  form 17 rc=%d %s\n", rc, sdmi_last_error()); bad = 1; }
    for (size_t i = 0; i < on && !bad; ++i)
        if (!std::isfinite((float)o[i])) { printf("  form 27: non-finite output at %zu\n", i); bad = 1; }
    if (memcmp(o, o17, on * 2) != 0) { printf("  form 27 differs from form 17 (B %d H %d N %d M %d)\n", B, H, N, M); bad = 1; }
    free(qb); if (!stacked) free(kb); free(vt); free(o17); free(o);
    printf("B %d H %d N %d M %d %s: %s\n", B, H, N, M, stacked ? "stacked" : "dense", bad ? "BAD" : "ok");
    return bad;
}

int main() {
    setenv("SDMI_HOSTEMU", "1", 1);
    emu_set_threaded(1);
    int bad = 0;
    bad |= attn(1, 2, 1064, 1064, true);       // 16 full tiles + 40 keys, ragged query block; the last K row ends the allocation
    bad |= attn(1, 1, 1064, 1064, false);      // K of exactly 1064 rows of 40
    bad |= attn(1, 1, 200, 1088, false);       // 17 full tiles: the unclamped path reads the last rows of K itself
    bad |= attn(2, 1, 130, 104, false);        // one full tile + 40 keys
    bad |= attn(1, 2, 40, 40, true);           // no full tile at all
    bad |= attn(2, 8, 232, 232, true);         // the engine's layout: two images, eight heads (row stride 640, batch stride, all query blocks of a
                                               // head on one XCD), three full tiles + 40 keys
    printf(bad ? "attn_l0_asan_driver: FAILED\n" : "attn_l0_asan_driver: ok\n");
    return bad;
}
