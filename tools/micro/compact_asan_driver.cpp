// compact_asan_driver.cpp — bounds audit of the compact Real-ESRGAN conv kernel on the CPU: a stand-alone program (its own main, no
// Python) that drives sdmi_compact_conv and sdmi_compact_run of an AddressSanitizer build of the host-emulated library on heap buffers
// of exactly the size a launch addresses (input rows exactly cin wide, output rows exactly n_real wide; 12 x 20, 17 x 13 and 33 x 35
// tiles, one workgroup walking every tile of two images, every tail store for r = 1 .. 4 with uint8 and fp32 base; the x1 .. x4 networks
// with uint8 and fp32 in / out).  Global memory and the kernel's LDS array (static in this build) are instrumented; a clean run prints
// "ASAN DRIVER DONE bad=0".
//
//   L=$(SDMI_HOSTEMU_ASAN=1 python tests/hostemu/build.py)
//   clang++ -std=c++17 -O1 -g1 -fsanitize=address -shared-libasan -Iinclude tools/micro/compact_asan_driver.cpp $L \
//       -Wl,-rpath,$(dirname $L) -Wl,-rpath,$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so)) -o compact_asan_driver
//   ASAN_OPTIONS=detect_leaks=0 ./compact_asan_driver
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sdmi.h"
extern "C" void emu_set_threaded(int);
typedef _Float16 half_t;
static float rnd() { return (float)(rand() & 0xFFFF) / 65536.0f - 0.5f; }
// ep 0 / 1: fp16 rows of exactly n_real channels.  ep 2 (tail): r, base_u8, out_u8.
int conv(int B, int H, int W, int cin, int n_real, int ep, int r, int base_u8, int out_u8, int grid_cap) {
    const size_t M = (size_t)B * H * W;
    half_t* in = (half_t*)aligned_alloc(16, M * cin * 2);                       // cin 32 / 64: a multiple of 16 bytes, exact
    for (size_t i = 0; i < M * cin; ++i) in[i] = (half_t)rnd();
    half_t* w = (half_t*)aligned_alloc(16, (size_t)64 * 9 * cin * 2);
    for (size_t i = 0; i < (size_t)64 * 9 * cin; ++i) w[i] = (half_t)(rnd() * 0.05f);
    float* bias = (float*)aligned_alloc(16, 64 * 4);
    float* slope = (float*)aligned_alloc(16, 64 * 4);
    for (int i = 0; i < 64; ++i) { bias[i] = rnd(); slope[i] = rnd(); }
    const size_t bb = M * 3 * (base_u8 ? 1 : 4);
    char* base = (char*)malloc(bb);
    for (size_t i = 0; i < bb; ++i) base[i] = base_u8 ? (char)(rand() & 255) : 0;
    const size_t ob = ep == 2 ? M * r * r * 3 * (out_u8 ? 1 : 4) : M * n_real * 2;
    char* out = (char*)malloc(ob);                                  // exact size: ASan sees one byte past it
    sdmi_compact_desc d{};
    d.in = in; d.w = w; d.bias = bias; d.slope = slope; d.base = base; d.out = out;
    d.B = B; d.H = H; d.W = W; d.cin = cin; d.lda = cin; d.ldo = ep == 2 ? 0 : n_real; d.n_real = n_real;
    d.ep = ep; d.r = r; d.base_u8 = base_u8; d.out_u8 = out_u8; d.grid_cap = grid_cap;
    int rc = sdmi_compact_conv(&d, nullptr);
    if (rc) printf("  rc=%d %s\n", rc, sdmi_last_error());
    free(in); free(w); free(bias); free(slope); free(base); free(out);
    return rc;
}
int main() {
    setenv("SDMI_HOSTEMU", "1", 1);
    emu_set_threaded(2);
    int bad = 0;
    const int geo[3][2] = {{12, 20}, {17, 13}, {33, 35}};
    for (auto& g : geo) {
        bad |= conv(1, g[0], g[1], 64, 64, 1, 0, 0, 0, 0);
        bad |= conv(2, g[0], g[1], 32, 64, 0, 0, 0, 0, 0);
    }
    bad |= conv(2, 33, 35, 64, 64, 1, 0, 0, 0, 1);                // one workgroup, 18 tiles, both halo slots
    bad |= conv(2, 17, 13, 64, 20, 0, 0, 0, 0, 1);                // 20 of 64 channels stored, rows exactly 40 bytes
    for (int r = 1; r <= 4; ++r)
        for (int form = 0; form < 4; ++form) bad |= conv(2, 17, 13, 64, 3 * r * r, 2, r, form & 1, form >> 1, form == 3 ? 1 : 0);
    printf("op-level launches done, bad=%d\n", bad);
    for (int scale = 1; scale <= 4; ++scale) {
        const int num_conv = 2;
        const int64_t n = sdmi_compact_blob_floats(num_conv, scale);
        std::vector<float> blob(n);
        for (auto& v : blob) v = rnd() * 0.05f;
        sdmi_engine* e = sdmi_engine_create(0);
        sdmi_compact* net = sdmi_compact_create(e, blob.data(), n, num_conv, scale);
        if (!net) { printf("create failed: %s\n", sdmi_last_error()); return 1; }
        const int B = 2, H = 17, W = 19;
        unsigned char* img = (unsigned char*)malloc((size_t)B * H * W * 3);
        for (size_t i = 0; i < (size_t)B * H * W * 3; ++i) img[i] = rand() & 255;
        unsigned char* o8 = (unsigned char*)malloc((size_t)B * H * scale * W * scale * 3);
        int rc = sdmi_compact_run(net, img, 1, B, H, W, o8, 1, nullptr);
        float* o32 = (float*)malloc((size_t)B * H * scale * W * scale * 3 * 4);
        float* i32 = (float*)malloc((size_t)B * H * W * 3 * 4);
        for (size_t i = 0; i < (size_t)B * H * W * 3; ++i) i32[i] = rnd() + 0.5f;
        rc |= sdmi_compact_run(net, i32, 0, B, H, W, o32, 0, nullptr);
        printf("compact x%d %dx%d rc=%d %s\n", scale, H, W, rc, rc ? sdmi_last_error() : "");
        bad |= rc;
        free(img); free(o8); free(o32); free(i32);
        sdmi_compact_destroy(net);
        sdmi_engine_destroy(e);
    }
    printf("ASAN DRIVER DONE bad=%d\n", bad);
    return bad;
}
