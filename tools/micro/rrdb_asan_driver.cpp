// rrdb_asan_driver.cpp — bounds audit of the RRDBNet conv kernel on the CPU: a stand-alone program (its own main, no Python) that drives
// sdmi_rrdb_conv and sdmi_esrgan_run of an AddressSanitizer build of the host-emulated library on heap buffers of exactly the size a launch
// addresses (an output slot ending at the row end, input rows exactly cin wide, a ragged single tile, the fused x2 gather, images that
// straddle tiles with the fp32 NCHW and uint8 stores, both residual epilogues; the x4 / x2 / x1 networks with uint8 and fp32 in / out).
// Global memory and the kernels' static LDS arrays are instrumented; a clean run prints "ASAN DRIVER DONE bad=0".
//
//   L=$(SDMI_HOSTEMU_ASAN=1 python tests/hostemu/build.py)
//   clang++ -std=c++17 -O1 -g1 -fsanitize=address -shared-libasan -Iinclude tools/micro/rrdb_asan_driver.cpp $L \
//       -Wl,-rpath,$(dirname $L) -Wl,-rpath,$(dirname $(clang++ -print-file-name=libclang_rt.asan-x86_64.so)) -o rrdb_asan_driver
//   ASAN_OPTIONS=detect_leaks=0 ./rrdb_asan_driver
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sdmi.h"
extern "C" void emu_set_threaded(int);
typedef _Float16 half_t;
static float rnd() { return (float)(rand() & 0xFFFF) / 65536.0f - 0.5f; }
int conv(int B, int H, int W, int cin, int lda, int nout, int n_real, int up, int ep, int store, int ldo, int off) {
    const int Hi = up ? H / 2 : H, Wi = up ? W / 2 : W;
    half_t* in = (half_t*)aligned_alloc(16, ((size_t)B * Hi * Wi * lda * 2 + 15) / 16 * 16);
    for (size_t i = 0; i < (size_t)B * Hi * Wi * lda; ++i) in[i] = (half_t)rnd();
    half_t* w = (half_t*)aligned_alloc(16, (size_t)nout * 9 * cin * 2);
    for (size_t i = 0; i < (size_t)nout * 9 * cin; ++i) w[i] = (half_t)(rnd() * 0.05f);
    float* bias = (float*)aligned_alloc(16, nout * 4);
    for (int i = 0; i < nout; ++i) bias[i] = rnd();
    const size_t M = (size_t)B * H * W;
    half_t* r1 = (half_t*)aligned_alloc(16, (M * 64 * 2 + 15) / 16 * 16);
    half_t* r2 = (half_t*)aligned_alloc(16, (M * 72 * 2 + 15) / 16 * 16);
    for (size_t i = 0; i < M * 64; ++i) r1[i] = (half_t)rnd();
    for (size_t i = 0; i < M * 72; ++i) r2[i] = (half_t)rnd();
    size_t ob = store == 0 ? M * ldo * 2 : store == 1 ? M * n_real * 4 : M * n_real;
    char* out = (char*)malloc(ob);                                  // exact size: ASan sees one byte past it
    sdmi_rrdb_desc d{};
    d.in = in; d.w = w; d.bias = bias; d.r1 = r1; d.r2 = r2; d.out = store == 0 ? out + 2 * off : out;
    d.B = B; d.H = H; d.W = W; d.cin = cin; d.lda = lda; d.up = up; d.nout = nout; d.n_real = n_real;
    d.ldo = ldo; d.ldr1 = 64; d.ldr2 = 72; d.ep = ep; d.store = store; d.alpha = 0.2f; d.beta = 0.2f;
    int rc = sdmi_rrdb_conv(&d, nullptr);
    if (rc) printf("  rc=%d %s\n", rc, sdmi_last_error());
    free(in); free(w); free(bias); free(r1); free(r2); free(out);
    return rc;
}
int main() {
    setenv("SDMI_HOSTEMU", "1", 1);
    emu_set_threaded(2);
    int bad = 0;
    bad |= conv(2, 12, 20, 64, 192, 32, 32, 0, 1, 0, 96, 64);     // slot ends exactly at the row end
    bad |= conv(2, 12, 20, 192, 192, 64, 64, 0, 3, 0, 64, 0);
    bad |= conv(1, 17, 13, 96, 96, 32, 32, 0, 1, 0, 32, 0);       // ragged single tile, input rows exactly cin wide
    bad |= conv(1, 14, 18, 64, 64, 64, 64, 1, 1, 0, 64, 0);       // fused x2 gather from 7 x 9
    bad |= conv(2, 9, 31, 64, 64, 32, 3, 0, 0, 1, 0, 0);          // conv_last fp32 NCHW, 279 pixels per image
    bad |= conv(2, 9, 31, 64, 64, 32, 3, 0, 0, 2, 0, 0);          // conv_last uint8
    bad |= conv(1, 5, 7, 32, 32, 64, 64, 0, 2, 0, 64, 0);
    printf("op-level launches done, bad=%d\n", bad);
    for (int scale : {4, 2, 1}) {
        const int in_ch = scale == 4 ? 3 : scale == 2 ? 12 : 48, f = 4 / scale;
        const int64_t n = sdmi_esrgan_blob_floats(1, in_ch);
        std::vector<float> blob(n);
        for (auto& v : blob) v = rnd() * 0.05f;
        sdmi_engine* e = sdmi_engine_create(0);
        sdmi_esrgan* net = sdmi_esrgan_create(e, blob.data(), n, 1, in_ch, scale);
        if (!net) { printf("create failed: %s\n", sdmi_last_error()); return 1; }
        const int B = 2, H = 3 * f * (scale == 4 ? 3 : 2), W = 5 * f;
        unsigned char* img = (unsigned char*)malloc((size_t)B * H * W * 3);
        for (size_t i = 0; i < (size_t)B * H * W * 3; ++i) img[i] = rand() & 255;
        unsigned char* o8 = (unsigned char*)malloc((size_t)B * H * scale * W * scale * 3);
        int rc = sdmi_esrgan_run(net, img, 1, B, H, W, o8, 1, nullptr);
        float* o32 = (float*)malloc((size_t)B * H * scale * W * scale * 3 * 4);
        float* i32 = (float*)malloc((size_t)B * H * W * 3 * 4);
        for (size_t i = 0; i < (size_t)B * H * W * 3; ++i) i32[i] = rnd() + 0.5f;
        rc |= sdmi_esrgan_run(net, i32, 0, B, H, W, o32, 0, nullptr);
        printf("esrgan x%d %dx%d rc=%d %s\n", scale, H, W, rc, rc ? sdmi_last_error() : "");
        bad |= rc;
        free(img); free(o8); free(o32); free(i32);
        sdmi_esrgan_destroy(net);
        sdmi_engine_destroy(e);
    }
    printf("ASAN DRIVER DONE bad=%d\n", bad);
    return bad;
}
