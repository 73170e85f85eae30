// rrdb.hip — the 3x3 convolution of the RRDBNet upscalers (ESRGAN / Real-ESRGAN; BasicSR basicsr/archs/rrdbnet_arch.py) for gfx950.
//
// One shape family: stride 1, pad 1, at most 192 input channels, 32 or 64 output channels, LeakyReLU(0.2), ReLU (ScuNET's conv_block) or a
// scaled residual after it.
// A dense block's cat(x, x1, ..., xk) is never built: the block lives in ONE 192-channel NHWC buffer, a conv reads the first `cin`
// channels of its rows (row stride lda) and writes its NOUT channels at a channel offset into rows of stride ldo.
//
// Implicit GEMM on v_mfma_f32_16x16x32_f16, fp32 accumulation.  A workgroup (4 waves) owns 256 consecutive pixels of M = B*H*W, a wave 64 of
// them (4 MFMA column blocks) times all NOUT channels.  The MFMA operands are swapped (weights as A, pixels as B), so a lane ends up with 4
// consecutive CHANNELS of one pixel: 8-byte epilogue accesses.
//   * pixels: each lane gathers its 16-byte operand fragments (8 channels of one pixel at one tap) straight from global memory, one
//     K step (one tap of one 32-channel block) ahead of the MFMAs that use them.  Neighbour validity is per pixel (a tile may straddle two
//     images); out-of-image taps read the zero page.  With `up` the tap (y, x) of the OUTPUT grid reads input pixel (y >> 1, x >> 1):
//     nearest x2 fused into the gather.
//   * weights [NOUT][9][cin]: staged by LDS-DMA in groups of G taps of one channel block, double-buffered, shared by the 4 waves.  The LDS
//     image is XOR-swizzled (16-byte segment s of row n holds k-segment s ^ ((n >> 2) & 3)) so the 16 rows a quarter-wave reads with
//     ds_read_b128 fall into distinct banks; LDS-DMA writes lanes consecutively, so the swizzle is applied to the SOURCE address.
// K walk: channel block outer, the 9 taps inner (the nine shifted reads of a channel block follow each other and hit L2).
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace sdmi {

// The host-emulated test build compiles this file as plain C++ (as part of engine.cpp, see its end): no address spaces there, and its
// LDS-direct load completes at issue, so there is nothing to wait for.
#ifdef __HIP__
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
#define RRDB_WAIT_LDS_LOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
typedef const void* gptr_t;
typedef void* lptr_t;
#define RRDB_WAIT_LDS_LOADS() ((void)0)
#endif

template <int NOUT, int G>
__global__ __launch_bounds__(256) void rrdb_conv_kernel(const RrdbP p) {
    static_assert(NOUT == 32 || NOUT == 64, "RRDBNet growth / feature widths");
    static_assert(9 % G == 0 && G % 2 == 1, "a stage is G taps of one channel block");
    constexpr int NJ = NOUT / 16;                       // 16-channel row blocks of the (swapped) MFMA
    constexpr int STAGE = G * NOUT * 64;                // bytes: G taps x NOUT rows x 32 channels
    constexpr int NI = STAGE / 1024;                    // wave-wide LDS-DMA instructions (64 lanes x 16 bytes) per stage
    constexpr int NIW = (NI + 3) / 4;                   // ... per wave: every wave issues exactly this many (a fixed count lets the
                                                        // compiler wait for the pixel gathers by count instead of draining the queue);
    constexpr int SLOT = NIW * 4 * 1024;                // instructions past NI land in the padding of the stage's slot
    constexpr int SPC = 9 / G;                          // stages per channel block
    __shared__ __attribute__((aligned(16))) char wl[2 * SLOT];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, q = lane >> 4;
    const int H = p.H, W = p.W;
    const int Hi = p.up ? H >> 1 : H, Wi = p.up ? W >> 1 : W;
    const unsigned HW = (unsigned)H * (unsigned)W;
    const long long m0 = (long long)blockIdx.x * 256 + wave * 64;

    int pb[4], py[4], px[4];                            // per pixel: first input row of its image, (y, x) on the output grid
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const long long m = m0 + mi * 16 + l16;
        if (m < p.M) {
            const unsigned um = (unsigned)m, b = um / HW, rem = um - b * HW, y = rem / (unsigned)W;
            pb[mi] = (int)(b * (unsigned)(Hi * Wi)); py[mi] = (int)y; px[mi] = (int)(rem - y * (unsigned)W);
        } else {
            pb[mi] = 0; py[mi] = -4; px[mi] = 0;        // rows past M: every tap is "outside", they compute zeros and store nothing
        }
    }

    auto load_a = [&](int kidx, h8* a) {
        const int c = kidx / 9, t = kidx - 9 * c;
        const int dy = t / 3 - 1, dx = t - 3 * (t / 3) - 1;
        const half_t* base = p.in + c * 32 + q * 8;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int yy = py[mi] + dy, xx = px[mi] + dx;
            const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            const int sy = p.up ? yy >> 1 : yy, sx = p.up ? xx >> 1 : xx;
            const long long row = (long long)(pb[mi] + sy * Wi + sx);
            const half_t* src = ok ? base + row * p.lda : p.zero;
            a[mi] = *reinterpret_cast<const h8*>(src);
        }
    };
    auto stage = [&](int sidx) {
        const int c = sidx / SPC, t0 = (sidx - c * SPC) * G;
        char* buf = wl + (sidx & 1) * SLOT;
#pragma unroll
        for (int u = 0; u < NIW; ++u) {
            const int i = wave + 4 * u;
            const int pseg = i * 64 + lane;
            const int s = pseg & 3, n = (pseg >> 2) % NOUT, tl = min(pseg / (4 * NOUT), G - 1);
            const int ks = s ^ ((n >> 2) & 3);
            const half_t* src = p.w + (long long)n * p.ldw + (t0 + tl) * p.cin + c * 32 + ks * 8;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(buf + i * 1024), 16, 0, 0);
        }
    };

    f4 acc[4][NJ];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[mi][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int nk = (p.cin / 32) * 9, nstages = nk / G;
    const int wseg = (q ^ (l16 >> 2)) * 16;             // this lane's swizzled segment inside a weight row (rows j * 16 + l16)
    // one K step: the MFMAs of step kidx on `cur` while the gather of step kidx + 1 lands in `nxt` (the two register sets alternate,
    // so no copy ties the loads to this step; the last step gathers its own operands again rather than branch around the loads)
    auto step = [&](int kidx, const char* wb, const h8* cur, h8* nxt) {
        load_a(min(kidx + 1, nk - 1), nxt);
        h8 wf[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) wf[j] = *reinterpret_cast<const h8*>(wb + j * 1024);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[mi][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], cur[mi], acc[mi][j], 0, 0, 0);
    };
    h8 a0[4], a1[4];
    // one stage: G steps on the weights of stage sidx, the LDS-DMA of stage sidx + 1 in flight.  `odd`: which register set holds step 0
    auto run_stage = [&](int sidx, bool odd) {
        RRDB_WAIT_LDS_LOADS();                                    // my share of stage sidx has landed ...
        __syncthreads();                                            // ... everybody's has, and everybody is done reading the other buffer
        if (sidx + 1 < nstages) stage(sidx + 1);
        const char* wb = wl + (sidx & 1) * SLOT + l16 * 64 + wseg;
#pragma unroll
        for (int tl = 0; tl < G; ++tl) {
            if (((tl & 1) != 0) == odd) step(sidx * G + tl, wb + tl * (NOUT * 64), a0, a1);
            else step(sidx * G + tl, wb + tl * (NOUT * 64), a1, a0);
        }
    };
    stage(0);
    load_a(0, a0);
    int sidx = 0;
    for (; sidx + 1 < nstages; sidx += 2) {                 // G is odd: two stages bring the register sets back to where they were
        run_stage(sidx, false);
        run_stage(sidx + 1, true);
    }
    if (sidx < nstages) run_stage(sidx, false);

    // epilogue: lane owns channels j * 16 + 4 q .. + 3 of pixel m0 + mi * 16 + l16
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const long long m = m0 + mi * 16 + l16;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n0 = j * 16 + 4 * q;
            if (n0 >= p.n_real) continue;
            const f4 bv = *reinterpret_cast<const f4*>(p.bias + n0);
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = acc[mi][j][r] + bv[r];
            if (p.ep == RRDB_EP_LRELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = v[r] > 0.f ? v[r] : 0.2f * v[r];
            } else if (p.ep == RRDB_EP_RELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
            } else if (p.ep >= RRDB_EP_RES1) {
                const h4 r1 = *reinterpret_cast<const h4*>(p.r1 + m * p.ldr1 + n0);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = p.alpha * v[r] + (float)r1[r];
                if (p.ep == RRDB_EP_RES2) {
                    const h4 r2 = *reinterpret_cast<const h4*>(p.r2 + m * p.ldr2 + n0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = p.beta * v[r] + (float)r2[r];
                }
            }
            if (p.store == RRDB_ST_F16) {
                half_t* o = reinterpret_cast<half_t*>(p.out) + m * p.ldo + n0;
                if (n0 + 4 <= p.n_real) {
                    *reinterpret_cast<h4*>(o) = h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) if (n0 + r < p.n_real) o[r] = (half_t)v[r];
                }
            } else if (p.store == RRDB_ST_F32_NCHW) {
                const unsigned um = (unsigned)m, b = um / HW, rem = um - b * HW;
                float* o = reinterpret_cast<float*>(p.out) + ((long long)b * p.n_real + n0) * HW + rem;
#pragma unroll
                for (int r = 0; r < 4; ++r) if (n0 + r < p.n_real) o[(long long)r * HW] = v[r];
            } else {                                    // uint8 HWC: clamp(0, 1) * 255, round half to even (np.round)
                uint8_t* o = reinterpret_cast<uint8_t*>(p.out) + m * p.n_real + n0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + r < p.n_real) o[r] = (uint8_t)rintf(fminf(fmaxf(v[r], 0.f), 1.f) * 255.f);
            }
        }
    }
}

// The network's input: an RGB image as uint8 HWC (scaled by 1/255, modules/upscaler_utils.py) or fp32 NCHW, pixel-unshuffled by f
// (channel c * f * f + dy * f + dx of pixel (y, x) = channel c of pixel (y f + dy, x f + dx): torch pixel_unshuffle, what the x2 / x1
// models start with) -> NHWC fp16 rows of cpad channels, zero padded.
__global__ __launch_bounds__(256) void rrdb_input_kernel(const void* in, int u8, half_t* out, int C, int H, int W, int f, int cpad, long long n) {
    const int h = H / f, w = W / f, cf = C * f * f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % cpad);
        const long long pix = i / cpad;
        const int x = (int)(pix % w), y = (int)((pix / w) % h);
        const long long b = pix / ((long long)w * h);
        float v = 0.f;
        if (ch < cf) {
            const int c = ch / (f * f), dy = (ch / f) % f, dx = ch % f;
            const long long Y = (long long)y * f + dy, X = (long long)x * f + dx;
            v = u8 ? (float)reinterpret_cast<const uint8_t*>(in)[((b * H + Y) * W + X) * C + c] / 255.f
                   : reinterpret_cast<const float*>(in)[((b * C + c) * H + Y) * W + X];
        }
        out[i] = (half_t)v;
    }
}
int launch_rrdb_input(const void* in, int u8, half_t* out, int B, int C, int H, int W, int f, int cpad, hipStream_t s) {
    SDMI_REQUIRE(f >= 1 && H % f == 0 && W % f == 0 && C * f * f <= cpad, "pixel-unshuffle: H and W must be multiples of the factor");
    const long long n = (long long)B * (H / f) * (W / f) * cpad;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    ProfScope ps("rrdb_input", 0.0, 2.0 * n, s);
    hipLaunchKernelGGL(rrdb_input_kernel, dim3(grid), dim3(256), 0, s, in, u8, out, C, H, W, f, cpad, n);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_rrdb_conv(const RrdbP& pin, int nout, hipStream_t s) {
    RrdbP p = pin;
    SDMI_REQUIRE(nout == 32 || nout == 64, "rrdb_conv is built for 32 and 64 output channels");
    SDMI_REQUIRE(p.cin >= 32 && p.cin <= 192 && p.cin % 32 == 0, "input channels: a multiple of 32 up to 192");
    SDMI_REQUIRE(p.in && p.out, "null input / output");
    SDMI_REQUIRE(p.lda >= p.cin && p.lda % 8 == 0 && ((uintptr_t)p.in & 15) == 0, "input rows: stride >= cin, 16-byte aligned");
    SDMI_REQUIRE(p.w && ((uintptr_t)p.w & 15) == 0, "packed weights [NOUT][9][cin], 16-byte aligned");
    SDMI_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0, "empty image");
    SDMI_REQUIRE(!p.up || (p.H % 2 == 0 && p.W % 2 == 0), "the x2 gather writes an even output grid");
    SDMI_REQUIRE((long long)p.B * p.H * p.W < (1ll << 31) - 256, "B*H*W must stay below 2^31 pixels");
    SDMI_REQUIRE(p.n_real >= 1 && p.n_real <= nout, "n_real in [1, NOUT]");
    SDMI_REQUIRE(p.ep >= RRDB_EP_NONE && p.ep <= RRDB_EP_RELU, "unknown epilogue");
    SDMI_REQUIRE(p.store >= RRDB_ST_F16 && p.store <= RRDB_ST_U8_HWC, "unknown store form");
    if (p.store == RRDB_ST_F16)
        SDMI_REQUIRE(p.ldo >= p.n_real && p.ldo % 4 == 0 && ((uintptr_t)p.out & 7) == 0, "fp16 output rows: 8-byte aligned channel slots");
    if (p.ep == RRDB_EP_RES1 || p.ep == RRDB_EP_RES2)
        SDMI_REQUIRE(p.r1 && p.ldr1 >= nout && p.ldr1 % 4 == 0 && ((uintptr_t)p.r1 & 7) == 0 && p.n_real == nout,
                     "residual r1: 8-byte aligned rows of at least NOUT channels, all NOUT channels stored");
    if (p.ep == RRDB_EP_RES2)
        SDMI_REQUIRE(p.r2 && p.ldr2 >= nout && p.ldr2 % 4 == 0 && ((uintptr_t)p.r2 & 7) == 0, "residual r2: 8-byte aligned rows of at least NOUT channels");
    if (p.store != RRDB_ST_F16) SDMI_REQUIRE(p.ldo == 0, "ldo belongs to the fp16 store: the fp32 NCHW / uint8 HWC outputs are dense");
    p.M = (long long)p.B * p.H * p.W;
    p.zero = zero_page();
    if (!p.bias) p.bias = reinterpret_cast<const float*>(zero_page());
    if (p.ldw == 0) p.ldw = 9 * p.cin;
    const unsigned grid = (unsigned)((p.M + 255) / 256);
    const double flops = 2.0 * (double)p.M * nout * 9.0 * p.cin;
    const double bytes = (double)p.M * (p.up ? 0.25 : 1.0) * p.cin * 2.0 + (double)p.M * p.n_real * (p.store == RRDB_ST_F16 ? 2.0 : p.store == RRDB_ST_F32_NCHW ? 4.0 : 1.0);
    if (nout == 32) {
        ProfScope ps(p.up ? "rrdb_conv32_up" : "rrdb_conv32", flops, bytes, s);
        hipLaunchKernelGGL((rrdb_conv_kernel<32, 9>), dim3(grid), dim3(256), 0, s, p);
    } else {
        ProfScope ps(p.up ? "rrdb_conv64_up" : "rrdb_conv64", flops, bytes, s);
        hipLaunchKernelGGL((rrdb_conv_kernel<64, 3>), dim3(grid), dim3(256), 0, s, p);
    }
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
