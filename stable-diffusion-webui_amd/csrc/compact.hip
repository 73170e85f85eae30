// compact.hip — the 3x3 convolution of the compact Real-ESRGAN upscalers (SRVGGNetCompact, Real-ESRGAN realesrgan/archs/srvgg_arch.py:
// General 4xV3, General WDN 4xV3, AnimeVideo) for gfx950.
//
// One shape family: stride 1, pad 1, fp16 NHWC, cin 32 (the first layer: 3 real channels zero-padded, as launch_rrdb_input writes them) or
// 64 -> 64 output channels of which n_real are stored; fp32 accumulation on v_mfma_f32_16x16x32_f16.  A compact network is this one shape
// 16 - 32 times over, so the kernel keeps in LDS what rrdb_conv (rrdb.hip) re-fetches: the whole layer's weights and a pixel tile with
// its halo.
//   * Persistent workgroups (4 waves): grid = min(tiles, CUs, grid_cap); a workgroup walks 16 x 16-pixel output tiles of the B images,
//     tile index t = blockIdx.x, + gridDim.x, ...   One workgroup per CU (LDS).
//   * Weights [64][9][cin] -> LDS ONCE per workgroup by LDS-DMA (72 KiB at cin 64), as 9 cin / 32 K-step images of [64 rows][64 bytes].
//   * Per tile the 18 x 18 x cin halo -> LDS by LDS-DMA (16-byte pieces, out-of-image pixels from the zero page), double-buffered: the
//     pieces of tile t + 1 are issued right after the barrier that opens tile t and land while tile t computes.
//     LDS: 73 728 + 2 x 41 984 = 157 696 bytes (a halo slot is 41 whole 1 KiB wave pieces; 324 pixels fill 40.5 of them).
//   * A tile's K loop is (cin / 32) x 9 steps of 8 ds_read_b128 (4 weight, 4 pixel fragments) and 16 MFMAs per wave, with no global load and
//     no barrier in it: one s_waitcnt vmcnt(0) + one barrier per TILE.  A wave owns 4 rows of the tile (one MFMA column block each) x all
//     64 channels; operands are swapped as in rrdb_conv (weights A, pixels B), so a lane ends with 4 consecutive channels of one pixel.
//
// Bank argument (ds_read_b128: bank = (addr / 4) % 64, i.e. sixteen 16-byte slots; the instruction is served in four groups of 16 lanes
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, {32-35, 44-47, 52-59}, {36-43, 48-51, 60-63} — the LDS table of the micro-architecture
// guide).  With lane = 16 q + l16, group a (0..3) holds every l16 once, with q = a for l16 in {0-3, 12-15} and q = a ^ 1 for l16 in
// {4-11}: q = a ^ e(l16), e = bit 2 ^ bit 3 of l16.  LDS-DMA writes a wave's 64 pieces consecutively, so both swizzles are applied to the
// SOURCE address of the piece.
//   Weights: row n (= 16 j + l16) of a K step is 64 bytes = 4 slots, so the slot of a lane is 4 (l16 & 3) + segment (mod 16): the four
//     lanes of a group that share l16 & 3 (h = l16 >> 2 = 0..3) need four different segments.  Segment s of row n holds k-segment
//     s ^ (3 * ((n >> 3) & 1)); the lane reads segment q ^ 3 (h >> 1) = a ^ e(h) ^ 3 (h >> 1) = a ^ {0, 1, 2, 3}[h]: distinct.
//   Pixels: the 16 pixels of an MFMA column block are one tile row, but lane l16 does NOT take pixel l16: the lanes with e = 0
//     (l16 0-3, 12-15) take the even columns 0, 2, .. 14 and the lanes with e = 1 (l16 4-11) the odd ones (xl below).  cin 64: a pixel
//     is 128 bytes = 8 slots, halo pixel p (18 per row, even) sits at slots 8 (p & 1) + segment, and segment s holds channel segment
//     s ^ ((p >> 1) & 7).  In a group the e = 0 lanes read channel segment 4 c + a of 8 pixels of ONE parity whose p >> 1 are consecutive
//     (a tap shifts all of them alike) -> 8 different segments of one 128-byte half; the e = 1 lanes read 4 c + (a ^ 1) of 8 pixels of the
//     other parity -> the other half.  16 distinct slots.  cin 32: a pixel is 4 slots at 4 (p & 3) + segment, swizzle (p >> 2) & 3: each
//     parity class splits into two classes of p & 3 with 4 pixels whose p >> 2 are consecutive -> 4 distinct segments each.
//   (Unswizzled, a lane group would see 2 (cin 64) or 4 (cin 32) distinct segments per pixel class: 4-way conflicts.)
// Price per K step and wave: 8 ds_read_b128 = 32 LDS-array cycles against 16 MFMAs (>= 64 cycles of the matrix pipe); four waves
// per CU ask 128 of the 256 bytes / clock the array delivers.
//
// Epilogues: acc + bias, then NONE | PRELU (v > 0 ? v : slope[c] v) -> fp16 NHWC rows of stride ldo; or TAIL, the network's last launch:
// pixel shuffle by r (channel c r^2 + dy r + dx of pixel (y, x) -> channel c of pixel (y r + dy, x r + dx)) + the nearest-upsampled
// ORIGINAL input (uint8 HWC / 255 or fp32 NCHW, added in fp32) -> fp32 NCHW, or uint8 HWC with clamp, x255, round-half-even.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace sdmi {

// The host-emulated test build compiles this file as plain C++ (as part of engine.cpp, see its end): no address spaces and no dynamic
// LDS there, and its LDS-direct load completes at issue, so there is nothing to wait for.
#ifdef __HIP__
typedef const __attribute__((address_space(1))) void* cgptr_t;
typedef __attribute__((address_space(3))) void* clptr_t;
#define COMPACT_WAIT_LDS_LOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// a value the compiler may not reason about: comparisons against it are made where they are used, per tile, instead of being hoisted
// out of the persistent loop as dozens of live lane masks (SGPR pairs)
#define COMPACT_OPAQUE(x) asm volatile("" : "+v"(x))
#else
typedef const void* cgptr_t;
typedef void* clptr_t;
#define COMPACT_WAIT_LDS_LOADS() ((void)0)
#define COMPACT_OPAQUE(x) ((void)0)
#endif

constexpr int kCompactHaloSlot = 41 * 1024;                          // 18 x 18 pixels x 128 bytes = 40.5 wave pieces of 1 KiB
constexpr int kCompactLds = 64 * 9 * 64 * 2 + 2 * kCompactHaloSlot;  // 157 696

template <int CIN>
__global__ __launch_bounds__(256) void compact_conv_kernel(const CompactP p) {
    static_assert(CIN == 32 || CIN == 64, "first layer (3 channels padded to 32) and the 64-wide body");
    constexpr int SEGS = CIN / 8;                       // 16-byte channel segments of a pixel
    constexpr int PSH = SEGS == 8 ? 1 : 2;              // pixel p's segments are XORed with (p >> PSH) & (SEGS - 1)
    constexpr int NK = (CIN / 32) * 9;                  // K steps: channel block outer, tap inner
    constexpr int HINSTR = (324 * SEGS + 63) / 64;      // wave-wide LDS-DMA instructions (64 x 16 bytes) per halo
    static_assert(HINSTR * 1024 <= kCompactHaloSlot && NK * 4096 + 2 * kCompactHaloSlot <= kCompactLds, "LDS layout");
#ifdef __HIP__
    extern __shared__ __attribute__((aligned(16))) char smem[];
#else
    __shared__ __attribute__((aligned(16))) char smem[kCompactLds];
#endif
    char* const wl = smem;
    char* const hl = smem + 64 * 9 * 64 * 2;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, q = lane >> 4;
    const int H = p.H, W = p.W;

    // ---- the layer's weights, once: wave piece 4 u + wave is this wave's quarter of K step u, so a lane's row n and segment are the
    // same in every step and the source moves by a constant ----
    {
        const int n = tid >> 2, ks = (tid & 3) ^ (3 * ((n >> 3) & 1));
        const half_t* src = p.w + n * (9 * CIN) + ks * 8;
        char* dst = wl + wave * 1024;
#pragma unroll
        for (int k = 0; k < NK; ++k)
            __builtin_amdgcn_global_load_lds((cgptr_t)(src + (k % 9) * CIN + (k / 9) * 32), (clptr_t)(dst + k * 4096), 16, 0, 0);
    }

    // a halo: wave piece 4 u + wave again, so a lane's channel segment is fixed (256 pieces are 256 / SEGS pixels, a multiple of 8 or
    // 16: the swizzle term does not move) and its pixel advances by 256 / SEGS per u
    const int hseg = ((tid % SEGS) ^ ((tid >> 4) & (SEGS - 1))) * 8;
    auto stage_halo = [&](int t, char* buf) {
        const unsigned ut = (unsigned)t, txn = (unsigned)p.tiles_x, tyn = (unsigned)p.tiles_y;
        const unsigned rest = ut / txn, b = rest / tyn;
        const int y0 = (int)(rest - b * tyn) * 16 - 1, x0 = (int)(ut - rest * txn) * 16 - 1;
        const half_t* img = p.in + (long long)b * H * W * p.lda + hseg;
        char* dst = buf + wave * 1024;
        auto piece = [&](int u) {
            const int pix = u * (256 / SEGS) + tid / SEGS;          // pixels past 323 (second half of the last piece) land in the slot's padding
            const int ry = pix / 18, rx = pix - ry * 18;
            const int y = y0 + ry, x = x0 + rx;
            const bool ok = pix < 324 && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const half_t* src = ok ? img + ((long long)y * W + x) * p.lda : p.zero;
            __builtin_amdgcn_global_load_lds((cgptr_t)src, (clptr_t)(dst + u * 4096), 16, 0, 0);
        };
#pragma unroll
        for (int u = 0; u < HINSTR / 4; ++u) piece(u);
        if (wave < HINSTR % 4) piece(HINSTR / 4);                   // wave-uniform
    };

    // lane l16's pixel column inside a tile row (the bank argument above), its swizzled weight segment, its first halo pixel
    const int xl = l16 < 4 ? 2 * l16 : l16 < 12 ? 2 * (l16 - 4) + 1 : 2 * (l16 - 8);
    const int woff = l16 * 64 + ((q ^ (3 * (l16 >> 3))) << 4);
    const int pix0 = wave * 4 * 18 + xl;

    const float inv_r = 1.f / (float)p.r, inv_rr = inv_r * inv_r;   // TAIL: channel -> (c, dy, dx) without integer divisions (exact: ch < 64)
    int t = (int)blockIdx.x;                            // tiles < 2^31 - 256 and gridDim.x <= 256 (the launcher): t + gridDim.x fits
    if (t < p.tiles) stage_halo(t, hl);
    for (int it = 0; t < p.tiles; t += (int)gridDim.x, ++it) {
        COMPACT_WAIT_LDS_LOADS();                                   // my pieces of this tile's halo (and of the weights) have landed ...
        __syncthreads();                                            // ... everybody's have, and everybody is done reading the other slot
        if (t + (int)gridDim.x < p.tiles) stage_halo(t + (int)gridDim.x, hl + ((it + 1) & 1) * kCompactHaloSlot);
        const char* hb = hl + (it & 1) * kCompactHaloSlot;

        f4 acc[4][4];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[mi][j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int c = k / 9, tap = k - 9 * c;
            const int ty = tap / 3, tx = tap - 3 * ty;
            h8 wf[4], af[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const h8*>(wl + k * 4096 + j * 1024 + woff);
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                const int pix = pix0 + (mi + ty) * 18 + tx;
                af[mi] = *reinterpret_cast<const h8*>(hb + pix * (SEGS * 16) + (((c * 4 + q) ^ ((pix >> PSH) & (SEGS - 1))) << 4));
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[mi][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], af[mi], acc[mi][j], 0, 0, 0);
        }

        // epilogue: lane owns channels 16 j + 4 q .. + 3 of pixels (y0 + mi, x), mi = 0 .. 3
        const unsigned ut = (unsigned)t, txn = (unsigned)p.tiles_x, tyn = (unsigned)p.tiles_y;
        const unsigned rest = ut / txn, b = rest / tyn;
        const int x = (int)(ut - rest * txn) * 16 + xl, y0 = (int)(rest - b * tyn) * 16 + wave * 4;
        const long long m0 = ((long long)b * H + y0) * W + x;         // pixel (y0 + mi, x) is row m0 + mi W
        int n_real = p.n_real;
        COMPACT_OPAQUE(n_real);
        if (p.ep != COMPACT_EP_TAIL) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n0 = j * 16 + 4 * q;
                const f4 bv = *reinterpret_cast<const f4*>(p.bias + n0);
                f4 sl = f4{1.f, 1.f, 1.f, 1.f};
                if (p.ep == COMPACT_EP_PRELU) sl = *reinterpret_cast<const f4*>(p.slope + n0);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) {
                    if (x < W && y0 + mi < H && n0 < n_real) {
                        float v[4];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            v[r] = acc[mi][j][r] + bv[r];
                            v[r] = v[r] > 0.f ? v[r] : sl[r] * v[r];
                        }
                        half_t* o = reinterpret_cast<half_t*>(p.out) + (m0 + (long long)mi * W) * p.ldo + n0;
                        if (n0 + 4 <= n_real) {
                            *reinterpret_cast<h4*>(o) = h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r) if (n0 + r < n_real) o[r] = (half_t)v[r];
                        }
                    }
                }
            }
        } else {                                        // pixel shuffle + the nearest-upsampled input, fp32
            const int rs = p.r, rr = rs * rs;
            const long long Ho = (long long)H * rs, Wo = (long long)W * rs;
#pragma unroll
            for (int j = 0; j < 3; ++j) {               // 3 r^2 <= 48 channels
                const f4 bv = *reinterpret_cast<const f4*>(p.bias + j * 16 + 4 * q);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ch = j * 16 + 4 * q + r;
                    const int c = (int)(((float)ch + 0.5f) * inv_rr), rem = ch - c * rr;
                    const int dy = (int)(((float)rem + 0.5f) * inv_r), dx = rem - dy * rs;
#pragma unroll
                    for (int mi = 0; mi < 4; ++mi) {
                        const int y = y0 + mi;
                        if (x < W && y < H && ch < n_real) {
                            const float base = p.base_u8 ? (float)reinterpret_cast<const uint8_t*>(p.base)[(m0 + (long long)mi * W) * 3 + c] / 255.f
                                                         : reinterpret_cast<const float*>(p.base)[(((long long)b * 3 + c) * H + y) * W + x];
                            const float o = acc[mi][j][r] + bv[r] + base;
                            const long long oy = (long long)y * rs + dy, ox = (long long)x * rs + dx;
                            if (p.out_u8)               // clamp(0, 1) * 255, round half to even (np.round)
                                reinterpret_cast<uint8_t*>(p.out)[(((long long)b * Ho + oy) * Wo + ox) * 3 + c] = (uint8_t)rintf(fminf(fmaxf(o, 0.f), 1.f) * 255.f);
                            else
                                reinterpret_cast<float*>(p.out)[(((long long)b * 3 + c) * Ho + oy) * Wo + ox] = o;
                        }
                    }
                }
            }
        }
    }
}

static int compact_cus() {
    static int cus[64] = {};
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) d = 0;
    d &= 63;
    if (cus[d] == 0) {
        hipDeviceProp_t prop;
        cus[d] = hipGetDeviceProperties(&prop, d) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return cus[d];
}

int launch_compact_conv(const CompactP& pin, hipStream_t s) {
    CompactP p = pin;
    SDMI_REQUIRE(p.cin == 32 || p.cin == 64, "compact_conv is built for 32 or 64 input channels (and 64 output channels)");
    SDMI_REQUIRE(p.in && p.out, "null input / output");
    SDMI_REQUIRE(p.lda >= p.cin && p.lda % 8 == 0 && ((uintptr_t)p.in & 15) == 0, "input rows: stride >= cin, 16-byte aligned");
    SDMI_REQUIRE(p.w && ((uintptr_t)p.w & 15) == 0, "packed weights [64][9][cin], 16-byte aligned");
    SDMI_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0, "empty image");
    SDMI_REQUIRE((long long)p.B * p.H * p.W < (1ll << 31) - 256, "B*H*W must stay below 2^31 pixels");
    SDMI_REQUIRE(p.ep >= COMPACT_EP_NONE && p.ep <= COMPACT_EP_TAIL, "unknown epilogue");
    if (p.ep == COMPACT_EP_TAIL)
        SDMI_REQUIRE(p.r >= 1 && p.r <= 4 && p.n_real == 3 * p.r * p.r, "tail: scale r in 1..4 and n_real = 3 r^2 channels to shuffle");
    SDMI_REQUIRE(p.n_real >= 1 && p.n_real <= 64, "n_real in [1, 64]");
    SDMI_REQUIRE(p.grid_cap >= 0, "grid_cap: 0 (default) or a positive number of workgroups");
    const long long M = (long long)p.B * p.H * p.W;
    if (p.ep == COMPACT_EP_PRELU) SDMI_REQUIRE(p.slope && ((uintptr_t)p.slope & 15) == 0, "PReLU needs its 64 fp32 slopes, 16-byte aligned");
    if (p.ep == COMPACT_EP_TAIL) {
        SDMI_REQUIRE(p.base, "tail: the network's input image (uint8 HWC or fp32 NCHW) is added to the shuffled output");
        SDMI_REQUIRE(p.ldo == 0, "ldo belongs to the fp16 store: the tail's fp32 NCHW / uint8 HWC outputs are dense");
    } else {
        SDMI_REQUIRE(p.ldo >= p.n_real && p.ldo % 4 == 0 && ((uintptr_t)p.out & 7) == 0, "fp16 output rows: stride >= n_real, 8-byte aligned");
        const char* i0 = (const char*)p.in; const char* o0 = (const char*)p.out;
        // (the bytes the rows really span: the last row ends after its channels, not after a whole stride — with M * ld a buffer that
        // starts within one row stride behind the other tensor's last row was refused as if it overlapped)
        SDMI_REQUIRE(o0 + ((M - 1) * p.ldo + p.n_real) * 2 <= i0 || i0 + ((M - 1) * p.lda + p.cin) * 2 <= o0,
                     "in-place use: a tile's halo is read after its neighbours were written");
    }
    SDMI_REQUIRE(!p.bias || ((uintptr_t)p.bias & 15) == 0, "bias: 64 fp32 values, 16-byte aligned");
    p.tiles_x = (p.W + 15) / 16; p.tiles_y = (p.H + 15) / 16;
    p.tiles = p.B * p.tiles_x * p.tiles_y;                     // <= B*H*W < 2^31 - 256
    p.zero = zero_page();
    if (!p.bias) p.bias = reinterpret_cast<const float*>(zero_page());
    int grid = std::min(p.tiles, std::min(compact_cus(), 256));     // <= 256: the kernel's 32-bit tile counter (t + grid) cannot wrap
    if (p.grid_cap > 0) grid = std::min(grid, p.grid_cap);
    const double flops = 2.0 * (double)M * 64 * 9.0 * p.cin;
    const double bytes = (double)M * p.cin * 2.0 + (p.ep == COMPACT_EP_TAIL ? (double)M * p.n_real * (p.out_u8 ? 1.0 : 4.0) : (double)M * p.n_real * 2.0);
    ProfScope ps(p.ep == COMPACT_EP_TAIL ? "compact_conv_tail" : "compact_conv", flops, bytes, s);
    if (p.cin == 32) {
        auto kern = compact_conv_kernel<32>;
        static PerDeviceOnce attr;
        if (attr.need()) SDMI_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kCompactLds));
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), kCompactLds, s, p);
    } else {
        auto kern = compact_conv_kernel<64>;
        static PerDeviceOnce attr;
        if (attr.need()) SDMI_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kCompactLds));
        hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(256), kCompactLds, s, p);
    }
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
