// hat.hip — the kernels of the HAT upscalers (Chen et al., "Activating More Pixels in Image Super-Resolution Transformer", CVPR 2023)
// that the rest of the library has no form of, for gfx950: attention in 16 x 16 windows (256 queries against the window's own 256 keys,
// or against the 576 keys of the 24 x 24 window around it), the gate of the channel-attention conv branch and the sum that adds that
// branch to the stream.  The linears and convs of the network run on gemm.hip, LayerNorm and the input / output / shuffle passes on
// swinir.hip, the 64-channel conv_last on rrdb.hip (upscalers.cpp hat_pass).
//
// Token rows are fp16 with a head's D <= 32 channels in a 32-wide slot (dims D .. 31 zero): q, k, v and the attention's output are
// [tokens][32 heads] in that layout.
//
// hat_window_attn<OV>: one workgroup (256 threads, 4 waves) per (image, window, head) on a token grid whose sides are multiples of 16 (the
// network pads, the kernel does not).  The 256 queries are the tokens of the 16 x 16 window (wy, wx).
//   self form (OV = false): the keys are the same 256 tokens.  The cyclic shift (torch.roll by -shift, shift = 0 | 8), the partition and
//   their inverses are index arithmetic: token a of the window sits at (ys, xs) = (16 wy + a / 16, 16 wx + a % 16) of the shifted grid,
//   i.e. at ((ys + shift) % H, (xs + shift) % W) of the grid.  When shifted, -100 (not -inf) is added between tokens whose region ids on
//   the shifted grid differ (the slices [0, -16), [-16, -8), [-8, end) of each axis).  The bias is the head's column of the [961][heads]
//   table, read at (ya - yb + 15) * 31 + (xa - xb + 15).
//   overlap form (OV = true): the keys are the 24 x 24 tokens at rows 16 wy - 4 .. 16 wy + 19, columns 16 wx - 4 .. 16 wx + 19; a key
//   outside the grid is a zero row (k = v = 0) that still takes part in the softmax with score 0 + bias, as nn.Unfold's zero padding of the
//   k | v maps has it.  The bias is the head's column of the offset-ordered [39][39][heads] table, read at (yb - ya + 15) * 39 +
//   (xb - xa + 15).  No shift, no mask.
// Sizing: all keys of a window stay resident and a wave takes 16 queries against all of them in one go (S^T = K Q^T on
// v_mfma_f32_16x16x32_f16, a lane holds keys 16 nj + 4 (lane / 16) + r of query lane % 16; the probabilities of two key tiles are the B
// fragment of O^T = V^T P^T as they lie, dat_window_attn's register layout).  For the overlap form that is 144 score VGPRs per lane and
// 89 KB of LDS, so one workgroup (one wave per SIMD) per CU.  The alternative, walking the keys in chunks with a running max and sum,
// would not lift that: K and V^T of the window are what fills the LDS, not the scores, and a chunked walk still has to stage them once
// per (window, head); it would add a rescale of the accumulators per chunk and round unnormalised probabilities.  With the scores in
// registers the softmax is exact two-pass, the probabilities are normalised before they are rounded to fp16 (as in the other window
// kernels), and the 512 VGPRs a lone wave per SIMD may use are there to be used.  The self form is dat_window_attn<256>'s size.
// LDS (static): K [NK][40] fp16 (80-byte rows: the 16-byte fragment reads of 16 consecutive rows fall on distinct banks), V^T [32][NK + 4]
// fp16, the bias column (961 | 1521 fp32) and, in the self form, the region ids (256 bytes):
//   self:    20480 + 16640 + 3844 + 256 = 41220 bytes (41232 with alignment);
//   overlap: 46080 + 37120 + 6084 = 89284 bytes.
// Launch configuration: grid B * (H / 16) * (W / 16) * heads workgroups, block 256 threads, no dynamic LDS; 176 (self) / 380 (overlap, 144
// of them accumulation registers) VGPRs, no scratch.
// Scores, bias, mask and softmax are fp32; the normalised probabilities are rounded to fp16 for the second product.
//
// hat_channel_gate: gate[b][c] = sigmoid(W3 relu(W1 mean_n(y[b][n]) + b1) + b3) in two launches: the sums of every channel over blocks of
// HAT_POOL_TOKENS tokens (strided token groups added in order, then the groups in order), then one workgroup per image adds the blocks in
// order: no atomics, every sum has one fixed order, two runs give the same bits.
// hat_cab_add: out = t + conv_scale * gate[image][c] * conv, one pass over the rows (out may be t: a thread reads what it then writes).
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace sdmi {

namespace {
constexpr int HAT_KLD = 40;                                 // row stride (halfs) of the K image

__device__ __forceinline__ int hat_region(int u, int n) { return u < n - 16 ? 0 : (u < n - 8 ? 1 : 2); }
__device__ __forceinline__ float hat_sigmoid(float a) { return 1.0f / (1.0f + __expf(-a)); }
}  // namespace

template <bool OV>
__global__ __launch_bounds__(256) void hat_window_attn_kernel(const HatAttnP p) {
    constexpr int NK = OV ? 576 : 256;                      // keys of a window
    constexpr int VLD = NK + 4;                             // row stride (halfs) of the V^T image: 8-byte aligned rows
    constexpr int TAB = OV ? 39 * 39 : 31 * 31;
    __shared__ __attribute__((aligned(16))) half_t ks[NK * HAT_KLD];
    __shared__ __attribute__((aligned(16))) half_t vt[32 * VLD];
    __shared__ float tab[TAB];
    __shared__ __attribute__((aligned(4))) unsigned char reg[OV ? 4 : 256];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int h = (int)(blockIdx.x % (unsigned)p.heads);
    const int nwx = p.W >> 4, nwin = nwx * (p.H >> 4);
    const int win = (int)((blockIdx.x / (unsigned)p.heads) % (unsigned)nwin);
    const long long b = (long long)(blockIdx.x / ((unsigned)p.heads * (unsigned)nwin));
    const int wy = win / nwx, wx = win - wy * nwx;

    for (int a = tid; a < NK; a += 256) {
        int y, x;
        bool in = true;
        if constexpr (OV) {
            y = 16 * wy - 4 + a / 24;
            x = 16 * wx - 4 + a % 24;
            in = y >= 0 && y < p.H && x >= 0 && x < p.W;
        } else {
            const int ys = 16 * wy + (a >> 4), xs = 16 * wx + (a & 15);
            y = ys + p.shift;
            x = xs + p.shift;
            if (y >= p.H) y -= p.H;
            if (x >= p.W) x -= p.W;
            reg[a] = (unsigned char)(3 * hat_region(ys, p.H) + hat_region(xs, p.W));
        }
        const long long row = in ? (b * p.H + y) * p.W + x : 0;
        const half_t* src = p.qkv + row * p.ldq + (p.heads + h) * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            h8 kv = h8{0, 0, 0, 0, 0, 0, 0, 0}, vv = h8{0, 0, 0, 0, 0, 0, 0, 0};
            if (in) {
                kv = *reinterpret_cast<const h8*>(src + 8 * c);
                vv = *reinterpret_cast<const h8*>(src + p.heads * 32 + 8 * c);
            }
            *reinterpret_cast<h8*>(ks + a * HAT_KLD + 8 * c) = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(8 * c + e) * VLD + a] = vv[e];
        }
    }
    for (int i = tid; i < TAB; i += 256) tab[i] = p.bias[(long long)i * p.heads + h];
    __syncthreads();

    for (int qt = wave; qt < 16; qt += 4) {                 // wave-uniform: query row qt of the window, query column l16
        const int aq = 16 * qt + l16;
        int yq = 16 * wy + qt, xq = 16 * wx + l16;
        if constexpr (!OV) {
            yq += p.shift;
            xq += p.shift;
            if (yq >= p.H) yq -= p.H;
            if (xq >= p.W) xq -= p.W;
        }
        const long long rq = (b * p.H + yq) * p.W + xq;
        const h8 qf = *reinterpret_cast<const h8*>(p.qkv + rq * p.ldq + h * 32 + 8 * g);
        f4 s[NK / 16];                                      // [nj]: keys 16 nj + 4 g + r of query 16 qt + l16
#pragma unroll
        for (int nj = 0; nj < NK / 16; ++nj) {
            const h8 kf = *reinterpret_cast<const h8*>(ks + (16 * nj + l16) * HAT_KLD + 8 * g);
            s[nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            if ((nj & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // at most four K fragments in flight: the unrolled loop's loads are not all hoisted
        }
        const int regq = OV ? 0 : (int)reg[aq];
        const int qbase = OV ? (15 - qt) * 39 + 15 - l16 : (qt + 15) * 31 + l16 + 15;
        float mx = -3.0e38f;
#pragma unroll
        for (int nj = 0; nj < NK / 16; ++nj) {
            const int ak = 16 * nj + 4 * g;                 // keys ak .. ak + 3 lie in one row of the key window (16 and 24 are multiples of 4)
            int kb;
            unsigned rk = 0;
            if constexpr (OV) {
                const int yb = ak / 24;
                kb = qbase + yb * 39 + (ak - 24 * yb);
            } else {
                kb = qbase - (ak >> 4) * 31 - (ak & 15);
                rk = *reinterpret_cast<const unsigned*>(reg + ak);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float m = 0.0f;
                if constexpr (!OV) m = (p.shift && (int)((rk >> (8 * r)) & 255u) != regq) ? -100.0f : 0.0f;
                const float v = fmaf(s[nj][r], p.scale, tab[OV ? kb + r : kb - r]) + m;
                s[nj][r] = v;
                mx = fmaxf(mx, v);
            }
            if (nj & 1) __builtin_amdgcn_sched_barrier(0);              // eight bias reads in flight
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int nj = 0; nj < NK / 16; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(s[nj][r] - mx);
                s[nj][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        f4 o0 = f4{0.f, 0.f, 0.f, 0.f}, o1 = f4{0.f, 0.f, 0.f, 0.f};       // dims 4 g + r and 16 + 4 g + r of query 16 qt + l16
#pragma unroll
        for (int kk = 0; kk < NK / 32; ++kk) {              // k slot 8 g + e = key 16 (2 kk + e / 4) + 4 g + e % 4 on both operands
            h8 pf;                                          // the B fragment of O^T = V^T P^T: the normalised probabilities as they lie
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[e] = (half_t)(s[2 * kk + (e >> 2)][e & 3] * inv);
            const half_t* src = vt + l16 * VLD + 32 * kk + 4 * g;
            const h4 lo0 = *reinterpret_cast<const h4*>(src), hi0 = *reinterpret_cast<const h4*>(src + 16);
            const h4 lo1 = *reinterpret_cast<const h4*>(src + 16 * VLD), hi1 = *reinterpret_cast<const h4*>(src + 16 * VLD + 16);
            o0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(h8{lo0[0], lo0[1], lo0[2], lo0[3], hi0[0], hi0[1], hi0[2], hi0[3]}, pf, o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(h8{lo1[0], lo1[1], lo1[2], lo1[3], hi1[0], hi1[1], hi1[2], hi1[3]}, pf, o1, 0, 0, 0);
            if ((kk & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        h4 ov0, ov1;                                        // the slot's tail D .. 31 is stored as zero
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            ov0[r] = 4 * g + r < p.D ? (half_t)o0[r] : (half_t)0.f;
            ov1[r] = 16 + 4 * g + r < p.D ? (half_t)o1[r] : (half_t)0.f;
        }
        half_t* dst = p.out + rq * p.ldo + h * 32 + 4 * g;
        *reinterpret_cast<h4*>(dst) = ov0;
        *reinterpret_cast<h4*>(dst + 16) = ov1;
    }
}

int launch_hat_window_attention(const HatAttnP& p, hipStream_t s) {
    SDMI_REQUIRE(p.qkv && p.bias && p.out, "null qkv / bias / out");
    SDMI_REQUIRE(p.mode == 0 || p.mode == 1, "mode 0 (self: the window's own 256 keys) | 1 (overlap: the 576 keys of the 24 x 24 window)");
    SDMI_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0, "empty token grid");
    SDMI_REQUIRE(p.H % 16 == 0 && p.W % 16 == 0, "the token grid's sides must be multiples of 16 (the network pads)");
    SDMI_REQUIRE(p.heads >= 1 && p.heads <= 1024, "heads must be in 1..1024");
    SDMI_REQUIRE(p.D >= 1 && p.D <= 32, "head dim D must be in 1..32 (one 32-wide slot per head)");
    SDMI_REQUIRE(p.mode == 0 ? (p.shift == 0 || p.shift == 8) : p.shift == 0, "shift must be 0 or 8 in the self form, 0 in the overlap form");
    SDMI_REQUIRE(p.ldq >= 96 * p.heads, "qkv rows hold 3 x heads slots of 32: ldq >= 96 heads");
    SDMI_REQUIRE(p.ldo >= 32 * p.heads, "out rows hold heads slots of 32: ldo >= 32 heads");
    SDMI_REQUIRE(p.ldq % 8 == 0 && p.ldo % 8 == 0 && ((uintptr_t)p.qkv & 15) == 0 && ((uintptr_t)p.out & 15) == 0 && ((uintptr_t)p.bias & 3) == 0,
                 "misaligned: qkv / out bases on 16 bytes, the bias table on 4, ldq and ldo multiples of 8");
    SDMI_REQUIRE((const void*)p.qkv != (const void*)p.out, "out must not alias qkv (other workgroups read the rows as keys)");
    const long long tokens = (long long)p.B * p.H * p.W, windows = tokens / 256;
    SDMI_REQUIRE(tokens < (1ll << 31) - 256 && windows * p.heads < (1ll << 31), "B*H*W must stay below 2^31 tokens");
    const int NK = p.mode ? 576 : 256;
    ProfScope ps(p.mode ? "hat_window_attn_overlap" : "hat_window_attn_self", (double)tokens * p.heads * (2.0 * NK * 32 * 2),
                 (double)tokens * p.heads * 32 * 2.0 * (2 + 2.0 * NK / 256), s);
    const dim3 grid((unsigned)(windows * p.heads));
    if (p.mode) hipLaunchKernelGGL(hat_window_attn_kernel<true>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(hat_window_attn_kernel<false>, grid, dim3(256), 0, s, p);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the gate of the channel-attention conv branch ---------------------------------------------------------------------------------------
// ws[(b nblk + blk)][C]: the sums of y over the tokens [blk T, min(N, (blk + 1) T)), T = HAT_POOL_TOKENS.  Thread tid owns the 8 channels
// 8 (tid % (C / 8)) of token group tg = tid / (C / 8) < G = 256 / (C / 8): it adds the tokens tg, tg + G, ... of the block in order (16-byte
// loads), then a thread per channel adds the G groups' sums in group order through LDS (G C <= 2048 fp32 = 8192 bytes).  Launch: grid
// B * nblk, block 256.
__global__ __launch_bounds__(256) void hat_pool_partial_kernel(const half_t* y, float* ws, int N, int C, int ld, int nblk) {
    __shared__ float red[2048];
    const int blk = (int)(blockIdx.x % (unsigned)nblk);
    const long long b = blockIdx.x / (unsigned)nblk;
    const int t_begin = blk * HAT_POOL_TOKENS, t_end = min(N, t_begin + HAT_POOL_TOKENS);
    const int c8n = C >> 3, G = 256 / c8n;
    const int c8 = (int)threadIdx.x % c8n, tg = (int)threadIdx.x / c8n;
    if (tg < G) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = t_begin + tg; t < t_end; t += G) {
            const h8 v = *reinterpret_cast<const h8*>(y + (b * N + t) * ld + 8 * c8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[tg * C + 8 * c8 + e] = acc[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float sum = 0.f;
        for (int k = 0; k < G; ++k) sum += red[k * C + c];
        ws[(long long)blockIdx.x * C + c] = sum;
    }
}
// One workgroup per image: the partials added in block order -> the mean; hidden = relu(w1 mean + b1); gate = sigmoid(w3 hidden + b3).
// LDS: (1024 + 128) fp32 = 4608 bytes.  Launch: grid B, block 256.
__global__ __launch_bounds__(256) void hat_channel_gate_kernel(const float* ws, const float* w1, const float* b1, const float* w3, const float* b3,
                                                               float* gate, int N, int C, int Cs, int nblk) {
    __shared__ float mean[1024];
    __shared__ float hid[128];
    const long long b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float sum = 0.f;
        for (int k = 0; k < nblk; ++k) sum += ws[(b * nblk + k) * C + c];
        mean[c] = sum / (float)N;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < Cs; j += 256) {
        float a = b1[j];
        for (int c = 0; c < C; ++c) a = fmaf(w1[j * C + c], mean[c], a);
        hid[j] = fmaxf(a, 0.f);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = b3[c];
        for (int j = 0; j < Cs; ++j) a = fmaf(w3[c * Cs + j], hid[j], a);
        gate[b * C + c] = hat_sigmoid(a);
    }
}

int launch_hat_channel_gate(const half_t* y, const float* w1, const float* b1, const float* w3, const float* b3, float* ws, float* gate, int B,
                            int N, int C, int Cs, int ld, hipStream_t s) {
    SDMI_REQUIRE(y && w1 && b1 && w3 && b3 && ws && gate, "null argument");
    SDMI_REQUIRE(B > 0 && N > 0, "empty tensor");
    SDMI_REQUIRE(C >= 8 && C <= 1024 && C % 8 == 0 && Cs >= 1 && Cs <= 128, "channels a multiple of 8 in 8..1024, squeezed width in 1..128");
    SDMI_REQUIRE(ld >= C, "rows narrower than the channels");
    SDMI_REQUIRE(((uintptr_t)y & 15) == 0 && ld % 8 == 0 &&
                     (((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w3 | (uintptr_t)b3 | (uintptr_t)ws | (uintptr_t)gate) & 3) == 0,
                 "misaligned: y on 16 bytes, ld a multiple of 8, fp32 arguments on 4 bytes");
    SDMI_REQUIRE((long long)B * N < (1ll << 31) - 256, "B*N must stay below 2^31 tokens");
    const int nblk = (N + HAT_POOL_TOKENS - 1) / HAT_POOL_TOKENS;
    {
        ProfScope ps("hat_pool_partial", (double)B * N * C, 2.0 * B * N * C, s);
        hipLaunchKernelGGL(hat_pool_partial_kernel, dim3((unsigned)(B * nblk)), dim3(256), 0, s, y, ws, N, C, ld, nblk);
        SDMI_CHECK_HIP(hipGetLastError());
    }
    ProfScope ps("hat_channel_gate", 4.0 * B * C * Cs, 4.0 * B * nblk * C, s);
    hipLaunchKernelGGL(hat_channel_gate_kernel, dim3((unsigned)B), dim3(256), 0, s, ws, w1, b1, w3, b3, gate, N, C, Cs, nblk);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the sum that adds the conv branch to the stream ---------------------------------------------------------------------------------------
// out[row][c] = t[row][c] + conv_scale * gate[row / rows_per_image][c] * conv[row][c] in fp32, one rounding; a thread per 8 channels of a row.
// Launch: grid-stride over rows * C / 8, block 256.
__global__ __launch_bounds__(256) void hat_cab_add_kernel(const half_t* t, const half_t* conv, const float* gate, half_t* out, int rows_per_image,
                                                          int C, int ldt, int ldc, int ldo, float conv_scale, long long n8) {
    const int c8n = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const int c = 8 * (int)(i % c8n);
        const long long row = i / c8n;
        const float* gt = gate + (row / rows_per_image) * C + c;
        const h8 tv = *reinterpret_cast<const h8*>(t + row * ldt + c);
        const h8 cv = *reinterpret_cast<const h8*>(conv + row * ldc + c);
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)fmaf(conv_scale * gt[e], (float)cv[e], (float)tv[e]);
        *reinterpret_cast<h8*>(out + row * ldo + c) = o;
    }
}

int launch_hat_cab_add(const half_t* t, const half_t* conv, const float* gate, half_t* out, long long rows, int rows_per_image, int C, int ldt,
                       int ldc, int ldo, float conv_scale, hipStream_t s) {
    SDMI_REQUIRE(t && conv && gate && out, "null argument");
    SDMI_REQUIRE(rows > 0 && rows_per_image > 0 && rows % rows_per_image == 0, "rows must be a positive multiple of rows_per_image");
    SDMI_REQUIRE(C >= 8 && C % 8 == 0, "channels must be a positive multiple of 8");
    SDMI_REQUIRE(ldt >= C && ldc >= C && ldo >= C, "rows narrower than the channels");
    SDMI_REQUIRE(ldt % 8 == 0 && ldc % 8 == 0 && ldo % 8 == 0 && ((((uintptr_t)t | (uintptr_t)conv | (uintptr_t)out) & 15) == 0) &&
                     ((uintptr_t)gate & 3) == 0,
                 "misaligned: t / conv / out on 16 bytes, gate on 4, row strides multiples of 8");
    SDMI_REQUIRE((const void*)out != (const void*)conv, "out may alias t, not conv");
    SDMI_REQUIRE(rows * (long long)std::max(ldt, std::max(ldc, ldo)) < (1ll << 40), "tensor too large");
    const long long n8 = rows * (C / 8);
    const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 65536);
    ProfScope ps("hat_cab_add", 16.0 * n8, 48.0 * n8, s);
    hipLaunchKernelGGL(hat_cab_add_kernel, dim3(grid), dim3(256), 0, s, t, conv, gate, out, rows_per_image, C, ldt, ldc, ldo, conv_scale, n8);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
