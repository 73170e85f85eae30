// dat.hip — the kernels of the DAT upscalers (Chen et al., "Dual Aggregation Transformer for Image Super-Resolution", ICCV 2023) that
// the rest of the library has no form of, for gfx950: attention in rectangular windows on the two halves of the heads at once, the
// channel attention's Gram matrix and its softmax, a depthwise 3x3 conv on token rows and the two gates of the adaptive interaction
// module.  The linears and convs of the network run on gemm.hip, LayerNorm and the input / output / shuffle passes on swinir.hip, the
// 64-channel conv_last on rrdb.hip (engine.cpp dat_pass).
//
// Token rows are fp16 with a head's D <= 32 channels in a 32-wide slot (dims D .. 31 zero): q, k, v, att, conv and proj's input are all
// [tokens][32 heads] in that layout.
//
// dat_window_attn<N>: one workgroup (256 threads, 4 waves) per (image, window, head); N = s0 s1 = 128 | 256 tokens per window.  Heads
// [0, heads / 2) are branch 0, windows of s0 rows x s1 columns, the others branch 1, windows of s1 rows x s0 columns: both branches in one
// launch.  The token grid is padded right / bottom to multiples of max(s0, s1) with tokens whose q = k = v = 0 (they are keys: score
// 0 + bias); the cyclic shift (torch.roll by minus half the window on the PADDED grid), the partition and their inverses are index
// arithmetic: token a of window (wy, wx) sits at (ys, xs) = (Hs wy + a / Ws, Ws wx + a % Ws) of the shifted grid, i.e. at
// ((ys + Hs / 2) % Hpad, (xs + Ws / 2) % Wpad) of the padded grid; it is read from and written back to that row, or is a zero row when
// that lies outside the image.  The shift mask is computed from the region ids of the two tokens on the shifted padded grid (-100 where
// they differ, not -inf); the bias is read from the head's column of the [(2 Hs - 1)(2 Ws - 1)][heads / 2] table, staged in LDS, at
// (ya - yb + Hs - 1)(2 Ws - 1) + (xa - xb + Ws - 1).
// LDS (static): K [N][40] fp16 (80-byte rows: the 16-byte fragment reads of 16 consecutive rows fall on distinct banks), V^T [32][N + 4]
// fp16, the bias column 945 fp32, the token rows N int32 and region ids N bytes: N = 256: 20480 + 16640 + 3780 + 1024 + 256 = 42180 bytes
// (42192 with alignment); N = 128: 10240 + 8448 + 3780 + 512 + 128 = 23108 bytes (23120).  Launch configuration: grid
// B * (Hpad Wpad / N) * heads workgroups, block 256 threads, no dynamic LDS; 212 / 100 VGPRs, no scratch.
// A wave takes the query tiles qt = wave, wave + 4, ...: 16 queries against all N keys on v_mfma_f32_16x16x32_f16 with swin_window_attn's
// register layout (S^T = K Q^T, a lane holds keys 16 nj + 4 (lane / 16) + r of query lane % 16; the probabilities of two key tiles are
// the B fragment of O^T = V^T P^T as they lie).  Scores, bias, mask and softmax are fp32; the normalised probabilities are rounded to fp16.
//
// Channel attention: dat_channel_gram sums q_i k_j, q_i^2, k_j^2 over blocks of DAT_GRAM_TOKENS tokens per (image, head) in fp32 (a
// thread owns 4 entries of the 32 x 32 matrix and walks its block's tokens in order); dat_channel_softmax adds the blocks' partials in
// block order (no atomics: two runs give the same bits), divides by max(|q_i|, 1e-12) max(|k_j|, 1e-12), multiplies by the head's
// temperature, takes the row softmax and writes the head's D x D block of a block-diagonal [32 heads][32 heads] fp16 matrix per image,
// zeros elsewhere: att = v A^T is then a batched GEMM with per-image weights.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace sdmi {

namespace {
constexpr int DAT_KLD = 40;                                 // row stride (halfs) of the K image
constexpr int DAT_TAB = 63 * 15;                            // entries of the largest bias table column: (2 * 32 - 1) * (2 * 8 - 1)

__device__ __forceinline__ int dat_region(int u, int n, int s) { return u < n - s ? 0 : (u < n - (s >> 1) ? 1 : 2); }
__device__ __forceinline__ float dat_gelu(float a) { return 0.5f * a * (1.0f + erff(a * 0.70710678118654752f)); }
__device__ __forceinline__ float dat_sigmoid(float a) { return 1.0f / (1.0f + __expf(-a)); }
}  // namespace

template <int N>
__global__ __launch_bounds__(256) void dat_window_attn_kernel(const DatAttnP p) {
    constexpr int VLD = N + 4;                              // row stride (halfs) of the V^T image: 8-byte aligned rows
    __shared__ __attribute__((aligned(16))) half_t ks[N * DAT_KLD];
    __shared__ __attribute__((aligned(16))) half_t vt[32 * VLD];
    __shared__ float tab[DAT_TAB];
    __shared__ int rows[N];
    __shared__ __attribute__((aligned(4))) unsigned char reg[N];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int hh = p.heads >> 1;
    const int h = (int)(blockIdx.x % (unsigned)p.heads);
    const int br = h >= hh ? 1 : 0, hb = h - br * hh;
    const int Hs = br ? p.s1 : p.s0, Ws = br ? p.s0 : p.s1; // the window: Hs rows x Ws columns, Ws a power of two
    const int lw = Ws == 8 ? 3 : (Ws == 16 ? 4 : 5);
    const int nwx = p.Wpad / Ws, nwin = nwx * (p.Hpad / Hs);
    const int win = (int)((blockIdx.x / (unsigned)p.heads) % (unsigned)nwin);
    const long long b = (long long)(blockIdx.x / ((unsigned)p.heads * (unsigned)nwin));
    const int wy = win / nwx, wx = win - wy * nwx;
    const int shy = p.shifted ? Hs >> 1 : 0, shx = p.shifted ? Ws >> 1 : 0;
    const int tw = 2 * Ws - 1;

    for (int a = tid; a < N; a += 256) {
        const int ys = wy * Hs + (a >> lw), xs = wx * Ws + (a & (Ws - 1));
        int y = ys + shy, x = xs + shx;
        if (y >= p.Hpad) y -= p.Hpad;
        if (x >= p.Wpad) x -= p.Wpad;
        const bool in = y < p.H && x < p.W;
        const long long row = (b * p.H + y) * p.W + x;
        rows[a] = in ? (int)row : -1;
        reg[a] = (unsigned char)(3 * dat_region(ys, p.Hpad, Hs) + dat_region(xs, p.Wpad, Ws));
        const half_t* src = p.qkv + (in ? row : 0) * p.ldq + (p.heads + h) * 32;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            h8 kv = h8{0, 0, 0, 0, 0, 0, 0, 0}, vv = h8{0, 0, 0, 0, 0, 0, 0, 0};
            if (in) {
                kv = *reinterpret_cast<const h8*>(src + 8 * c);
                vv = *reinterpret_cast<const h8*>(src + p.heads * 32 + 8 * c);
            }
            *reinterpret_cast<h8*>(ks + a * DAT_KLD + 8 * c) = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) vt[(8 * c + e) * VLD + a] = vv[e];
        }
    }
    const float* table = br ? p.bias1 : p.bias0;
    for (int i = tid; i < (2 * Hs - 1) * tw; i += 256) tab[i] = table[(long long)i * hh + hb];
    __syncthreads();

    for (int qt = wave; qt < N / 16; qt += 4) {             // wave-uniform
        const int aq = 16 * qt + l16;
        const int rq = rows[aq];
        h8 qf = h8{0, 0, 0, 0, 0, 0, 0, 0};
        if (rq >= 0) qf = *reinterpret_cast<const h8*>(p.qkv + (long long)rq * p.ldq + h * 32 + 8 * g);
        f4 s[N / 16];                                       // [nj]: keys 16 nj + 4 g + r of query 16 qt + l16
#pragma unroll
        for (int nj = 0; nj < N / 16; ++nj) {
            const h8 kf = *reinterpret_cast<const h8*>(ks + (16 * nj + l16) * DAT_KLD + 8 * g);
            s[nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            if ((nj & 3) == 3) __builtin_amdgcn_sched_barrier(0);       // at most four K fragments in flight: the unrolled loop's loads are not all hoisted
        }
        const int regq = reg[aq];
        const int qbase = ((aq >> lw) + Hs - 1) * tw + (aq & (Ws - 1)) + Ws - 1;
        float mx = -3.0e38f;
#pragma unroll
        for (int nj = 0; nj < N / 16; ++nj) {
            const int ak = 16 * nj + 4 * g;                 // keys ak .. ak + 3 lie in one window row (Ws >= 8)
            const int kb = qbase - (ak >> lw) * tw - (ak & (Ws - 1));
            const unsigned rk = *reinterpret_cast<const unsigned*>(reg + ak);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float m = (p.shifted && (int)((rk >> (8 * r)) & 255u) != regq) ? -100.0f : 0.0f;
                const float v = fmaf(s[nj][r], p.scale, tab[kb - r]) + m;
                s[nj][r] = v;
                mx = fmaxf(mx, v);
            }
            if (nj & 1) __builtin_amdgcn_sched_barrier(0);              // eight bias reads in flight
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int nj = 0; nj < N / 16; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = __expf(s[nj][r] - mx);
                s[nj][r] = e;
                sum += e;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        const float inv = 1.0f / sum;
        h8 pf[N / 32];                                      // [kk]: the B fragments of O^T = V^T P^T
#pragma unroll
        for (int kk = 0; kk < N / 32; ++kk)
#pragma unroll
            for (int e = 0; e < 8; ++e) pf[kk][e] = (half_t)(s[2 * kk + (e >> 2)][e & 3] * inv);
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
            f4 o = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < N / 32; ++kk) {           // k slot 8 g + e = key 16 (2 kk + e / 4) + 4 g + e % 4 on both operands
                const half_t* src = vt + (16 * nb + l16) * VLD + 32 * kk + 4 * g;
                const h4 lo = *reinterpret_cast<const h4*>(src), hi = *reinterpret_cast<const h4*>(src + 16);
                const h8 vf = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[kk], o, 0, 0, 0);
                if ((kk & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
            const int d0 = 16 * nb + 4 * g;                 // dims d0 .. d0 + 3 of query 16 qt + l16; the slot's tail D .. 31 is stored as zero
            h4 ov;
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[r] = d0 + r < p.D ? (half_t)o[r] : (half_t)0.f;
            if (rq >= 0) *reinterpret_cast<h4*>(p.out + (long long)rq * p.ldo + h * 32 + d0) = ov;
        }
    }
}

int launch_dat_window_attention(const DatAttnP& p0, hipStream_t s) {
    DatAttnP p = p0;
    SDMI_REQUIRE(p.qkv && p.bias0 && p.bias1 && p.out, "null qkv / bias0 / bias1 / out");
    SDMI_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0, "empty token grid");
    SDMI_REQUIRE(p.heads >= 2 && p.heads <= 1024 && p.heads % 2 == 0, "heads must be even (half of them per branch)");
    SDMI_REQUIRE(p.D >= 1 && p.D <= 32, "head dim D must be in 1..32 (one 32-wide slot per head)");
    SDMI_REQUIRE(p.s0 == 8 && (p.s1 == 16 || p.s1 == 32), "split must be (8, 16) or (8, 32)");
    SDMI_REQUIRE(p.shifted == 0 || p.shifted == 1, "shift must be (0, 0) or half the split");
    SDMI_REQUIRE(p.ldq >= 96 * p.heads, "qkv rows hold 3 x heads slots of 32: ldq >= 96 heads");
    SDMI_REQUIRE(p.ldo >= 32 * p.heads, "out rows hold heads slots of 32: ldo >= 32 heads");
    SDMI_REQUIRE(p.ldq % 8 == 0 && p.ldo % 8 == 0 && ((uintptr_t)p.qkv & 15) == 0 && ((uintptr_t)p.out & 15) == 0 && ((uintptr_t)p.bias0 & 3) == 0 &&
                     ((uintptr_t)p.bias1 & 3) == 0,
                 "misaligned: qkv / out bases on 16 bytes, the bias tables on 4, ldq and ldo multiples of 8");
    p.Hpad = (p.H + p.s1 - 1) / p.s1 * p.s1;
    p.Wpad = (p.W + p.s1 - 1) / p.s1 * p.s1;
    const long long windows = (long long)p.B * p.Hpad * p.Wpad / (p.s0 * p.s1);
    SDMI_REQUIRE((long long)p.B * p.Hpad * p.Wpad < (1ll << 31) - 256 && windows * p.heads < (1ll << 31), "B*H*W (padded) must stay below 2^31 tokens");
    const int N = p.s0 * p.s1;
    const double tokens = (double)windows * N;
    ProfScope ps("dat_window_attn", tokens * p.heads * (2.0 * N * 32 * 2), tokens * p.heads * 32 * 2.0 * 4, s);
    const dim3 grid((unsigned)(windows * p.heads));
    if (N == 256) hipLaunchKernelGGL(dat_window_attn_kernel<256>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(dat_window_attn_kernel<128>, grid, dim3(256), 0, s, p);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- channel attention -------------------------------------------------------------------------------------------------------------
// part[((b heads + h) nblk + blk)][1088]: [0, 1024) sum q_i k_j at i * 32 + j, [1024, 1056) sum q_i^2, [1056, 1088) sum k_j^2 over the tokens
// [blk T, min(N, (blk + 1) T)), T = DAT_GRAM_TOKENS.  Thread tid owns row i = tid / 8, columns 4 (tid % 8) .. + 3; tokens are staged 64 at a
// time (LDS 2 x 64 x 32 fp16 = 8192 bytes) and walked in order.  Launch: grid B * heads * nblk, block 256.
__global__ __launch_bounds__(256) void dat_channel_gram_kernel(const half_t* qkv, float* part, int N, int heads, int ldq, int nblk) {
    __shared__ __attribute__((aligned(16))) half_t qs[64 * 32];
    __shared__ __attribute__((aligned(16))) half_t kq[64 * 32];
    const int tid = threadIdx.x;
    const int blk = (int)(blockIdx.x % (unsigned)nblk);
    const int bh = (int)(blockIdx.x / (unsigned)nblk);
    const int h = bh % heads;
    const long long b = bh / heads;
    const int i = tid >> 3, j0 = (tid & 7) * 4;
    const int t_begin = blk * DAT_GRAM_TOKENS, t_end = min(N, t_begin + DAT_GRAM_TOKENS);
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, sk[4] = {0.f, 0.f, 0.f, 0.f}, sq = 0.f;
    for (int t0 = t_begin; t0 < t_end; t0 += 64) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = tid + 256 * u, tok = idx >> 3, part8 = idx & 7;
            h8 v = h8{0, 0, 0, 0, 0, 0, 0, 0};
            if (t0 + tok < t_end)
                v = *reinterpret_cast<const h8*>(qkv + (b * N + t0 + tok) * ldq + ((part8 >> 2) * heads + h) * 32 + 8 * (part8 & 3));
            *reinterpret_cast<h8*>((part8 >> 2 ? kq : qs) + tok * 32 + 8 * (part8 & 3)) = v;
        }
        __syncthreads();
        for (int t = 0; t < 64; ++t) {
            const float qv = (float)qs[t * 32 + i];
            const h4 kv = *reinterpret_cast<const h4*>(kq + t * 32 + j0);
            sq = fmaf(qv, qv, sq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float kf = (float)kv[r];
                acc[r] = fmaf(qv, kf, acc[r]);
                sk[r] = fmaf(kf, kf, sk[r]);
            }
        }
        __syncthreads();
    }
    float* dst = part + (long long)blockIdx.x * 1088;
    *reinterpret_cast<f4*>(dst + i * 32 + j0) = f4{acc[0], acc[1], acc[2], acc[3]};
    if (j0 == 0) dst[1024 + i] = sq;
    if (i == 0) *reinterpret_cast<f4*>(dst + 1056 + j0) = f4{sk[0], sk[1], sk[2], sk[3]};
}

int launch_dat_channel_gram(const half_t* qkv, float* part, int B, int N, int heads, int ldq, hipStream_t s) {
    SDMI_REQUIRE(qkv && part, "null qkv / partials");
    SDMI_REQUIRE(B > 0 && N > 0 && heads >= 1 && heads <= 1024, "empty tensor");
    SDMI_REQUIRE(ldq >= 64 * heads, "qkv rows hold the q and k slots of every head: ldq >= 64 heads");
    SDMI_REQUIRE(ldq % 8 == 0 && ((uintptr_t)qkv & 15) == 0 && ((uintptr_t)part & 15) == 0, "misaligned: qkv / partials on 16 bytes, ldq a multiple of 8");
    SDMI_REQUIRE((long long)B * N < (1ll << 31) - 256, "B*N must stay below 2^31 tokens");
    const int nblk = (N + DAT_GRAM_TOKENS - 1) / DAT_GRAM_TOKENS;
    SDMI_REQUIRE((long long)B * heads * nblk < (1ll << 31), "too many blocks");
    ProfScope ps("dat_channel_gram", 2.0 * B * N * heads * 1088, 2.0 * B * N * heads * 64, s);
    hipLaunchKernelGGL(dat_channel_gram_kernel, dim3((unsigned)(B * heads * nblk)), dim3(256), 0, s, qkv, part, N, heads, ldq, nblk);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// One workgroup per (image, head): the partials added in block order, normalised, scaled, the row softmax over j < D, written as the
// head's block of A [B][32 heads][32 heads] fp16; the rest of the head's 32 rows is written as zeros.  Launch: grid B * heads, block 256.
__global__ __launch_bounds__(256) void dat_channel_softmax_kernel(const float* part, const float* temperature, half_t* A, int heads, int D,
                                                                  int nblk) {
    const int tid = threadIdx.x;
    const int h = (int)(blockIdx.x % (unsigned)heads);
    const long long b = blockIdx.x / (unsigned)heads;
    const int i = tid >> 3, j0 = (tid & 7) * 4;
    const float* src = part + (long long)blockIdx.x * nblk * 1088;
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, sk[4] = {0.f, 0.f, 0.f, 0.f}, sq = 0.f;
    for (int k = 0; k < nblk; ++k, src += 1088) {
        sq += src[1024 + i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc[r] += src[i * 32 + j0 + r];
            sk[r] += src[1056 + j0 + r];
        }
    }
    const float iq = temperature[h] / fmaxf(sqrtf(sq), 1e-12f);
    float v[4], mx = -3.0e38f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = acc[r] * iq / fmaxf(sqrtf(sk[r]), 1e-12f);
        if (j0 + r < D) mx = fmaxf(mx, v[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = j0 + r < D ? __expf(v[r] - mx) : 0.f;
        sum += v[r];
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    const float inv = i < D ? 1.0f / sum : 0.f;
    const int ld = 32 * heads;
    half_t* row = A + (b * ld + h * 32 + i) * ld;
    for (int c = j0; c < ld; c += 32) {
        h4 o = h4{0, 0, 0, 0};
        if (c == h * 32 + j0) o = h4{(half_t)(v[0] * inv), (half_t)(v[1] * inv), (half_t)(v[2] * inv), (half_t)(v[3] * inv)};
        *reinterpret_cast<h4*>(row + c) = o;
    }
}

int launch_dat_channel_softmax(const float* part, const float* temperature, half_t* A, int B, int N, int heads, int D, hipStream_t s) {
    SDMI_REQUIRE(part && temperature && A, "null partials / temperature / A");
    SDMI_REQUIRE(B > 0 && N > 0 && heads >= 1 && heads <= 1024, "empty tensor");
    SDMI_REQUIRE(D >= 1 && D <= 32, "head dim D must be in 1..32 (one 32-wide slot per head)");
    SDMI_REQUIRE(((uintptr_t)part & 15) == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)temperature & 3) == 0, "misaligned: partials / A on 16 bytes, temperature on 4");
    const int nblk = (N + DAT_GRAM_TOKENS - 1) / DAT_GRAM_TOKENS;
    ProfScope ps("dat_channel_softmax", 1088.0 * B * heads * nblk, 4352.0 * B * heads * nblk + 2048.0 * B * heads * heads, s);
    hipLaunchKernelGGL(dat_channel_softmax_kernel, dim3((unsigned)(B * heads)), dim3(256), 0, s, part, temperature, A, heads, D, nblk);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- depthwise 3x3 conv on token rows ------------------------------------------------------------------------------------------------
// out[pixel][c] = ep(bias[c] + sum over the 9 taps of w[tap][c] x[neighbour][c]), zero padding, fp32 sums; a thread per 8 channels of a
// pixel.  ep 0: exact (erf) GELU; ep 1: times mul[pixel][c].  Launch: grid-stride over B*H*W*C / 8, block 256.
__global__ __launch_bounds__(256) void dat_dwconv3x3_kernel(const half_t* x, const float* w, const float* bias, const half_t* mul, half_t* out, int H,
                                                            int W, int C, int ldx, int ldm, int ldo, int ep, long long n8) {
    const int c8n = C >> 3;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const int c = 8 * (int)(i % c8n);
        const long long pix = i / c8n;
        const int xx = (int)(pix % W), y = (int)((pix / W) % H);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = bias[c + e];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (y + dy < 0 || y + dy >= H || xx + dx < 0 || xx + dx >= W) continue;
                const h8 v = *reinterpret_cast<const h8*>(x + (pix + dy * W + dx) * ldx + c);
                const float* wt = w + ((dy + 1) * 3 + dx + 1) * C + c;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf((float)v[e], wt[e], acc[e]);
            }
        h8 o;
        if (ep == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)dat_gelu(acc[e]);
        } else {
            const h8 m = *reinterpret_cast<const h8*>(mul + pix * ldm + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)(acc[e] * (float)m[e]);
        }
        *reinterpret_cast<h8*>(out + pix * ldo + c) = o;
    }
}

int launch_dat_dwconv3x3(const half_t* x, const float* w, const float* bias, const half_t* mul, half_t* out, int B, int H, int W, int C, int ldx,
                         int ldm, int ldo, int ep, hipStream_t s) {
    SDMI_REQUIRE(x && w && bias && out, "null x / weight / bias / out");
    SDMI_REQUIRE(ep == 0 || ep == 1, "epilogue 0 (GELU) | 1 (times mul)");
    SDMI_REQUIRE(ep == 0 || mul, "null mul with the gate epilogue");
    SDMI_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && C % 8 == 0, "empty tensor, or channels not a multiple of 8");
    SDMI_REQUIRE(ldx >= C && ldo >= C && (ep == 0 || ldm >= C), "rows narrower than the channels");
    SDMI_REQUIRE(ldx % 8 == 0 && ldo % 8 == 0 && (ep == 0 || ldm % 8 == 0) && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                     ((uintptr_t)mul & 15) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)bias & 3) == 0,
                 "misaligned: x / mul / out on 16 bytes, weight / bias on 4, row strides multiples of 8");
    SDMI_REQUIRE(x != out && mul != out, "out must not alias an input (a pixel's neighbours read it)");
    const long long n8 = (long long)B * H * W * (C / 8);
    SDMI_REQUIRE((long long)B * H * W * std::max(ldx, std::max(ldo, ldm)) < (1ll << 40), "tensor too large");
    const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 65536);
    ProfScope ps(ep ? "dat_dwconv3x3_gate" : "dat_dwconv3x3_gelu", 18.0 * 8 * n8, (ep ? 48.0 : 32.0) * n8, s);
    hipLaunchKernelGGL(dat_dwconv3x3_kernel, dim3(grid), dim3(256), 0, s, x, w, bias, mul, out, H, W, C, ldx, ldm, ldo, ep, n8);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the channel gate of the adaptive interaction module ---------------------------------------------------------------------------------
// ws[(b nblk + blk)][C]: the sums of x over the tokens [blk T, min(N, (blk + 1) T)), T = DAT_POOL_TOKENS.  Thread tid owns the 8 channels
// 8 (tid % (C / 8)) of token group tg = tid / (C / 8) < G = 256 / (C / 8): it adds the tokens tg, tg + G, ... of the block in order (16-byte
// loads), then a thread per channel adds the G groups' sums in group order through LDS (G C <= 2048 fp32 = 8192 bytes): every sum has one
// fixed order.  Launch: grid B * nblk, block 256.
__global__ __launch_bounds__(256) void dat_pool_partial_kernel(const half_t* x, float* ws, int N, int C, int ld, int nblk) {
    __shared__ float red[2048];
    const int blk = (int)(blockIdx.x % (unsigned)nblk);
    const long long b = blockIdx.x / (unsigned)nblk;
    const int t_begin = blk * DAT_POOL_TOKENS, t_end = min(N, t_begin + DAT_POOL_TOKENS);
    const int c8n = C >> 3, G = 256 / c8n;
    const int c8 = (int)threadIdx.x % c8n, tg = (int)threadIdx.x / c8n;
    if (tg < G) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = t_begin + tg; t < t_end; t += G) {
            const h8 v = *reinterpret_cast<const h8*>(x + (b * N + t) * ld + 8 * c8);
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
// One workgroup per image: the partials added in block order -> the mean; hidden = GELU(w1 mean + b1); gate = sigmoid(w2 hidden + b2).
// LDS: (1024 + 128) fp32 = 4608 bytes.  Launch: grid B, block 256.
__global__ __launch_bounds__(256) void dat_pool_gate_kernel(const float* ws, const float* w1, const float* b1, const float* w2, const float* b2,
                                                            float* gate, int N, int C, int C8, int nblk) {
    __shared__ float mean[1024];
    __shared__ float hid[128];
    const long long b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float sum = 0.f;
        for (int k = 0; k < nblk; ++k) sum += ws[(b * nblk + k) * C + c];
        mean[c] = sum / (float)N;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < C8; j += 256) {
        float a = b1[j];
        for (int c = 0; c < C; ++c) a = fmaf(w1[j * C + c], mean[c], a);
        hid[j] = dat_gelu(a);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = b2[c];
        for (int j = 0; j < C8; ++j) a = fmaf(w2[c * C8 + j], hid[j], a);
        gate[b * C + c] = dat_sigmoid(a);
    }
}

int launch_dat_pool_gate(const half_t* x, const float* w1, const float* b1, const float* w2, const float* b2, float* ws, float* gate, int B, int N,
                         int C, int C8, int ld, hipStream_t s) {
    SDMI_REQUIRE(x && w1 && b1 && w2 && b2 && ws && gate, "null argument");
    SDMI_REQUIRE(B > 0 && N > 0, "empty tensor");
    SDMI_REQUIRE(C >= 8 && C <= 1024 && C % 8 == 0 && C8 >= 1 && C8 <= 128, "channels a multiple of 8 in 8..1024, hidden width in 1..128");
    SDMI_REQUIRE(ld >= C, "rows narrower than the channels");
    SDMI_REQUIRE(((uintptr_t)x & 15) == 0 && ld % 8 == 0 &&
                     (((uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)ws | (uintptr_t)gate) & 3) == 0,
                 "misaligned: x on 16 bytes, ld a multiple of 8, fp32 arguments on 4 bytes");
    SDMI_REQUIRE((long long)B * N < (1ll << 31) - 256, "B*N must stay below 2^31 tokens");
    const int nblk = (N + DAT_POOL_TOKENS - 1) / DAT_POOL_TOKENS;
    {
        ProfScope ps("dat_pool_partial", (double)B * N * C, 2.0 * B * N * C, s);
        hipLaunchKernelGGL(dat_pool_partial_kernel, dim3((unsigned)(B * nblk)), dim3(256), 0, s, x, ws, N, C, ld, nblk);
        SDMI_CHECK_HIP(hipGetLastError());
    }
    ProfScope ps("dat_pool_gate", 4.0 * B * C * C8, 4.0 * B * nblk * C, s);
    hipLaunchKernelGGL(dat_pool_gate_kernel, dim3((unsigned)B), dim3(256), 0, s, ws, w1, b1, w2, b2, gate, N, C, C8, nblk);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the spatial gate and the sum that proj reads ------------------------------------------------------------------------------------
// A wave per token row: sg = sigmoid(w2 . GELU(w1 S + b1) + b2) of the row of S (the spatial MLP C -> C16 -> 1), then
// out = S cg[image] + T sg.  w1 [C16][C] is staged in LDS once per workgroup (at most 8192 fp32 = 32768 bytes), a workgroup walks rows
// blockIdx.x * 4 + wave with a grid stride.  Launch: grid min(rows / 4, 2048), block 256.
__global__ __launch_bounds__(256) void dat_aim_combine_kernel(const DatAimP p) {
    __shared__ float w1s[8192];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < p.C16 * p.C; i += 256) w1s[i] = p.w1[i];
    __syncthreads();
    const int U = p.C >> 6;
    for (long long row = (long long)blockIdx.x * 4 + wave; row < p.rows; row += (long long)gridDim.x * 4) {     // wave-uniform
        const half_t* sr = p.s + row * p.lds;
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) sv[u] = u < U ? (float)sr[lane + 64 * u] : 0.f;
        float z = p.b2;
        for (int j = 0; j < p.C16; ++j) {
            float d = 0.f;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u < U) d = fmaf(sv[u], w1s[j * p.C + lane + 64 * u], d);
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) d += __shfl_xor(d, m);
            z = fmaf(p.w2[j], dat_gelu(d + p.b1[j]), z);
        }
        const float sg = dat_sigmoid(z);
        const float* cg = p.cg + (row / p.rows_per_image) * p.C;
        const half_t* tr = p.t + row * p.ldt;
        half_t* orow = p.out + row * p.ldo;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (u < U) orow[lane + 64 * u] = (half_t)fmaf(sv[u], cg[lane + 64 * u], (float)tr[lane + 64 * u] * sg);
    }
}

int launch_dat_aim_combine(const DatAimP& p, hipStream_t s) {
    SDMI_REQUIRE(p.s && p.t && p.cg && p.w1 && p.b1 && p.w2 && p.out, "null argument");
    SDMI_REQUIRE(p.rows > 0 && p.rows_per_image > 0 && p.rows % p.rows_per_image == 0, "rows must be a positive multiple of rows_per_image");
    SDMI_REQUIRE(p.C >= 64 && p.C <= 512 && p.C % 64 == 0, "channels must be a multiple of 64 in 64..512");
    SDMI_REQUIRE(p.C16 >= 1 && (long long)p.C16 * p.C <= 8192, "the spatial MLP's first layer must fit 8192 weights");
    SDMI_REQUIRE(p.lds >= p.C && p.ldt >= p.C && p.ldo >= p.C, "rows narrower than the channels");
    SDMI_REQUIRE(((((uintptr_t)p.s | (uintptr_t)p.t | (uintptr_t)p.out) & 1) == 0) &&
                     ((((uintptr_t)p.cg | (uintptr_t)p.w1 | (uintptr_t)p.b1 | (uintptr_t)p.w2) & 3) == 0),
                 "misaligned: fp32 arguments on 4 bytes");
    SDMI_REQUIRE(p.rows * (long long)std::max(p.lds, std::max(p.ldt, p.ldo)) < (1ll << 40), "tensor too large");
    const unsigned grid = (unsigned)std::min<long long>((p.rows + 3) / 4, 2048);
    ProfScope ps("dat_aim_combine", 2.0 * p.rows * p.C * (p.C16 + 2), 6.0 * p.rows * p.C, s);
    hipLaunchKernelGGL(dat_aim_combine_kernel, dim3(grid), dim3(256), 0, s, p);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
