// swinir.hip — the kernels of the window-transformer upscalers that the rest of the library has no form of, for gfx950: SwinIR (Liang et
// al., "SwinIR: Image Restoration Using Swin Transformer") and Swin2SR (Conde et al., "Swin2SR: SwinV2 Transformer for Compressed Image
// Super-Resolution and Restoration"); ScuNET's wide levels use the attention and the LayerNorm as well.  Shifted-window attention with a
// scaled or a cosine score, the row LayerNorm of padded token rows with or without the residual add of res-post-norm, the small input /
// output / activation passes, and the pixel shuffles of Swin2SR's `pixelshuffle` / `pixelshuffledirect` tails.  The linears and convs of
// the networks run on gemm.hip, the 64-channel tails on rrdb.hip (engine.cpp swinir_pass).
//
// swin_window_attn: one workgroup (4 waves) per 8 x 8 window, a wave per head, walking ceil(heads / 4) heads.  The cyclic shift
// (torch.roll by -shift), the window partition and their inverses are index arithmetic: token a of window (wy, wx) sits at
// (ys, xs) = (8 wy + a / 8, 8 wx + a % 8) of the SHIFTED grid, i.e. in row ((ys + shift) % H, (xs + shift) % W) of the token tensor, and
// is read from and written back to that row.  The shift mask is computed from the region ids of the two tokens on the shifted grid
// (-100 where they differ, as the reference has it; not -inf), the relative-position bias is read as fp32 [heads][64][64].
//
// Per head, on v_mfma_f32_16x16x32_f16 with fp32 accumulation (head dim <= 32: ONE k step):
//   S^T = K Q^T    16 tiles; operands are the 64-byte q / k slots of the token rows, read as 16-byte fragments straight from global memory
//                  (a slot row is exactly the four k-groups of the MFMA).  A lane ends up with keys 16 nj + 4 (lane / 16) + r, r = 0..3, of
//                  QUERY 16 mi + lane % 16: the softmax of a query is a reduction over a lane's own 16 values and the 4 lanes
//                  {l, l + 16, l + 32, l + 48} (two shuffles), and the 8 probabilities of two key tiles are, as they lie in the registers,
//                  the B fragment of
//   O^T = V^T P^T  16 MFMAs; the k slots of a 32-key step are permuted (slot 8 g + e = key 16 (2 kk + e / 4) + 4 g + e % 4) on both
//                  operands alike.  V^T comes from LDS: each wave transposes its head's V [64 tokens][32] into its own [32][68] image.
//                  A lane ends up with 4 consecutive dims of one query: 8-byte stores.
// Scores, bias, mask and softmax are fp32; the normalised probabilities are rounded to fp16 for the second MFMA.
//
// The cosine form (template argument COSINE; Swin2SR's Swin-V2 blocks) has the same geometry and register layout with the score
//   cos(q, k) tau_h + bias + mask = (q . k) / (max(|q|, 1e-12) max(|k|, 1e-12)) head_scale[h] + bias[h][a][b] + mask.
// The MFMA runs on the fp16 q / k AS STORED; the two inverse norms are taken in fp32 from the same slot values and multiply the fp32
// score.  (Normalising the operands first and rounding them to fp16 again would put the rounding of a unit vector, times tau up to 100,
// into the logit.)  A lane's 8 q and 8 k values of token 16 j + l16 are a quarter of its slot: the squared norms are two shuffles over
// {l, l + 16, l + 32, l + 48}.  The query norms are then where the S^T tiles want them (query 16 mi + l16); the norm of key
// 16 nj + 4 g + r sits in lane 4 g + r: one __shfl each.  A zero row has score 0 x 1e12 = 0: bias and mask alone, never NaN.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace sdmi {

namespace {
constexpr int SWIN_VLD = 68;                                // row stride (halfs) of the V^T image: 136 bytes, 8-byte aligned, not a multiple of 128

__device__ __forceinline__ int swin_region(int u, int n) { return u < n - 8 ? 0 : (u < n - 4 ? 1 : 2); }
}  // namespace

template <bool COSINE>
__global__ __launch_bounds__(256) void swin_window_attn_kernel(const SwinAttnP p) {
    __shared__ __attribute__((aligned(16))) half_t vt[4][32 * SWIN_VLD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int H = p.H, W = p.W, nwx = W >> 3, nwy = H >> 3;
    const int wx = (int)(blockIdx.x % (unsigned)nwx), wy = (int)((blockIdx.x / (unsigned)nwx) % (unsigned)nwy);
    const long long img = (long long)(blockIdx.x / (unsigned)(nwx * nwy)) * H * W;
    // token a of this window -> its row in the token tensor
    auto row_of = [&](int a) -> long long {
        int y = 8 * wy + (a >> 3) + p.shift, x = 8 * wx + (a & 7) + p.shift;
        if (y >= H) y -= H;
        if (x >= W) x -= W;
        return img + (long long)y * W + x;
    };
    long long rq[4];                                        // rows of the tokens 16 j + l16: the Q / K fragments and the output
    int idq[4];                                             // their region ids on the shifted grid
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int a = 16 * j + l16;
        rq[j] = row_of(a);
        idq[j] = 3 * swin_region(8 * wy + (a >> 3), H) + swin_region(8 * wx + (a & 7), W);
    }
    // keys 16 nj + 4 g + r: y = 8 wy + 2 nj + g / 2, x = 8 wx + 4 (g % 2) + r.  masked[mi]: bit 4 nj + r is set where the key's region differs
    // from query mi's (one register per query instead of 64 lane masks)
    unsigned masked[4] = {0u, 0u, 0u, 0u};
    if (p.shift > 0) {
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int idk = 3 * swin_region(8 * wy + 2 * nj + (g >> 1), H) + swin_region(8 * wx + 4 * (g & 1) + r, W);
#pragma unroll
                for (int mi = 0; mi < 4; ++mi) masked[mi] |= (idk != idq[mi] ? 1u : 0u) << (4 * nj + r);
            }
    }
    const long long rv = row_of(lane);                      // V: lane t transposes token t
    half_t* myvt = vt[wave];

    const int iters = (p.heads + 3) >> 2;
    for (int it = 0; it < iters; ++it) {
        const int h = 4 * it + wave;
        const bool act = h < p.heads;                       // wave-uniform
        if (act) {
            const half_t* vs = p.qkv + rv * p.ldq + (2 * p.heads + h) * 32;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const h8 v = *reinterpret_cast<const h8*>(vs + 8 * c);
#pragma unroll
                for (int e = 0; e < 8; ++e) myvt[(8 * c + e) * SWIN_VLD + lane] = v[e];
            }
        }
        __syncthreads();
        if (act) {
            h8 qf[4], kf[4];
            [[maybe_unused]] float iq[4], ik[4], tau = 0.f; // COSINE: head_scale / max(|q|, 1e-12) and 1 / max(|k|, 1e-12) of token 16 j + l16
            if constexpr (COSINE) tau = p.head_scale[h];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const half_t* src = p.qkv + rq[j] * p.ldq + h * 32 + 8 * g;
                qf[j] = *reinterpret_cast<const h8*>(src);
                kf[j] = *reinterpret_cast<const h8*>(src + p.heads * 32);
                if constexpr (COSINE) {
                    float sq = 0.f, sk = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float a = (float)qf[j][e], b = (float)kf[j][e];
                        sq = fmaf(a, a, sq);
                        sk = fmaf(b, b, sk);
                    }
                    sq += __shfl_xor(sq, 16); sk += __shfl_xor(sk, 16);
                    sq += __shfl_xor(sq, 32); sk += __shfl_xor(sk, 32);
                    iq[j] = tau / fmaxf(sqrtf(sq), 1e-12f);
                    ik[j] = 1.0f / fmaxf(sqrtf(sk), 1e-12f);
                }
            }
            f4 s[4][4];                                     // [nj][mi]: keys 16 nj + 4 g + r of query 16 mi + l16
#pragma unroll
            for (int nj = 0; nj < 4; ++nj)
#pragma unroll
                for (int mi = 0; mi < 4; ++mi)
                    s[nj][mi] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[nj], qf[mi], f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            [[maybe_unused]] f4 kn[4];                      // COSINE, [nj][r]: the inverse norm of key 16 nj + 4 g + r, from lane 4 g + r
            if constexpr (COSINE) {
#pragma unroll
                for (int nj = 0; nj < 4; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) kn[nj][r] = __shfl(ik[nj], 4 * g + r);
            }
            const float* bh = p.bias + (long long)h * 4096;
            h8 pf[4][2];                                    // [mi][kk]: the B fragments of O^T = V^T P^T
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) {
                float mx = -3.0e38f;
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) {
                    const f4 bv = *reinterpret_cast<const f4*>(bh + (16 * mi + l16) * 64 + 16 * nj + 4 * g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {                   // the multiplier of the raw score: a constant-folded ternary, evaluated where p.scale was
                        const float v = fmaf((float)((masked[mi] >> (4 * nj + r)) & 1u), -100.0f,
                                             fmaf(s[nj][mi][r], COSINE ? iq[mi] * kn[nj][r] : p.scale, bv[r]));
                        s[nj][mi][r] = v;
                        mx = fmaxf(mx, v);
                    }
                }
                mx = fmaxf(mx, __shfl_xor(mx, 16));
                mx = fmaxf(mx, __shfl_xor(mx, 32));
                float sum = 0.f;
#pragma unroll
                for (int nj = 0; nj < 4; ++nj)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float e = __expf(s[nj][mi][r] - mx);
                        s[nj][mi][r] = e;
                        sum += e;
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[mi][kk][e] = (half_t)(s[2 * kk + (e >> 2)][mi][e & 3] * inv);
            }
            h8 vf[2][2];                                    // [nb][kk]: dims 16 nb + l16, the same permuted key slots
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const half_t* src = myvt + (16 * nb + l16) * SWIN_VLD + 32 * kk + 4 * g;
                    const h4 lo = *reinterpret_cast<const h4*>(src), hi = *reinterpret_cast<const h4*>(src + 16);
                    vf[nb][kk] = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    f4 o = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[nb][kk], pf[mi][kk], o, 0, 0, 0);
                    const int d0 = 16 * nb + 4 * g;         // dims d0 .. d0 + 3 of query 16 mi + l16; the slot's tail D .. 31 is stored as zero
                    h4 ov;
#pragma unroll
                    for (int r = 0; r < 4; ++r) ov[r] = d0 + r < p.D ? (half_t)o[r] : (half_t)0.f;
                    *reinterpret_cast<h4*>(p.out + rq[mi] * p.ldo + h * 32 + d0) = ov;
                }
        }
        __syncthreads();                                    // the next head's V^T goes over this one's
    }
}

int launch_swin_attention(const SwinAttnP& p, hipStream_t s) {
    SDMI_REQUIRE(p.qkv && p.bias && p.out && (!p.cosine || p.head_scale), "null qkv / bias / out / head_scale");
    SDMI_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0 && p.H % 8 == 0 && p.W % 8 == 0, "H and W must be positive multiples of the window size 8");
    SDMI_REQUIRE(p.heads >= 1 && p.heads <= 1024, "heads");
    SDMI_REQUIRE(p.D >= 1 && p.D <= 32, "head dim D must be in 1..32 (one 32-wide slot per head)");
    SDMI_REQUIRE(p.shift == 0 || p.shift == 4, "shift must be 0 or 4 (half a window)");
    SDMI_REQUIRE(p.ldq >= 96 * p.heads, "qkv rows hold 3 x heads slots of 32: ldq >= 96 heads");
    SDMI_REQUIRE(p.ldo >= 32 * p.heads, "out rows hold heads slots of 32: ldo >= 32 heads");
    SDMI_REQUIRE(p.ldq % 8 == 0 && p.ldo % 8 == 0 && ((uintptr_t)p.qkv & 15) == 0 && ((uintptr_t)p.out & 15) == 0 && ((uintptr_t)p.bias & 15) == 0 &&
                     (!p.cosine || ((uintptr_t)p.head_scale & 3) == 0),
                 "misaligned: qkv / out / bias bases on 16 bytes, head_scale on 4, ldq and ldo multiples of 8");
    SDMI_REQUIRE((long long)p.B * p.H * p.W < (1ll << 31) - 256, "B*H*W must stay below 2^31 tokens");
    const long long windows = (long long)p.B * (p.H / 8) * (p.W / 8);
    const double tokens = (double)windows * 64.0;
    ProfScope ps(p.cosine ? "swin2_window_attn" : "swin_window_attn", tokens * p.heads * (2.0 * 64 * 32 * 2), tokens * p.heads * 32 * 2.0 * 4 + (double)windows * p.heads * 16384.0, s);
    if (p.cosine) hipLaunchKernelGGL(swin_window_attn_kernel<true>, dim3((unsigned)windows), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(swin_window_attn_kernel<false>, dim3((unsigned)windows), dim3(256), 0, s, p);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// Row LayerNorm over the first C columns of ld-wide fp16 rows: fp32 statistics, centred variance (mean first, then sum (x - mean)^2).
// Columns C .. Cp - 1 (Cp = C rounded up to 64: the width the MFMA GEMMs read) are written as zeros; the input's own pad columns are
// never used.  A wave per row, three passes over the row (the second and third hit the cache).  A form with 16 lanes per row and the
// row held in registers was measured slower on the MI355X (231 us against 136 us per launch at 262144 x 256), so there is only this one.
__global__ __launch_bounds__(256) void swin_layernorm_kernel(const half_t* x, const float* gamma, const float* beta, half_t* out,
                                                             long long rows, int C, int Cp, int ld, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                // wave-uniform
    const half_t* xr = x + row * ld;
    half_t* orow = out + row * ld;
    float sum = 0.f;
    for (int c = 2 * lane; c < C; c += 128) {
        const h2 v = *reinterpret_cast<const h2*>(xr + c);
        sum += (float)v[0] + (c + 1 < C ? (float)v[1] : 0.f);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    const float mean = sum / (float)C;
    float m2 = 0.f;
    for (int c = 2 * lane; c < C; c += 128) {
        const h2 v = *reinterpret_cast<const h2*>(xr + c);
        const float d0 = (float)v[0] - mean, d1 = c + 1 < C ? (float)v[1] - mean : 0.f;
        m2 += d0 * d0 + d1 * d1;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) m2 += __shfl_xor(m2, m);
    const float rstd = 1.0f / sqrtf(m2 / (float)C + eps);
    for (int c = 2 * lane; c < Cp; c += 128) {
        h2 o = h2{(half_t)0.f, (half_t)0.f};
        if (c < C) {
            const h2 v = *reinterpret_cast<const h2*>(xr + c);
            o[0] = (half_t)(((float)v[0] - mean) * rstd * gamma[c] + beta[c]);
            if (c + 1 < C) o[1] = (half_t)(((float)v[1] - mean) * rstd * gamma[c + 1] + beta[c + 1]);
        }
        *reinterpret_cast<h2*>(orow + c) = o;
    }
}

// res-post-norm: out = resid + LN(y) over the first C columns of ld-wide fp16 rows, fp32 statistics, centred variance, one rounding of
// the fp32 sum.  Columns C .. Cp - 1 of out are written as zeros.  swin_layernorm's form: a wave per row, three passes over y's row.
// out == resid is allowed (a lane reads the two resid values it then writes); y must not be out.
// A kernel of its own, not a template argument of swin_layernorm_kernel: with resid as a last parameter its kernarg load is sunk in front
// of the third pass and waited for once per row, and the network's time on the MI355X fell outside the parent build's run-to-run spread
// (profiles/swin_merge_time.md); with resid here, the plain form's code changes instead.
__global__ __launch_bounds__(256) void swin2_layernorm_add_kernel(const half_t* y, const float* gamma, const float* beta, const half_t* resid,
                                                                  half_t* out, long long rows, int C, int Cp, int ld, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                // wave-uniform
    const half_t* yr = y + row * ld;
    const half_t* rr = resid + row * ld;
    half_t* orow = out + row * ld;
    float sum = 0.f;
    for (int c = 2 * lane; c < C; c += 128) {
        const h2 v = *reinterpret_cast<const h2*>(yr + c);
        sum += (float)v[0] + (c + 1 < C ? (float)v[1] : 0.f);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    const float mean = sum / (float)C;
    float m2 = 0.f;
    for (int c = 2 * lane; c < C; c += 128) {
        const h2 v = *reinterpret_cast<const h2*>(yr + c);
        const float d0 = (float)v[0] - mean, d1 = c + 1 < C ? (float)v[1] - mean : 0.f;
        m2 += d0 * d0 + d1 * d1;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) m2 += __shfl_xor(m2, m);
    const float rstd = 1.0f / sqrtf(m2 / (float)C + eps);
    for (int c = 2 * lane; c < Cp; c += 128) {
        h2 o = h2{(half_t)0.f, (half_t)0.f};
        if (c < C) {
            const h2 v = *reinterpret_cast<const h2*>(yr + c);
            const h2 x = *reinterpret_cast<const h2*>(rr + c);
            o[0] = (half_t)((float)x[0] + (((float)v[0] - mean) * rstd * gamma[c] + beta[c]));
            if (c + 1 < C) o[1] = (half_t)((float)x[1] + (((float)v[1] - mean) * rstd * gamma[c + 1] + beta[c + 1]));
        }
        *reinterpret_cast<h2*>(orow + c) = o;
    }
}

// one body for both forms: resid == nullptr is the plain LayerNorm
static int swin_layernorm_launch(const half_t* x, const float* gamma, const float* beta, const half_t* resid, half_t* out, int64_t rows, int C,
                                 int ld, float eps, hipStream_t s) {
    SDMI_REQUIRE(rows > 0 && C > 0, "empty tensor");
    const int Cp = (C + 63) / 64 * 64;
    SDMI_REQUIRE(ld >= Cp && ld % 2 == 0, "rows must be at least C rounded up to 64 wide (the pad columns are written as zeros)");
    SDMI_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)resid & 3) == 0 && ((uintptr_t)out & 3) == 0, "x / resid / out must be 4-byte aligned");
    SDMI_REQUIRE(rows * (int64_t)ld < (1ll << 40), "tensor too large");
    const dim3 grid((unsigned)((rows + 3) / 4));
    ProfScope ps(resid ? "swin2_layernorm_add" : "swin_layernorm", (resid ? 9.0 : 8.0) * rows * C, (resid ? 6.0 : 4.0) * rows * C, s);
    if (resid) hipLaunchKernelGGL(swin2_layernorm_add_kernel, grid, dim3(256), 0, s, x, gamma, beta, resid, out, (long long)rows, C, Cp, ld, eps);
    else hipLaunchKernelGGL(swin_layernorm_kernel, grid, dim3(256), 0, s, x, gamma, beta, out, (long long)rows, C, Cp, ld, eps);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_swin_layernorm(const half_t* x, const float* gamma, const float* beta, half_t* out, int64_t rows, int C, int ld, float eps,
                          hipStream_t s) {
    SDMI_REQUIRE(x && gamma && beta && out, "null argument");
    return swin_layernorm_launch(x, gamma, beta, nullptr, out, rows, C, ld, eps, s);
}

int launch_swin2_layernorm_add(const half_t* y, const float* gamma, const float* beta, const half_t* resid, half_t* out, int64_t rows, int C,
                               int ld, float eps, hipStream_t s) {
    SDMI_REQUIRE(y && gamma && beta && resid && out, "null argument");
    SDMI_REQUIRE(y != out, "y must not be the output (resid may be)");
    return swin_layernorm_launch(y, gamma, beta, resid, out, rows, C, ld, eps, s);
}

// The network's input: RGB as uint8 HWC (/ 255) or fp32 NCHW -> reflect-padded right / bottom to Hp x Wp (F.pad(..., 'reflect'):
// row H + k is row H - 2 - k), minus the dataset mean -> NHWC fp16 rows of cpad channels, zero padded.
__global__ __launch_bounds__(256) void swin_input_kernel(const void* in, int u8, half_t* out, int H, int W, int Hp, int Wp, int cpad, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % cpad);
        const long long pix = i / cpad;
        const int x = (int)(pix % Wp), y = (int)((pix / Wp) % Hp);
        const long long b = pix / ((long long)Wp * Hp);
        float v = 0.f;
        if (ch < 3) {
            const int sy = y < H ? y : 2 * H - 2 - y, sx = x < W ? x : 2 * W - 2 - x;
            v = u8 ? (float)reinterpret_cast<const uint8_t*>(in)[((b * H + sy) * W + sx) * 3 + ch] / 255.f
                   : reinterpret_cast<const float*>(in)[((b * 3 + ch) * H + sy) * W + sx];
            v -= ch == 0 ? 0.4488f : (ch == 1 ? 0.4371f : 0.4040f);
        }
        out[i] = (half_t)v;
    }
}
int launch_swin_input(const void* in, int u8, half_t* out, int B, int H, int W, int Hp, int Wp, int cpad, hipStream_t s) {
    SDMI_REQUIRE(in && out && B > 0 && cpad >= 3, "null / empty input");
    SDMI_REQUIRE(Hp >= H && Wp >= W && Hp - H < H && Wp - W < W, "reflect padding must be smaller than the side it pads");
    const long long n = (long long)B * Hp * Wp * cpad;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    ProfScope ps("swin_input", 0.0, 2.0 * n, s);
    hipLaunchKernelGGL(swin_input_kernel, dim3(grid), dim3(256), 0, s, in, u8, out, H, W, Hp, Wp, cpad, n);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// LeakyReLU in place, for the convs that run as GEMMs (0.2 inside the 3conv residual connection, 0.01 after conv_before_upsample)
__global__ __launch_bounds__(256) void swin_lrelu_kernel(half_t* x, long long n8, float slope) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        h8 v = *reinterpret_cast<h8*>(x + 8 * i);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
            v[e] = (half_t)(f > 0.f ? f : slope * f);
        }
        *reinterpret_cast<h8*>(x + 8 * i) = v;
    }
}
int launch_swin_lrelu(half_t* x, int64_t n, float slope, hipStream_t s) {
    SDMI_REQUIRE(x && n > 0 && n % 8 == 0 && ((uintptr_t)x & 15) == 0, "LeakyReLU pass: 16-byte aligned, a multiple of 8 elements");
    const unsigned grid = (unsigned)std::min<long long>((n / 8 + 255) / 256, 65536);
    ProfScope ps("swin_lrelu", (double)n, 4.0 * n, s);
    hipLaunchKernelGGL(swin_lrelu_kernel, dim3(grid), dim3(256), 0, s, x, (long long)(n / 8), slope);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// The network's output: fp32 [B][3][Hp][Wp] (the padded grid) cropped to [H][W] -> fp32 NCHW, or uint8 HWC = round_half_even(clamp(y, 0, 1) * 255)
__global__ __launch_bounds__(256) void swin_output_kernel(const float* src, void* out, int u8, int H, int W, int Hp, int Wp, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int c, x, y;
        long long b;
        if (u8) {
            c = (int)(i % 3); x = (int)((i / 3) % W); y = (int)((i / (3ll * W)) % H); b = i / (3ll * W * H);
        } else {
            x = (int)(i % W); y = (int)((i / W) % H); c = (int)((i / ((long long)W * H)) % 3); b = i / (3ll * W * H);
        }
        const float v = src[((b * 3 + c) * Hp + y) * Wp + x];
        if (u8) reinterpret_cast<uint8_t*>(out)[i] = (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
        else reinterpret_cast<float*>(out)[i] = v;
    }
}
int launch_swin_output(const float* src, void* out, int out_u8, int B, int H, int W, int Hp, int Wp, hipStream_t s) {
    SDMI_REQUIRE(src && out && B > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W, "null / empty output");
    const long long n = (long long)B * 3 * H * W;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    ProfScope ps("swin_output", 0.0, (out_u8 ? 5.0 : 8.0) * n, s);
    hipLaunchKernelGGL(swin_output_kernel, dim3(grid), dim3(256), 0, s, src, out, out_u8, H, W, Hp, Wp, n);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// PixelShuffle(f) of a 64-channel tensor whose producing conv was packed with its output channels in (i, j, c) order: src rows
// [B*H*W][f*f*64] -> dst [B][H f][W f][64]; the 128 bytes of sub-pixel (i, j) of pixel (y, x) go to pixel (y f + i, x f + j).  A thread
// per 16 bytes, the reads contiguous.
__global__ __launch_bounds__(256) void swin2_pixel_shuffle_kernel(const half_t* src, half_t* dst, int H, int W, int f, long long n8) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const int c8 = (int)(i & 7);
        const int sub = (int)((i >> 3) % (f * f));
        const long long pix = (i >> 3) / (f * f);
        const int x = (int)(pix % W), y = (int)((pix / W) % H);
        const long long b = pix / ((long long)W * H);
        const long long row = (b * H * f + (long long)y * f + sub / f) * ((long long)W * f) + (long long)x * f + sub % f;
        *reinterpret_cast<h8*>(dst + row * 64 + 8 * c8) = *reinterpret_cast<const h8*>(src + 8 * i);
    }
}
int launch_swin2_pixel_shuffle(const half_t* src, half_t* dst, int B, int H, int W, int f, hipStream_t s) {
    SDMI_REQUIRE(src && dst && src != dst && B > 0 && H > 0 && W > 0 && (f == 2 || f == 3), "pixel shuffle: null / empty tensor, or a factor other than 2 | 3");
    SDMI_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0, "pixel shuffle: 16-byte aligned tensors");
    const long long n8 = (long long)B * H * W * f * f * 8;
    SDMI_REQUIRE(n8 * 8 < (1ll << 40), "tensor too large");
    const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 65536);
    ProfScope ps("swin2_pixel_shuffle", 0.0, 32.0 * n8, s);
    hipLaunchKernelGGL(swin2_pixel_shuffle_kernel, dim3(grid), dim3(256), 0, s, src, dst, H, W, f, n8);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// The output pass of the `pixelshuffledirect` tail: src fp16 rows [B*Hp*Wp][ld] whose columns c f^2 + i f + j are nn.PixelShuffle(f)'s
// input channels -> + mean, cropped to [H f][W f] -> fp32 NCHW, or uint8 HWC = round_half_even(clamp(y, 0, 1) * 255)
__global__ __launch_bounds__(256) void swin2_output_shuffle_kernel(const half_t* src, void* out, int u8, int H, int W, int Hp, int Wp, int f, int ld,
                                                                   long long n) {
    const int Ho = H * f, Wo = W * f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        int c, x, y;
        long long b;
        if (u8) {
            c = (int)(i % 3); x = (int)((i / 3) % Wo); y = (int)((i / (3ll * Wo)) % Ho); b = i / (3ll * Wo * Ho);
        } else {
            x = (int)(i % Wo); y = (int)((i / Wo) % Ho); c = (int)((i / ((long long)Wo * Ho)) % 3); b = i / (3ll * Wo * Ho);
        }
        const float v = (float)src[((b * Hp + y / f) * Wp + x / f) * ld + c * f * f + (y % f) * f + x % f] +
                        (c == 0 ? 0.4488f : (c == 1 ? 0.4371f : 0.4040f));
        if (u8) reinterpret_cast<uint8_t*>(out)[i] = (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.f);
        else reinterpret_cast<float*>(out)[i] = v;
    }
}
int launch_swin2_output_shuffle(const half_t* src, void* out, int out_u8, int B, int H, int W, int Hp, int Wp, int f, int ld, hipStream_t s) {
    SDMI_REQUIRE(src && out && B > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W, "null / empty output");
    SDMI_REQUIRE(f >= 2 && f <= 4 && ld >= 3 * f * f, "output shuffle: factor 2..4, rows of at least 3 f^2 channels");
    const long long n = (long long)B * 3 * H * f * W * f;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    ProfScope ps("swin2_output_shuffle", 0.0, (out_u8 ? 3.0 : 6.0) * n, s);
    hipLaunchKernelGGL(swin2_output_shuffle_kernel, dim3(grid), dim3(256), 0, s, src, out, out_u8, H, W, Hp, Wp, f, ld, n);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
