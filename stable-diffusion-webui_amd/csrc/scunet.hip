// scunet.hip — the kernels of the ScuNET denoisers / upscalers (Zhang et al., "Practical Blind Denoising via Swin-Conv-UNet and Data
// Synthesis", network_scunet.py) that the rest of the library has no form of, for gfx950: the transformer `Block` of a ConvTransBlock at
// the two narrow levels (trans_dim 32 and 64), whole, one 8 x 8 window at a time; and, at the end of the file, the network's input pass,
// the 2 x 2 regrouping around its stride-2 / transposed convs and the skip sum.  Everything else of the network runs on gemm.hip,
// rrdb.hip and swinir.hip (engine.cpp scunet_pass); the cropped fp32 / uint8 output is swinir.hip's swin_output as it is.
//
// scu_block_kernel<C>: a workgroup (4 waves) computes, for the 64 tokens of one window,
//     x1 = x + linear(softmax(q k^T / sqrt(32) + bias + mask) v),   q, k, v = embedding_layer(LN1(x))
//     y  = x1 + fc2(GELU(fc1(LN2(x1))))
// and reads / writes nothing but those 64 token rows (C fp16 each): both window types partition the image into disjoint windows and
// everything but the attention is per token.  The cyclic shift of the 'SW' blocks is index arithmetic as in swin_window_attn (token a of
// window (wy, wx) lives in row ((8 wy + a / 8 + shift) % H, (8 wx + a % 8 + shift) % W) and is written back there), the mask is computed:
// in the last row of windows pairs with (ya < 4) != (yb < 4) are -inf, in the last column pairs with (xa < 4) != (xb < 4).
//
// Every product is v_mfma_f32_16x16x32_f16 with swapped operands (weights / keys / V^T as A, tokens as B): a lane ends up with 4
// consecutive features of ONE token, so epilogues are 8-byte LDS / global accesses and the result, written token-major, is the next
// product's B operand as it lies.  The four matrices (24 KB fp16 at C = 32, 96 KB at C = 64) are staged into LDS ONCE per workgroup and the
// workgroups walk the windows with a grid stride (2 workgroups per CU fit at C = 32, 1 at C = 64: 56 KB / 156 KB of the 160 KB); rows are
// padded by 8 halfs so the 16 rows a quarter-wave reads with ds_read_b128 fall into distinct banks.  The 13 C fp32 norm / bias
// parameters and the relative-position bias [heads][64][64] are read from global memory (L1 / L2 hits).
// Work split: a product with NB 16-feature blocks is 2 NB units (block, half of the 64 tokens) dealt round-robin to the waves (a weight
// fragment is read once per two MFMAs); the attention gives wave w the queries 16 w .. 16 w + 15 of every head.  S^T = K Q^T is computed
// transposed as in swin_window_attn: a query's softmax is a reduction over a lane's 16 values and two shuffles, and the probabilities
// are, as they lie, the B fragment of O^T = V^T P^T; V is written transposed by the qkv epilogue.
// LN statistics (centred variance), scores, softmax, GELU and both residual sums are fp32; the normalised rows, q / k / v, the
// probabilities, x1 and the hidden layer are rounded to fp16 in LDS and never reach HBM.
#include "common.h"
#include "prof.h"

#include <algorithm>

namespace sdmi {

namespace {
// byte offsets of the packed weights (= their LDS image) and of the activation buffers behind them
template <int C> struct ScuL {
    static constexpr int KS = C + 8;                    // row stride (halfs) of [.][C] matrices and token buffers
    static constexpr int HS = 4 * C + 8;                // ... of fc2's weight and the hidden layer
    static constexpr int QS = 2 * C + 8;                // ... of the q | k token buffer
    static constexpr int VS = 72;                       // ... of V^T [C][64 tokens]
    static constexpr int WQKV = 0, WPROJ = WQKV + 3 * C * KS * 2, W1 = WPROJ + C * KS * 2, W2 = W1 + 4 * C * KS * 2;
    static constexpr int WEND = W2 + C * HS * 2;        // the fp32 parameters follow in the pack (not staged)
    static constexpr int XS = WEND, XN = XS + 64 * KS * 2, U = XN + 64 * KS * 2;      // x / x1, LN output / attention output, union:
    static constexpr int QK = U, VT = QK + 64 * QS * 2;                                // q | k and V^T, later
    static constexpr int HID = U;                                                      // the hidden layer
    static constexpr int UEND = (VT + C * VS * 2 > HID + 64 * HS * 2) ? VT + C * VS * 2 : HID + 64 * HS * 2;
    static constexpr int LDS = UEND;
    // fp32 parameters (float index behind WEND)
    static constexpr int G1 = 0, B1N = C, BQKV = 2 * C, BPROJ = 5 * C, G2 = 6 * C, B2N = 7 * C, BFC1 = 8 * C, BFC2 = 12 * C, NF = 13 * C;
    static constexpr int PACK = WEND + NF * 4;
};
static_assert(ScuL<64>::LDS <= 160 * 1024 && 2 * ScuL<32>::LDS <= 160 * 1024, "LDS budget of a gfx950 CU");

__device__ __forceinline__ float scu_gelu_erf(float g) {      // gemm.hip's gelu_erf (exact-erf GELU, A&S 7.1.26)
    const float x = fabsf(g) * 0.70710678118654752f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, x, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(x * x * -1.4426950408889634f);
    const float erf_v = copysignf(fmaf(-(poly * t), e, 1.0f), g);
    const float hg = 0.5f * g;
    return fmaf(hg, erf_v, hg);
}

// D[n][token] = sum_k w[n][k] x[token][k] for NB 16-row blocks of w (row stride WS) and the 64 token rows of x (stride XSD); ep(n0, token,
// acc) receives features n0 .. n0 + 3 of one token
template <int K, int NB, int WS, int XSD, typename Ep>
__device__ __forceinline__ void scu_gemm(const half_t* w, const half_t* x, int wave, int l16, int g, Ep ep) {
    for (int u = wave; u < 2 * NB; u += 4) {
        const int j = u >> 1, th = u & 1;
        f4 acc[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kk = 0; kk < K / 32; ++kk) {
            const h8 a = *reinterpret_cast<const h8*>(w + (16 * j + l16) * WS + 32 * kk + 8 * g);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const h8 b = *reinterpret_cast<const h8*>(x + (16 * (2 * th + t) + l16) * XSD + 32 * kk + 8 * g);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) ep(16 * j + 4 * g, 16 * (2 * th + t) + l16, acc[t]);
    }
}

// LayerNorm of the 64 rows of xs into xn: 4 threads per token, C / 4 columns each
template <int C>
__device__ __forceinline__ void scu_layernorm(const half_t* xs, half_t* xn, const float* gamma, const float* beta, int tid) {
    constexpr int KS = ScuL<C>::KS, PER = C / 4;
    const int a = tid >> 2, c0 = (tid & 3) * PER;
    float v[PER];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < PER; i += 8) {
        const h8 t = *reinterpret_cast<const h8*>(xs + a * KS + c0 + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[i + e] = (float)t[e]; sum += v[i + e]; }
    }
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    const float mean = sum * (1.0f / C);
    float m2 = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { v[i] -= mean; m2 += v[i] * v[i]; }
    m2 += __shfl_xor(m2, 1);
    m2 += __shfl_xor(m2, 2);
    const float rstd = 1.0f / sqrtf(m2 * (1.0f / C) + 1e-5f);
#pragma unroll
    for (int i = 0; i < PER; i += 8) {
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (half_t)(v[i + e] * rstd * gamma[c0 + i + e] + beta[c0 + i + e]);
        *reinterpret_cast<h8*>(xn + a * KS + c0 + i) = o;
    }
}
}  // namespace

template <int C>
__global__ __launch_bounds__(256) void scu_block_kernel(const ScuBlockP p) {
    using L = ScuL<C>;
    constexpr int NH = C / 32, KS = L::KS, HS = L::HS, QS = L::QS, VS = L::VS;
#ifdef __HIP__
    extern __shared__ __attribute__((aligned(16))) char smem[];
#else
    __shared__ __attribute__((aligned(16))) char smem[L::LDS];
#endif
    const half_t* wqkv = reinterpret_cast<const half_t*>(smem + L::WQKV);
    const half_t* wproj = reinterpret_cast<const half_t*>(smem + L::WPROJ);
    const half_t* w1 = reinterpret_cast<const half_t*>(smem + L::W1);
    const half_t* w2 = reinterpret_cast<const half_t*>(smem + L::W2);
    half_t* xs = reinterpret_cast<half_t*>(smem + L::XS);
    half_t* xn = reinterpret_cast<half_t*>(smem + L::XN);
    half_t* qk = reinterpret_cast<half_t*>(smem + L::QK);
    half_t* vt = reinterpret_cast<half_t*>(smem + L::VT);
    half_t* hid = reinterpret_cast<half_t*>(smem + L::HID);
    const float* fp = reinterpret_cast<const float*>(reinterpret_cast<const char*>(p.packs) + L::WEND);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    const int H = p.H, W = p.W, nwx = W >> 3, nwy = H >> 3;

    for (int i = tid; i < L::WEND / 16; i += 256)
        *reinterpret_cast<h8*>(smem + 16 * i) = *reinterpret_cast<const h8*>(reinterpret_cast<const char*>(p.packs) + 16 * i);
    // (the first barrier of the window loop publishes the weights)

    for (long long win = blockIdx.x; win < p.windows; win += gridDim.x) {
        const int wx = (int)(win % nwx), wy = (int)((win / nwx) % nwy);
        const long long img = (win / ((long long)nwx * nwy)) * H * W;
        auto row_of = [&](int a) -> long long {
            int y = 8 * wy + (a >> 3) + p.shift, x = 8 * wx + (a & 7) + p.shift;
            if (y >= H) y -= H;
            if (x >= W) x -= W;
            return img + (long long)y * W + x;
        };
        // the window's 64 rows -> xs (every load of the window happens here, before its first store: out may alias x)
        {
            constexpr int PER = C / 4;
            const int a = tid >> 2, c0 = (tid & 3) * PER;
            const half_t* src = p.x + row_of(a) * p.ldx + c0;
#pragma unroll
            for (int i = 0; i < PER; i += 8) *reinterpret_cast<h8*>(xs + a * KS + c0 + i) = *reinterpret_cast<const h8*>(src + i);
        }
        scu_layernorm<C>(xs, xn, fp + L::G1, fp + L::B1N, tid);       // a thread normalises what it loaded itself
        __syncthreads();

        // q | k token-major, V transposed
        scu_gemm<C, 3 * C / 16, KS, KS>(wqkv, xn, wave, l16, g, [&](int n0, int tok, const f4& acc) {
            const f4 bv = *reinterpret_cast<const f4*>(fp + L::BQKV + n0);
            if (n0 < 2 * C) {
                *reinterpret_cast<h4*>(qk + tok * QS + n0) =
                    h4{(half_t)(acc[0] + bv[0]), (half_t)(acc[1] + bv[1]), (half_t)(acc[2] + bv[2]), (half_t)(acc[3] + bv[3])};
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) vt[(n0 - 2 * C + r) * VS + tok] = (half_t)(acc[r] + bv[r]);
            }
        });
        __syncthreads();

        // attention: wave w owns queries 16 w + l16 of every head; keys 16 nj + 4 g + r
        {
            const int a = 16 * wave + l16;
            const bool qy = (a >> 3) < 4, qx = (a & 7) < 4;
            const bool my = p.shift > 0 && wy == nwy - 1, mx_ = p.shift > 0 && wx == nwx - 1;
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const h8 qf = *reinterpret_cast<const h8*>(qk + a * QS + h * 32 + 8 * g);
                f4 s[4];
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) {
                    const h8 kf = *reinterpret_cast<const h8*>(qk + (16 * nj + l16) * QS + C + h * 32 + 8 * g);
                    s[nj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                }
                const float* bh = p.bias + h * 4096 + a * 64;
                float mx = -3.0e38f;
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) {
                    const f4 bv = *reinterpret_cast<const f4*>(bh + 16 * nj + 4 * g);
                    const bool ky = (2 * nj + (g >> 1)) < 4, kx = (g & 1) == 0;      // key (y, x) = (2 nj + g / 2, 4 (g % 2) + r)
                    const bool masked = (my && ky != qy) || (mx_ && kx != qx);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = masked ? -INFINITY : fmaf(s[nj][r], 0.17677669529663689f, bv[r]);
                        s[nj][r] = v;
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
                        const float e = __expf(s[nj][r] - mx);
                        s[nj][r] = e;
                        sum += e;
                    }
                sum += __shfl_xor(sum, 16);
                sum += __shfl_xor(sum, 32);
                const float inv = 1.0f / sum;
                h8 pf[2];                                   // k slot 8 g + e of step kk = key 16 (2 kk + e / 4) + 4 g + e % 4, on both operands
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int e = 0; e < 8; ++e) pf[kk][e] = (half_t)(s[2 * kk + (e >> 2)][e & 3] * inv);
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    f4 o = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        const half_t* src = vt + (h * 32 + 16 * nb + l16) * VS + 32 * kk + 4 * g;
                        const h4 lo = *reinterpret_cast<const h4*>(src), hi = *reinterpret_cast<const h4*>(src + 16);
                        o = __builtin_amdgcn_mfma_f32_16x16x32_f16(h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}, pf[kk], o, 0, 0, 0);
                    }
                    // xn is free: the qkv product, its only reader, finished before the last barrier
                    *reinterpret_cast<h4*>(xn + a * KS + h * 32 + 16 * nb + 4 * g) = h4{(half_t)o[0], (half_t)o[1], (half_t)o[2], (half_t)o[3]};
                }
            }
        }
        __syncthreads();

        // x1 = x + linear(attention), in place in xs (an element belongs to one lane)
        scu_gemm<C, C / 16, KS, KS>(wproj, xn, wave, l16, g, [&](int n0, int tok, const f4& acc) {
            const f4 bv = *reinterpret_cast<const f4*>(fp + L::BPROJ + n0);
            half_t* xr = xs + tok * KS + n0;
            const h4 r = *reinterpret_cast<const h4*>(xr);
            *reinterpret_cast<h4*>(xr) = h4{(half_t)((float)r[0] + acc[0] + bv[0]), (half_t)((float)r[1] + acc[1] + bv[1]),
                                            (half_t)((float)r[2] + acc[2] + bv[2]), (half_t)((float)r[3] + acc[3] + bv[3])};
        });
        __syncthreads();
        scu_layernorm<C>(xs, xn, fp + L::G2, fp + L::B2N, tid);
        __syncthreads();

        scu_gemm<C, 4 * C / 16, KS, KS>(w1, xn, wave, l16, g, [&](int n0, int tok, const f4& acc) {
            const f4 bv = *reinterpret_cast<const f4*>(fp + L::BFC1 + n0);
            *reinterpret_cast<h4*>(hid + tok * HS + n0) = h4{(half_t)scu_gelu_erf(acc[0] + bv[0]), (half_t)scu_gelu_erf(acc[1] + bv[1]),
                                                             (half_t)scu_gelu_erf(acc[2] + bv[2]), (half_t)scu_gelu_erf(acc[3] + bv[3])};
        });
        __syncthreads();

        scu_gemm<4 * C, C / 16, HS, HS>(w2, hid, wave, l16, g, [&](int n0, int tok, const f4& acc) {
            const f4 bv = *reinterpret_cast<const f4*>(fp + L::BFC2 + n0);
            const h4 r = *reinterpret_cast<const h4*>(xs + tok * KS + n0);
            *reinterpret_cast<h4*>(p.out + row_of(tok) * p.ldo + n0) =
                h4{(half_t)((float)r[0] + acc[0] + bv[0]), (half_t)((float)r[1] + acc[1] + bv[1]), (half_t)((float)r[2] + acc[2] + bv[2]),
                   (half_t)((float)r[3] + acc[3] + bv[3])};
        });
        __syncthreads();                                    // the next window's rows go over xs, its q | k over the hidden layer
    }
}

size_t scu_block_pack_bytes(int C) { return C == 32 ? (size_t)ScuL<32>::PACK : C == 64 ? (size_t)ScuL<64>::PACK : 0; }

// torch-order fp16 matrices and fp32 vectors -> the pack: padded rows (the pad columns zero), then the 13 C floats
template <int C>
__global__ __launch_bounds__(256) void scu_block_pack_kernel(const ScuPackP p) {
    using L = ScuL<C>;
    half_t* hw = reinterpret_cast<half_t*>(p.packs);
    float* fw = reinterpret_cast<float*>(reinterpret_cast<char*>(p.packs) + L::WEND);
    const int nthreads = (int)gridDim.x * 256, t0 = (int)blockIdx.x * 256 + (int)threadIdx.x;
    auto matrix = [&](const half_t* src, int off, int rows, int cols, int stride) {
        for (int i = t0; i < rows * stride; i += nthreads) {
            const int r = i / stride, c = i - r * stride;
            hw[off / 2 + i] = c < cols ? src[r * cols + c] : (half_t)0.f;
        }
    };
    matrix(p.wqkv, L::WQKV, 3 * C, C, L::KS);
    matrix(p.wproj, L::WPROJ, C, C, L::KS);
    matrix(p.w1, L::W1, 4 * C, C, L::KS);
    matrix(p.w2, L::W2, C, 4 * C, L::HS);
    auto vec = [&](const float* src, int off, int n) {
        for (int i = t0; i < n; i += nthreads) fw[off + i] = src[i];
    };
    vec(p.ln1_g, L::G1, C); vec(p.ln1_b, L::B1N, C); vec(p.bqkv, L::BQKV, 3 * C); vec(p.bproj, L::BPROJ, C);
    vec(p.ln2_g, L::G2, C); vec(p.ln2_b, L::B2N, C); vec(p.b1, L::BFC1, 4 * C); vec(p.b2, L::BFC2, C);
}

int launch_scu_block_pack(const ScuPackP& p, int C, hipStream_t s) {
    SDMI_REQUIRE(C == 32 || C == 64, "scu_block is built for trans_dim 32 and 64");
    SDMI_REQUIRE(p.ln1_g && p.ln1_b && p.wqkv && p.bqkv && p.wproj && p.bproj && p.ln2_g && p.ln2_b && p.w1 && p.b1 && p.w2 && p.b2 && p.packs,
                 "null argument");
    SDMI_REQUIRE(((uintptr_t)p.packs & 15) == 0, "packs must be 16-byte aligned");
    if (C == 32) hipLaunchKernelGGL(scu_block_pack_kernel<32>, dim3(32), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(scu_block_pack_kernel<64>, dim3(32), dim3(256), 0, s, p);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

template <int C>
static int scu_block_go(const ScuBlockP& p, unsigned grid, hipStream_t s) {
    auto kern = scu_block_kernel<C>;
#ifdef __HIP__
    static PerDeviceOnce attr;
    if (attr.need()) SDMI_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, ScuL<C>::LDS));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), ScuL<C>::LDS, s, p);
#else
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, s, p);
#endif
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_scu_block(const ScuBlockP& pin, int C, hipStream_t s) {
    ScuBlockP p = pin;
    SDMI_REQUIRE(p.x && p.out && p.packs && p.bias, "null x / out / packs / bias");
    SDMI_REQUIRE(C == 32 || C == 64, "scu_block is built for trans_dim C = 32 (1 head) and 64 (2 heads)");
    SDMI_REQUIRE(p.shift == 0 || p.shift == 4, "shift must be 0 ('W') or 4 ('SW': half a window)");
    SDMI_REQUIRE(p.B > 0 && p.H > 0 && p.W > 0 && p.H % 8 == 0 && p.W % 8 == 0, "H and W must be positive multiples of the window size 8");
    SDMI_REQUIRE(p.ldx >= C && p.ldo >= C, "row strides too small: ldx and ldo must be at least C");
    SDMI_REQUIRE(p.ldx % 8 == 0 && p.ldo % 8 == 0 && ((uintptr_t)p.x & 15) == 0 && ((uintptr_t)p.out & 15) == 0 &&
                     ((uintptr_t)p.packs & 15) == 0 && ((uintptr_t)p.bias & 15) == 0,
                 "misaligned: x / out / packs / bias bases on 16 bytes, ldx and ldo multiples of 8");
    SDMI_REQUIRE((long long)p.B * p.H * p.W < (1ll << 31) - 256, "B*H*W must stay below 2^31 tokens");
    p.windows = (long long)p.B * (p.H / 8) * (p.W / 8);
    // a workgroup stages the weights once and walks windows: as many workgroups as the 256 CUs hold at once
    const unsigned grid = (unsigned)std::min<long long>(p.windows, C == 32 ? 512 : 256);
    const double tokens = (double)p.windows * 64.0;
    ProfScope ps(C == 32 ? "scu_block32" : "scu_block64", tokens * (24.0 * C * C + 4.0 * 64 * C), tokens * C * 4.0 + (double)p.windows * (C / 32) * 16384.0, s);
    return C == 32 ? scu_block_go<32>(p, grid, s) : scu_block_go<64>(p, grid, s);
}

// ---- the data-movement passes of the network that nothing else covers ----------------------------------------------------------------

// The network's input: RGB as uint8 HWC (/ 255) or fp32 NCHW -> padded right / bottom to Hp x Wp by replication
// (nn.ReplicationPad2d((0, padR, 0, padB)): row H + k is row H - 1) -> NHWC fp16 rows of cpad channels, zero padded.
__global__ __launch_bounds__(256) void scu_input_kernel(const void* in, int u8, half_t* out, int H, int W, int Hp, int Wp, int cpad, long long n) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int ch = (int)(i % cpad);
        const long long pix = i / cpad;
        const int x = (int)(pix % Wp), y = (int)((pix / Wp) % Hp);
        const long long b = pix / ((long long)Wp * Hp);
        float v = 0.f;
        if (ch < 3) {
            const int sy = y < H ? y : H - 1, sx = x < W ? x : W - 1;
            v = u8 ? (float)reinterpret_cast<const uint8_t*>(in)[((b * H + sy) * W + sx) * 3 + ch] / 255.f
                   : reinterpret_cast<const float*>(in)[((b * 3 + ch) * H + sy) * W + sx];
        }
        out[i] = (half_t)v;
    }
}
int launch_scu_input(const void* in, int u8, half_t* out, int B, int H, int W, int Hp, int Wp, int cpad, hipStream_t s) {
    SDMI_REQUIRE(in && out && B > 0 && H > 0 && W > 0 && cpad >= 3, "null / empty input");
    SDMI_REQUIRE(Hp >= H && Wp >= W, "the padded grid cannot be smaller than the image");
    const long long n = (long long)B * Hp * Wp * cpad;
    const unsigned grid = (unsigned)std::min<long long>((n + 255) / 256, 65536);
    ProfScope ps("scu_input", 0.0, 2.0 * n, s);
    hipLaunchKernelGGL(scu_input_kernel, dim3(grid), dim3(256), 0, s, in, u8, out, H, W, Hp, Wp, cpad, n);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// 16-byte pieces between hi [B][2h][2w][C] and lo [B][h][w][4][C]; i walks lo
__global__ __launch_bounds__(256) void scu_patch2_kernel(const half_t* src, half_t* dst, int h, int w, int c8, int to_lo, long long n8) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % c8), slot = (int)((i / c8) & 3);
        const long long pix = i / (4ll * c8);
        const int x = (int)(pix % w), y = (int)((pix / w) % h);
        const long long b = pix / ((long long)w * h);
        const long long hi = (((b * 2 * h + 2 * y + (slot >> 1)) * 2 * w + 2 * x + (slot & 1)) * c8 + c) * 8;
        if (to_lo) *reinterpret_cast<h8*>(dst + 8 * i) = *reinterpret_cast<const h8*>(src + hi);
        else *reinterpret_cast<h8*>(dst + hi) = *reinterpret_cast<const h8*>(src + 8 * i);
    }
}
int launch_scu_patch2(const half_t* src, half_t* dst, int B, int h, int w, int C, int to_lo, hipStream_t s) {
    SDMI_REQUIRE(src && dst && B > 0 && h > 0 && w > 0 && C > 0 && C % 8 == 0, "2 x 2 regrouping: channels in 16-byte pieces");
    SDMI_REQUIRE((((uintptr_t)src | (uintptr_t)dst) & 15) == 0, "2 x 2 regrouping: 16-byte aligned tensors");
    const long long n8 = (long long)B * h * w * 4 * (C / 8);
    const unsigned grid = (unsigned)std::min<long long>((n8 + 255) / 256, 65536);
    ProfScope ps(to_lo ? "scu_gather2" : "scu_scatter2", 0.0, 32.0 * n8, s);
    hipLaunchKernelGGL(scu_patch2_kernel, dim3(grid), dim3(256), 0, s, src, dst, h, w, C / 8, to_lo, n8);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void scu_add_kernel(half_t* x, const half_t* y, long long n8) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        h8 a = *reinterpret_cast<h8*>(x + 8 * i);
        const h8 b = *reinterpret_cast<const h8*>(y + 8 * i);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = (half_t)((float)a[e] + (float)b[e]);
        *reinterpret_cast<h8*>(x + 8 * i) = a;
    }
}
int launch_scu_add(half_t* x, const half_t* y, int64_t n, hipStream_t s) {
    SDMI_REQUIRE(x && y && n > 0 && n % 8 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0, "skip add: 16-byte aligned, a multiple of 8 elements");
    const unsigned grid = (unsigned)std::min<long long>((n / 8 + 255) / 256, 65536);
    ProfScope ps("scu_add", (double)n, 6.0 * n, s);
    hipLaunchKernelGGL(scu_add_kernel, dim3(grid), dim3(256), 0, s, x, y, (long long)(n / 8));
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
