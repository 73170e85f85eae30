// norm.hip — GroupNorm(+SiLU) and LayerNorm on NHWC fp16 activations for gfx950; statistics in fp32.
//
// GroupNorm replaces ldm's GroupNorm32 (fp32 compute, /root/reference/modules/devices.py:284-295) followed by SiLU
// (/root/reference/modules/sd_hijack.py:69), and — by reading TWO channel-concatenated sources and writing one tensor —
// the torch.cat of UNet skip connections (/root/reference/modules/sd_hijack_unet.py:10-33).  Both kernels are HBM-bound:
// every access is a 16-byte (8 x fp16) vector, rows are read fully coalesced, and the statistics pass writes only
// per-(image, chunk, group) partial statistics (no atomics => bit-reproducible).
//   pass 1  gn_stats : grid (chunks, B); a block owns `rows` pixels x all channels; thread t keeps per-channel
//                      sum / sum-of-squares of its 8-channel vector in registers, stores them in its own LDS slot
//                      (one writer per slot), then 8 lanes per group reduce its channels in a fixed order
//                      -> partial[b][chunk][g] = (mean, M2) of the chunk's elements of the group, M2 = sum (x - mean)^2
//   pass 2  gn_apply : grid (blocks, B); prologue merges the chunks' (mean, M2) in chunk order (Chan et al.: the element count
//                      of a chunk follows from the geometry) to mean / rstd per group in LDS, then a
//                      grid-stride elementwise pass y = silu((x - mean) * rstd * gamma + beta).
// No pass forms sum(x^2) / n - mean^2: that difference loses (mean / std)^2 of the fp32 mantissa, 1e-2 of the output at a group
// whose mean is 300 standard deviations.  Every sum of squares is taken around a value of the data itself.
// LayerNorm: one wave per token row, row held in registers, two-pass (mean, then centred variance) in fp32.
#include "common.h"
#include "prof.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace sdmi {

static constexpr int GN_MAX_C = 4096;

// HILO (engine option "residual_fp32"): the input is the carried stream kept as a (hi, lo) pair of fp16 tensors — x = hi + lo with
// hi = fp16(x), lo = fp16(x - hi), ~22 bits of x — and the statistics / normalisation are taken from the sum.  l0 / l1: the lo parts.
template <bool HILO = false>
__global__ __launch_bounds__(256) void gn_stats_kernel(const half_t* x0, const half_t* x1, int c0, int c1, int HW,
                                                       int groups, int rows_per_chunk, float* partial, const half_t* l0 = nullptr,
                                                       const half_t* l1 = nullptr) {
    __shared__ float s_sum[GN_MAX_C];
    __shared__ float s_sq[GN_MAX_C];
    const int C = c0 + c1, VP = C / 8;
    const int chunk = blockIdx.x, b = blockIdx.y, nchunk = gridDim.x;
    const int tid = threadIdx.x;
    const int TP = VP < 256 ? VP : 256;          // threads across one pixel row
    const int R = 256 / TP;                      // pixel rows processed in parallel (R * C <= 2048 when R > 1)
    const int p_begin = chunk * rows_per_chunk;
    const int p_end = min(HW, p_begin + rows_per_chunk);
    if (tid < TP * R) {
        const int tr = tid / TP, tc = tid - tr * TP;
        for (int cv = tc; cv < VP; cv += TP) {
            const int c = cv * 8;
            const half_t* src;
            int cc, ld;
            if (c < c0) { src = x0; cc = c; ld = c0; } else { src = x1; cc = c - c0; ld = c1; }
            const half_t* base = src + (long)b * HW * ld + cc;
            [[maybe_unused]] const half_t* lbase = HILO ? (c < c0 ? l0 : l1) + (long)b * HW * ld + cc : nullptr;
            // sums of (x - k) and (x - k)^2 around the thread's FIRST value k of the channel: k lies inside the data, so the sum of
            // squares carries the spread and not the offset
            float a[8], q[8], k[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { a[e] = 0.f; q[e] = 0.f; k[e] = 0.f; }
            int pix = p_begin + tr;
            const int n_t = pix < p_end ? (p_end - pix + R - 1) / R : 0;        // pixels this thread reads
            if (pix < p_end) {
                const h8 v = *reinterpret_cast<const h8*>(base + (long)pix * ld);
                h8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
                if constexpr (HILO) lv = *reinterpret_cast<const h8*>(lbase + (long)pix * ld);
#pragma unroll
                for (int e = 0; e < 8; ++e) k[e] = HILO ? (float)v[e] + (float)lv[e] : (float)v[e];
                pix += R;
            }
            // 4 independent 16-byte loads in flight per thread (the pass is pure streaming: latency must be covered by ILP)
            for (; pix + 3 * R < p_end; pix += 4 * R) {
                h8 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const h8*>(base + (long)(pix + u * R) * ld);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    h8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
                    if constexpr (HILO) lv = *reinterpret_cast<const h8*>(lbase + (long)(pix + u * R) * ld);
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float f = (HILO ? (float)v[u][e] + (float)lv[e] : (float)v[u][e]) - k[e]; a[e] += f; q[e] = fmaf(f, f, q[e]); }
                }
            }
            for (; pix < p_end; pix += R) {
                const h8 v = *reinterpret_cast<const h8*>(base + (long)pix * ld);
                h8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
                if constexpr (HILO) lv = *reinterpret_cast<const h8*>(lbase + (long)pix * ld);
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float f = (HILO ? (float)v[e] + (float)lv[e] : (float)v[e]) - k[e]; a[e] += f; q[e] = fmaf(f, f, q[e]); }
            }
            // -> (mean, M2) of the thread's n_t values of each channel; one writer per slot
            const float inv = n_t > 0 ? 1.0f / (float)n_t : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { s_sum[tr * C + c + e] = fmaf(a[e], inv, k[e]); s_sq[tr * C + c + e] = fmaxf(q[e] - a[e] * a[e] * inv, 0.f); }
        }
    }
    __syncthreads();
    {
        // 8 lanes per group walk the group's R x cpg LDS slots in a fixed order, then an 8-lane shuffle tree (deterministic) — twice:
        // the mean of the slot means (weighted by the slots' pixel counts, around the first slot's mean), then
        // M2 = sum over slots of M2_slot + count_slot * (mean_slot - mean)^2, the exact decomposition of the centred sum of squares
        const int g = tid >> 3, l8 = tid & 7;
        const int cpg = C / groups, n = R * cpg;
        const int np = max(p_end - p_begin, 0);                // pixels of this chunk (an image whose rows do not fill the last chunks: 0)
        const float pv = g < groups ? s_sum[g * cpg] : 0.f;
        float a = 0.f;
        if (g < groups)
            for (int i = l8; i < n; i += 8) {
                const int r = i / cpg, c = g * cpg + (i - r * cpg);
                a = fmaf((float)max((np - r + R - 1) / R, 0), s_sum[r * C + c] - pv, a);
            }
        for (int off = 4; off > 0; off >>= 1) a += __shfl_xor(a, off);
        const float mean = np > 0 ? pv + a / ((float)np * (float)cpg) : 0.f;
        float q = 0.f;
        if (g < groups)
            for (int i = l8; i < n; i += 8) {
                const int r = i / cpg, c = g * cpg + (i - r * cpg);
                const float d = s_sum[r * C + c] - mean;
                q += fmaf((float)max((np - r + R - 1) / R, 0) * d, d, s_sq[r * C + c]);
            }
        for (int off = 4; off > 0; off >>= 1) q += __shfl_xor(q, off);
        if (g < groups && l8 == 0) {
            float* dst = partial + (((long)b * nchunk + chunk) * groups + g) * 2;
            dst[0] = mean; dst[1] = np > 0 ? q : 0.f;
        }
    }
}

// Two sets of (count, mean, M2) into one (Chan, Golub, LeVeque 1979); an empty second set changes nothing.
__device__ __forceinline__ void gn_merge(float& n, float& mean, float& m2, float nb, float mb, float qb) {
    if (nb > 0.f) {
        const float r = nb / (n + nb), d = mb - mean;
        mean = fmaf(d, r, mean);
        m2 = (m2 + qb) + d * d * n * r;
        n += nb;
    }
}

// U 16-byte vectors per thread are in flight at a time, and the first U are requested BEFORE the prologue (they do not depend on it):
// with two in flight and the loads behind the prologue (rounds 1-4) a workgroup was a chain of load latencies — 8 dependent trips for
// its 16 vectors per thread at ~1.3 workgroups per CU: B16 HW1024 C640 ran at 18 us against 9 us for a plain copy of the same bytes
// (profiles/r05_copy_rate.txt).  The per-channel tables live in dynamic LDS (2 C floats) so that small-C launches keep their occupancy.
template <bool HILO = false, int U = 8>
__global__ __launch_bounds__(256) void gn_apply_kernel(const half_t* x0, const half_t* x1, int c0, int c1, int HW,
                                                       int groups, int nchunk, int chunk_rows, int chunk_period, const float* partial,
                                                       const float* gamma, const float* beta, half_t* out, float eps,
                                                       int silu, const half_t* l0 = nullptr, const half_t* l1 = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [C] scale | [C] shift (floats)
    __shared__ float s_mean[64], s_rstd[64];
    const int C = c0 + c1, VP = C / 8, cpg = C / groups;
    float* s_scale = reinterpret_cast<float*>(smem);
    float* s_shift = s_scale + C;
    const int b = blockIdx.y, tid = threadIdx.x;
    // grid-stride walk over the (pixel, 8-channel vector) pairs of image b.  The pair is advanced by the stride's quotient / remainder
    // instead of dividing the linear index each time: the 64-bit divisions by the runtime VP were ~130 of the loop's 330 VALU
    // instructions (23 of them quarter-rate multiplies) — static ISA review, docs/DESIGN_experiments.md.
    const int stride = (int)gridDim.x * 256;                       // HW * C < 2^31, HW < 2^24 (launch_groupnorm)
    const int sp = stride / VP, sr = stride - sp * VP;
    const int spU = (U * stride) / VP, srU = U * stride - spU * VP;
    const int i_init = (int)blockIdx.x * 256 + tid;
    int pix_u[U], cv_u[U];
    unsigned iv[U];                                                // linear vector index: the output offset is iv * 8
    pix_u[0] = i_init / VP; cv_u[0] = i_init - pix_u[0] * VP; iv[0] = (unsigned)i_init;
#pragma unroll
    for (int u = 1; u < U; ++u) {
        iv[u] = iv[u - 1] + (unsigned)stride;
        pix_u[u] = pix_u[u - 1] + sp; cv_u[u] = cv_u[u - 1] + sr;
        if (cv_u[u] >= VP) { cv_u[u] -= VP; ++pix_u[u]; }
    }
    const half_t* x0b = x0 + (long)b * HW * c0;
    const half_t* x1b = x1 ? x1 + (long)b * HW * c1 : nullptr;
    [[maybe_unused]] const half_t* l0b = HILO ? l0 + (long)b * HW * c0 : nullptr;
    [[maybe_unused]] const half_t* l1b = (HILO && l1) ? l1 + (long)b * HW * c1 : nullptr;
    half_t* outb = out + (long)b * HW * C;
    h8 v[U];
    [[maybe_unused]] h8 lv[HILO ? U : 1];
    int cs[U];
    bool ok[U];
    auto request = [&]() {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ok[u] = pix_u[u] < HW;
            const unsigned pix = ok[u] ? (unsigned)pix_u[u] : 0u;
            const int c = (ok[u] ? cv_u[u] : 0) * 8;
            cs[u] = c;
            const half_t* src;
            unsigned cc, ld;
            if (c < c0) { src = x0b; cc = (unsigned)c; ld = (unsigned)c0; } else { src = x1b; cc = (unsigned)(c - c0); ld = (unsigned)c1; }
            v[u] = *reinterpret_cast<const h8*>(src + (__umul24(pix, ld) + cc));
            if constexpr (HILO) lv[u] = *reinterpret_cast<const h8*>((c < c0 ? l0b : l1b) + (__umul24(pix, ld) + cc));
        }
    };
    request();
    {
        // 8 threads per group merge the chunks' (mean, M2) in a fixed order (deterministic), then an 8-lane shuffle tree of merges.
        // Chunk ch holds the rows [j * chunk_rows, (j + 1) * chunk_rows) of HW, j = ch % chunk_period (banded images: chunk_period chunks
        // per band of HW rows, every band's chunks side by side; otherwise chunk_period = nchunk).
        const int g = tid >> 3, l8 = tid & 7;
        float n = 0.f, mean = 0.f, m2 = 0.f;
        if (g < groups)
            for (int ch = l8; ch < nchunk; ch += 8) {
                const float* src = partial + (((long)b * nchunk + ch) * groups + g) * 2;
                const int j = ch % chunk_period;
                gn_merge(n, mean, m2, (float)(max(min(chunk_rows, HW - j * chunk_rows), 0) * cpg), src[0], src[1]);
            }
        for (int off = 4; off > 0; off >>= 1) {
            const float nb = __shfl_xor(n, off), mb = __shfl_xor(mean, off), qb = __shfl_xor(m2, off);
            gn_merge(n, mean, m2, nb, mb, qb);
        }
        if (g < groups && l8 == 0) {
            s_mean[g] = mean;
            s_rstd[g] = rsqrtf(m2 / n + eps);
        }
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
        const int g = c / cpg;
        const float sc = s_rstd[g] * gamma[c];
        s_scale[c] = sc;
        s_shift[c] = beta[c] - s_mean[g] * sc;
    }
    __syncthreads();
    while (true) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!ok[u]) continue;
            const f4 sa = *reinterpret_cast<const f4*>(&s_scale[cs[u]]), sb = *reinterpret_cast<const f4*>(&s_scale[cs[u] + 4]);
            const f4 ha = *reinterpret_cast<const f4*>(&s_shift[cs[u]]), hb = *reinterpret_cast<const f4*>(&s_shift[cs[u] + 4]);
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float sc = e < 4 ? sa[e] : sb[e - 4], sh = e < 4 ? ha[e] : hb[e - 4];
                float y = fmaf(HILO ? (float)v[u][e] + (float)lv[HILO ? u : 0][e] : (float)v[u][e], sc, sh);
                if (silu) y = y * __builtin_amdgcn_rcpf(1.0f + __expf(-y));
                o[e] = (half_t)y;
            }
            *reinterpret_cast<h8*>(outb + iv[u] * 8u) = o;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            iv[u] += (unsigned)(U * stride);
            pix_u[u] += spU; cv_u[u] += srU;
            if (cv_u[u] >= VP) { cv_u[u] -= VP; ++pix_u[u]; }
        }
        if (pix_u[0] >= HW) break;
        request();
    }
}

// Single-launch GroupNorm(+SiLU) for the small levels (8x8 / 16x16 / 32x32 latents: 2.6 - 40 MB tensors that the two-pass pair above
// spends ~20 us on whatever their size — two dependent launches of 32 workgroups each, one pixel loop per thread): one workgroup per
// (image, group) holds the group's HW x cpg values in registers (<= NVT 16-byte vectors per thread, NVT = 4 or 12), so the tensor is read ONCE;
// mean first, then the centred sum of squares (two-pass in registers), fixed reduction order (lane partials -> wave shuffle tree ->
// LDS -> every thread adds the 4 wave sums in order): deterministic.  Needs cpg % 8 == 0 (C = 256, 512, 1280, 2560 at 32 groups).
// HILO (engine option "residual_fp32"): the input as (hi, lo) fp16 pairs — the value is hi + lo (gn_stats_kernel's note); NVT <= 6 there.
template <int NVT, bool HILO = false>
__global__ __launch_bounds__(256) void gn_fused_small_kernel(const half_t* x0, const half_t* x1, int c0, int c1, int HW, int groups,
                                                             const float* gamma, const float* beta, half_t* out, float eps, int silu,
                                                             const half_t* l0 = nullptr, const half_t* l1 = nullptr) {
    __shared__ float red[2][4];
    const int C = c0 + c1, cpg = C / groups, VW = cpg / 8;
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int cbase = g * cpg;
    // the group lies in one source or straddles the concatenation point at a vector boundary (c0 % 8 == 0)
    const half_t* x0b = x0 + (long)b * HW * c0;
    const half_t* x1b = x1 ? x1 + (long)b * HW * c1 : nullptr;
    h8 v[NVT];
    [[maybe_unused]] h8 vl[HILO ? NVT : 1];
    [[maybe_unused]] const half_t* l0b = HILO ? l0 + (long)b * HW * c0 : nullptr;
    [[maybe_unused]] const half_t* l1b = (HILO && l1) ? l1 + (long)b * HW * c1 : nullptr;
    int off[NVT], cch[NVT];                                  // element offset of the vector in the OUTPUT image (pixel * C + channel); channel
    float s = 0.f;
    // (pixel, vector) pairs advanced by the stride's quotient / remainder: no division by the runtime VW per vector
    const int sp = 256 / VW, sr = 256 - sp * VW;
    int pix = tid / VW, vc = tid - pix * VW;
#pragma unroll
    for (int k = 0; k < NVT; ++k) {
        const bool ok = pix < HW;
        const int pp = ok ? pix : 0;
        const int c = cbase + vc * 8;
        off[k] = ok ? pp * C + c : -1;
        cch[k] = c;
        const half_t* src = c < c0 ? x0b + (long)pp * c0 + c : x1b + (long)pp * c1 + (c - c0);
        h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        v[k] = ok ? *reinterpret_cast<const h8*>(src) : z;
        if constexpr (HILO) {
            const half_t* srcl = c < c0 ? l0b + (long)pp * c0 + c : l1b + (long)pp * c1 + (c - c0);
            vl[k] = ok ? *reinterpret_cast<const h8*>(srcl) : z;
        }
        pix += sp; vc += sr;
        if (vc >= VW) { vc -= VW; ++pix; }
    }
#pragma unroll
    for (int k = 0; k < NVT; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) s += HILO ? (float)v[k][e] + (float)vl[HILO ? k : 0][e] : (float)v[k][e];      // vectors past the end hold zeros
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) red[0][tid >> 6] = s;
    __syncthreads();
    const float n = (float)cpg * (float)HW;
    const float mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / n;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NVT; ++k)
        if (off[k] >= 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = (HILO ? (float)v[k][e] + (float)vl[HILO ? k : 0][e] : (float)v[k][e]) - mean; q = fmaf(d, d, q); }
        }
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    if ((tid & 63) == 0) red[1][tid >> 6] = q;
    __syncthreads();
    const float rstd = rsqrtf(((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / n + eps);
    half_t* outb = out + (long)b * HW * C;
#pragma unroll
    for (int k = 0; k < NVT; ++k) {
        if (off[k] < 0) continue;
        const int c = cch[k];
        const f4 g0 = *reinterpret_cast<const f4*>(gamma + c), g1 = *reinterpret_cast<const f4*>(gamma + c + 4);
        const f4 b0 = *reinterpret_cast<const f4*>(beta + c), b1 = *reinterpret_cast<const f4*>(beta + c + 4);
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float gm = e < 4 ? g0[e] : g1[e - 4], bt = e < 4 ? b0[e] : b1[e - 4];
            float y = fmaf(((HILO ? (float)v[k][e] + (float)vl[HILO ? k : 0][e] : (float)v[k][e]) - mean) * rstd, gm, bt);
            if (silu) y = y * __builtin_amdgcn_rcpf(1.0f + __expf(-y));
            o[e] = (half_t)y;
        }
        *reinterpret_cast<h8*>(outb + off[k]) = o;
    }
}

int g_gn_apply_blocks = 0;
int g_gn_small = [] { const char* e = getenv("SDMI_GN_SMALL"); return e ? atoi(e) : 1; }();

static inline int gn_chunks(int B, int HW) {
    // ~1024 workgroups over the batch (4 per CU), >= 32 pixels per chunk, <= 64 chunks: few enough partials that the
    // apply kernel's prologue (a dependent chain of global loads per workgroup) stays short
    int n = (1024 + B - 1) / B;
    if (n > HW / 32) n = HW / 32;
    if (n > 64) n = 64;
    if (n < 1) n = 1;
    return n;
}

// Images beyond the 32-bit offsets of the kernels (HW * C >= 2^31 elements or HW >= 2^24 pixels: a 4096 x 4096 VAE decode at 128 channels)
// are normalised in `nb` equal bands of rows (nb a power of two dividing HW): per (image, band) one statistics launch over the band as if it
// were an image of its own, the chunk statistics of all bands of an image side by side in the workspace, so that the apply launches — again
// one per (image, band), each merging ALL of the image's chunks (gn_apply_kernel's chunk_period) —
// normalise with the image's mean and variance.  Host-side only: the kernels are the ones every other tensor runs.
// g_gn_band_elems (tests): the element limit that triggers banding, so the path runs on small tensors too.
long g_gn_band_elems = 0;
static inline long gn_band_limit() { return g_gn_band_elems > 0 ? g_gn_band_elems : (1L << 31); }
static inline int gn_row_limit() { return g_gn_band_elems > 0 ? (1 << 30) : (1 << 24); }
static int gn_bands(int HW, int C) {                      // 1: no banding; 0: the image does not split
    if ((long)HW * C < gn_band_limit() && HW < gn_row_limit()) return 1;
    for (int nb = 2; nb <= 8192; nb *= 2)
        if (HW % nb == 0 && (long)(HW / nb) * C < gn_band_limit() && HW / nb < gn_row_limit()) return nb;
    return 0;
}

int64_t groupnorm_ws_bytes(int B, int HW, int groups) {
    int64_t chunks = gn_chunks(B, HW);
    if ((long)HW * GN_MAX_C >= gn_band_limit() || HW >= gn_row_limit()) {   // may be banded for some C <= GN_MAX_C (gn_bands bands from HW * C >= the limit): room for the worst case
        int nb = 2;
        while (nb < 8192 && !((long)(HW / nb) * GN_MAX_C < gn_band_limit() && HW / nb < gn_row_limit())) nb *= 2;
        chunks = std::max<int64_t>(chunks, (int64_t)nb * 64);
    }
    return (int64_t)B * chunks * groups * 2 * sizeof(float);
}

static int groupnorm_banded(const half_t* x0, const half_t* x1, int c0, int c1, const float* gamma, const float* beta, half_t* out, int B,
                            int HW, int groups, float eps, bool silu, float* ws, hipStream_t s, int nb) {
    const int C = c0 + c1, HWb = HW / nb;
    const int nchunk_b = gn_chunks(1, HWb), rows = cdiv(HWb, nchunk_b), nchunk = nb * nchunk_b;
    // the caller sized `ws` with groupnorm_ws_bytes: nb * nchunk_b chunks of partials per image must fit what that provisions
    SDMI_REQUIRE((int64_t)B * nchunk * groups * 2 * (int64_t)sizeof(float) <= groupnorm_ws_bytes(B, HW, groups),
                 "banded GroupNorm: partial sums exceed the workspace groupnorm_ws_bytes provisions");
    char pname[64];
    snprintf(pname, sizeof pname, "groupnorm_silu_banded B%d HW%d C%d x%d", B, HW, C, nb);
    ProfScope ps(pname, 0.0, 3.0 * B * (double)HW * C * 2.0, s);
    const long per_image = (long)nchunk * groups * 2;
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nb; ++k) {
            const long row0 = (long)b * HW + (long)k * HWb;
            hipLaunchKernelGGL(gn_stats_kernel<false>, dim3(nchunk_b, 1), dim3(256), 0, s, x0 + row0 * c0, x1 ? x1 + row0 * c1 : nullptr, c0, c1, HWb,
                               groups, rows, ws + b * per_image + (long)k * nchunk_b * groups * 2, nullptr, nullptr);
            SDMI_CHECK_HIP(hipGetLastError());
        }
    const long nvec = (long)HWb * (C / 8);
    const long trips = std::max<long>(1, cdiv(nvec, 2048L * 2048));
    int blocks = (int)std::max<long>(1, cdiv(nvec, 2048 * trips));
    if (g_gn_apply_blocks > 0) blocks = g_gn_apply_blocks;
    const size_t smem = (size_t)2 * C * sizeof(float);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < nb; ++k) {
            const long row0 = (long)b * HW + (long)k * HWb;
            hipLaunchKernelGGL((gn_apply_kernel<false, 8>), dim3(blocks, 1), dim3(256), smem, s, x0 + row0 * c0, x1 ? x1 + row0 * c1 : nullptr, c0, c1,
                               HWb, groups, nchunk, rows, nchunk_b, ws + b * per_image, gamma, beta, out + row0 * C, eps, silu ? 1 : 0, nullptr, nullptr);
            SDMI_CHECK_HIP(hipGetLastError());
        }
    return 0;
}


int launch_groupnorm(const half_t* x0, const half_t* x1, int c0, int c1, const float* gamma, const float* beta,
                     half_t* out, int B, int HW, int groups, float eps, bool silu, float* ws, hipStream_t s, int pre_nchunk,
                     const half_t* x0_lo, const half_t* x1_lo) {
    const int C = c0 + c1;
    const bool hilo = x0_lo != nullptr;
    SDMI_REQUIRE(!hilo || (x1 == nullptr) == (x1_lo == nullptr), "GroupNorm (hi, lo) input: both sources as pairs");
    SDMI_REQUIRE(C % 8 == 0 && c0 % 8 == 0, "GroupNorm channels must be multiples of 8");
    SDMI_REQUIRE(C <= GN_MAX_C && groups <= 32 && C % groups == 0, "GroupNorm: C <= 4096, groups <= 32, C % groups == 0");
    if (const int nb = gn_bands(HW, C); nb != 1) {
        SDMI_REQUIRE(nb > 1, "GroupNorm: an image of 2^31 elements or more must split into equal power-of-two bands of rows below that limit");
        SDMI_REQUIRE(!hilo && pre_nchunk <= 0, "GroupNorm beyond 2^31 elements per image: fp16 input with its own statistics pass only");
        return groupnorm_banded(x0, x1, c0, c1, gamma, beta, out, B, HW, groups, eps, silu, ws, s, nb);
    }
    char pname[64];
    {
        const int cpg = C / groups;
        const long nv = (long)HW * (cpg / 8);
        // (<= 12 vectors per thread: the 24-vector instantiation needs all 256 VGPRs — one workgroup per SIMD — and ran the 32x32-latent
        // C = 1280 norm at 77 us against 33 us for the two-pass pair: GPU run 2 of round 3)
        if (pre_nchunk <= 0 && g_gn_small && cpg % 8 == 0 && nv <= (hilo ? 6 : 12) * 256) {
            snprintf(pname, sizeof pname, "groupnorm_silu_fused B%d HW%d C%d", B, HW, C);
            ProfScope ps(pname, 0.0, (hilo ? 3.0 : 2.0) * B * (double)HW * C * 2.0, s);             // read once + write once
            const dim3 grid(groups, B);
#define SDMI_GNS(NVT, HL) hipLaunchKernelGGL((gn_fused_small_kernel<NVT, HL>), grid, dim3(256), 0, s, x0, x1, c0, c1, HW, groups, gamma, beta, out, eps, silu ? 1 : 0, x0_lo, x1_lo)
            if (hilo) { if (nv <= 2 * 256) SDMI_GNS(2, true); else SDMI_GNS(6, true); }
            else if (nv <= 4 * 256) SDMI_GNS(4, false);
            else SDMI_GNS(12, false);
#undef SDMI_GNS
            SDMI_CHECK_HIP(hipGetLastError());
            return 0;
        }
    }
    const int nchunk = pre_nchunk > 0 ? pre_nchunk : gn_chunks(B, HW);
    const int rows = cdiv(HW, nchunk);
    snprintf(pname, sizeof pname, pre_nchunk > 0 ? "groupnorm_silu_apply B%d HW%d C%d" : "groupnorm_silu B%d HW%d C%d", B, HW, C);
    ProfScope ps(pname, 0.0, (pre_nchunk > 0 ? 2.0 : 3.0) * B * (double)HW * C * 2.0, s);      // read (twice) + write once
    if (pre_nchunk <= 0) {
        if (hilo) hipLaunchKernelGGL(gn_stats_kernel<true>, dim3(nchunk, B), dim3(256), 0, s, x0, x1, c0, c1, HW, groups, rows, ws, x0_lo, x1_lo);
        else hipLaunchKernelGGL(gn_stats_kernel<false>, dim3(nchunk, B), dim3(256), 0, s, x0, x1, c0, c1, HW, groups, rows, ws, nullptr, nullptr);
        SDMI_CHECK_HIP(hipGetLastError());
    }
    const long nvec = (long)HW * (C / 8);
    // Whole trips of 8 vectors per thread (a ragged last trip costs a full load latency for a fraction of the bytes), as few of them as
    // ~8 workgroups per CU over the batch allow: one trip for every UNet tensor of the benchmarked job.  The first trip's loads overlap
    // the prologue.  (Tried: fewer, longer-lived workgroups so that each streams >= 4x the bytes its prologue reads — the chunk partials of
    // its image + gamma / beta, 16 + 15 KB at C = 1920 with 64 chunks: slower, 1.28 -> 1.34 ms of GroupNorm per forward; the trips are
    // dependent and the prologues of co-resident workgroups overlap.)
    const long cap = std::max(1, 2048 / B);
    const long trips = std::max<long>(1, cdiv(nvec, 2048 * cap));
    int blocks = (int)std::max<long>(1, cdiv(nvec, 2048 * trips));
    if (g_gn_apply_blocks > 0) blocks = g_gn_apply_blocks;       // tests: several trips per thread on a small tensor
    const size_t smem = (size_t)2 * C * sizeof(float);
    if (hilo)
        hipLaunchKernelGGL((gn_apply_kernel<true, 4>), dim3(blocks, B), dim3(256), smem, s, x0, x1, c0, c1, HW, groups, nchunk, rows, nchunk, ws, gamma,
                           beta, out, eps, silu ? 1 : 0, x0_lo, x1_lo);
    else
        hipLaunchKernelGGL((gn_apply_kernel<false, 8>), dim3(blocks, B), dim3(256), smem, s, x0, x1, c0, c1, HW, groups, nchunk, rows, nchunk, ws, gamma,
                           beta, out, eps, silu ? 1 : 0, nullptr, nullptr);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm: one wave per token row; lane holds K = ceil(C/512) <= 4 vectors of 8 channels.  A wave
// works on RPW rows at once (all of their loads issued before the first reduction) so that a CU keeps enough bytes in
// flight to cover HBM latency: with one 640-byte row per wave the kernel was latency-, not bandwidth-bound.
// ---------------------------------------------------------------------------------------------------------------
#define LN_VAL(r, k, e) (HILO ? (float)v[r][k][e] + (float)vl[HILO ? (r) : 0][HILO ? (k) : 0][e] : (float)v[r][k][e])
template <int K, int RPW, bool HILO = false>
__global__ __launch_bounds__(256) void layernorm_kernel(const half_t* x, const float* gamma, const float* beta,
                                                        half_t* out, long rows, int C, float eps, const half_t* xlo = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = ((long)blockIdx.x * 4 + wave) * RPW;
    if (row0 >= rows) return;
    const int VP = C / 8;
    const float inv_c = 1.0f / (float)C;
    h8 v[RPW][K];
    [[maybe_unused]] h8 vl[HILO ? RPW : 1][HILO ? K : 1];    // HILO: the lo parts of a (hi, lo) stream (gn_stats_kernel's note)
    float sum[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long row = min(row0 + r, rows - 1);           // clamped duplicate rows are computed but not stored
        const half_t* src = x + row * C;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int cv = lane + k * 64;
            h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            v[r][k] = cv < VP ? *reinterpret_cast<const h8*>(src + cv * 8) : z;
            if constexpr (HILO) vl[r][k] = cv < VP ? *reinterpret_cast<const h8*>(xlo + row * C + cv * 8) : z;
        }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) a += LN_VAL(r, k, e);      // padding lanes hold zeros
        sum[r] = a;
    }
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int r = 0; r < RPW; ++r) sum[r] += __shfl_xor(sum[r], off);
    float mean[RPW], sq[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        mean[r] = sum[r] * inv_c;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int cv = lane + k * 64;
            if (cv < VP) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = LN_VAL(r, k, e) - mean[r]; q = fmaf(d, d, q); }
            }
        }
        sq[r] = q;
    }
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int r = 0; r < RPW; ++r) sq[r] += __shfl_xor(sq[r], off);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int cv = lane + k * 64;
        if (cv < VP) {
            const f4 g0 = *reinterpret_cast<const f4*>(gamma + cv * 8), g1 = *reinterpret_cast<const f4*>(gamma + cv * 8 + 4);
            const f4 b0 = *reinterpret_cast<const f4*>(beta + cv * 8), b1 = *reinterpret_cast<const f4*>(beta + cv * 8 + 4);
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                if (row0 + r >= rows) continue;
                const float rstd = rsqrtf(fmaf(sq[r], inv_c, eps));
                h8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float g = e < 4 ? g0[e] : g1[e - 4], bb = e < 4 ? b0[e] : b1[e - 4];
                    o[e] = (half_t)((LN_VAL(r, k, e) - mean[r]) * rstd * g + bb);
                }
                *reinterpret_cast<h8*>(out + (row0 + r) * C + cv * 8) = o;
            }
        }
    }
}

#undef LN_VAL

// Row statistics only (LayerNorm folded into the consuming GEMMs, GemmP::ln_stats): the same two-pass arithmetic as
// layernorm_kernel — mean, then the centred sum of squares, both from the fp16 values the GEMM will read — but nothing is written
// back except (mean, rstd) per row.
template <int K, int RPW>
__global__ __launch_bounds__(256) void ln_rowstats_kernel(const half_t* x, float* stats, long rows, int C, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long row0 = ((long)blockIdx.x * 4 + wave) * RPW;
    if (row0 >= rows) return;
    const int VP = C / 8;
    const float inv_c = 1.0f / (float)C;
    h8 v[RPW][K];
    float sum[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        const long row = min(row0 + r, rows - 1);
        const half_t* src = x + row * C;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int cv = lane + k * 64;
            h8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            v[r][k] = cv < VP ? *reinterpret_cast<const h8*>(src + cv * 8) : z;
        }
    }
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) a += (float)v[r][k][e];
        sum[r] = a;
    }
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int r = 0; r < RPW; ++r) sum[r] += __shfl_xor(sum[r], off);
    float mean[RPW], sq[RPW];
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
        mean[r] = sum[r] * inv_c;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int cv = lane + k * 64;
            if (cv < VP) {
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = (float)v[r][k][e] - mean[r]; q = fmaf(d, d, q); }
            }
        }
        sq[r] = q;
    }
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int r = 0; r < RPW; ++r) sq[r] += __shfl_xor(sq[r], off);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RPW; ++r)
            if (row0 + r < rows) {
                stats[(row0 + r) * 2 + 0] = mean[r];
                stats[(row0 + r) * 2 + 1] = rsqrtf(fmaf(sq[r], inv_c, eps));
            }
    }
}

int launch_ln_rowstats(const half_t* x, float* stats, int64_t rows, int C, float eps, hipStream_t s) {
    SDMI_REQUIRE(C % 8 == 0 && C <= 2048, "LayerNorm statistics: C % 8 == 0 and C <= 2048");
    char pname[48];
    snprintf(pname, sizeof pname, "ln_rowstats rows%ld C%d", (long)rows, C);
    ProfScope ps(pname, 0.0, (double)rows * C * 2.0, s);
    const int K = cdiv(C / 8, 64);
#define SDMI_LNS(KK, RR)                                                                                             \
    hipLaunchKernelGGL((ln_rowstats_kernel<KK, RR>), dim3(cdiv(rows, 4 * RR)), dim3(256), 0, s, x, stats, (long)rows, C, eps)
    if (K == 1) SDMI_LNS(1, 4);
    else if (K == 2) SDMI_LNS(2, 2);
    else if (K == 3) SDMI_LNS(3, 1);
    else SDMI_LNS(4, 1);
#undef SDMI_LNS
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

// One workgroup per packed weight row: fold gamma into the row, sum the folded (fp16-rounded) row and dot the original row with
// beta.  Fixed reduction order (per-thread strided partials -> wave shuffles -> LDS -> thread 0): bit-reproducible.
__global__ __launch_bounds__(256) void ln_fold_weights_kernel(const half_t* w, const float* gamma, const float* beta, const float* bias,
                                                              half_t* wf, float* s_out, float* c_out, int K, int C) {
    __shared__ float red[2][4];
    const int n = blockIdx.x, tid = threadIdx.x;
    const half_t* src = w + (long)n * K;
    half_t* dst = wf + (long)n * K;
    float s = 0.f, c = 0.f;
    for (int k = tid; k < K; k += 256) {
        const float wv = (float)src[k];
        const float g = k < C ? gamma[k] : 0.f, bt = k < C ? beta[k] : 0.f;
        const half_t f = (half_t)(wv * g);
        dst[k] = f;
        s += (float)f;
        c = fmaf(bt, wv, c);
    }
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); c += __shfl_xor(c, off); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = s; red[1][tid >> 6] = c; }
    __syncthreads();
    if (tid == 0) {
        s_out[n] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        c_out[n] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) + (bias ? bias[n] : 0.f);
    }
}

int launch_ln_fold_weights(const half_t* w, const float* gamma, const float* beta, const float* bias, half_t* wf, float* s_out,
                           float* c_out, int n_rows, int K, int C, hipStream_t s) {
    SDMI_REQUIRE(n_rows > 0 && K >= C && C > 0, "LayerNorm weight fold: bad shape");
    hipLaunchKernelGGL(ln_fold_weights_kernel, dim3(n_rows), dim3(256), 0, s, w, gamma, beta, bias, wf, s_out, c_out, K, C);
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_layernorm(const half_t* x, const float* gamma, const float* beta, half_t* out, int64_t rows, int C,
                     float eps, hipStream_t s, const half_t* x_lo) {
    SDMI_REQUIRE(C % 8 == 0 && C <= 3072, "LayerNorm: C % 8 == 0 and C <= 3072");
    SDMI_REQUIRE(x_lo == nullptr || C <= 2048, "LayerNorm (hi, lo) input: C <= 2048");
    char pname[48];
    snprintf(pname, sizeof pname, "layernorm rows%ld C%d", (long)rows, C);
    ProfScope ps(pname, 0.0, 2.0 * (double)rows * C * 2.0, s);
    const int K = cdiv(C / 8, 64);
#define SDMI_LN(KK, RR)                                                                                                        \
    do {                                                                                                                       \
        if (x_lo) hipLaunchKernelGGL((layernorm_kernel<KK, (KK <= 2 ? 1 : RR), true>), dim3(cdiv(rows, 4 * (KK <= 2 ? 1 : RR))), dim3(256), 0, s, x, gamma, \
                                     beta, out, (long)rows, C, eps, x_lo);                                                     \
        else hipLaunchKernelGGL((layernorm_kernel<KK, RR, false>), dim3(cdiv(rows, 4 * RR)), dim3(256), 0, s, x, gamma, beta, out, (long)rows, C, \
                                eps, nullptr);                                                                                 \
    } while (0)
    if (K == 1) SDMI_LN(1, 4);
    else if (K == 2) SDMI_LN(2, 2);
    else if (K == 3) SDMI_LN(3, 1);
    else if (K == 4) SDMI_LN(4, 1);
    else if (K == 5) SDMI_LN(5, 1);                          // C up to 2560: the hidden layer of a [1, 2, 1] hypernetwork on the 1280-wide levels
    else SDMI_LN(6, 1);
#undef SDMI_LN
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
