// xattn_chain.hip — the cross-attention third of a BasicTransformerBlock at the 320-wide level as ONE launch (gfx950; fp16 operands,
// fp32 accumulation):
//     x2 = x1 + Wo . attention( Wq . LN2(x1), K, V ) + bo          K / V^T: the text context's cached projections (engine set_context)
// As four launches (LayerNorm, to_q GEMM, attention over the 77 text keys, to_out GEMM + residual) the normalised tokens, q and the
// attention output — 42 MB each at the C1 level-0 shape — go to HBM and come straight back.  Here a workgroup owns 128 whole token rows
// (one image, so one context) and those three tensors live in LDS only; x1 is read and x2 written, nothing else touches the token stream.
//
// The chain is a tiled GEMM, not a lane-owns-row chain (the removed round-5 form needed a fresh 1 KB LDS fragment per MFMA):
//   * 512 threads = 8 waves as 2 row halves (wr) x 4 column quarters (wc).  Wave (wr, wc) owns rows [64 wr, +64) and columns
//     [80 wc, +80) of the tile = heads 2 wc and 2 wc + 1 (d = 40), in all four phases — so q and the attention output are written by the
//     wave that reads them and the attention phase needs no barrier of its own.
//   * A-image (80 KB of LDS): the tile's 128 rows x 320 fp16, first LN2(x1), then q, then the attention output, last x1 again for the
//     residual.  Rows are 640 bytes = 40 16-byte slots; slot c of row r sits at slot c ^ ((r >> 1) & 7) of its row.  The XOR stays inside
//     an aligned group of 8 slots (40 = 5 x 8); a row starts at bank slot 8 (r & 1) of the 16 the LDS has, so the 16 rows of any
//     ds_read_b128 lane group (rows with the same column: the MFMA fragment reads of both shapes) cover 16 different slots.
//   * projections on v_mfma_f32_16x16x32_f16 with the operands swapped (weights A, tokens B: a lane ends with 4 consecutive columns of
//     one row): a 64 x 80 wave tile feeds 20 MFMAs from 4 + 5 fragment reads per 32-wide K chunk.  The packed [N][K] weights are streamed
//     in K chunks of 32 ([320 rows][64 bytes] = 20 KB, k-segments XORed with 3 ((n >> 3) & 1) on the SOURCE side of the LDS-direct load
//     — compact.hip's weight image) through a ring of three 24 KB stages, two chunks ahead of their use: every wave issues three
//     1 KB pieces per chunk (pieces 20 .. 23 re-read row 319 into the stage's padding), so `s_waitcnt vmcnt(3)` retires a chunk while the
//     next one stays in flight across the step's single barrier.
//   * attention in attention.hip's formulation per (head, 32-query block): S^T = K Q^T on v_mfma_f32_32x32x16_f16 (K rows read with bits
//     2 / 3 of the row index swapped), softmax state per lane, O^T = V^T P^T with P rounded to fp16 and the row sum taken by a ones row
//     (O^T row 40).  The context goes through the same ring in 32-key blocks — K rows [32][640 bytes] (the A-image's swizzle) and V^T
//     [320][64 bytes] (a weight chunk of a [320][Lpad] matrix) — with the online-softmax recurrence, so any context length works.  Keys
//     >= L are masked behind a real branch; the rows staged for them are clamped to key L - 1 and V^T's padding columns are never weighted
//     (P is exactly 0 there).  The softmax scale is applied to the fp32 scores.
// fp16 rounding points: LN2(x1), q, P, the attention output and x2 — those of the four launches.  Every global access is in bounds by
// construction (rows % 128 == 0; clamped rows for the padding pieces).
#include "common.h"
#include "prof.h"

#include <algorithm>
#include <cmath>

namespace sdmi {

// The host-emulated test build compiles this file as plain C++ (as part of engine.cpp, see its end): no address spaces, no dynamic LDS
// and no inline assembly there; its LDS-direct load completes at issue, so there is nothing to wait for.
#ifdef __HIP__
typedef const __attribute__((address_space(1))) void* xgptr_t;
typedef __attribute__((address_space(3))) void* xlptr_t;
#define XC_WAIT_VM3() asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory")
#define XC_WAIT_VM0() asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory")
#define XC_FENCE() asm volatile("" ::: "memory")
#define XC_REAL_BRANCH() asm volatile("")
// a value the compiler may not reason about: what is computed from it is computed where it is used, instead of being hoisted out of
// the step loops as long-lived per-lane source addresses (the attention phase has no registers to spare for them)
#define XC_OPAQUE(x) asm volatile("" : "+v"(x))
#else
typedef const void* xgptr_t;
typedef void* xlptr_t;
#define XC_WAIT_VM3() ((void)0)
#define XC_WAIT_VM0() ((void)0)
#define XC_FENCE() ((void)0)
#define XC_REAL_BRANCH() ((void)0)
#define XC_OPAQUE(x) ((void)0)
#endif

constexpr int kXcC = 320, kXcD = 40, kXcRows = 128;
constexpr int kXcRowBytes = kXcC * 2;                      // 640
constexpr int kXcImage = kXcRows * kXcRowBytes;            // 81 920
constexpr int kXcStage = 24 * 1024;                        // a 20 KB chunk + the 4 padding pieces
constexpr int kXcLds = kXcImage + 3 * kXcStage;            // 155 648: one workgroup per CU

struct XattnP {
    const half_t* x;          // [rows][320]: LayerNorm input and residual
    half_t* out;              // [rows][320]
    const float* gamma;       // norm2 affine
    const float* beta;
    const half_t* wq;         // attn2.to_q  [320][320] (no bias)
    const half_t* wo;         // attn2.to_out.0 [320][320]
    const float* bo;          // [320] (the launcher substitutes zeros for a null pointer)
    const half_t* k;          // [images][L][320]
    const half_t* vt;         // [images][320][Lpad]
    int rows_per_image;
    int L, Lpad;
    float eps, scale_log2, tau;
};

// byte offset of columns [col, col + 8) (col % 8 == 0; + (col & 7) * 2 for a part of them) of row `row` in the A-image
__device__ __forceinline__ int xc_img(int row, int col) { return row * kXcRowBytes + ((((col >> 3) ^ ((row >> 1) & 7))) << 4) + (col & 7) * 2; }

__global__ __launch_bounds__(512) void rowchain_xattn_kernel(const XattnP p) {
#ifdef __HIP__
    extern __shared__ __attribute__((aligned(16))) char smem[];
#else
    __shared__ __attribute__((aligned(16))) char smem[kXcLds];
#endif
    char* const img = smem;
    char* const ring = smem + kXcImage;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int l16 = lane & 15, q4 = lane >> 4;               // the 16x16x32 fragment coordinates
    const int lq = lane & 31, half = lane >> 5;              // the 32x32x16 ones
    const long row0 = (long)blockIdx.x * kXcRows;
    const int image = (int)(row0 / p.rows_per_image);
    const half_t* const kimg = p.k + (long)image * p.L * kXcC;
    const half_t* const vimg = p.vt + (long)image * kXcC * p.Lpad;
    const int nblk = (p.L + 31) >> 5;                        // 32-key blocks of the context
    const int nsteps = 20 + 2 * nblk;                        // chunks: Wq 0..9 | (K, V^T) of block 0, 1, .. | Wo 0..9

    // ---- the operand stream: chunk `seq` -> ring stage seq % 3; three 1 KB pieces per wave --------------------------------------
    // a [320][32]-column block (columns k0 ..) of a row-major fp16 matrix of row stride ld
    auto stage_cols = [&](const half_t* w, int ld, int k0, char* buf) {
        int ln = lane;
        XC_OPAQUE(ln);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int pb = u * 8 + wave;
            const int n = pb * 16 + (ln >> 2);
            const int seg = (ln & 3) ^ (3 * ((n >> 3) & 1));
            const half_t* src = w + (long)min(n, kXcC - 1) * ld + k0 + seg * 8;
            __builtin_amdgcn_global_load_lds((xgptr_t)src, (xlptr_t)(buf + pb * 1024), 16, 0, 0);
        }
    };
    // K rows [key0, key0 + 32) of the image's context, keys >= L clamped to L - 1 (masked by the consumer)
    auto stage_keys = [&](int key0, char* buf) {
        int ln = lane;
        XC_OPAQUE(ln);
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const int pb = u * 8 + wave;
            const int pc = pb * 64 + ln;
            const int r = pc / 40, ps = pc - r * 40;
            const int rr = min(r, 31);
            const int key = min(key0 + rr, p.L - 1);
            const half_t* src = kimg + (long)key * kXcC + ((ps ^ ((rr >> 1) & 7)) << 3);
            __builtin_amdgcn_global_load_lds((xgptr_t)src, (xlptr_t)(buf + pb * 1024), 16, 0, 0);
        }
    };
    auto issue = [&](int seq) {
        if (seq >= nsteps) return;
        char* buf = ring + (seq % 3) * kXcStage;
        if (seq < 10) stage_cols(p.wq, kXcC, seq * 32, buf);
        else if (seq < 10 + 2 * nblk) {
            const int blk = (seq - 10) >> 1;
            if ((seq - 10) & 1) stage_cols(vimg, p.Lpad, blk * 32, buf);
            else stage_keys(blk * 32, buf);
        } else stage_cols(p.wo, kXcC, (seq - 10 - 2 * nblk) * 32, buf);
    };
    // step s opens: my pieces of chunk s have landed (chunk s + 1 may stay in flight), everybody's have, and everybody has left step s - 1,
    // so its stage takes chunk s + 2
    auto open_step = [&](int s) -> const char* {
        if (s + 1 < nsteps) XC_WAIT_VM3(); else XC_WAIT_VM0();
        __builtin_amdgcn_s_barrier();
        XC_FENCE();
        issue(s + 2);
        return ring + (s % 3) * kXcStage;
    };

    issue(0);
    issue(1);

    // ---- phase 1: x1 -> LayerNorm (two-pass statistics from the fp16 values, as layernorm_kernel) -> the A-image --------------------
    // 8 lanes per row: a wave instruction reads 8 rows x one whole 128-byte line
    {
        const int sub = tid & 7;
        const float inv_c = 1.0f / (float)kXcC;
        h8 v[2][5];
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const half_t* src = p.x + (row0 + ps * 64 + (tid >> 3)) * kXcC + sub * 8;
#pragma unroll
            for (int i = 0; i < 5; ++i) v[ps][i] = *reinterpret_cast<const h8*>(src + i * 64);
        }
#pragma unroll
        for (int ps = 0; ps < 2; ++ps) {
            const int row = ps * 64 + (tid >> 3);
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) a += (float)v[ps][i][e];
            for (int off = 4; off > 0; off >>= 1) a += __shfl_xor(a, off);
            const float mean = a * inv_c;
            float sq = 0.f;
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float d = (float)v[ps][i][e] - mean; sq = fmaf(d, d, sq); }
            for (int off = 4; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
            const float rstd = rsqrtf(fmaf(sq, inv_c, p.eps));
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const int c0 = (i * 8 + sub) * 8;
                const f4 g0 = *reinterpret_cast<const f4*>(p.gamma + c0), g1 = *reinterpret_cast<const f4*>(p.gamma + c0 + 4);
                const f4 b0 = *reinterpret_cast<const f4*>(p.beta + c0), b1 = *reinterpret_cast<const f4*>(p.beta + c0 + 4);
                h8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float g = e < 4 ? g0[e] : g1[e - 4], bb = e < 4 ? b0[e] : b1[e - 4];
                    o[e] = (half_t)(((float)v[ps][i][e] - mean) * rstd * g + bb);
                }
                *reinterpret_cast<h8*>(img + xc_img(row, c0)) = o;
            }
        }
    }

    // ---- projections: acc[mi][j][r] = out[64 wr + 16 mi + l16][80 wc + 16 j + 4 q4 + r] --------------------------------------------
    const int a_off = (64 * wr + l16) * kXcRowBytes, a_sw = (l16 >> 1) & 7;
    const int w_off = (80 * wc + l16) * 64 + ((q4 ^ (3 * (l16 >> 3))) << 4);
    f4 acc[4][5];
    auto zero_acc = [&]() {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[mi][j] = f4{0.f, 0.f, 0.f, 0.f};
    };
    auto gemm_step = [&](const char* buf, int kc) {
        h8 af[4], wf[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) wf[j] = *reinterpret_cast<const h8*>(buf + w_off + j * 1024);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) af[mi] = *reinterpret_cast<const h8*>(img + a_off + mi * 16 * kXcRowBytes + (((kc * 4 + q4) ^ a_sw) << 4));
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int j = 0; j < 5; ++j) acc[mi][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], af[mi], acc[mi][j], 0, 0, 0);
    };

    // ---- phase 2: q = LN2(x1) Wq^T ----------------------------------------------------------------------------------------------
    zero_acc();
    int s = 0;
#pragma unroll 1
    for (; s < 10; ++s) {
        const char* buf = open_step(s);
        gemm_step(buf, s);
    }

    // ---- phase 3: attention of this wave's 2 heads x 2 query blocks over the context -----------------------------------------------
    // The first K step opens here: every wave is past its last read of LN2(x1), and q (fp16) takes its place, each wave its own rows x
    // columns (outside the block loop, so that the projection's accumulators are dead before the attention state is born)
    const char* kb = open_step(s++);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const h4 hv = {(half_t)acc[mi][j][0], (half_t)acc[mi][j][1], (half_t)acc[mi][j][2], (half_t)acc[mi][j][3]};
            *reinterpret_cast<h4*>(img + xc_img(64 * wr + 16 * mi + l16, 80 * wc + 16 * j + 4 * q4)) = hv;
        }
    XC_FENCE();
    __builtin_amdgcn_wave_barrier();                         // (the other lanes of this wave read what this lane wrote)
    // state st = 2 * (head - 2 wc) + query block
    f16v o[4][2];
    float m_run[4];
    h8 pb[4][2];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        m_run[st] = -1e30f;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[st][db][r] = 0.f;
    }
    const int krow = (lq & 0x13) | ((lq & 4) << 1) | ((lq & 8) >> 1);
    const int k_off = krow * kXcRowBytes, k_sw = (krow >> 1) & 7, q_sw = (lq >> 1) & 7;
    const h8 ones = {(half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f, (half_t)1.f};
    const h8 zeros = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int blk = 0; blk < nblk; ++blk) {
        // -- K step: S^T and the softmax of the block
        if (blk > 0) kb = open_step(s++);
        const bool ragged = blk * 32 + 32 > p.L;
        const int lim = p.L - blk * 32 - 8 * half;           // local keys >= lim are past the end
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            const int hs = (2 * wc + (st >> 1)) * 5;         // first slot of the head's columns
            const int qrow = 64 * wr + 32 * (st & 1) + lq;
            f16v sc;
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[r] = 0.f;
#pragma unroll
            for (int dc = 0; dc < 3; ++dc) {
                // d = 40 .. 47 (dc 2, upper half-wave) is padding: Q is zero there and K re-reads d = 32 .. 39
                const bool padk = dc == 2 && half == 1;
                const int c = hs + dc * 2 + (dc == 2 ? 0 : half);
                h8 qf = *reinterpret_cast<const h8*>(img + qrow * kXcRowBytes + ((c ^ q_sw) << 4));
                if (padk) qf = zeros;
                const h8 kf = *reinterpret_cast<const h8*>(kb + k_off + ((c ^ k_sw) << 4));
                sc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf, sc, 0, 0, 0);
            }
            // register r <-> local key 16 (r >> 3) + 8 half + (r & 7)
            if (ragged) {
                XC_REAL_BRANCH();
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (16 * (r >> 3) + (r & 7) >= lim) sc[r] = -INFINITY;
            }
            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[r]);
            float mlo = mx, mhi = mx;
#ifdef __HIP__
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(mlo), "+v"(mhi));
#else
            emu_permlane32_swap(mlo, mhi);
#endif
            mx = fmaxf(mlo, mhi) * p.scale_log2;              // scale > 0: max commutes with the scaling
            // exponent base: attention.hip's rule — re-based (wave-wide, O^T rescaled) when some query's block maximum exceeds it by more than tau
            const bool moved = p.tau < 0.f || __builtin_amdgcn_ballot_w64(mx > m_run[st] + fmaxf(p.tau, 0.f)) != 0;
            const float m_new = moved ? fmaxf(m_run[st], mx) : m_run[st];
            const float alpha = __builtin_amdgcn_exp2f(m_run[st] - m_new);
            m_run[st] = m_new;
#pragma unroll
            for (int r = 0; r < 16; ++r) pb[st][r >> 3][r & 7] = (half_t)__builtin_amdgcn_exp2f(fmaf(sc[r], p.scale_log2, -m_new));
            if (moved) {
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int r = 0; r < 16; ++r) o[st][db][r] *= alpha;
            }
            // (keeps the fragment reads of the next state from being hoisted over this one: with the four O^T tiles resident, the
            // fragments of all four states at once do not fit the register file)
            __builtin_amdgcn_sched_barrier(0);
        }
        // -- V step: O^T += V^T P^T; O^T row 40 (block 1, row 8) is the ones row = the softmax denominator
        const char* vb = open_step(s++);
#pragma unroll
        for (int h2 = 0; h2 < 2; ++h2) {
            h8 vf[2][2];
#pragma unroll
            for (int db = 0; db < 2; ++db)
#pragma unroll
                for (int sb = 0; sb < 2; ++sb) {
                    const int n = (2 * wc + h2) * kXcD + db * 32 + lq;      // < 344: rows past 319 are the stage's padding pieces
                    vf[db][sb] = *reinterpret_cast<const h8*>(vb + n * 64 + (((sb * 2 + half) ^ (3 * ((n >> 3) & 1))) << 4));
                    if (db == 1 && lq == 8) vf[db][sb] = ones;
                }
#pragma unroll
            for (int qb = 0; qb < 2; ++qb)
#pragma unroll
                for (int db = 0; db < 2; ++db)
#pragma unroll
                    for (int sb = 0; sb < 2; ++sb)
                        o[h2 * 2 + qb][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[db][sb], pb[h2 * 2 + qb][sb], o[h2 * 2 + qb][db], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the normalised attention output (fp16) over this wave's own q:  o[st][db][r] is O[query lq][d = 32 db + 8 (r >> 2) + 4 half + (r & 3)]
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const float l_tot = __shfl(o[st][1][4], lq);          // row 40, held by the lower half-wave
        const float inv = 1.0f / l_tot;
        const int qrow = 64 * wr + 32 * (st & 1) + lq;
        const int col0 = (2 * wc + (st >> 1)) * kXcD;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (db * 32 + g * 8 >= kXcD) continue;
                h4 hv;
#pragma unroll
                for (int e = 0; e < 4; ++e) hv[e] = (half_t)(o[st][db][g * 4 + e] * inv);
                *reinterpret_cast<h4*>(img + xc_img(qrow, col0 + db * 32 + g * 8 + half * 4)) = hv;
            }
    }

    // ---- phase 4: x2 = a2 Wo^T + bo + x1 (the step's barrier orders every wave's a2 before the first fragment read) -----------------
    zero_acc();
#pragma unroll 1
    for (int kc = 0; kc < 10; ++kc) {
        const char* buf = open_step(s++);
        gemm_step(buf, kc);
    }
    XC_WAIT_VM0();
    __builtin_amdgcn_s_barrier();                            // every wave is past its last read of a2: x1 comes back into the image
    XC_FENCE();
#pragma unroll
    for (int u = 0; u < 10; ++u) {
        const int pc = u * 512 + tid;
        const int r = pc / 40, ps = pc - r * 40;
        const half_t* src = p.x + (row0 + r) * kXcC + ((ps ^ ((r >> 1) & 7)) << 3);
        __builtin_amdgcn_global_load_lds((xgptr_t)src, (xlptr_t)(img + (u * 8 + wave) * 1024), 16, 0, 0);
    }
    XC_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    XC_FENCE();
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int col = 80 * wc + 16 * j + 4 * q4;
        const f4 bb = *reinterpret_cast<const f4*>(p.bo + col);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            h4* cell = reinterpret_cast<h4*>(img + xc_img(64 * wr + 16 * mi + l16, col));
            const h4 res = *cell;
            h4 hv;
#pragma unroll
            for (int e = 0; e < 4; ++e) hv[e] = (half_t)((acc[mi][j][e] + bb[e]) + (float)res[e]);
            *cell = hv;
        }
    }
    XC_WAIT_VM0();
    __builtin_amdgcn_s_barrier();
    XC_FENCE();
#pragma unroll
    for (int u = 0; u < 10; ++u) {
        const int pc = u * 512 + tid;
        const int r = pc / 40, ps = pc - r * 40;
        const h8 hv = *reinterpret_cast<const h8*>(img + pc * 16);
        *reinterpret_cast<h8*>(p.out + (row0 + r) * kXcC + ((ps ^ ((r >> 1) & 7)) << 3)) = hv;
    }
}

int launch_xattn_chain(const half_t* x, half_t* out, const float* gamma, const float* beta, const half_t* wq, const half_t* wo,
                       const float* bo, const half_t* k, const half_t* vt, long rows, int rows_per_image, int C, int heads, int L, int Lpad,
                       float eps, hipStream_t s) {
    SDMI_REQUIRE(C == kXcC, "cross-attention chain: built for row width C = 320");
    SDMI_REQUIRE(heads * kXcD == C, "cross-attention chain: heads * 40 == C (8 heads of 40)");
    SDMI_REQUIRE(rows > 0 && rows % kXcRows == 0, "cross-attention chain: rows % 128 == 0");
    SDMI_REQUIRE(rows_per_image > 0 && rows_per_image % kXcRows == 0 && rows % rows_per_image == 0,
                 "cross-attention chain: rows_per_image % 128 == 0 (a tile lies in one image) and whole images");
    SDMI_REQUIRE(x && out && gamma && beta && wq && wo && k && vt, "cross-attention chain: null pointer");
    SDMI_REQUIRE(L >= 1, "cross-attention chain: context length L >= 1");
    SDMI_REQUIRE(Lpad >= L && Lpad % 32 == 0, "cross-attention chain: Lpad >= L, a multiple of 32 (whole 32-key blocks of V^T)");
    SDMI_REQUIRE(rows / kXcRows < (1l << 31), "cross-attention chain: too many tiles");
    SDMI_REQUIRE((((uintptr_t)x | (uintptr_t)out | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)wq | (uintptr_t)wo | (uintptr_t)bo |
                   (uintptr_t)k | (uintptr_t)vt) & 15) == 0, "cross-attention chain: 16-byte aligned operands");
    XattnP p{};
    p.x = x; p.out = out; p.gamma = gamma; p.beta = beta; p.wq = wq; p.wo = wo;
    p.bo = bo ? bo : reinterpret_cast<const float*>(zero_page());
    p.k = k; p.vt = vt; p.rows_per_image = rows_per_image; p.L = L; p.Lpad = Lpad; p.eps = eps;
    p.scale_log2 = (1.0f / sqrtf((float)kXcD)) * 1.4426950408889634f;
    p.tau = (float)(g_attn_tau < 0 ? -1 : g_attn_tau > 12 ? 12 : g_attn_tau);          // launch_attention's rule
    // the two projections (what the GEMM family counted for these launches); x1 in, x2 out, the two weight matrices
    ProfScope ps("rowchain_xattn", 4.0 * (double)rows * C * C, 4.0 * (double)rows * C + 4.0 * C * C, s);
    auto kern = rowchain_xattn_kernel;
#ifdef __HIP__
    static PerDeviceOnce attr;
    if (attr.need()) SDMI_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kXcLds));
    hipLaunchKernelGGL(kern, dim3((unsigned)(rows / kXcRows)), dim3(512), kXcLds, s, p);
#else
    hipLaunchKernelGGL(kern, dim3((unsigned)(rows / kXcRows)), dim3(512), 0, s, p);
#endif
    SDMI_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace sdmi
