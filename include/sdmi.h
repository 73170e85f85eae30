/* sdmi.h — C ABI of the MI355X-native Stable Diffusion hot-path engine (libsdmi.so).
 *
 * Drop-in boundary for ONE path of AUTOMATIC1111/stable-diffusion-webui: the txt2img/img2img UNet denoising
 * loop + k-diffusion/DDIM sampler arithmetic + VAE decode.  The reference has no FFI of its
 * own (it is pure Python over torch); each entry point below states the reference interface it replaces
 * (paths relative to /root/reference).  The Python/ctypes binding a webui maintainer adds is in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer on the engine's GPU unless the name ends in _host;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls are asynchronous on it;
 *   - return value: 0 = ok, non-zero = error; sdmi_last_error() returns a thread-local message;
 *   - fp16 = IEEE binary16 ("half"); all accumulation is fp32; activations inside the engine are NHWC fp16;
 *   - no torch / python types appear here.
 */
#ifndef SDMI_H
#define SDMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDMI_VERSION 100

enum { SDMI_F16 = 0, SDMI_F32 = 1 };

typedef struct sdmi_engine sdmi_engine;

int sdmi_version(void);
const char* sdmi_last_error(void);
/* 1 if a gfx950 device is visible to HIP, else 0 (never throws). */
int sdmi_device_ok(void);

/* ------------------------------------------------------------------------------------------------------------
 * Op-level entry points (boundary B2 "SdOptimization", and the units the parity tests exercise one by one).
 * ---------------------------------------------------------------------------------------------------------- */

/* Fused QK^T * scale -> softmax -> PV, never materialising the score matrix.
 * Replaces: the attention math inside every CrossAttention.forward the webui can select —
 *   modules/sd_hijack_optimizations.py:221-281 (split_cross_attention_forward, GPU default),
 *   :508-546 (sdp), :480-503 (xformers), modules/hypernetworks/hypernetwork.py:382-407 (baseline),
 *   algorithm twin modules/sub_quadratic_attention.py:141-215.
 * q   [B, N, ldq]  head h at columns [h*D, (h+1)*D)            (fp16)
 * k   [B, M, ldk]  same head layout                             (fp16)
 * v   [B, M, ldv]  same head layout (row-major; transposed internally into `workspace`)
 * out [B, N, ldo]                                                (fp16)
 * workspace: at least sdmi_attention_workspace_bytes(B,H,M,D) bytes of device memory.
 * D in {40, 64, 80, 128, 160} runs the MFMA kernel; any other D <= 512 runs the generic HIP kernel. */
int64_t sdmi_attention_workspace_bytes(int B, int H, int M, int D);
int sdmi_attention(const void* q, const void* k, const void* v, void* out,
                   int B, int H, int N, int M, int D,
                   int ldq, int ldk, int ldv, int ldo, float scale,
                   void* workspace, int64_t workspace_bytes, void* stream);

/* Single-head attention over a wide head: the VAE mid-block AttnBlock (d = C = 512, N = M = h*w) that every in-tree optimizer
 * also replaces — modules/sd_hijack_optimizations.py:554-610 (cross_attention_attnblock_forward), :613-634 (xformers), :637-655
 * (sdp), :658-676 (sub-quadratic).  Scores are materialised in fp32 one image at a time (GEMM, row softmax, GEMM: the engine's own
 * VAE attention).  q / k / v / out [B, N|M, ld*] fp16, D a multiple of 64, row strides multiples of 8 elements. */
int64_t sdmi_attention_wide_workspace_bytes(int B, int N, int M, int D);
int sdmi_attention_wide(const void* q, const void* k, const void* v, void* out,
                        int B, int N, int M, int D,
                        int ldq, int ldk, int ldv, int ldo, float scale,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Same, with V already transposed by the producer: vt [B, H*D, Mpad] (row = h*D+d, Mpad = vt_ld >= M rounded up to 64,
 * padding columns must be finite).  This is what the engine's UNet uses (its V projection writes V^T directly). */
int sdmi_attention_vt(const void* q, const void* k, const void* vt, void* out,
                      int B, int H, int N, int M, int D,
                      int ldq, int ldk, int vt_ld, int ldo, float scale, int force_generic, void* stream);

/* sdmi_attention_vt with the operands' scaling and the kernel form stated by the caller (tests and timing tools).
 *   prescaled != 0: q and k are ALREADY multiplied by sqrt(scale * log2(e)) each — as the engine's stacked q | k projection leaves them
 *                   for the level-0 self-attention — and `scale` is ignored;
 *   form:           0 = the default dispatch; otherwise an "attn_occ" value that holds for this call only (d = 40: 15, 16, 17, and 27 = 17 for pre-scaled
 *                   operands with the staging address arithmetic out of the KV loop; 27 without prescaled is an error).  The form travels with the call: no
 *                   process-wide knob is touched, other threads' launches are not affected. */
int sdmi_attention_vt_ex(const void* q, const void* k, const void* vt, void* out,
                         int B, int H, int N, int M, int D,
                         int ldq, int ldk, int vt_ld, int ldo, float scale, int prescaled, int form, int force_generic, void* stream);

/* Implicit-GEMM convolution / linear layer on NHWC fp16 activations (MFMA, LDS-staged):
 *   out[m, n] = epilogue( alpha * sum_{tap,c} A(m, tap, c) * W[n, tap*Cin + c] )
 * Replaces the torch ops issued by ldm's ResBlock / Downsample / Upsample / SpatialTransformer / FeedForward modules
 * (third-party; layer names pinned at extensions-builtin/Lora/networks.py:43-98; op inventory SURVEY.md 2.3 K1,K4,K7,K8).
 * All fields are plain values / device pointers.
 *
 * Per batch element z (grid.z, 0 <= z < batch), output row m = (b, yo, xo) and output column n:
 *   out_z[m][n] = alpha * sum_{tap,c} A_z(m, tap, c) * W_z[n][tap*Cin + c] + bias[n or m] + rowbias[b][n] + resid_z[m][n]
 * with A_z read at a0 / a1 + z*a_bs + pixel*lda0 / lda1 + c (both sources move by the same a_bs), W_z at w + z*w_bs, resid_z at
 * resid + z*r_bs + m*ldr + n and out_z stored at out + z*o_bs + m*ldo + n — SDMI_EP_GEGLU: N/2 columns; SDMI_EP_TRANSPOSE:
 * out + z*o_bs + (b*N + n)*ldo + (m - b*Ho*Wo); SDMI_EP_NCHW: out + z*o_bs + ((b*n_real + n)*Ho + yo)*Wo + xo, ldo unused.  All strides
 * count elements.  bias and rowbias are shared by all batch elements.  Only the stored columns of the stored rows are written: the
 * elements between them (ldo wider than the columns, o_bs larger than one element's rows) keep their contents.
 *
 * Zero means: lda0 / lda1 = 0 -> c0 / c1 (dense pixels); ldo = 0 -> the stored columns (N; N/2 with GEGLU; Ho*Wo transposed); ldr = 0
 * -> N; stride = 0 -> 1; alpha = 0 -> 1 (a product scaled by zero cannot be asked for); n_real = 0 -> N; batch <= 0 -> 1.
 * a_bs = 0, w_bs = 0 or r_bs = 0 with batch > 1 is a broadcast: every batch element reads the same A, W or residual.
 *
 * Refused before anything is launched (non-zero return, sdmi_last_error): a null a0 / w / out; B, Hi, Wi, Ho, Wo, N or c0 (c1 with a1)
 * not positive; taps other than 1 / 9; a stride other than 1 / 2; c0 or c1 not a multiple of 8; lda0 < c0 or lda1 < c1; ldo smaller
 * than the stored columns; ldr < N with a residual; n_real outside 1 .. N with SDMI_EP_NCHW; SDMI_EP_GEGLU with N % 64 != 0; a
 * negative batch stride; batch > 1 with o_bs smaller than the elements one batch element stores (o_bs = 0: every element would write
 * the same memory).
 *
 * Alignment.  The MFMA kernels load 16 bytes at a time: they run when N, c0 + c1 (and c0, with a second source) are multiples of 64,
 * lda0 / lda1 multiples of 8, a0 / a1 / w, a column bias and rowbias 16-byte aligned and, with batch > 1, a_bs and w_bs multiples
 * of 8.  Anything else runs the generic kernel, which takes any stride and base (force_generic = 1 asks for it).  On the MFMA
 * kernels the stores are 4 elements wide at least: ldo, ldr and (batch > 1) o_bs, r_bs must be multiples of 4, out 8-byte aligned
 * (16 with SDMI_EP_OUT_F32; 4 with SDMI_EP_NCHW) and resid 8-byte aligned, or the call is refused; multiples of 8 and 16-byte
 * aligned bases get the 16-byte epilogue, with the same bits. */
typedef struct sdmi_conv_desc {
    const void* a0;        /* source 0, NHWC fp16 [B,Hi,Wi,c0] (pixel stride lda0 elements) */
    const void* a1;        /* optional source 1 (channel-concatenated after source 0), or NULL */
    const void* w;         /* packed weights fp16 [N][taps*(c0+c1)], k = tap*Cin + c, tap = ky*3+kx */
    const void* bias;      /* fp32 [N] (or [M] when SDMI_EP_BIAS_ROW), or NULL */
    const void* rowbias;   /* fp32 [B][N] added to every pixel of image b (ResBlock emb add), or NULL */
    const void* resid;     /* fp16 [M][ldr] added before the store, or NULL */
    void* out;             /* fp16 or fp32, row-major [M][ldo] or NCHW fp32 */
    int32_t c0, c1, lda0, lda1;
    int32_t B, Hi, Wi, Ho, Wo;
    int32_t taps;          /* 1 or 9 */
    int32_t stride;        /* 1 or 2 (0 = 1) */
    int32_t pad;           /* 1: symmetric "padding=1"; 0: none (VAE-encoder downsample pads right/bottom only) */
    int32_t up;            /* 1: nearest x2 upsample of the source fused into the gather */
    int32_t N;             /* output channels as packed (multiple of 64 for the MFMA kernel) */
    int32_t n_real;        /* output channels actually stored (NCHW mode), else = N */
    int32_t ldo, ldr;      /* row strides of out / resid in elements (0 = dense) */
    int32_t flags;         /* SDMI_EP_* */
    float alpha;           /* 0 = 1 */
    int32_t batch;         /* grid.z batched GEMM count (>=1) with the strides below (elements) */
    int64_t a_bs, w_bs, o_bs, r_bs;
    int32_t force_generic; /* 1: run the simple non-MFMA HIP kernel (debug / unsupported shapes) */
    int32_t reserved;
    void* splitk_workspace;          /* optional fp32 scratch enabling deterministic split-K on small-M / large-K shapes */
    int64_t splitk_workspace_bytes;  /* >= sdmi_conv_splitk_workspace_bytes(M, N, K, batch) or the workspace is ignored */
} sdmi_conv_desc;

enum {
    SDMI_EP_OUT_F32  = 1,   /* store fp32 instead of fp16 */
    SDMI_EP_GEGLU    = 2,   /* W rows packed in (32 value | 32 gate) groups; out has N/2 columns: a*gelu(g) */
    SDMI_EP_NCHW     = 4,   /* store fp32 NCHW [B][n_real][Ho][Wo] */
    SDMI_EP_BIAS_ROW = 8,   /* bias indexed by output row m instead of column n */
    SDMI_EP_WRAP = 128,     /* 3x3 taps wrap around the image (Conv2d padding_mode = 'circular') instead of reading zero padding */
    SDMI_EP_TRANSPOSE = 64  /* store out^T per image: out[b][n][m - b*Ho*Wo], row stride ldo (fp16; Ho*Wo % 4 == 0; no residual /
                               rowbias): how the V projection is handed to the attention kernel as V^T [C][tokens] */
};
int sdmi_conv_gemm(const sdmi_conv_desc* d, void* stream);
int64_t sdmi_conv_splitk_workspace_bytes(int M, int N, int K, int batch);

/* TEST ENTRY (tests and timing tools; the engine fills these fields itself): sdmi_conv_gemm plus the epilogue forms the public
 * descriptor does not carry.  x == NULL is exactly sdmi_conv_gemm(d, stream).  Nothing here touches a process-wide knob.
 *   stats_out / stats_cpg  GroupNorm statistics of the stored tensor: per (image b, chunk of BM rows, group of stats_cpg channels) the
 *                          mean and the centred sum of squares of the fp16-rounded outputs (of hi + lo with out_lo), fp32, at
 *                          stats_out[((b * stats_nchunk + chunk) * (N / stats_cpg) + g) * 2 + {0, 1}].  stats_nchunk is written back:
 *                          rows per image / BM of the tile that ran, or 0 when the launch could not produce them (nothing is written then).
 *   lnp_out                LayerNorm row partials: per row m and column tile t the sum and the sum of squares of the fp16-rounded
 *                          outputs, at lnp_out[(m * lnp_np + t) * 2 + {0, 1}].  lnp_np is written back (N / BN, or 0: nothing written).
 *   ln_stats, ln_s, ...    with flag SDMI_EP_LNFOLD in d->flags: A is the un-normalised input of a LayerNorm folded into the weights
 *                          (sdmi_ln_fold_weights), out[m][n] = rstd[m] * (acc[m][n] - mean[m] * ln_s[n]) + bias[n].  ln_np == 0: ln_stats
 *                          holds (mean, rstd) per row (sdmi_ln_rowstats); ln_np > 0: [M][ln_np][2] row partials as lnp_out leaves them,
 *                          finished with ln_inv_c = 1 / C and ln_eps.
 *   out_lo / resid_lo      (hi, lo) stream tensors: out_lo receives fp16(x - fp16(x)) of every stored x in the layout of out; resid_lo
 *                          is added with resid, in its layout.
 *   bias_scale             the bias is added as bias * bias_scale (0 = 1).   gate: a device int; the launch is a no-op when it holds 0.
 * Refused before anything is launched, next to what sdmi_conv_gemm refuses: stats_out with stats_cpg <= 0 or N % stats_cpg != 0, or
 * stats_bytes < B * 64 * (N / stats_cpg) * 8; lnp_out with lnp_bytes < M * (N / 64) * 8; SDMI_EP_LNFOLD without ln_stats / ln_s, with
 * ln_stats_bytes < M * max(1, ln_np) * 8 or ln_s_bytes < N * 4; out_lo / resid_lo with out_lo_bytes / resid_lo_bytes smaller than
 * ((M - 1) * ldo + N) * 2 / ((M - 1) * ldr + N) * 2; resid_lo without resid; either pair or SDMI_EP_LNFOLD with batch > 1. */
enum { SDMI_EP_LNFOLD = 0x4000 };
typedef struct sdmi_gemm_extras {
    float* stats_out; int32_t stats_cpg; int32_t stats_nchunk;
    const float* ln_stats; const float* ln_s; int32_t ln_np; float ln_inv_c, ln_eps;
    float* lnp_out; int32_t lnp_np;
    float bias_scale;
    void* out_lo; const void* resid_lo;
    const int32_t* gate;
    int64_t stats_bytes, lnp_bytes, ln_stats_bytes, ln_s_bytes, out_lo_bytes, resid_lo_bytes;
} sdmi_gemm_extras;
int sdmi_conv_gemm_ex(const sdmi_conv_desc* d, sdmi_gemm_extras* x, void* stream);

/* Repack helpers (device side, run once at load): OIHW fp16/fp32 conv weight -> [O][ky*3+kx][I(+pad)] fp16. */
int sdmi_pack_conv_weight(const void* w_oihw, int dtype, void* out_f16, int O, int I, int kh, int kw,
                          int O_pad, int I_pad, int geglu, void* stream);

/* GroupNorm(32 groups, fp32 statistics) [+ SiLU] over NHWC fp16, optionally reading two channel-concatenated sources
 * and writing one tensor.  Replaces ldm GroupNorm32 + SiLU (fp32 contract: modules/devices.py:284-295; SiLU forced at
 * modules/sd_hijack.py:69) and the torch.cat of skip connections (modules/sd_hijack_unet.py:10-33). */
int sdmi_groupnorm(const void* x0, const void* x1, int c0, int c1, const void* gamma_f32, const void* beta_f32,
                   void* out_f16, int B, int HW, int groups, float eps, int silu,
                   void* workspace_f32, int64_t workspace_bytes, void* stream);
int64_t sdmi_groupnorm_workspace_bytes(int B, int HW, int groups);

/* LayerNorm over the last dim of [rows, C] fp16 (fp32 statistics, eps 1e-5). */
int sdmi_layernorm(const void* x, const void* gamma_f32, const void* beta_f32, void* out_f16,
                   int64_t rows, int C, float eps, void* stream);

/* TEST ENTRIES (tests and timing tools) for the norm forms only the engine launches.
 * sdmi_groupnorm_ex: sdmi_groupnorm with pre_nchunk > 0 — the workspace already holds (mean, centred sum of squares) fp32
 * [B][pre_nchunk][groups][2] of HW / pre_nchunk rows each, as sdmi_conv_gemm_ex's stats_out leaves them, and only the apply pass runs
 * (pre_nchunk > 64, negative, or not dividing HW is refused; pre_nchunk == 0 runs the ordinary statistics pass, as sdmi_groupnorm does)
 * — and with x0_lo / x1_lo, the lo halves of (hi, lo) input pairs, or NULL.
 * sdmi_ln_rowstats: (mean, rstd) fp32 [rows][2] of x fp16 [rows][C] (C % 8 == 0, C <= 2048).
 * sdmi_ln_fold_weights: wf[n][k] = fp16(w[n][k] * gamma[k]) for k < C and 0 up to K, s_out[n] = sum_k wf[n][k] (fp32),
 * c_out[n] = sum_k beta[k] * w[n][k] + (bias ? bias[n] : 0); w and wf fp16 [n_rows][K], K >= C.  The product w * gamma (exact in 35 bits)
 * reaches fp16 in ONE rounding on gfx950, where the multiply and the conversion compile to one mixed-precision instruction; a build that
 * rounds to fp32 first (the host emulation) stores another fp16 neighbour for about one element in 2^13.  s_out is the sum of the wf
 * actually stored, so either way the folded epilogue subtracts exactly what the matrix core accumulated. */
int sdmi_groupnorm_ex(const void* x0, const void* x1, int c0, int c1, const void* gamma_f32, const void* beta_f32,
                      void* out_f16, int B, int HW, int groups, float eps, int silu,
                      void* workspace_f32, int64_t workspace_bytes, int pre_nchunk, const void* x0_lo, const void* x1_lo, void* stream);
int sdmi_ln_rowstats(const void* x, void* stats_f32, int64_t rows, int C, float eps, void* stream);
int sdmi_ln_fold_weights(const void* w, const void* gamma_f32, const void* beta_f32, const void* bias_or_null, void* wf, void* s_out,
                         void* c_out, int n_rows, int K, int C, void* stream);

/* TEST ENTRIES for the elementwise helpers only the engine launches (csrc/elementwise.hip), one launch each.  Every entry refuses, before
 * anything is launched, null pointers (other than the ones marked "or NULL"), sizes <= 0, dtype codes other than SDMI_F16 / SDMI_F32 and
 * what is listed with it.
 * sdmi_small_linear: out[b][n] = act_out(sum_k act_in(a[b][k]) * w[n][k] + bias[n]) + add[b][n]; a fp32 [B][lda], w fp16 [N][K] dense,
 *   bias fp32 [N] or NULL, add fp32 [B][ldo] or NULL (may be out itself), out fp32 [B][ldo]; act = SiLU where silu_in / silu_out != 0.
 *   Columns [N, ldo) of out and [K, lda) of a are not touched.  Refused: K % 8, lda % 4, lda < K, ldo < N, a or w off a 16-byte boundary.
 *   The kernel form follows B, K and N (B <= 16, 16 rows x K fp32 within 96 KB of LDS and N >= 256: activations staged in LDS) and the
 *   debug knob small_linear_lds (0: always one wave per column); both forms give the same bits.
 * sdmi_silu_f32: y[i] = x[i] / (1 + expf(-x[i])), fp32, the expression of small_linear's silu_in.
 * sdmi_timestep_embedding: out fp32 [B][dim] = [cos(t[b] f_j) | sin(t[b] f_j)], f_j = expf(-ln(10000) j / (dim / 2)), j < dim / 2, and a
 *   last column of 0 where dim is odd; t [B] in t_dtype.  Refused: dim < 2.
 * sdmi_nchw_to_nhwc: out fp16 [B][HW][cpad] from x [B][C][HW] (x_dtype): channel c = fp16(fp32(x) * scale), or, with mix_w fp32 [C][C]
 *   (and mix_b fp32 [C] or NULL), fp16(mix_b[o] + sum_c mix_w[o][c] * (x[c] * scale)) accumulated with fmaf in c order; with lo_ch != 0
 *   channels [C, 2C) = fp16(v - fp32(fp16(v))), v = fp32(x) * scale; the remaining channels up to cpad are 0.
 *   Refused: C > 16, cpad < C, lo_ch without 2C <= cpad or together with mix_w, mix_b without mix_w.
 * sdmi_add_nchw_residual: f = (fp32(src) + fp32(src_lo)) + fp32(ctrl); dst = fp16(f), dst_lo = fp16(f - fp32(dst)); src / dst (and the
 *   lo halves, both or neither) fp16 NHWC [B][HW][C], dst may be src; ctrl NCHW [B][C][HW] in ctrl_dtype.  Refused: C % 8, one-sided lo.
 * sdmi_ctx_compare: *gate (int32, zeroed by the caller) = 1 if the bits of fp16(src[b][l][c]) differ anywhere from cached[b][l][c];
 *   src [B][L][C] in src_dtype, cached fp16 [B][Lpad][C].  sdmi_ctx_update_gated: if *gate != 0, cached[b][l][c] = fp16(src[b][l][c]) for
 *   l < L; rows [L, Lpad) are never written.  Refused: Lpad < L.
 * sdmi_hn_act: x fp16 [n] in place, x = fp16(act(fp32(x))); kind 0 identity, 1 relu, 2 leakyrelu, 3 elu, 4 hardswish, 5 tanh, 6 sigmoid,
 *   7 silu, 8 gelu (erf), 9 mish, 10 relu6, 11 selu, 12 softplus, 13 softsign, 14 hardtanh, 15 hardsigmoid.  Refused: any other kind.
 * sdmi_axpy_f16: y = fp16(fp32(x) + a * fp32(h)), the product and the sum each rounded to fp32; fp16 [n].
 * sdmi_clip_embed: out fp16 [B][L][C] = fp16(v + pos_emb[l][c]), v = inputs_embeds[b][l][c] (fp32) when given, else
 *   fp32(tok_emb[clamp(tokens[b][l], 0, vocab - 1)][c]); tokens int32 [B][L] (not read with inputs_embeds, may then be NULL),
 *   tok_emb [vocab][C] in tok_dtype, pos_emb fp32 [L][C].  Refused: vocab <= 0.
 * sdmi_clip_pool: pooled fp32 [B][C] = fp32(hidden[b][argmax_l tokens[b][l]][:]), the first maximum; hidden fp16 [B][L][C].
 * sdmi_convert: dst[i] = (dst_dtype)src[i], n elements (F32 -> F16 through the engine's copy-out launch). */
int sdmi_small_linear(const void* a_f32, const void* w_f16, const void* bias_f32, const void* add_f32, void* out_f32, int B, int N, int K,
                      int lda, int ldo, int silu_in, int silu_out, void* stream);
int sdmi_silu_f32(const void* x_f32, void* y_f32, int64_t n, void* stream);
int sdmi_timestep_embedding(const void* t, int t_dtype, void* out_f32, int B, int dim, void* stream);
int sdmi_nchw_to_nhwc(const void* x, int x_dtype, void* out_f16, int B, int C, int HW, int cpad, float scale, const void* mix_w_f32,
                      const void* mix_b_f32, int lo_ch, void* stream);
int sdmi_add_nchw_residual(const void* src_f16, const void* src_lo_f16, const void* ctrl, int ctrl_dtype, void* dst_f16, void* dst_lo_f16,
                           int B, int C, int HW, void* stream);
int sdmi_ctx_compare(const void* src, int src_dtype, const void* cached_f16, int B, int L, int Lpad, int C, void* gate_i32, void* stream);
int sdmi_ctx_update_gated(const void* src, int src_dtype, void* cached_f16, int B, int L, int Lpad, int C, const void* gate_i32,
                          void* stream);
int sdmi_hn_act(void* x_f16, int64_t n, int kind, void* stream);
int sdmi_axpy_f16(void* y_f16, const void* x_f16, const void* h_f16, float a, int64_t n, void* stream);
int sdmi_clip_embed(const void* tokens_i32, const void* tok_emb, int tok_dtype, const void* pos_emb_f32, const void* inputs_embeds_f32,
                    void* out_f16, int B, int L, int C, int vocab, void* stream);
int sdmi_clip_pool(const void* tokens_i32, const void* hidden_f16, void* pooled_f32, int B, int L, int C, void* stream);
int sdmi_convert(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* The feed-forward chain of a BasicTransformerBlock as one launch (csrc/rowchain.hip; row width C = 320, rows % 128 == 0).  It
 * replaces, for the ff third of ldm's BasicTransformerBlock._forward as the webui runs it (modules/sd_hijack_unet.py:83-102), the launch
 * sequence LayerNorm -> GEGLU proj -> Linear -> + x.  (Round 5's cross-attention chain, sdmi_rowchain_xattn* — lane-owns-row, projections
 * folded into per-image matrices — was measured slower than the launches it replaced and removed in round 6; the tiled chain that took
 * its place is sdmi_xattn_chain below.)
 *   sdmi_rowchain_ff_pack     w1 [2*hidden][C] fp16 (torch order: value rows, then gate rows), b1 [2*hidden] fp32 or null,
 *                             w2 [C][hidden] fp16 -> the packed operand stream (sdmi_rowchain_ff_pack_bytes)
 *   sdmi_rowchain_ff          out = x + (w2 GEGLU(w1 LN(x) + b1) + b2) */
int64_t sdmi_rowchain_ff_pack_bytes(int C, int hidden);
int sdmi_rowchain_ff_pack(const void* w1_f16, const void* b1_f32_or_null, const void* w2_f16, void* packs, int C, int hidden,
                          void* stream);
int sdmi_rowchain_ff(const void* x_f16, void* out_f16, const void* ln_gamma_f32, const void* ln_beta_f32, const void* packs,
                     const void* b2_f32_or_null, int64_t rows, int C, int hidden, float eps, void* stream);

/* The cross-attention third of a BasicTransformerBlock as one launch (csrc/xattn_chain.hip): replaces the launch sequence
 * LayerNorm (norm2) -> attn2.to_q -> attention over the text context -> attn2.to_out.0 + bias + x,
 *   out = x + wo attention(wq LN(x), k, vt) + bo
 * with the fp16 rounding points of those launches (LN(x), q, the softmax weights, the attention output, out).  x / out [rows][C] fp16;
 * wq / wo [C][C] fp16 (torch Linear layout, to_q has no bias); bo fp32 [C] or null; k [images][L][C] fp16 = the context's to_k
 * projection, vt [images][C][Lpad] fp16 = its to_v projection transposed (columns >= L are never weighted).  Refused (non-zero, message
 * in sdmi_last_error, nothing written) unless C == 320, heads * 40 == C, rows and rows_per_image are positive multiples of 128, rows is
 * whole images, L >= 1, Lpad >= L is a multiple of 32 and every pointer except bo is non-null and 16-byte aligned. */
int sdmi_xattn_chain(const void* x_f16, void* out_f16, const void* ln_gamma_f32, const void* ln_beta_f32, const void* wq_f16,
                     const void* wo_f16, const void* bo_f32_or_null, const void* k_f16, const void* vt_f16, int64_t rows,
                     int rows_per_image, int C, int heads, int L, int Lpad, float eps, void* stream);


/* Philox4x32-10 + Box-Muller normal draws, bit-compatible with the reference's "NV" noise source
 * (modules/rng_philox.py:32-102): out[i] = randn(counter=[offset,0,i,0], key=seed). */
int sdmi_philox_randn(void* out_f32, int64_t n, uint64_t seed, uint32_t offset, void* stream);

/* Variation seeds: slerp(val, low, high) of modules/rng.py:85-96 on ONE image's noise tensors [C][H][W] (fp32) — the angle per
 * (c, w) column along H, linear fallback low*val + high*(1-val) when the mean cosine exceeds 0.9995 (sic: the reference's weights).
 * scratch: C*W floats.  Called from ImageRNG.first (modules/rng.py:120-127) when subseed_strength != 0. */
int sdmi_slerp(void* out_f32, const void* low_f32, const void* high_f32, float val, int C, int H, int W, void* scratch_f32,
               void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sampler arithmetic (boundary B3): the elementwise work of CFGDenoiser + CompVisDenoiser + the k-diffusion /
 * DDIM update, fused.  x is the fp32 sampler state [B,4,h,w] (NCHW, as the webui keeps it).
 * ---------------------------------------------------------------------------------------------------------- */

/* x_in[r*B + b] = x[b] * c_in[b]  for r in 0..reps-1, written NCHW [reps*B, C, h, w] in out_dtype (SDMI_F16/F32).
 * Replaces modules/sd_samplers_cfg_denoiser.py:203-205 (x_in = cat(cond copies, uncond)) + k-diffusion
 * CompVisDenoiser's `input * c_in` + the cast to dtype_unet (modules/sd_hijack_unet.py:50). c_in_f32 may be NULL (=1). */
int sdmi_cfg_prepare_input(const void* x_f32, const void* c_in_f32, void* x_in, int out_dtype,
                           int B, int reps, int64_t chw, void* stream);

/* The same for checkpoints whose UNet input is cat([x, c_concat], dim=1) — inpainting (9 channels: x | mask | masked-image
 * latent) and InstructPix2Pix (8: x | image latent); ldm's DiffusionWrapper does the cat for conditioning_key "hybrid" /
 * "concat", fed by make_condition_dict at modules/sd_samplers_cfg_denoiser.py:193-209:
 *   x_in[r*B + b, 0:C] = x[b] * c_in[b],   x_in[r*B + b, C:C+Cc] = c_concat[b]   (zeros when bit r of zero_reps is set:
 *   the third, image-unconditional group of the edit model, :209).  x [B,C,h,w], c_concat [B,Cc,h,w] fp32, hw = h*w. */
int sdmi_cfg_prepare_concat(const void* x_f32, const void* c_in_f32, const void* c_concat_f32, void* x_in, int out_dtype,
                            int B, int reps, int C, int Cc, int64_t hw, uint32_t zero_reps, void* stream);

/* denoised[b] = u + (c - u) * cond_scale  with  c = x + eps_c * c_out[b], u = x + eps_u * c_out[b]
 * (eps = [cond(B) | uncond(B)], fp32 NCHW).  Replaces CompVisDenoiser's `input + eps * c_out` and
 * CFGDenoiser.combine_denoised (modules/sd_samplers_cfg_denoiser.py:74-82) for one cond of weight 1 per image.
 * mode 0: sigma-space (above);  mode 1: timestep-space (DDIM): out = eps_u + (eps_c - eps_u) * cond_scale.
 * Optional mask blend (img2img, :174-187): out = out*nmask + init_latent*mask when mask != NULL. */
int sdmi_cfg_combine(const void* x_f32, const void* eps_f32, const void* c_out_f32, float cond_scale, int mode,
                     const void* mask_f32, const void* nmask_f32, const void* init_latent_f32,
                     void* denoised_f32, int B, int64_t chw, void* stream);

/* CFG combine for v-prediction checkpoints (SD 2.x 768-v; `parameterization == "v"`, modules/sd_models_config.py:86-94):
 * each half of the UNet output goes through d = out * c_out[b] + x * c_skip[b] first — k-diffusion's CompVisVDenoiser in
 * sigma space (denoised; c_skip = 1/(s^2+1), c_out = -s/sqrt(s^2+1), selected at modules/sd_samplers_kdiffusion.py:60-62)
 * or CompVisTimestepsVDenoiser.predict_eps_from_z_and_v in timestep space (eps; c_out = sqrt(a_t), c_skip = sqrt(1 - a_t),
 * modules/sd_samplers_timesteps.py:33-45) — then u + (c - u) * cond_scale and the optional mask blend as above. */
int sdmi_cfg_combine_affine(const void* x_f32, const void* out_f32, const void* c_out_f32, const void* c_skip_f32,
                            float cond_scale, const void* mask_f32, const void* nmask_f32, const void* init_latent_f32,
                            void* denoised_f32, int B, int64_t chw, void* stream);

/* k-diffusion sample_euler_ancestral / sample_euler update (pinned k-diffusion@ab527a9; to_d per
 * modules/sd_schedulers.py:10-15):  d=(x-den)/sigma; x+=d*(sigma_down-sigma); x+=noise*s_noise*sigma_up (if noise). */
int sdmi_euler_step(void* x_f32, const void* denoised_f32, const void* noise_f32_or_null,
                    float sigma, float sigma_down, float sigma_up, float s_noise, int64_t n, void* stream);

/* k-diffusion sample_dpmpp_2m update: x = ratio*x - em1*(c1*den - c2*old_den)  (c2 = 0 on first/last step).
   With old_den null the c2 term is absent and c1 still scales den: x = ratio*x - em1*c1*den (the host passes c1 = 1 there). */
int sdmi_dpmpp2m_step(void* x_f32, const void* denoised_f32, const void* old_denoised_f32_or_null,
                      float ratio, float em1, float c1, float c2, int64_t n, void* stream);

/* DDIM update (modules/sd_samplers_timesteps_impl.py:30-36):
 *   pred_x0=(x-sqrt_one_minus_at*e)/sqrt(a_t); x = sqrt(a_prev)*pred_x0 + sqrt(1-a_prev-sigma_t^2)*e + sigma_t*noise. */
int sdmi_ddim_step(void* x_f32, const void* e_t_f32, const void* noise_f32_or_null, void* pred_x0_f32_or_null,
                   float a_t, float a_prev, float sigma_t, float sqrt_one_minus_at, int64_t n, void* stream);

/* y = a*x + b*z elementwise fp32 (x*sigmas[0]; init_latent + noise*sigma: modules/sd_samplers_kdiffusion.py:143,199). */
int sdmi_axpby(void* y_f32, const void* x_f32, float a, const void* z_f32_or_null, float b, int64_t n, void* stream);

/* out = sum_k coefs[k] * terms[k] (1..6 fp32 tensors of n elements, accumulated left to right; out may alias a term).
 * The update rules of the k-diffusion samplers that have no dedicated kernel (Heun, DPM2, DPM2 a, LMS, DPM++ 2S a:
 * names at modules/sd_samplers_kdiffusion.py:11-27) and of PLMS (modules/sd_samplers_timesteps_impl.py:85-137) are
 * linear combinations of x, denoiser outputs and noise; `terms` / `coefs` are HOST arrays. */
int sdmi_lincomb(void* out_f32, const void* const* terms_f32, const float* coefs, int n_terms, int64_t n, void* stream);

/* DPM adaptive (k-diffusion DPMSolver.dpm_solver_adaptive; table row modules/sd_samplers_kdiffusion.py:25): the squared error of the
 * embedded solver pair under the mixed tolerance, sum_i ((lo_i - hi_i) / max(atol, rtol * max(|lo_i|, |prev_i|)))^2, as 256
 * per-block partial sums (fp32, fixed summation order: reproducible); the host adds them and takes sqrt(sum / n). */
int sdmi_dpm_error_partials(const void* x_low_f32, const void* x_high_f32, const void* x_prev_f32, float atol, float rtol,
                            void* partial256_f32, int64_t n, void* stream);

/* Latent upscale of the hires-fix pass: torch.nn.functional.interpolate(samples, size=(ho, wo), mode, antialias=False) on
 * `planes` = B*C fp32 planes of hi x wi (modules/processing.py:1392 with the "Latent*" upscalers of modules/shared.py:54-62).
 * mode: 0 "nearest", 1 "nearest-exact", 2 "bilinear", 3 "bicubic" (align_corners = False, ATen index arithmetic); 4 / 5: bilinear /
 * bicubic with antialias = True ("Latent (antialiased)", "Latent (bicubic antialiased)": ATen's separable area filter — windows that
 * widen with the scale when shrinking, weights renormalised inside the image, Keys a = -0.5 for the cubic). */
int sdmi_latent_resize(const void* in_f32, void* out_f32, int planes, int hi, int wi, int ho, int wo, int mode, void* stream);

/* x = init*mask + nmask*x, all fp32 tensors of n elements: the inpainting blend CFGDenoiser applies before / after
 * denoising (modules/sd_samplers_cfg_denoiser.py:206-209, 279-280). */
int sdmi_mask_blend(void* x_f32, const void* init_f32, const void* mask_f32, const void* nmask_f32, int64_t n, void* stream);

/* clamp((x+1)/2,0,1)*255 truncated to uint8, NCHW fp32 -> NHWC uint8 (modules/processing.py:1004-1005,1034-1035). */
int sdmi_image_to_u8(const void* img_f32_nchw, void* out_u8_nhwc, int B, int C, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Engine (boundaries B1 "SdUnet" and B4 VAE): whole-UNet forward and whole-VAE decode on packed weights.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct sdmi_unet_config {
    int32_t in_channels, out_channels, model_channels;
    int32_t num_levels;
    int32_t channel_mult[8];
    int32_t num_res_blocks;
    int32_t attn_level[8];          /* 1 if that level has SpatialTransformers */
    int32_t transformer_depth[8];
    int32_t num_heads;              /* used when num_head_channels == -1 */
    int32_t num_head_channels;
    int32_t context_dim;
    int32_t adm_in_channels;        /* 0 = none */
    int32_t reserved[4];
} sdmi_unet_config;

typedef struct sdmi_vae_config {
    int32_t ch, num_levels;
    int32_t ch_mult[8];
    int32_t num_res_blocks, in_channels, out_ch, z_channels;
    float scale_factor;
    int32_t reserved[4];
} sdmi_vae_config;

sdmi_engine* sdmi_engine_create(int device);
void sdmi_engine_destroy(sdmi_engine* e);

/* Weight hand-over, one tensor at a time, by checkpoint key WITHOUT the "model.diffusion_model." / "first_stage_model."
 * prefix.  Replaces the torch module tree the reference loader fills (modules/sd_models.py:410-538 load_model_weights):
 * the caller keeps using read_state_dict (:312-329) and streams the dict here.  `data` may be a device or host pointer
 * (on_device flag); fp16 or fp32; shape as in the checkpoint (OIHW conv / [out,in] linear). */
int sdmi_unet_configure(sdmi_engine* e, const sdmi_unet_config* cfg);
int sdmi_unet_load_tensor(sdmi_engine* e, const char* key, const void* data, int dtype, int ndim,
                          const int64_t* shape, int on_device);
int sdmi_unet_finalize(sdmi_engine* e);            /* packs layouts; errors if a required key is missing */

/* Replace ONE conv / linear weight ("<layer>.weight", same shape as loaded) of the finalized UNet: re-packed in place.
 * This is where the weight rewrite of extensions-builtin/Lora/networks.py:411-480 (network_apply_weights: restore the
 * backup, add every loaded network's delta, copy into the layer) lands for a UNet that no longer owns torch modules.
 * Call sdmi_unet_set_context again afterwards (cached cross-attention projections depend on attn2.to_k / to_v). */
int sdmi_unet_update_weight(sdmi_engine* e, const char* key, const void* data, int dtype, int ndim,
                            const int64_t* shape, int on_device);

/* Hypernetworks (modules/hypernetworks/hypernetwork.py): per feature width (320 / 640 / 768 / 1280 ...) a pair of small MLPs that
 * transform the attention context before to_k / to_v — context_k = x + multiplier * MLP_k(x) (HypernetworkModule.forward :104-105,
 * apply_hypernetworks :358-379, called from every CrossAttention.forward: sd_hijack_optimizations.py:231, hypernetwork.py:388).  The
 * engine applies them inside its attention layers (self-attention: on the normalised tokens; cross-attention: on the text context
 * when its K / V are projected).  Hand-over: clear, then per loaded hypernetwork `begin(multiplier)` followed, for every width `dim`
 * and `which` (0 = K module, 1 = V module), by its op sequence in order: linear ([out, in] weight + bias, nn.Linear layout),
 * activation (1 relu, 2 leakyrelu, 3 elu, 4 hardswish = the webui's "swish", 5 tanh, 6 sigmoid, 7 silu, 8 gelu, 9 mish, 10 relu6,
 * 11 selu, 12 softplus, 13 softsign, 14 hardtanh, 15 hardsigmoid), layer norm.  Dropout layers are the identity at inference. */
int sdmi_unet_hypernet_clear(sdmi_engine* e);
int sdmi_unet_hypernet_begin(sdmi_engine* e, float multiplier);
int sdmi_unet_hypernet_linear(sdmi_engine* e, int dim, int which, const void* w, const void* b, int dtype, int out_features,
                              int in_features, int on_device);
int sdmi_unet_hypernet_act(sdmi_engine* e, int dim, int which, int act);
int sdmi_unet_hypernet_layernorm(sdmi_engine* e, int dim, int which, const void* gamma, const void* beta, int dtype, int n, int on_device);

/* The same for a 1-D parameter: "<layer>.bias" of a conv / linear layer, "<norm>.weight" / "<norm>.bias" of a GroupNorm / LayerNorm.
 * Where the bias deltas (`ex_bias`: network_full.py diff_b) and the LyCORIS norm modules (network_norm.py w_norm / b_norm) of
 * extensions-builtin/Lora/networks.py:411-480 land. */
int sdmi_unet_update_vector(sdmi_engine* e, const char* key, const void* data, int dtype, int64_t n, int on_device);

/* out[rows*cols] fp32 = W + scale * (up[rows][rank] @ down[rank][cols]); W / up / down fp16 or fp32 device tensors.
 * The LoRA delta of extensions-builtin/Lora/network_lora.py:65-80 with lyco_helpers.rebuild_conventional (:9-15) and
 * network.py:196-216 finalize_updown (scale = alpha / rank * multiplier) folded into the weight in one pass. */
int sdmi_lora_merge(void* out_f32, const void* w, int w_dtype, const void* up, int up_dtype, const void* down, int down_dtype,
                    int rows, int cols, int rank, float scale, void* stream);

/* The other LyCORIS module types of extensions-builtin/Lora (dispatch order networks.py:26-36), all on fp32 device buffers with the
 * layer's current weight W viewed [rows][cols], cols = Cin*kh*kw; the small factor products they start from are plain
 * sdmi_lora_merge calls over a zero W.
 *   hadamard  LoHa, network_hada.py:28-55:   out = W + scale * a * b                      (a, b = the two rebuilt products)
 *   kron      LoKr, network_lokr.py:19-23:   out = W + scale * kron(w1[r1][c1], w2[r2][c2][k])   (k = kh*kw taps of w2)
 *   ia3       IA3,  network_ia3.py:18-30:    out = W + scale * W * v[col if on_input else row]
 *   dora      DoRA, network.py:175-194:      out = W + mult * ((W + delta) * dora_scale[j] / ||(W + delta)[:, j]|| - W), the
 *             norm per input channel j over (out, kh, kw); delta = the module's updown * calc_scale (fp32 [rows][cin][k]). */
int sdmi_weight_hadamard(void* out_f32, const void* w_f32, const void* a_f32, const void* b_f32, float scale, int64_t n, void* stream);
int sdmi_weight_kron(void* out_f32, const void* w_f32, const void* w1_f32, const void* w2_f32, int r1, int c1, int r2, int c2, int k,
                     float scale, void* stream);
int sdmi_weight_ia3(void* out_f32, const void* w_f32, const void* v_f32, int rows, int cols, int on_input, float scale, void* stream);
int sdmi_weight_dora(void* out_f32, const void* w_f32, const void* delta_f32, const void* dora_scale_f32, int rows, int cin, int k,
                     float mult, void* stream);

int sdmi_vae_configure(sdmi_engine* e, const sdmi_vae_config* cfg);
int sdmi_vae_load_tensor(sdmi_engine* e, const char* key, const void* data, int dtype, int ndim,
                         const int64_t* shape, int on_device);
int sdmi_vae_finalize(sdmi_engine* e);

/* eps = UNet(x, timesteps, context[, y]).  Replaces SdUnet.forward (modules/sd_unet.py:75-83), called from the patched
 * UNetModel.forward (modules/sd_unet.py:86-93, modules/sd_hijack.py:41-45).
 * x [Bn, Cin, h, w] NCHW (io_dtype), timesteps [Bn] (io_dtype), context [Bn, L, context_dim] (io_dtype) or NULL to reuse
 * the K/V projections cached by the previous call / sdmi_unet_set_context, y [Bn, adm] or NULL, out [Bn, Cout, h, w]. */
int sdmi_unet_set_context(sdmi_engine* e, const void* context, int io_dtype, int Bn, int L, void* stream);
/* The same for a caller that cannot tell whether `context` changed since the previous call — the webui hands SdUnet.forward a
 * freshly catenated cond | uncond tensor on every sampling step (modules/sd_samplers_cfg_denoiser.py:246; it only really changes
 * when a prompt-editing schedule switches).  The decision is taken ON THE DEVICE, without a host synchronisation: a compare kernel
 * raises a flag if any fp16-converted element differs from the cached copy, and the copy and all K / V^T projection launches are
 * predicated on that flag (empty launches otherwise).  Follow with sdmi_unet_forward(..., context = NULL, ...). */
int sdmi_unet_set_context_cached(sdmi_engine* e, const void* context, int io_dtype, int Bn, int L, void* stream);
int sdmi_unet_forward(sdmi_engine* e, const void* x, const void* timesteps, const void* context, const void* y,
                      void* out, int io_dtype, int Bn, int h, int w, int L, void* stream);
/* The same with the caller's PROMISES about this call's data as an argument of the call (round 6; ADVICE r4 / VERDICT r5: as sticky
 * engine options — sdmi_engine_set_option "uniform_t" / "cfg_pairs", still accepted by sdmi_unet_forward — a stale promise silently
 * overwrote the second half of a later batch).  call_flags, valid for THIS call only:
 *   SDMI_CALL_UNIFORM_T   every row sits at the same timestep (the samplers' CFG batch, modules/sd_samplers_cfg_denoiser.py:230-246):
 *                         the timestep-embedding path runs for one row; same bits
 *   SDMI_CALL_CFG_PAIRS   rows [Bn/2, Bn) repeat the latent and timestep of rows [0, Bn/2) (the [cond | uncond] batch): the layers in
 *                         front of the first cross-attention run for one half
 *   SDMI_CALL_DERIVE      neither is known (the stock CFG denoiser behind SdUnet.forward, modules/sd_unet.py:86-93): the engine derives
 *                         both from x and timesteps — one synchronising device -> host compare */
enum { SDMI_CALL_UNIFORM_T = 1, SDMI_CALL_CFG_PAIRS = 2, SDMI_CALL_DERIVE = 4 };
/* Extra UNet inputs of SdUnet.forward(x, timesteps, context, *args, **kwargs) (modules/sd_unet.py:76-77, 87-91 pass them through): the
 * ControlNet residuals `control` of ldm's ControlledUnetModel.forward (cldm.py) for the NEXT sdmi_unet_forward[_ex] call only — n =
 * (number of input blocks) + 1 device tensors in the io dtype of that call, NCHW, tensor i shaped like input block i's output
 * [Bn, C_i, h_i, w_i] and the last like the middle block's; numel[i] is checked against that shape.  They are added to the skip
 * connections as the output blocks read them and to the middle block's output; only_mid_control: the last one alone.  n = 0 clears. */
int sdmi_unet_set_control(sdmi_engine* e, const void* const* tensors, const int64_t* numel, int n, int only_mid_control);
int sdmi_unet_forward_ex(sdmi_engine* e, const void* x, const void* timesteps, const void* context, const void* y,
                         void* out, int io_dtype, int Bn, int h, int w, int L, int call_flags, void* stream);

/* image = decoder(post_quant_conv(z / scale_factor)), all B latents in one batched pass.
 * Replaces decode_latent_batch's per-image loop (modules/processing.py:625-672) -> decode_first_stage
 * (modules/sd_samplers_common.py:73-76) -> LatentDiffusion.decode_first_stage / AutoencoderKL.decode (third-party).
 * z [B, 4, h, w] NCHW (io_dtype); out fp32 NCHW [B, 3, 8h, 8w] in [-1, 1] (what the caller .float()s anyway). */
int sdmi_vae_decode(sdmi_engine* e, const void* z, int io_dtype, void* out_f32, int B, int h, int w, void* stream);

/* latent moments = quant_conv(encoder(x)); x [B,3,H,W] NCHW in [-1,1]; out fp32 NCHW [B, 2*z, H/8, W/8] (mean | logvar).
 * Replaces encode_first_stage (modules/sd_samplers_common.py:87-112 -> third-party AutoencoderKL.encode). */
int sdmi_vae_encode(sdmi_engine* e, const void* x, int io_dtype, void* out_f32, int B, int H, int W, void* stream);

/* Introspection for tests / bench. */
int64_t sdmi_engine_arena_bytes(sdmi_engine* e);
int sdmi_engine_set_option(sdmi_engine* e, const char* name, int value);   /* "force_generic", "glds", "trace" (activation taps),
                                                                               "tiling" (p.tiling: padded 3x3 convs wrap around, modules/sd_hijack.py:311-318),
                                                                               "vae_range_extend" (VAE decoder residual stream at 1/64 scale: the
                                                                               engine's form of the fp16 -> fp32 VAE fallback, modules/processing.py:636-665),
                                                                               "cfg_pairs" / "uniform_t" (promises of the caller about the next forwards' x and t:
                                                                               rows [Bn/2, Bn) repeat rows [0, Bn/2); one timestep for all rows),
                                                                               "auto_promises" (both derived per forward from x and t by a synchronising compare:
                                                                               for callers that cannot know), "fuse_rows", "residual_fp32"  */

/* Activation taps for the parity error budget (tests/test_gpu_c1_parity.py): with option "trace" = 1 the engine records, by
 * the reference's module name ("input_blocks.4.1", "middle_block.1.transformer_blocks.0", "decoder.up.2.block.1", ...), the
 * NHWC fp16 output of every block of the LAST UNet forward / VAE decode / VAE encode ("encoder.down.0.block.0", ...) / CLIP
 * forward ("embeddings", "encoder.layers.3.self_attn+x", "encoder.layers.3", "final_layer_norm", "pooled.final_layer_norm":
 * [B][H = L][W = 1][C = hidden]); the tensors stay valid until the next forward
 * (the activation arena never reuses memory within one).  tap_read copies tap `index` ([B][H][W][C] fp16) to a device buffer. */
int sdmi_engine_tap_count(sdmi_engine* e);
int sdmi_engine_tap_info(sdmi_engine* e, int index, char* name_out, int capacity, int64_t* dims_bhwc);
int sdmi_engine_tap_read(sdmi_engine* e, int index, void* out_f16_nhwc, void* stream);

/* Tuning knobs for benchmarks: "gemm_cfg" (-1 heuristic, 0..7 force a tile configuration when it fits the shape),
 * "attn_kvt" (0 heuristic, 64 force 64-key tiles), "attn_tau" (slack of the flash kernels' lazy exponent re-basing in log2 units:
 * default 8; 0 = re-base whenever a running maximum moves, -1 = also rescale O in every tile — both give the round-2 bits),
 * "attn_fold_min_m" (shortest d = 40 self-attention that takes the folded-shift form: default 1024, 0 = never). */
int sdmi_debug_set(const char* name, int value);
/* String-valued knob: "gemm_override" = "M,N,K,taps,kind:cfg:split;..." forces a tile configuration / split-K factor for exact GEMM
 * shapes (kind 0 plain epilogue, 1 GEGLU, 2 transposed output; "" clears) — the in-engine shape autotuner tools/gpu/shape_tune.py. */
int sdmi_debug_set_str(const char* name, const char* value);

/* Optional per-launch HIP-event profiler: between begin and end every kernel launch of the library is bracketed by events
 * on its own stream; end() synchronises once and writes {"kernels":[{"name","launches","ms","flops","bytes"},...]} with the
 * ALGORITHMIC flops / bytes of each launch into json_out. */
int sdmi_profile_begin(void);
int sdmi_profile_end(char* json_out, int capacity);

/* Micro-benchmarks used by bench.py's roofline block (HIP-event timed inside the library; returns ms per launch). */
int sdmi_bench_conv_gemm(const sdmi_conv_desc* d, int iters, float* ms_out, void* stream);

/* ---- CLIP text encoder ---------------------------------------------------------------------------
 * The transformer behind FrozenCLIPEmbedderWithCustomWords.encode_with_transformers (modules/sd_hijack_clip.py:351-360:
 * `self.wrapped.transformer(input_ids=tokens, output_hidden_states=-opts.CLIP_stop_at_last_layers)`, i.e. transformers'
 * CLIPTextModel; in-repo plain-torch twin modules/models/sd3/other_impls.py:61-150): token + position embeddings,
 * `layers` pre-LN blocks (causal self-attention, MLP with quick_gelu or gelu), final LayerNorm.  Prompt parsing, chunking,
 * emphasis and textual-inversion vector injection stay on the host (they feed `inputs_embeds`).  Two slots: SDXL carries
 * two text encoders. */
typedef struct sdmi_clip_config {
    int vocab_size;        /* 49408 */
    int max_positions;     /* 77 */
    int hidden;            /* 768 (CLIP-L), 1280 (OpenCLIP bigG) */
    int layers;            /* 12 / 32 */
    int heads;             /* hidden / 64 */
    int intermediate;      /* 4 * hidden */
    int act;               /* 0 = quick_gelu, 1 = gelu (erf) */
    float eps;             /* LayerNorm eps, 1e-5 */
} sdmi_clip_config;

int sdmi_clip_configure(sdmi_engine* e, int slot, const sdmi_clip_config* cfg);
/* keys as in transformers' CLIPTextModel state dict below "text_model.": "embeddings.token_embedding.weight",
 * "embeddings.position_embedding.weight", "encoder.layers.<i>.{layer_norm1,layer_norm2}.{weight,bias}",
 * "encoder.layers.<i>.self_attn.{q_proj,k_proj,v_proj,out_proj}.{weight,bias}", "encoder.layers.<i>.mlp.{fc1,fc2}.{weight,bias}",
 * "final_layer_norm.{weight,bias}", and optionally "text_projection.weight" [proj_dim, hidden] (nn.Linear layout). */
int sdmi_clip_load_tensor(sdmi_engine* e, int slot, const char* key, const void* data, int dtype, int ndim,
                          const int64_t* shape, int on_device);
int sdmi_clip_finalize(sdmi_engine* e, int slot);
/* tokens int32 [B, L] (device); inputs_embeds fp32 [B, L, hidden] or NULL (token embeddings already looked up / patched by
 * the caller: textual inversion, modules/sd_hijack.py EmbeddingsWithFixes).  Runs the first `layers - skip + 1` blocks
 * (skip = opts.CLIP_stop_at_last_layers >= 1: hidden_states[-skip]) and, if apply_final_ln, final_layer_norm — which is
 * last_hidden_state for skip = 1 and the clip-skip branch of sd_hijack_clip.py:354-356 otherwise; SDXL's CLIP-L takes
 * hidden_states[-2] without the norm (sd_hijack_clip.py:369-377).  out fp32 [B, L, hidden]; pooled fp32 [B, proj_dim or
 * hidden] or NULL = final_layer_norm(last block)'s row at the EOS (largest id) position, times text_projection when loaded
 * (transformers pooler_output / text_embeds; open_clip `pool(ln_final(x)) @ text_projection`, the SDXL "pooled" vector read
 * at modules/sd_hijack_open_clip.py:60-66) — always taken after the LAST block, whatever `skip` is. */
int sdmi_clip_forward(sdmi_engine* e, int slot, const void* tokens_i32, const void* inputs_embeds_f32_or_null, int B, int L,
                      int skip, int apply_final_ln, void* out_f32, void* pooled_f32_or_null, void* stream);

/* ---- RRDBNet upscalers (ESRGAN / Real-ESRGAN) ------------------------------------------------------------------------------------ */

/* One launch of the RRDBNet 3x3 conv (csrc/rrdb.hip): stride 1, pad 1, fp16 NHWC, fp32 accumulation.  Replaces one
 * `lrelu(convK(torch.cat((x, x1, ...), 1)))` / `x5 * 0.2 + x` line of ResidualDenseBlock.forward (basicsr/archs/rrdbnet_arch.py, the
 * webui's modules/esrgan_model.py loads the same network through spandrel): the concat is a channel PREFIX of one 192-wide buffer. */
enum {
    SDMI_RRDB_EP_NONE = 0,   /* acc + bias */
    SDMI_RRDB_EP_LRELU = 1,  /* LeakyReLU(0.2) */
    SDMI_RRDB_EP_RES1 = 2,   /* alpha * v + r1                  (RDB exit x5 * 0.2 + x; alpha = 1: feat + conv_body(...)) */
    SDMI_RRDB_EP_RES2 = 3,   /* beta * (alpha * v + r1) + r2    (third RDB of an RRDB: also the RRDB's out * 0.2 + x) */
    SDMI_RRDB_EP_RELU = 4    /* ReLU                            (the conv_block of a ScuNET ConvTransBlock) */
};
enum {
    SDMI_RRDB_ST_F16 = 0,       /* fp16 NHWC rows of stride ldo, `out` already offset to the first output channel */
    SDMI_RRDB_ST_F32_NCHW = 1,  /* fp32 [B][n_real][H][W] */
    SDMI_RRDB_ST_U8_HWC = 2     /* uint8 [B][H][W][n_real] = round_half_even(clamp(v, 0, 1) * 255): modules/upscaler_utils.py */
};
typedef struct sdmi_rrdb_desc {
    const void* in;        /* fp16 NHWC, row stride lda >= cin; with up = 1 the (H/2) x (W/2) tensor (nearest x2 fused into the gather) */
    const void* w;         /* fp16 [nout][9][cin] (sdmi_pack_conv_weight with O_pad = nout, I_pad = cin) */
    const void* bias;      /* fp32 [nout] or NULL */
    const void* r1;        /* fp16 residual rows (nout channels) of stride ldr1 / ldr2, or NULL */
    const void* r2;
    void* out;
    int32_t B, H, W;       /* output grid */
    int32_t cin;           /* multiple of 32, <= 192 */
    int32_t lda, up;
    int32_t nout;          /* 32 or 64 */
    int32_t n_real;        /* channels stored, <= nout (conv_last: 3) */
    int32_t ldo, ldr1, ldr2;
    int32_t ep, store;
    float alpha, beta;
} sdmi_rrdb_desc;
int sdmi_rrdb_conv(const sdmi_rrdb_desc* d, void* stream);

/* A whole RRDBNet held by an engine (scratch from the engine's arena).  Replaces the model call inside upscale_without_tiling
 * (modules/upscaler_utils.py:44-60, reached from UpscalerESRGAN.do_upscale, modules/esrgan_model.py:36-48, and
 * UpscalerRealESRGAN.do_upscale, modules/realesrgan_model.py:36-69) run on the image whole (ESRGAN_tile = 0).
 * blob: host fp32, for every conv in checkpoint order (conv_first, body.{i}.rdb{1..3}.conv{1..5}, conv_body, conv_up1, conv_up2,
 * conv_hr, conv_last) the OIHW weight followed by the bias; sdmi_esrgan_blob_floats gives its length.  num_feat = 64, growth = 32.
 * in_ch / scale: 3 / 4, 12 / 2 or 48 / 1 (the x2 / x1 models pixel-unshuffle by 2 / 4 in front of conv_first).  NULL on error. */
typedef struct sdmi_esrgan sdmi_esrgan;
int64_t sdmi_esrgan_blob_floats(int num_block, int in_ch);
sdmi_esrgan* sdmi_esrgan_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, int num_block, int in_ch, int scale);
void sdmi_esrgan_destroy(sdmi_esrgan* h);
/* arena bytes a run on B images of H x W needs (the caller refuses inputs that cannot fit) */
int64_t sdmi_esrgan_scratch_bytes(sdmi_esrgan* h, int B, int H, int W);
/* in: RGB, uint8 HWC [B][H][W][3] (in_u8 = 1; divided by 255 on the way in) or fp32 NCHW [B][3][H][W] in [0, 1] (device memory).
 * out: fp32 NCHW [B][3][H s][W s], or (out_u8 = 1) uint8 HWC [B][H s][W s][3] with the reference's clamp / x255 / np.round. */
int sdmi_esrgan_run(sdmi_esrgan* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

/* ---- compact Real-ESRGAN upscalers (SRVGGNetCompact) --------------------------------------------------------------------------------- */

/* One launch of the compact networks' 3x3 conv (csrc/compact.hip): stride 1, pad 1, fp16 NHWC, 32 or 64 input and 64 output channels,
 * fp32 accumulation, the layer's weights and an 18 x 18 halo tile resident in LDS.  Replaces one `conv` + `PReLU` pair of the
 * `for i in range(0, len(self.body)): out = self.body[i](out)` loop of SRVGGNetCompact.forward (realesrgan/archs/srvgg_arch.py:58-60;
 * the webui's modules/realesrgan_model.py loads the network through spandrel), and with SDMI_COMPACT_EP_TAIL the last conv together with
 * `out = self.upsampler(out)`, `base = F.interpolate(x, scale_factor=self.upscale, mode='nearest')`, `out += base` (:62-65). */
enum {
    SDMI_COMPACT_EP_NONE = 0,   /* acc + bias -> fp16 NHWC rows of stride ldo */
    SDMI_COMPACT_EP_PRELU = 1,  /* v > 0 ? v : slope[c] * v (nn.PReLU(num_parameters=64)) -> fp16 NHWC */
    SDMI_COMPACT_EP_TAIL = 2    /* pixel_shuffle(r) + nearest-upsampled `base` -> fp32 NCHW, or uint8 HWC (clamp, x255, np.round) */
};
typedef struct sdmi_compact_desc {
    const void* in;        /* fp16 NHWC, row stride lda >= cin; must not overlap out */
    const void* w;         /* fp16 [64][9][cin] (sdmi_pack_conv_weight with O_pad = 64, I_pad = cin) */
    const void* bias;      /* fp32 [64] or NULL */
    const void* slope;     /* fp32 [64] (PRELU) */
    const void* base;      /* TAIL: the network's input, uint8 [B][H][W][3] (base_u8 = 1; / 255) or fp32 [B][3][H][W] */
    void* out;             /* fp16 rows | TAIL: fp32 [B][3][H r][W r], or (out_u8 = 1) uint8 [B][H r][W r][3] */
    int32_t B, H, W;
    int32_t cin;           /* 32 or 64 */
    int32_t lda, ldo;      /* ldo: fp16 store only (0 with TAIL) */
    int32_t n_real;        /* channels stored, <= 64; TAIL: 3 r^2 */
    int32_t ep;
    int32_t r;             /* TAIL: pixel-shuffle factor 1..4 */
    int32_t base_u8, out_u8;
    int32_t grid_cap;      /* 0: min(tiles, CUs) persistent workgroups; n > 0: at most n */
} sdmi_compact_desc;
int sdmi_compact_conv(const sdmi_compact_desc* d, void* stream);

/* A whole SRVGGNetCompact (num_feat 64, PReLU) held by an engine (scratch from the engine's arena).  Replaces the model call inside
 * upscale_without_tiling / tiled_upscale (modules/upscaler_utils.py:44-60, :63-140, reached from UpscalerRealESRGAN.do_upscale,
 * modules/realesrgan_model.py:36-69, for "R-ESRGAN General 4xV3", "R-ESRGAN General WDN 4xV3" and "R-ESRGAN AnimeVideo", :72-130), run
 * on the image whole.  blob: host fp32, per conv in checkpoint order (body.0, body.2, ...) the OIHW weight, the bias, then (all but the
 * last conv) the 64 PReLU slopes; sdmi_compact_blob_floats gives its length.  NULL on error. */
typedef struct sdmi_compact sdmi_compact;
int64_t sdmi_compact_blob_floats(int num_conv, int scale);
sdmi_compact* sdmi_compact_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, int num_conv, int scale);
void sdmi_compact_destroy(sdmi_compact* h);
/* arena bytes a run on B images of H x W needs: the padded input and two 64-wide low-resolution buffers */
int64_t sdmi_compact_scratch_bytes(sdmi_compact* h, int B, int H, int W);
/* in / out as sdmi_esrgan_run: uint8 HWC or fp32 NCHW in, fp32 NCHW or uint8 HWC [B][H s][W s][3] out (device memory). */
int sdmi_compact_run(sdmi_compact* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

/* ---- SwinIR upscalers ---------------------------------------------------------------------------------------------------------------- */

/* Shifted-window attention of one SwinTransformerBlock (csrc/swinir.hip), window size 8, head dim <= 32.  Replaces, in
 * SwinTransformerBlock.forward (the webui's extensions-builtin/SwinIR/swinir_model_arch.py), `torch.roll(x, (-shift, -shift), (1, 2))`,
 * `window_partition`, WindowAttention.forward between its qkv and proj linears (`q * scale @ k^T + relative_position_bias + mask`,
 * softmax, `@ v`), `window_reverse` and the roll back: the roll and the partition are index arithmetic (a token is read from and
 * written back to its own row), the mask (-100 between tokens of different regions of the shifted grid, applied when shift > 0) is
 * computed, never stored.  Scores, bias, mask and softmax in fp32; the probabilities are rounded to fp16 for the second product.
 * Refused (non-zero, message in sdmi_last_error, nothing written): null pointers; H or W not a positive multiple of 8; D outside 1..32;
 * shift not 0 or 4; ldq < 96 heads; ldo < 32 heads; qkv / out / bias not 16-byte aligned, ldq or ldo not a multiple of 8. */
typedef struct sdmi_swin_attn_desc {
    const void* qkv;       /* fp16 token rows [B*H*W][ldq]: head h has q, k, v in 32-wide slots at columns h*32, (heads + h)*32,
                              (2 heads + h)*32; dims 0 .. D-1 real, the tail of every slot zero */
    const void* bias;      /* fp32 [heads][64][64]: bias[h][a][b] = table[(ya - yb + 7) * 15 + (xa - xb + 7)][h] for window-local tokens a, b */
    void* out;             /* fp16 token rows [B*H*W][ldo]: head h at columns h*32, dims D .. 31 stored as zero; columns >= 32 heads untouched */
    int32_t B, H, W;       /* the token grid (row-major rows) */
    int32_t heads, D;
    int32_t ldq, ldo;
    int32_t shift;         /* 0 | 4 */
    float scale;           /* D^-1/2 */
} sdmi_swin_attn_desc;
int sdmi_swin_attention(const sdmi_swin_attn_desc* d, void* stream);

/* nn.LayerNorm(C) over the first C columns of fp16 rows of stride ld (norm1 / norm2 of a block, patch_embed.norm, the final norm): fp32
 * statistics, centred variance.  The engine's token rows are C rounded up to 64 wide (the MFMA GEMMs read dense multiples of 64):
 * columns C .. roundup(C, 64) - 1 of `out` are written as zeros.  gamma / beta fp32 [C].  Refused: null pointers, ld < roundup(C, 64),
 * odd ld.  sdmi_layernorm (dense rows of C) is unchanged. */
int sdmi_swin_layernorm(const void* x, const void* gamma, const void* beta, void* out, int64_t rows, int C, int ld, float eps, void* stream);

/* A whole SwinIR network with the `nearest+conv` upsampler (the real-world SR models: SwinIR-L x4 GAN, the M models x4 / x2) held by an
 * engine (scratch from the engine's arena).  Replaces the model call inside UpscalerSwinIR.do_upscale / `upscale` / `inference`
 * (extensions-builtin/SwinIR/scripts/swinir_model.py), run on the image whole instead of in SWIN_tile tiles.  Fixed: window_size 8, head
 * dim <= 32, 3 channels in / out, num_feat 64, img_range 1, scale 4 or 2.
 * blob: host fp32, every tensor flattened, in this order (weight then bias for convs, linears and norms):
 *   conv_first; patch_embed.norm;
 *   per layer i, per block j: norm1, attn.relative_position_bias_table [225][heads], attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2;
 *     then the layer's conv (resi_3conv: conv.0, conv.2, conv.4);
 *   norm; conv_after_body (resi_3conv: .0, .2, .4); conv_before_upsample.0; conv_up1; conv_up2 (scale 4 only); conv_hr; conv_last.
 * sdmi_swinir_blob_floats gives its length (0 for a config the engine refuses).  NULL on error: a blob of another length,
 * num_heads * 32 < embed_dim, embed_dim not a multiple of num_heads, embed_dim % 4 != 0 or embed_dim / 4 > 64 with resi_3conv,
 * scale not 2 or 4, more than 16 layers. */
typedef struct sdmi_swinir_config {
    int32_t embed_dim;
    int32_t num_layers;
    int32_t depths[16];    /* blocks per layer (RSTB) */
    int32_t num_heads;
    int32_t mlp_hidden;    /* mlp_ratio * embed_dim */
    int32_t resi_3conv;    /* 0: one 3x3 conv closes a layer; 1: 3x3 (C -> C/4), 1x1, 3x3 (C/4 -> C) with LeakyReLU(0.2) between */
    int32_t scale;         /* 4 | 2 */
} sdmi_swinir_config;
typedef struct sdmi_swinir sdmi_swinir;
int64_t sdmi_swinir_blob_floats(const sdmi_swinir_config* cfg);
sdmi_swinir* sdmi_swinir_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, const sdmi_swinir_config* cfg);
void sdmi_swinir_destroy(sdmi_swinir* h);
/* arena bytes a run on B images of H x W needs (0 for a refused size) */
int64_t sdmi_swinir_scratch_bytes(sdmi_swinir* h, int B, int H, int W);
/* in / out as sdmi_esrgan_run: uint8 HWC or fp32 NCHW in, fp32 NCHW or uint8 HWC [B][H s][W s][3] out (device memory).  Any H, W >= 8: the
 * image is reflect-padded to multiples of 8 on the way in and the output cropped.  Refused: a side below 8, tensors of 2^31 elements. */
int sdmi_swinir_run(sdmi_swinir* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

/* ---- Swin2SR upscalers --------------------------------------------------------------------------------------------------------------- */

/* Cosine window attention of one Swin-V2 block (csrc/swinir.hip), window size 8, head dim <= 32: sdmi_swin_attention's geometry,
 * layout, roll / partition / mask handling (-100, not -inf) and refusals, with WindowAttention.forward of Swin2SR's
 * network_swin2sr.py between its qkv and proj linears:
 *   softmax(normalize(q) normalize(k)^T * exp(min(logit_scale, ln 100)) + 16 sigmoid(cpb_mlp(coords))[index] + mask) v.
 * The first product runs on the fp16 q / k as stored; the fp32 score is multiplied by 1 / max(|q|, 1e-12), 1 / max(|k|, 1e-12) (fp32,
 * from the same values) and head_scale[h].  A token whose q or k slot is all zero scores bias + mask.  Refused in addition: a null or
 * misaligned (4 bytes) head_scale. */
typedef struct sdmi_swin2_attn_desc {
    const void* qkv;       /* as sdmi_swin_attn_desc */
    const void* bias;      /* fp32 [heads][64][64]: bias[h][a][b] = 16 sigmoid(table)[(ya - yb + 7) * 15 + (xa - xb + 7)][h] */
    void* out;
    int32_t B, H, W;
    int32_t heads, D;
    int32_t ldq, ldo;
    int32_t shift;         /* 0 | 4 */
    const void* head_scale;    /* fp32 [heads]: exp(min(logit_scale, ln 100)) */
} sdmi_swin2_attn_desc;
int sdmi_swin2_attention(const sdmi_swin2_attn_desc* d, void* stream);

/* res-post-norm of a Swin-V2 block: out = resid + nn.LayerNorm(C)(y) over the first C columns of fp16 rows of stride ld, fp32 statistics,
 * centred variance, the fp32 sum rounded once.  Columns C .. roundup(C, 64) - 1 of `out` are written as zeros; out == resid is allowed
 * (the stream updated in place), y == out is not.  Refused: null pointers, ld < roundup(C, 64), odd ld, y == out. */
int sdmi_swin_layernorm_add(const void* y, const void* gamma, const void* beta, const void* resid, void* out, int64_t rows, int C, int ld,
                            float eps, void* stream);

/* A whole Swin2SR network (Swin2SR.forward of network_swin2sr.py; the webui's swinir_model_arch_v2.py for *.v2.pth files) held by an
 * engine, the twin of sdmi_swinir_*: the trunk is SwinIR's with Swin-V2 blocks (x = x + norm1(attn(x)); x = x + norm2(mlp(x))).
 * Fixed: window_size 8, head dim <= 32, 3 channels in / out, num_feat 64, img_range 1.
 * upsampler 0 `nearest+conv` (scale 4): SwinIR's tail.  1 `pixelshuffle` (scale 2, 3, 4): conv_before_upsample.0 + LeakyReLU(0.01),
 * per step a 3x3 conv 64 -> 4*64 (9*64 for x3) and PixelShuffle, conv_last.  2 `pixelshuffledirect` (scale 2, 3, 4): one 3x3 conv
 * C -> 3 scale^2 and PixelShuffle(scale).
 * blob: host fp32, every tensor flattened, in this order (weight then bias for convs, linears and norms):
 *   conv_first; patch_embed.proj (the 1x1 conv C -> C of Swin2SR's PatchEmbed; the identity for a network without one); patch_embed.norm;
 *   per layer i, per block j: attn.qkv weight, a [3C] bias (q_bias | 0 | v_bias); the bias table 16 sigmoid(cpb_mlp(coords)) [225][heads];
 *     head_scale [heads] = exp(min(logit_scale, ln 100)); attn.proj; norm1; mlp.fc1; mlp.fc2; norm2;
 *     then the layer's conv (resi_3conv: conv.0, conv.2, conv.4), the layer's own patch_embed.proj already multiplied into the last;
 *   norm; conv_after_body (resi_3conv: .0, .2, .4);
 *   upsampler 0: conv_before_upsample.0; conv_up1; conv_up2; conv_hr; conv_last
 *   upsampler 1: conv_before_upsample.0; upsample.0; upsample.2 (scale 4 only); conv_last
 *   upsampler 2: upsample.0
 * sdmi_swin2sr_blob_floats gives its length (0 for a config the engine refuses).  NULL on error: sdmi_swinir_create's refusals, an
 * upsampler outside 0..2, a scale its upsampler does not have. */
typedef struct sdmi_swin2sr_config {
    int32_t embed_dim;
    int32_t num_layers;
    int32_t depths[16];
    int32_t num_heads;
    int32_t mlp_hidden;
    int32_t resi_3conv;
    int32_t upsampler;     /* 0: nearest+conv; 1: pixelshuffle; 2: pixelshuffledirect */
    int32_t scale;         /* 4 for upsampler 0; 2 | 3 | 4 otherwise */
} sdmi_swin2sr_config;
typedef struct sdmi_swin2sr sdmi_swin2sr;
int64_t sdmi_swin2sr_blob_floats(const sdmi_swin2sr_config* cfg);
sdmi_swin2sr* sdmi_swin2sr_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, const sdmi_swin2sr_config* cfg);
void sdmi_swin2sr_destroy(sdmi_swin2sr* h);
int64_t sdmi_swin2sr_scratch_bytes(sdmi_swin2sr* h, int B, int H, int W);
/* in / out, padding, crop and refusals as sdmi_swinir_run */
int sdmi_swin2sr_run(sdmi_swin2sr* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

/* ---- ScuNET denoisers / upscalers ------------------------------------------------------------------------------------------------------ */

/* The transformer `Block` of one ConvTransBlock (csrc/scunet.hip), window size 8, head dim 32, trans_dim C = 32 (1 head) or 64 (2 heads),
 * as ONE launch: a workgroup per 8 x 8 window.  Replaces, in Block.forward / WMSA.forward of network_scunet.py,
 *   x = x + msa(ln1(x));  x = x + mlp(ln2(x))
 * with msa = roll by (-shift, -shift), window partition, embedding_layer, `einsum(q, k) * 32^-1/2 + relative bias`, the 'SW' mask,
 * softmax, `@ v`, linear, window merge, roll back, and mlp = Linear, exact GELU, Linear.  The roll and the partition are index arithmetic
 * (a token is read from and written back to its own row), the mask is computed (shift 4: in the last row of windows pairs with
 * (ya < 4) != (yb < 4) get -inf, in the last column pairs with (xa < 4) != (xb < 4)).  LN statistics, scores, softmax, GELU and the
 * residual sums are fp32; normalised rows, q / k / v, probabilities, the intermediate x and the hidden layer are rounded to fp16 on chip
 * and never written to memory.  `out` may alias `x` (a window loads its 64 rows before it stores any).
 * Refused (non-zero, message in sdmi_last_error, nothing written): null descriptor or pointers; C not 32 or 64; shift not 0 or 4; H or W
 * not a positive multiple of 8; ldx or ldo below C; x / out / packs / bias not 16-byte aligned, ldx or ldo not a multiple of 8;
 * B*H*W of 2^31 tokens. */
typedef struct sdmi_scu_block_desc {
    const void* x;         /* fp16 token rows [B*H*W][ldx]; columns 0 .. C-1 are the input (offset the pointer to read a column range) */
    void* out;             /* fp16 token rows [B*H*W][ldo]; columns 0 .. C-1 are written, the rest of a row is untouched */
    const void* packs;     /* sdmi_scu_block_pack's output for this C */
    const void* bias;      /* fp32 [C / 32][64][64]: bias[h][a][b] = relative_position_params[h][ya - yb + 7][xa - xb + 7] */
    int32_t B, H, W;       /* the token grid (row-major rows) */
    int32_t C;             /* 32 | 64 */
    int32_t ldx, ldo;
    int32_t shift;         /* 0 ('W' blocks) | 4 ('SW' blocks) */
} sdmi_scu_block_desc;
int sdmi_scu_block(const sdmi_scu_block_desc* d, void* stream);
/* The Block's weights (device memory, torch layouts: fp16 [out][in] matrices, fp32 vectors) -> the operand image the kernel stages:
 *   ln1.weight, ln1.bias [C]; msa.embedding_layer [3C][C] + [3C]; msa.linear [C][C] + [C]; ln2.weight, ln2.bias [C];
 *   mlp.0 [4C][C] + [4C]; mlp.2 [C][4C] + [C]  ->  packs (sdmi_scu_block_pack_bytes(C) bytes, 16-byte aligned; 0 bytes for a refused C).
 * Refused: C not 32 or 64, a null pointer, misaligned packs. */
int64_t sdmi_scu_block_pack_bytes(int C);
int sdmi_scu_block_pack(const void* ln1_g, const void* ln1_b, const void* wqkv_f16, const void* bqkv, const void* wproj_f16, const void* bproj,
                        const void* ln2_g, const void* ln2_b, const void* w1_f16, const void* b1, const void* w2_f16, const void* b2,
                        void* packs, int C, void* stream);

/* A whole SCUNet (in_nc 3, dim 64, head dim 32, window 8; "ScuNET GAN" / "ScuNET PSNR" are depths 4 x 7) held by an engine (scratch from
 * the engine's arena, a fixed set of buffers whatever the depths).  Replaces the model call inside UpscalerScuNET.do_upscale
 * (extensions-builtin/ScuNET/scripts/scunet_model.py), run on the image whole instead of in SCUNET_tile tiles.  Scale 1.
 * blob: host fp32, every tensor flattened in checkpoint layout, in this order:
 *   m_head.0.weight [64][3][3][3];
 *   for the stages m_down1, m_down2, m_down3, m_body, m_up3, m_up2, m_up1 (conv_dim = trans_dim = 32, 64, 128, 256, 128, 64, 32):
 *     (m_up* only, first) the ConvTranspose2d weight [4c][2c][2][2];
 *     per block: trans_block.ln1.weight, .bias; msa.relative_position_params [c/32][15][15]; msa.embedding_layer.weight, .bias;
 *       msa.linear.weight, .bias; ln2.weight, .bias; mlp.0.weight, .bias; mlp.2.weight, .bias; conv1_1.weight, .bias; conv1_2.weight, .bias;
 *       conv_block.0.weight; conv_block.2.weight;
 *     (m_down* only, last) the stride-2 Conv2d weight [4c][2c][2][2];
 *   m_tail.0.weight [3][64][3][3].
 * Block i of a stage is 'W' for even i, 'SW' for odd i.  sdmi_scunet_blob_floats gives the blob's length (0 for a config the engine
 * refuses).  dim is fixed at 64: a checkpoint of another width has a blob of another length.  NULL on error: a null argument, a depth
 * outside 1..64, a blob of another length. */
typedef struct sdmi_scunet_config {
    int32_t depths[7];     /* blocks of m_down1, m_down2, m_down3, m_body, m_up3, m_up2, m_up1, each 1 .. 64 */
} sdmi_scunet_config;
typedef struct sdmi_scunet sdmi_scunet;
int64_t sdmi_scunet_blob_floats(const sdmi_scunet_config* cfg);
sdmi_scunet* sdmi_scunet_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, const sdmi_scunet_config* cfg);
void sdmi_scunet_destroy(sdmi_scunet* h);
/* arena bytes a run on B images of H x W needs (0 for a refused size) */
int64_t sdmi_scunet_scratch_bytes(sdmi_scunet* h, int B, int H, int W);
/* in / out as sdmi_esrgan_run: uint8 HWC or fp32 NCHW in, fp32 NCHW or uint8 HWC [B][H][W][3] out (device memory).  Any H, W >= 1: the
 * image is padded right / bottom to multiples of 64 by replication on the way in and the output cropped.  Refused: null pointers, an
 * empty image, tensors of 2^31 elements (B * roundup(H, 64) * roundup(W, 64) * 64). */
int sdmi_scunet_run(sdmi_scunet* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

/* ---- DAT upscalers ------------------------------------------------------------------------------------------------------------------- */

/* All DAT token tensors below are fp16 rows with a head's D <= 32 channels in a 32-wide slot (dims D .. 31 zero): channel h * D + d of
 * the network sits at column h * 32 + d.  Every entry refuses (non-zero return, message in sdmi_last_error, nothing written) what its
 * comment lists. */

/* The spatial window attention of one adaptive spatial attention block (csrc/dat.hip), both branches in one launch: heads
 * [0, heads / 2) attend in windows of s0 rows x s1 columns, heads [heads / 2, heads) in windows of s1 rows x s0 columns.  Replaces, between
 * the qkv and proj linears, the zero padding of the q / k / v grids right and bottom to multiples of max(s0, s1) (padded tokens are
 * q = k = v = 0 and take part as keys with score 0 + bias), torch.roll by minus half the window on the padded grid (shift_h, shift_w =
 * s0 / 2, s1 / 2; branch 1 by s1 / 2, s0 / 2), the window partition, `(q * scale) k^T + bias[h][rel]` (+ the region mask of the padded
 * grid, -100 between tokens of different regions, when shifted), softmax, `@ v`, the inverses, and the crop to H x W: all index
 * arithmetic, no rolled copy, mask or score tensor in memory.  Scores, bias, mask and softmax in fp32; the probabilities are rounded to
 * fp16 for the second product.
 * Refused: null descriptor / pointers; B, H or W < 1; heads odd or < 2; D outside 1..32; a split other than (8, 16) and (8, 32); a shift
 * other than (0, 0) and (s0 / 2, s1 / 2); ldq < 96 heads; ldo < 32 heads; qkv / out not 16-byte aligned, a bias table not 4-byte aligned,
 * ldq or ldo not a multiple of 8; 2^31 padded tokens. */
typedef struct sdmi_dat_attn_desc {
    const void* qkv;       /* fp16 token rows [B*H*W][ldq]: head h has q, k, v at columns h*32, (heads + h)*32, (2 heads + h)*32 */
    const void* bias0;     /* fp32 [(2 s0 - 1)(2 s1 - 1)][heads / 2]: branch 0's dynamic position bias at the offsets (dy, dx), dy in
                              [1 - s0, s0 - 1], dx in [1 - s1, s1 - 1], row-major; read at (ya - yb + s0 - 1)(2 s1 - 1) + (xa - xb + s1 - 1) */
    const void* bias1;     /* fp32 [(2 s1 - 1)(2 s0 - 1)][heads / 2]: branch 1's, with s1 and s0 in each other's places */
    void* out;             /* fp16 token rows [B*H*W][ldo]: head h at columns h*32, dims D .. 31 stored as zero; columns >= 32 heads untouched */
    int32_t B, H, W;       /* the token grid (row-major rows), any size */
    int32_t heads, D;
    int32_t ldq, ldo;
    int32_t s0, s1;        /* (8, 16) | (8, 32) */
    int32_t shift_h, shift_w;  /* (0, 0) | (s0 / 2, s1 / 2) */
    float scale;           /* D^-1/2 */
} sdmi_dat_attn_desc;
int sdmi_dat_window_attention(const sdmi_dat_attn_desc* d, void* stream);

/* Channel attention of one adaptive channel attention block, first launch: per (image, head) and per block of 512 tokens the fp32 sums
 * over the block's tokens n of q[n][i] k[n][j] (i, j < 32), q[n][i]^2 and k[n][j]^2.  qkv as above ([B*N][ldq]; only q and k are read);
 * partials fp32 [B][heads][ceil(N / 512)][1088]: the 32 x 32 products at i * 32 + j, then the 32 + 32 squares.  Every sum is taken in token
 * order by one thread.  Refused: null pointers; B or N < 1; heads outside 1..1024; ldq < 64 heads; qkv / partials not 16-byte aligned, ldq
 * not a multiple of 8; 2^31 tokens. */
int sdmi_dat_channel_gram(const void* qkv, void* partials, int B, int N, int heads, int ldq, void* stream);
/* ... second launch: the partials added in block order (no atomics: two runs give the same bits), then
 *   A[i][j] = softmax_j(temperature[h] * G[i][j] / (max(|q_i|, 1e-12) max(|k_j|, 1e-12))),  i, j < D,
 * in fp32, written as fp16 into the head's diagonal block of A [B][32 heads][32 heads] (rows h*32 + i, columns h*32 + j), zeros
 * everywhere else: att = v A^T is then one batched 1x1 sdmi_conv_gemm with A as per-image weights.  temperature fp32 [heads].
 * Refused: null pointers; B or N < 1; D outside 1..32; partials / A not 16-byte aligned, temperature not 4-byte aligned. */
int sdmi_dat_channel_softmax(const void* partials, const void* temperature, void* A, int B, int N, int heads, int D, void* stream);

/* Depthwise 3x3 conv with zero padding on fp16 token rows x [B*H*W][ldx] (C channels read, C % 8 == 0): w fp32 [9][C] (tap (dy + 1) * 3 +
 * dx + 1 first, then the channel), bias fp32 [C], fp32 sums.  ep 0: out = GELU(conv) (exact erf form; the adaptive interaction module's
 * conv, its BatchNorm folded into w and bias).  ep 1: out = conv * mul (the feed-forward gate x1 * dwconv(norm(x2)); mul [B*H*W][ldm]).
 * out [B*H*W][ldo] must not alias x or mul.  Refused: null pointers (mul with ep 1); ep outside 0..1; an empty tensor; C % 8 != 0; a row
 * stride below C or not a multiple of 8; x / mul / out not 16-byte aligned; out aliasing an input. */
int sdmi_dat_dwconv3x3(const void* x, const void* w, const void* bias, const void* mul, void* out, int B, int H, int W, int C, int ldx, int ldm,
                       int ldo, int ep, void* stream);

/* The channel gate of the adaptive interaction module: gate fp32 [B][C] = sigmoid(w2 GELU(w1 mean_n(x[b][n]) + b1) + b2) of the fp16
 * token rows x [B*N][ld]: global average pool, Conv1x1 C -> C8 with its BatchNorm folded in (w1 fp32 [C8][C], b1 [C8]), GELU, Conv1x1
 * C8 -> C (w2 fp32 [C][C8], b2 [C]).  Two launches: per block of 256 tokens the sums of every channel into ws (fp32
 * [B][ceil(N / 256)][C]; strided token groups added in order, then the groups in order), then one workgroup per image adds the blocks
 * in order: every sum has one fixed order, two runs give the same bits.  Refused: null pointers; B or N < 1; C not a multiple of 8 in
 * 8..1024; C8 outside 1..128; ld < C or not a multiple of 8; x not 16-byte aligned, an fp32 argument not 4-byte aligned; 2^31 tokens. */
int sdmi_dat_pool_gate(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, void* ws, void* gate, int B, int N, int C,
                       int C8, int ld, void* stream);

/* The spatial gate and the sum that attn.proj reads, one pass per token row:
 *   sg = sigmoid(w2 . GELU(w1 s + b1) + b2)   (Conv1x1 C -> C16 with its BatchNorm folded in, GELU, Conv1x1 C16 -> 1)
 *   out = s * gate[image] + t * sg
 * with (s, t) = (att, conv) in a spatial block — out = att sigmoid(cmap(conv)) + sigmoid(smap(att)) conv — and (conv, att) in a channel
 * block — out = att sigmoid(smap(conv)) + conv sigmoid(cmap(att)); `gate` is sdmi_dat_pool_gate of t.  Refused: null pointers; rows not a
 * positive multiple of rows_per_image; C not a multiple of 64 in 64..512; C16 < 1 or C16 * C > 8192; a row stride below C; an fp32
 * argument not 4-byte aligned. */
typedef struct sdmi_dat_aim_desc {
    const void* s;         /* fp16 rows [rows][lds] */
    const void* t;         /* fp16 rows [rows][ldt] */
    const void* gate;      /* fp32 [rows / rows_per_image][C] */
    const void* w1;        /* fp32 [C16][C] */
    const void* b1;        /* fp32 [C16] */
    const void* w2;        /* fp32 [C16] */
    float b2;
    void* out;             /* fp16 rows [rows][ldo]; columns >= C untouched */
    int64_t rows;
    int32_t rows_per_image, C, C16;
    int32_t lds, ldt, ldo;
} sdmi_dat_aim_desc;
int sdmi_dat_aim_combine(const sdmi_dat_aim_desc* d, void* stream);

/* A whole DAT network (DAT.forward of basicsr's dat_arch.py with upsampler `pixelshuffle` and resi_connection `1conv`; the webui's
 * "DAT x2" / "DAT x3" / "DAT x4" of modules/dat_model.py) held by an engine (scratch from the engine's arena, a fixed set of buffers
 * whatever the depths).  Replaces the model call inside UpscalerDAT.do_upscale, run on the image whole instead of in DAT_tile tiles.
 * Fixed: head dim <= 32, an even head count, split (8, 16) or (8, 32), 3 channels in / out, num_feat 64, img_range 1, scale 2, 3 or 4.
 * Block j of a group is a spatial block for even j, a channel block for odd j; it is shifted when (group i even, j > 0, (j - 2) % 4 == 0)
 * or (i odd, j % 4 == 0).  C8 = embed_dim / 8, C16 = embed_dim / 16 (integer division), half = ffn_hidden / 2.
 * blob: host fp32, every tensor flattened in the checkpoint's channel order, in this order (weight then bias for convs, linears, norms):
 *   conv_first; before_RG.1;
 *   per group i, per block j:
 *     norm1; attn.qkv;
 *     spatial blocks: the dynamic position bias of attns.0 evaluated at its offsets [(2 s0 - 1)(2 s1 - 1)][heads / 2], then attns.1's
 *       [(2 s1 - 1)(2 s0 - 1)][heads / 2];  channel blocks: attn.temperature [heads];
 *     attn.dwconv with its BatchNorm folded in: [C][9], [C];
 *     attn.channel_interaction: .1 with .2 (BatchNorm) folded in [C8][C], [C8]; .4 [C][C8], [C];
 *     attn.spatial_interaction: .0 with .1 folded in [C16][C], [C16]; .3 [C16], [1];
 *     attn.proj; norm2; ffn.fc1 [ffn_hidden][C]; ffn.sg.norm [half]; ffn.sg.conv [half][9], [half]; ffn.fc2 [C][half];
 *     then the group's conv [C][C][3][3];
 *   norm; conv_after_body; conv_before_upsample.0; upsample.0; upsample.2 (scale 4 only); conv_last.
 * sdmi_dat_blob_floats gives its length (0 for a config the engine refuses).  NULL on error: a null argument, a blob of another length,
 * embed_dim not a multiple of num_heads, num_heads odd, num_heads * 32 < embed_dim, num_heads * 32 > 512, embed_dim < 16, a split other
 * than (8, 16) and (8, 32), ffn_hidden odd or < 2, a scale other than 2, 3, 4, more than 16 groups, a depth outside 1..64. */
typedef struct sdmi_dat_config {
    int32_t embed_dim;
    int32_t num_layers;
    int32_t depths[16];    /* blocks per residual group */
    int32_t num_heads;
    int32_t split0, split1;
    int32_t ffn_hidden;    /* expansion_factor * embed_dim */
    int32_t scale;         /* 2 | 3 | 4 */
} sdmi_dat_config;
typedef struct sdmi_dat sdmi_dat;
int64_t sdmi_dat_blob_floats(const sdmi_dat_config* cfg);
sdmi_dat* sdmi_dat_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, const sdmi_dat_config* cfg);
void sdmi_dat_destroy(sdmi_dat* h);
/* arena bytes a run on B images of H x W needs (0 for a refused size) */
int64_t sdmi_dat_scratch_bytes(sdmi_dat* h, int B, int H, int W);
/* in / out as sdmi_esrgan_run: uint8 HWC or fp32 NCHW in, fp32 NCHW or uint8 HWC [B][H s][W s][3] out (device memory).  Any H, W >= 1:
 * the network's own convs run on the H x W grid, only the attention windows see a padded grid.  Refused: null pointers, an empty image,
 * tensors of 2^31 elements. */
int sdmi_dat_run(sdmi_dat* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

/* ---- HAT upscalers ------------------------------------------------------------------------------------------------------------------- */

/* HAT token tensors are fp16 rows in the DAT section's layout: a head's D <= 32 channels in a 32-wide slot (dims D .. 31 zero), channel
 * h * D + d of the network at column h * 32 + d.  Every entry refuses (non-zero return, message in sdmi_last_error, nothing written) what
 * its comment lists. */

/* The attention of HAT in 16 x 16 windows (csrc/hat.hip), one workgroup per (image, window, head), on a token grid whose sides are
 * multiples of 16 (the network pads the image, this entry does not).
 * mode 0 (self), between attn.qkv and attn.proj of a hybrid attention block: replaces torch.roll by (-shift, -shift), the window
 *   partition, `(q * scale) k^T + table[index_SA]` (+ Swin's region mask, -100 between tokens of different regions of the shifted grid —
 *   the slices [0, -16), [-16, -8), [-8, end) of each axis — when shift = 8), softmax, `@ v`, and the inverses.  bias: the block's
 *   relative_position_bias_table, fp32 [961][heads], read at (ya - yb + 15) * 31 + (xa - xb + 15) for query a, key b of a window.
 * mode 1 (overlap), between qkv and proj of an overlapping cross-attention block: the 256 queries of window (wy, wx) attend to the 576
 *   keys of the 24 x 24 tokens at rows 16 wy - 4 .. 16 wy + 19, columns 16 wx - 4 .. 16 wx + 19.  Replaces nn.Unfold(24, stride 16,
 *   padding 4) of the k | v maps (a 2.25 x copy), the partitions, `(q * scale) k^T + table[index_OCA]`, softmax and `@ v`.  A key outside
 *   the grid is a zero row (k = v = 0: the zeros are put in after the linear) that takes part in the softmax with score 0 + bias.  bias:
 *   fp32 [39 * 39][heads] in OFFSET order, read at (yb - ya + 15) * 39 + (xb - xa + 15) with (ya, xa) = (a / 16, a % 16), (yb, xb) =
 *   (b / 24, b % 24): the loader reorders the checkpoint's table by its index buffer.  No shift, no mask.
 * All of it is index arithmetic: no rolled copy, unfolded K / V, mask or score tensor in memory.  Scores, bias, mask and softmax in fp32;
 * the normalised probabilities are rounded to fp16 for the second product.
 * Refused: null descriptor / pointers; a mode other than 0 and 1; B, H or W < 1; H or W not a multiple of 16; heads outside 1..1024; D
 * outside 1..32; a shift other than 0 and 8 (mode 0) or other than 0 (mode 1); ldq < 96 heads; ldo < 32 heads; qkv / out not 16-byte
 * aligned, the bias table not 4-byte aligned, ldq or ldo not a multiple of 8; out aliasing qkv; 2^31 tokens. */
typedef struct sdmi_hat_attn_desc {
    const void* qkv;       /* fp16 token rows [B*H*W][ldq]: head h has q, k, v at columns h*32, (heads + h)*32, (2 heads + h)*32 */
    const void* bias;      /* fp32 [961][heads] (mode 0) | [1521][heads] in offset order (mode 1) */
    void* out;             /* fp16 token rows [B*H*W][ldo]: head h at columns h*32, dims D .. 31 stored as zero; columns >= 32 heads untouched */
    int32_t B, H, W;       /* the token grid (row-major rows), sides multiples of 16 */
    int32_t heads, D;
    int32_t ldq, ldo;
    int32_t mode;          /* 0: self | 1: overlap */
    int32_t shift;         /* 0 | 8 (mode 0); 0 (mode 1) */
    float scale;           /* D^-1/2 */
} sdmi_hat_attn_desc;
int sdmi_hat_window_attention(const sdmi_hat_attn_desc* d, void* stream);

/* The gate of HAT's ChannelAttention (cab.3 of a hybrid attention block's conv branch): gate fp32 [B][C] = sigmoid(w3 relu(w1
 * mean_n(y[b][n]) + b1) + b3) of the fp16 token rows y [B*N][ld].  Replaces AdaptiveAvgPool2d(1), Conv1x1 C -> Cs (attention.1: w1 fp32
 * [Cs][C], b1 [Cs]), ReLU, Conv1x1 Cs -> C (attention.3: w3 fp32 [C][Cs], b3 [C]) and the sigmoid.  Two launches: per block of 256 tokens
 * the sums of every channel into ws (fp32 [B][ceil(N / 256)][C]; strided token groups added in order, then the groups in order), then one
 * workgroup per image adds the blocks in order: no atomics, two runs give the same bits.  Refused: null pointers; B or N < 1; C not a
 * multiple of 8 in 8..1024; Cs outside 1..128; ld < C or not a multiple of 8; y not 16-byte aligned, an fp32 argument not 4-byte
 * aligned; 2^31 tokens. */
int sdmi_hat_channel_gate(const void* y, const void* w1, const void* b1, const void* w3, const void* b3, void* ws, void* gate, int B, int N, int C,
                          int Cs, int ld, void* stream);

/* The sum that adds the conv branch to the stream: out[row][c] = t[row][c] + conv_scale * gate[row / rows_per_image][c] * conv[row][c] on
 * fp16 rows t [rows][ldt], conv [rows][ldc], out [rows][ldo] (C channels; columns >= C untouched), gate fp32 [rows / rows_per_image][C]
 * from sdmi_hat_channel_gate of conv; fp32 arithmetic, one rounding.  Replaces `conv * sigmoid-gate` of ChannelAttention and
 * `+ conv_x * self.conv_scale` of HAB.forward.  out may be t.  Refused: null pointers; rows not a positive multiple of rows_per_image; C not
 * a positive multiple of 8; a row stride below C or not a multiple of 8; t / conv / out not 16-byte aligned, gate not 4-byte aligned;
 * out aliasing conv. */
int sdmi_hat_cab_add(const void* t, const void* conv, const void* gate, void* out, int64_t rows, int rows_per_image, int C, int ldt, int ldc, int ldo,
                     float conv_scale, void* stream);

/* A whole HAT network (HAT.forward of hat_arch.py with upsampler `pixelshuffle`, resi_connection `1conv`, window_size 16, overlap_ratio
 * 0.5, img_range 1, no ape; the models spandrel loads for the webui's modules/hat_model.py) held by an engine (scratch from the engine's
 * arena, a fixed set of buffers whatever the depths).  Replaces the model call inside UpscalerHAT.do_upscale, run on the image whole
 * instead of in HAT_tile tiles.  Fixed: head dim <= 32, 3 channels in / out, num_feat 64, scale 2, 3 or 4.  Block j of a group is shifted
 * by 8 for odd j; every group ends with one overlapping cross-attention block and a 3x3 conv.
 * blob: host fp32, every tensor flattened in the checkpoint's channel order, in this order (weight then bias for convs, linears, norms):
 *   conv_first; patch_embed.norm;
 *   per group i (layers.i.):
 *     per block j (residual_group.blocks.j.): norm1; attn.relative_position_bias_table [961][heads]; attn.qkv; attn.proj;
 *       conv_block.cab.0 [cab_mid][C][3][3]; conv_block.cab.2 [C][cab_mid][3][3]; conv_block.cab.3.attention.1 [cab_squeeze][C];
 *       conv_block.cab.3.attention.3 [C][cab_squeeze]; norm2; mlp.fc1 [mlp_hidden][C]; mlp.fc2 [C][mlp_hidden];
 *     residual_group.overlap_attn.: norm1; qkv; the bias table in offset order [39][39][heads] (row (dy + 15) * 39 + (dx + 15) holds the
 *       checkpoint's relative_position_bias_table row that relative_position_index_OCA names for key offset (dy, dx) = (yb - ya, xb - xa));
 *       proj; norm2; mlp.fc1; mlp.fc2;
 *     then the group's conv [C][C][3][3];
 *   norm; conv_after_body; conv_before_upsample.0; upsample.0; upsample.2 (scale 4 only); conv_last.
 * sdmi_hat_blob_floats gives its length (0 for a config the engine refuses).  NULL on error: a null argument, a blob of another length,
 * embed_dim not a positive multiple of num_heads, num_heads * 32 < embed_dim, mlp_hidden < 1, cab_mid outside 1..64 (the mid conv is
 * packed to 64 channels), cab_squeeze outside 1..128, embed_dim > 1024, a conv_scale that is not finite, a scale other than 2, 3, 4, more
 * than 16 groups, a depth outside 1..64. */
typedef struct sdmi_hat_config {
    int32_t embed_dim;
    int32_t num_layers;
    int32_t depths[16];    /* hybrid attention blocks per residual group */
    int32_t num_heads;
    int32_t mlp_hidden;    /* mlp_ratio * embed_dim */
    int32_t cab_mid;       /* embed_dim / compress_ratio */
    int32_t cab_squeeze;   /* embed_dim / squeeze_factor */
    float conv_scale;      /* a constructor argument of the network (0.01), not in the checkpoint */
    int32_t scale;         /* 2 | 3 | 4 */
} sdmi_hat_config;
typedef struct sdmi_hat sdmi_hat;
int64_t sdmi_hat_blob_floats(const sdmi_hat_config* cfg);
sdmi_hat* sdmi_hat_create(sdmi_engine* e, const void* blob_f32, int64_t blob_floats, const sdmi_hat_config* cfg);
void sdmi_hat_destroy(sdmi_hat* h);
/* arena bytes a run on B images of H x W needs (0 for a refused size) */
int64_t sdmi_hat_scratch_bytes(sdmi_hat* h, int B, int H, int W);
/* in / out as sdmi_esrgan_run: uint8 HWC or fp32 NCHW in, fp32 NCHW or uint8 HWC [B][H s][W s][3] out (device memory).  Any H, W >= 9:
 * the image is reflect-padded right and bottom to multiples of 16 on the device (a pad must be smaller than the side it pads) and the
 * output cropped.  Refused: null pointers, a side below 9, tensors of 2^31 elements. */
int sdmi_hat_run(sdmi_hat* h, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDMI_H */
