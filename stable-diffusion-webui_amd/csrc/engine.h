// engine.h — host-side engine of libsdmi: weight registry, packed layouts, activation arena and the UNet / VAE
// launch graphs.  One engine per GPU, used by one caller at a time (the reference serialises all GPU jobs behind one
// FIFO lock: /root/reference/modules/call_queue.py:8, modules/fifo_lock.py:6-37).
#pragma once
#include "common.h"
#include "../../include/sdmi.h"

#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace sdmi {

struct RawTensor {
    void* ptr = nullptr;          // device copy (as given dtype)
    int dtype = 0;
    std::vector<int64_t> shape;
    size_t bytes = 0;
};

// packed conv / linear weights: w [n_pad][taps][cin_pad] fp16, b [n_pad] fp32 (may be null)
struct ConvW {
    half_t* w = nullptr;
    float* b = nullptr;
    int cin = 0, cin_pad = 0, cout = 0, n_pad = 0, taps = 1;
    bool geglu = false;
    // LayerNorm folded into this layer (engine option "ln_fold"; GemmP::ln_stats): w_ln = fp16(w * gamma), s_ln[n] = sum_k w_ln[n][k],
    // c_ln = beta . w^T + b.  Built lazily by ensure_ln_fold, rebuilt when fold_epoch falls behind the engine's weights_epoch (any
    // sdmi_unet_update_weight / _vector).  mutable: the packed model is const during a forward, the cache is not part of it.
    mutable half_t* w_ln = nullptr;
    mutable float* s_ln = nullptr;
    mutable float* c_ln = nullptr;
    mutable long fold_epoch = -1;
};
struct NormW {
    float* g = nullptr;
    float* b = nullptr;
    int c = 0;
};

struct ResW {
    NormW n1, n2;
    ConvW c1, c2, skip;
    bool has_skip = false;
    int cin = 0, cout = 0;
    int emb_off = -1;             // column offset into the fused emb projection output (UNet only)
};
struct TBlockW {
    NormW ln1, ln2, ln3;
    ConvW qk1;                    // [2C][C]  (to_q ; to_k)
    ConvW v1;                     // [C][C]   used as the "activation" operand of the V^T GEMM
    ConvW o1, q2, k2, v2, o2, ff1, ff2;
    int ctx_slot = -1;            // index into the per-layer context K / V^T cache
    // feed-forward chain (engine option "fuse_rows", rowchain.hip): packed operand stream of ff.net.0.proj / ff.net.2, built lazily,
    // rebuilt when it falls behind the engine's weights_epoch
    mutable char* ff_packs = nullptr;
    mutable long ff_epoch = -1;
};
struct STW {
    NormW norm;
    ConvW proj_in, proj_out;
    std::vector<TBlockW> blocks;
    int ch = 0, heads = 0, dhead = 0;
};
struct UNetLayer {
    enum Kind { CONV_IN, RES, ST, DOWN, UP } kind;
    ResW res;
    STW st;
    ConvW conv;                   // CONV_IN / DOWN / UP
    int c0 = 0, c1 = 0;           // RES in output blocks: split of the concatenated input (h, skip)
};
struct UNetW {
    sdmi_unet_config cfg{};
    ConvW te0, te2, le0, le2;     // time_embed / label_emb linears (small-M path: w is plain [N][K] fp16)
    ConvW emb_all;                // all ResBlock emb_layers.1 stacked: [sum Cout][ted]
    int emb_cols = 0;
    std::vector<std::vector<UNetLayer>> input, output;
    std::vector<UNetLayer> middle;
    NormW out_norm;
    ConvW out_conv;
    int n_ctx_slots = 0;
    bool ready = false;
};

struct VAEAttnW {
    NormW norm;
    ConvW qk, v, proj;
    int c = 0;
};
struct VAELevel {
    std::vector<ResW> blocks;
    ConvW resample;               // upsample.conv (decoder) / downsample.conv (encoder)
    bool has_resample = false;
};
struct ClipLayerW {
    NormW ln1, ln2;
    ConvW qk, v, o, fc1, fc2;     // q;k stacked, V separate (produced transposed), out_proj, MLP
};
struct ClipW {
    sdmi_clip_config cfg{};
    void* tok_emb = nullptr;      // [vocab][hidden] in the checkpoint dtype
    int tok_dtype = 0;
    float* pos_emb = nullptr;     // [max_positions][hidden] fp32
    std::vector<ClipLayerW> layers;
    NormW final_ln;
    half_t* text_proj = nullptr;  // optional [proj_dim][hidden] fp16 (rows = output features): pooled @ text_projection
    int proj_dim = 0;
    bool configured = false, ready = false;
};

struct VAEW {
    sdmi_vae_config cfg{};
    // decoder
    float* pqc_w = nullptr;       // post_quant_conv as fp32 [z][z]
    float* pqc_b = nullptr;
    ConvW d_conv_in, d_conv_out;
    ResW d_mid1, d_mid2;
    VAEAttnW d_attn;
    std::vector<VAELevel> d_up;   // index = level (0 = finest)
    NormW d_norm_out;
    // encoder
    ConvW e_conv_in, e_conv_out;  // e_conv_out has quant_conv folded in
    ResW e_mid1, e_mid2;
    VAEAttnW e_attn;
    std::vector<VAELevel> e_down;
    NormW e_norm_out;
    bool has_encoder = false;
    bool ready = false;
};

// Hypernetworks (modules/hypernetworks/hypernetwork.py): per feature width a pair of small MLPs (one for the K path, one for the V path)
// applied to the attention CONTEXT before to_k / to_v: context_k = x + multiplier * MLP_k(x) (forward, :104-105; apply_hypernetworks
// :358-379).  An MLP is a sequence of Linear / activation / LayerNorm ops (dropout is the identity at inference).
struct HnOp {
    int kind = 0;                 // 0 linear, 1 activation, 2 layer norm
    ConvW lin;
    int act = 0;
    NormW ln;
};
struct HnModule {
    std::vector<HnOp> ops;
};
struct HnNet {
    float multiplier = 1.f;
    std::map<int, std::pair<HnModule, HnModule>> by_dim;    // feature width -> (K module, V module)
};

class Arena {
public:
    char* base = nullptr;
    size_t cap = 0, off = 0, high = 0;
    bool dry = false;
    void reset() { off = 0; }
    size_t mark() const { return off; }
    void rewind(size_t m) { off = m; }            // everything taken since mark() is dead: later launches of the same stream may overwrite it
    void* take(size_t bytes) {
        const size_t a = (off + 255) & ~size_t(255);
        off = a + bytes;
        if (off > high) high = off;
        if (dry) return (void*)(uintptr_t)(0x1000 + a);   // never dereferenced in dry mode
        return base + a;
    }
};

}  // namespace sdmi

struct sdmi_engine {
    int device = 0;
    std::map<std::string, sdmi::RawTensor> raw_unet, raw_vae;
    // where each "<layer>.weight" of the UNet checkpoint landed in the packed weights (filled by the build), so that a single
    // layer can be re-packed in place when a LoRA changes it (sdmi_unet_update_weight)
    struct PackSite { half_t* dst; int O, cin, kh, Opad, cin_pad, geglu; };
    std::map<std::string, std::vector<PackSite>> unet_sites;
    // the same for the 1-D parameters ("<layer>.bias", "<norm>.weight", "<norm>.bias"): LyCORIS norm modules and bias deltas
    // (extensions-builtin/Lora/network_norm.py, network.py:196-216 ex_bias) rewrite them through sdmi_unet_update_vector
    struct VecSite { float* dst; int n, n_pad, geglu; };
    std::map<std::string, std::vector<VecSite>> unet_vec_sites;
    bool recording_unet_sites = false;
    std::vector<void*> owned;                 // persistent device allocations (weights)
    std::vector<void*> owned_vae;             // the VAE's packed weights: freed when another VAE is loaded (sd_vae.load_vae)
    std::vector<void*>* alloc_sink = nullptr; // where dev_alloc records (null = owned)
    std::vector<sdmi::HnNet> hypernets;       // loaded hypernetworks, in application order (shared.loaded_hypernetworks)
    std::vector<void*> owned_hn;
    char* hn_ctx_scratch = nullptr;           // intermediates of the hypernetwork pass over the text context (set_context)
    size_t hn_ctx_scratch_bytes = 0;
    sdmi::UNetW unet;
    sdmi::VAEW vae;
    sdmi::ClipW clip[2];
    std::map<std::string, sdmi::RawTensor> raw_clip[2];
    sdmi::Arena arena;
    // option "streams" (> 1): a UNet call's rows are cut into that many slices, each on its own HIP stream / arena (engine.cpp unet_forward)
    int n_streams = 1;
    int arena_reuse = 0;                      // 1: the temporaries of a ResBlock / transformer block are released when the block returns (option "arena_reuse")
    std::vector<hipStream_t> aux_streams;
    std::vector<sdmi::Arena> aux_arenas;
    std::vector<hipEvent_t> ev_join;
    hipEvent_t ev_fork = nullptr;
    // options
    bool force_generic = false;
    bool use_glds = true;
    // range-extended VAE decode (the engine's form of the reference's fp16 -> fp32 VAE fallback, modules/processing.py:636-665): the
    // decoder's residual stream is stored at this scale (1/64 when on), every GroupNorm that reads it uses eps * scale^2
    float vae_stream_scale = 1.f;
    // LayerNorm folded into the consuming GEMMs of the transformer blocks (norm1 -> to_q|to_k, to_v; norm2 -> attn2.to_q; norm3 ->
    // ff.net.0): only the per-row (mean, rstd) are computed, the normalised tensors never reach HBM.  Off by default until measured.
    int ln_fold = 0;                          // 1: row statistics from ln_rowstats_kernel; 2: also per-tile partial sums from the producing GEMMs' epilogues
    // The feed-forward chain of the transformer blocks at the 320-wide level as a single launch (rowchain.hip), option "fuse_rows" bit 1:
    // norm3 -> GEGLU -> ff.net.2 -> + x.  Default 2 (round 5, same-box A/Bs of the forward, profiles/r05_fwd_ab_*): 203-219 us against
    // 263 us of LayerNorm + GEGLU GEMM + GEMM.
    // Bit 0: the cross-attention third, norm2 -> attn2.to_q -> attention over the cached context -> attn2.to_out + x, as one launch
    // (xattn_chain.hip; a tiled GEMM over 128 whole token rows — round 5's lane-owns-row chain behind this bit was slower than the launches
    // and was removed).  Taken at the 320-wide level when the feed-forward chain's conditions hold, no hypernetwork of that width is
    // loaded and HW % 128 == 0; every other width and mode keeps the four launches.  Default 3: 70-75 us against 106-111 us for the four
    // launches at the C1 level-0 shape, and the same-box forward / job A/Bs of profiles/xattn_chain_time.md.
    int fuse_rows = [] { const char* e = getenv("SDMI_FUSE_ROWS"); return e ? atoi(e) : 3; }();
    // Accuracy mode (option "residual_fp32", off by default — the engine's counterpart of the reference's --no-half / upcast options,
    // modules/devices.py:284-295, modules/sd_hijack_optimizations.py:232-233): the UNet's carried stream — conv_in / ResBlock /
    // transformer-block / proj_out / down- and upsample outputs and the skip_connection 1x1 — is kept as (hi, lo) fp16 pairs
    // (GemmP::out_lo), i.e. with ~22 bits, so the residual sums are no longer rounded to fp16 once per block.  DESIGN.md section 7.
    bool residual_fp32 = false;
    long weights_epoch = 0;                   // bumped by every in-place weight / vector update: folded copies older than this are stale
    bool cfg_pairs = false;                   // rows [Bn/2, Bn) repeat the latent and timestep of rows [0, Bn/2): the layers in front of the first cross-attention run once (option "cfg_pairs")
    bool uniform_t = false;                   // every row of the call sits at the same timestep: the embedding path runs for one row (option "uniform_t")
    bool auto_promises = false;               // option "auto_promises": cfg_pairs / uniform_t are DERIVED per call from x and t (a synchronising device -> host
                                              // compare) instead of promised by the caller — for callers that cannot know: the stock CFG denoiser behind Mi355xUnet.forward
    bool tiling = false;                      // p.tiling: every padded 3x3 conv wraps around (modules/sd_hijack.py:311-318)
    // activation taps (parity error budget): with `trace` on, every block output of the last forward is recorded by name
    // — the arena never reuses memory within a forward, so the tensors stay readable until the next forward
    bool trace = false;
    struct Tap { std::string name; const half_t* ptr; int B, H, W, C; };
    std::vector<Tap> taps;
    // ControlNet residuals for the NEXT forward only (sdmi_unet_set_control; consumed and cleared by it): one NCHW tensor per input
    // block output + one for the middle block, in the caller's io dtype (ldm cldm.py ControlledUnetModel.forward)
    std::vector<const void*> control;
    std::vector<int64_t> control_numel;
    bool only_mid_control = false;
    // context cache (persistent between forwards)
    half_t* ctx_f16 = nullptr;                // [Bn][Lpad][ctx_dim]
    std::vector<half_t*> ctx_k;               // per slot [Bn*Lpad][C]
    std::vector<half_t*> ctx_vt;              // per slot [Bn][C][Lpad]
    std::vector<void*> ctx_owned;
    int ctx_B = 0, ctx_L = 0, ctx_Lpad = 0;
    bool ctx_valid = false;
    int* ctx_gate = nullptr;                  // device flag of the conditional re-projection (sdmi_unet_set_context_cached)

    ~sdmi_engine();
};

// What every upscaler net is: the engine whose arena its runs take their activations from, and the device allocations (packed weights)
// it owns.  A net is immutable after its sdmi_*_create.
struct sdmi_net {
    sdmi_engine* e = nullptr;
    std::vector<void*> owned;
    ~sdmi_net();
};

// RRDBNet upscaler (ESRGAN / Real-ESRGAN): packed weights of the rrdb_conv launches (rrdb.hip).  Activations come from the owning
// engine's arena, like the VAE's; the net itself is immutable after sdmi_esrgan_create.
struct sdmi_esrgan : sdmi_net {
    struct Conv { half_t* w = nullptr; float* b = nullptr; int cin = 0, nout = 0, n_real = 0; };
    int num_block = 0, in_ch = 0, scale = 0;
    int unshuffle = 1;                        // 4 / scale: pixel-unshuffle factor in front of conv_first (x2: 2, x1: 4)
    int cin0 = 0;                             // conv_first's input channels (3 / 12 / 48) padded to 32 / 32 / 64
    Conv first, body, up1, up2, hr, last;
    std::vector<Conv> rdb;                    // num_block x 3 x 5, in checkpoint order
};

// Compact Real-ESRGAN upscaler (SRVGGNetCompact, 64 features, PReLU): packed weights of the compact_conv launches (compact.hip).
// Activations come from the owning engine's arena; the net is immutable after sdmi_compact_create.
struct sdmi_compact : sdmi_net {
    struct Conv { half_t* w = nullptr; float* b = nullptr; float* slope = nullptr; };
    int num_conv = 0, scale = 0;
    std::vector<Conv> convs;                  // num_conv + 2: first (3 -> 64), body, last (64 -> 3 scale^2; no PReLU after it)
};

// SwinIR upscaler (nearest+conv upsampler): packed weights of the GEMM launches (linears and trunk convs, rows / columns padded to
// multiples of 64, qkv / proj permuted into 32-wide head slots), the expanded relative-position bias of every block, and the 64-channel
// tail as rrdb_conv weights.  Activations come from the owning engine's arena; the net is immutable after sdmi_swinir_create.
struct sdmi_swinir : sdmi_net {
    struct Block {
        sdmi::NormW n1, n2;
        sdmi::ConvW qkv, proj, fc1, fc2;
        float* bias = nullptr;                // [heads][64][64]
        float* head_scale = nullptr;          // Swin2SR: [heads]
    };
    struct Layer {
        std::vector<Block> blocks;
        sdmi::ConvW conv[3];                  // 1conv: conv[0]; 3conv: 3x3 (C -> C/4), 1x1, 3x3 (C/4 -> C)
    };
    sdmi_swinir_config cfg{};
    int C = 0, Cp = 0, D = 0, ldq = 0, lda = 0, hid_pad = 0;      // lda: row width of the attention output (32 heads rounded up to 64)
    sdmi::ConvW first, after[3], before, up1, up2, hr, last;
    sdmi::NormW pe_norm, norm;
    std::vector<Layer> layers;
    // Swin2SR (v2): Swin-V2 blocks — cosine attention, res-post-norm — in the same trunk; upsampler 0 nearest+conv (the tail above),
    // 1 pixelshuffle (before, ps[], last), 2 pixelshuffledirect (direct)
    int v2 = 0, upsampler = 0;
    sdmi::ConvW pe_proj;                      // patch_embed.proj: the 1x1 conv in front of patch_embed.norm
    sdmi::ConvW ps[2], direct;                // ps: 64 -> f*f*64, output channels in (i, j, c) order; direct: C -> 3 scale^2 (padded to 64)
};

// Swin2SR upscaler: SwinIR's trunk and buffers with v2 set (upscalers.cpp swinir_pass runs both)
struct sdmi_swin2sr : sdmi_swinir {
    sdmi_swin2sr_config cfg2{};
};

// DAT upscaler (pixelshuffle tail, 1conv groups): the linears and trunk convs as GEMM weights (token rows C rounded up to 64 wide; qkv's
// output, proj's input and everything between in 32-wide head slots, Sp = 32 heads columns; fc1's two halves each rounded up to 64), the
// fp32 operands of the dat.hip launches in the same layouts, the 64-channel tail as Swin2SR's.  Activations come from the owning engine's
// arena; the net is immutable after sdmi_dat_create.
struct sdmi_dat : sdmi_net {
    struct Block {
        bool spatial = true, shifted = false;
        sdmi::NormW n1, n2, sgn;              // sgn: ffn.sg.norm over ffn_hidden / 2
        sdmi::ConvW qkv, proj, fc1, fc2;
        float* tab0 = nullptr;                // spatial: the two bias tables
        float* tab1 = nullptr;
        float* temperature = nullptr;         // channel: [heads]
        float *dw_w = nullptr, *dw_b = nullptr;                           // [9][Sp], [Sp]
        float *ci_w1 = nullptr, *ci_b1 = nullptr, *ci_w2 = nullptr, *ci_b2 = nullptr;   // [C8][Sp], [C8], [Sp][C8], [Sp]
        float *si_w1 = nullptr, *si_b1 = nullptr, *si_w2 = nullptr;       // [C16][Sp], [C16], [C16]
        float si_b2 = 0.f;
        float *sg_w = nullptr, *sg_b = nullptr;                           // [9][Hh], [Hh]
    };
    struct Layer {
        std::vector<Block> blocks;
        sdmi::ConvW conv;
    };
    sdmi_dat_config cfg{};
    int C = 0, Cp = 0, D = 0, Sp = 0, half = 0, Hh = 0, C8 = 0, C16 = 0;      // half = ffn_hidden / 2, Hh = half rounded up to 64
    sdmi::ConvW first, after, before, ps[2], last;
    sdmi::NormW rg_norm, norm;
    std::vector<Layer> layers;
};

// HAT upscaler (pixelshuffle tail, 1conv groups, window 16, overlap ratio 0.5): the linears and convs as GEMM weights (token rows C rounded
// up to 64 wide; qkv's output and proj's input in 32-wide head slots, ldq = 96 heads and lda = 32 heads rounded up to 64; the conv branch's
// mid width rounded up to 64), the bias tables and the channel attention's two 1x1 convs as the fp32 operands of the hat.hip launches, the
// 64-channel tail as Swin2SR's.  Activations come from the owning engine's arena; the net is immutable after sdmi_hat_create.
struct sdmi_hat : sdmi_net {
    struct Block {                            // a hybrid attention block, or (overlap) the group's overlapping cross-attention block
        sdmi::NormW n1, n2;
        sdmi::ConvW qkv, proj, fc1, fc2;
        float* table = nullptr;               // [961][heads] | (overlap) [39 * 39][heads] in offset order
        sdmi::ConvW cab0, cab2;               // 3x3 C -> cab_mid (GELU), 3x3 cab_mid -> C
        float *ca_w1 = nullptr, *ca_b1 = nullptr, *ca_w3 = nullptr, *ca_b3 = nullptr;   // [Cs][Cp], [Cs], [Cp][Cs], [Cp]
    };
    struct Layer {
        std::vector<Block> blocks;
        Block overlap;
        sdmi::ConvW conv;
    };
    sdmi_hat_config cfg{};
    int C = 0, Cp = 0, D = 0, ldq = 0, lda = 0, hid_pad = 0, mid_pad = 0;
    sdmi::ConvW first, after, before, ps[2], last;
    sdmi::NormW pe_norm, norm;
    std::vector<Layer> layers;
};

// ScuNET (Swin-Conv-UNet, dim 64): per ConvTransBlock the two 1x1 convs as GEMM weights, the 3x3 pair as rrdb_conv (widths 32 / 64) or
// GEMM (128 / 256) weights, and the transformer Block either as one scu_block pack (trans_dim 32 / 64) or as the GEMM weights of the
// swin_layernorm + conv_gemm + swin_window_attn route (128 / 256).  Activations come from the owning engine's arena; the net is immutable
// after sdmi_scunet_create.
struct sdmi_scunet : sdmi_net {
    struct Block {
        int c = 0;                            // conv_dim = trans_dim
        sdmi::ConvW c11, c12, cb0, cb2;
        float* bias = nullptr;                // [c / 32][64][64]
        void* packs = nullptr;                // c <= 64
        sdmi::NormW n1, n2;                   // c >= 128
        sdmi::ConvW qkv, proj, fc1, fc2;
    };
    sdmi_scunet_config cfg{};
    sdmi::ConvW head, tail, down[3], up[3];   // down[l]: level l -> l + 1 (K = 4 Cin); up[l]: level l + 1 -> l (N = 4 Cout)
    std::vector<Block> stage[7];              // m_down1, m_down2, m_down3, m_body, m_up3, m_up2, m_up1
};

namespace sdmi {

// What engine.cpp and upscalers.cpp share: one pass over an arena and its GEMM launch
static inline int rup(int x, int m) { return (x + m - 1) / m * m; }

struct Run {
    sdmi_engine* e;
    hipStream_t s;
    bool dry;
    Arena* ar;                     // the activation arena this pass bump-allocates from (one per concurrent batch slice: option "streams")
    int b0 = 0, Btot = 0;          // UNet batch slices: first row of this slice / rows of the whole call (indexes the context cache)
    Run(sdmi_engine* e_, hipStream_t s_, bool dry_, Arena* ar_ = nullptr, int b0_ = 0, int Btot_ = 0)
        : e(e_), s(s_), dry(dry_), ar(ar_ ? ar_ : &e_->arena), b0(b0_), Btot(Btot_) {}
    half_t* H(size_t n) { return (half_t*)ar->take(n * sizeof(half_t)); }
    // Option "residual_fp32": a tensor of the carried stream is a (hi, lo) pair of fp16 tensors, allocated back to back — S(n) takes
    // room for both, lo(p, n) is the second half (null when the option is off: every consumer then sees a plain fp16 tensor).
    // (the pairs need the LDS-direct MFMA kernels: under force_generic / use_glds = 0 — cross-check settings — the forward falls back to
    // the plain fp16 stream instead of failing the job)
    bool acc() const { return e->residual_fp32 && !e->force_generic && e->use_glds; }
    half_t* S(size_t n) { return H(acc() ? 2 * n : n); }
    half_t* lo(const half_t* p, size_t n) const { return (acc() && p) ? const_cast<half_t*>(p) + n : nullptr; }
    // option "arena_reuse": a block's temporaries are released when the block returns — the next block's launches (same stream, so
    // ordered behind every reader) write over them while their lines are still in the 256 MB Infinity Cache, instead of every
    // activation of a forward (~10 GB) being written back to HBM once.  Not while block outputs are tapped or LayerNorm partials live.
    bool reuse() const { return e->arena_reuse && !e->trace && !e->ln_fold && !acc(); }
    float* F(size_t n) { return (float*)ar->take(n * sizeof(float)); }
    void tap(const std::string& name, const half_t* p, int B, int H, int W, int C) {
        if (!dry && e->trace) e->taps.push_back({name, p, B, H, W, C});
    }
    // GroupNorm statistics handed from a producing GEMM's epilogue to the norm that reads its output (launch_gemm: stats_out)
    const half_t* st_tensor = nullptr;
    float* st_ws = nullptr;
    int st_nchunk = 0;
    // LayerNorm row partial sums handed from a producing GEMM's epilogue to the folded consumers of its output (option "ln_fold"):
    // set lnp_want before the producer's run_conv; lnp_tensor / lnp_ws / lnp_np describe what the last run_conv produced
    bool lnp_want = false;
    const half_t* lnp_tensor = nullptr;
    float* lnp_ws = nullptr;
    int lnp_np = 0;
};

#define TRY(x)                  \
    do {                        \
        if ((x) != 0) return 1; \
    } while (0)

struct ConvArgs {
    const half_t* a0 = nullptr;
    const half_t* a1 = nullptr;
    int c0 = 0, c1 = 0;
    int lda0 = 0;                 // row stride of a0 when its rows are wider than c0 (0 = c0)
    int B = 1, Hi = 1, Wi = 1, Ho = 1, Wo = 1;
    int stride = 1, pad = 0, up = 0;
    const float* rowbias = nullptr;
    int ldrb = 0;
    const half_t* resid = nullptr;
    const half_t* resid_lo = nullptr;   // (hi, lo) stream tensors: GemmP::resid_lo / out_lo
    half_t* out_lo = nullptr;
    int ldr = 0;
    void* out = nullptr;
    int ldo = 0;
    int flags = 0;
    int n_real = 0;
    float alpha = 1.f;
    float bias_scale = 1.f;
    int batch = 1;
    long a_bs = 0, w_bs = 0, o_bs = 0, r_bs = 0;
    const int* gate = nullptr;
    int stats_C = 0;              // > 0: the output feeds a GroupNorm(32) over stats_C channels: emit its partial sums from the epilogue
    bool no_split = false;        // never take a split-K workspace from the arena (callers outside a sized forward pass)
    float* stats_ws_pre = nullptr;    // arena_reuse: room for the GroupNorm partial sums taken by the caller (it must outlive the caller's rewind)
};

int run_conv(Run& r, const ConvW& W, const ConvArgs& a);
int ensure_arena(Arena& ar, size_t need, hipStream_t s);

// Every forward is the same walk twice, walk(bool dry) -> int: dry to size the arena (pure host arithmetic: the walk only bump-allocates),
// then, the arena grown to that, the launches.  A walk that fails dry leaves the arena out of dry mode.
template <class Walk>
int two_pass(Arena& ar, hipStream_t s, Walk walk) {
    ar.dry = true; ar.high = 0;
    const int rc = walk(true);
    ar.dry = false;
    TRY(rc);
    TRY(ensure_arena(ar, ar.high, s));
    return walk(false);
}

// What capi.cpp calls: engine.cpp ...
extern int g_vae_attn_rows;
int unet_forward(sdmi_engine* e, const void* x, const void* t, const void* ctx, const void* y, void* out, int io_dtype,
                 int Bn, int h, int w, int L, hipStream_t s);
int vae_decode(sdmi_engine* e, const void* z, int io_dtype, float* out, int B, int h, int w, hipStream_t s);
int vae_encode(sdmi_engine* e, const void* x, int io_dtype, float* out, int B, int H, int W, hipStream_t s);
int engine_load_unet_tensor(sdmi_engine* e, const char* key, const void* data, int dtype, int ndim, const int64_t* shape, int on_device);
int engine_load_vae_tensor(sdmi_engine* e, const char* key, const void* data, int dtype, int ndim, const int64_t* shape, int on_device);
int engine_unet_finalize(sdmi_engine* e);
int engine_clip_configure(sdmi_engine* e, int slot, const sdmi_clip_config* cfg);
int engine_clip_load_tensor(sdmi_engine* e, int slot, const char* key, const void* data, int dtype, int ndim, const int64_t* shape, int on_device);
int engine_clip_finalize(sdmi_engine* e, int slot);
int engine_clip_forward(sdmi_engine* e, int slot, const int* tokens, const float* inputs_embeds, int B, int L, int skip,
                        int apply_final_ln, float* out, float* pooled, hipStream_t s);
int engine_unet_update_weight(sdmi_engine* e, const char* key, const void* data, int dtype, int ndim, const int64_t* shape, int on_device);
int engine_vae_finalize(sdmi_engine* e);
int engine_hypernet_clear(sdmi_engine* e);
int engine_hypernet_begin(sdmi_engine* e, float multiplier);
int engine_hypernet_linear(sdmi_engine* e, int dim, int which, const void* w, const void* b, int dtype, int out_f, int in_f, int on_device);
int engine_hypernet_act(sdmi_engine* e, int dim, int which, int act);
int engine_hypernet_layernorm(sdmi_engine* e, int dim, int which, const void* g, const void* b, int dtype, int n, int on_device);
int engine_unet_update_vector(sdmi_engine* e, const char* key, const void* data, int dtype, int64_t n, int on_device);
int engine_set_context(sdmi_engine* e, const void* ctx, int dtype, int Bn, int L, hipStream_t s, bool conditional = false);

// ... and upscalers.cpp.  Every family: the floats its weight blob holds (0: a config the engine refuses), the net off a host blob, the
// arena bytes one run takes (0: a size the run refuses), and the run.  in: the RGB image(s), uint8 HWC [B][H][W][3] (in_u8; scaled by
// 1/255) or fp32 NCHW [B][3][H][W] in [0, 1].  out: [B][3][H s][W s] fp32 NCHW, or (out_u8) uint8 HWC [B][H s][W s][3] =
// round_half_even(clamp(y, 0, 1) * 255); s = 1 for ScuNET.
int64_t esrgan_blob_floats(int num_block, int in_ch);
int esrgan_create(sdmi_engine* e, const float* blob, int64_t blob_floats, int num_block, int in_ch, int scale, sdmi_esrgan** out);
int64_t esrgan_scratch_bytes(const sdmi_esrgan* n, int B, int H, int W);
int esrgan_run(sdmi_esrgan* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s);
int64_t compact_blob_floats(int num_conv, int scale);
int compact_create(sdmi_engine* e, const float* blob, int64_t blob_floats, int num_conv, int scale, sdmi_compact** out);
int64_t compact_scratch_bytes(const sdmi_compact* n, int B, int H, int W);
int compact_run(sdmi_compact* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s);
int64_t swinir_blob_floats(const sdmi_swinir_config* cfg);
int swinir_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_swinir_config* cfg, sdmi_swinir** out);
int64_t swinir_scratch_bytes(const sdmi_swinir* n, int B, int H, int W);      // Swin2SR's too: an sdmi_swin2sr is an sdmi_swinir
int swinir_run(sdmi_swinir* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s);
int64_t swin2sr_blob_floats(const sdmi_swin2sr_config* cfg);
int swin2sr_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_swin2sr_config* cfg, sdmi_swin2sr** out);
int64_t scunet_blob_floats(const sdmi_scunet_config* cfg);
int scunet_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_scunet_config* cfg, sdmi_scunet** out);
int64_t scunet_scratch_bytes(const sdmi_scunet* n, int B, int H, int W);
int scunet_run(sdmi_scunet* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s);
int64_t dat_blob_floats(const sdmi_dat_config* cfg);
int dat_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_dat_config* cfg, sdmi_dat** out);
int64_t dat_scratch_bytes(const sdmi_dat* n, int B, int H, int W);
int dat_run(sdmi_dat* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s);
int64_t hat_blob_floats(const sdmi_hat_config* cfg);
int hat_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_hat_config* cfg, sdmi_hat** out);
int64_t hat_scratch_bytes(const sdmi_hat* n, int B, int H, int W);
int hat_run(sdmi_hat* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s);

}  // namespace sdmi
