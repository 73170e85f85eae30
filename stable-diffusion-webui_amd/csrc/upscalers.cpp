// upscalers.cpp — the upscaler nets of libsdmi (host side, C++): RRDBNet, compact SRVGGNet, SwinIR / Swin2SR, ScuNET, DAT and HAT.  What
// their builds share (the blob packer), what their passes share (the launches on a token grid, the pixelshuffle tail) and the two
// entries every family has (scratch bytes, run), then the families.  From engine.cpp they take one pass over an arena (Run, two_pass)
// and the GEMM launch (run_conv); nothing of the UNet, the VAE or CLIP.
#include "engine.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

namespace sdmi {

// ------------------------------------------------------------------------------------------------------------
// Upscaler nets (sdmi_net): what their builds and their runs share
// ------------------------------------------------------------------------------------------------------------
// a fresh allocation that the net owns, filled from `host` (null: left for a pack launch to fill)
static int net_upload(sdmi_net* net, const void* host, size_t bytes, void** dev) {
    SDMI_CHECK_HIP(hipMalloc(dev, std::max<size_t>(bytes, 256)));
    net->owned.push_back(*dev);
    if (host) SDMI_CHECK_HIP(hipMemcpy(*dev, host, bytes, hipMemcpyHostToDevice));
    return 0;
}

// a norm of width C off the blob cursor: gamma, then beta
static int net_norm(sdmi_net* net, const float*& src, int C, NormW* n) {
    n->c = C;
    TRY(net_upload(net, src, (size_t)C * sizeof(float), (void**)&n->g));
    TRY(net_upload(net, src + C, (size_t)C * sizeof(float), (void**)&n->b));
    src += 2 * C;
    return 0;
}

// the host blob on the device, for the builds whose pack launches read it there; freed when the build returns
struct StagedBlob {
    float* p = nullptr;
    ~StagedBlob() { (void)hipFree(p); }
    int stage(const float* blob, int64_t blob_floats) {
        SDMI_CHECK_HIP(hipMalloc((void**)&p, blob_floats * sizeof(float)));
        SDMI_CHECK_HIP(hipMemcpy(p, blob, blob_floats * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
};

// the relative-position table of an 8 x 8 window, entry (dy + 7) * 15 + (dx + 7) of head h at table[entry * entry_stride + h * head_stride],
// as the attention kernels read it: bias[h][a][b] = table entry (ya - yb, xa - xb) of head h
static int net_rel_bias(sdmi_net* net, const float* table, int heads, size_t entry_stride, size_t head_stride, float** dev) {
    std::vector<float> bias((size_t)heads * 4096);
    for (int h = 0; h < heads; ++h)
        for (int a = 0; a < 64; ++a)
            for (int b = 0; b < 64; ++b)
                bias[((size_t)h * 64 + a) * 64 + b] =
                    table[(size_t)(((a >> 3) - (b >> 3) + 7) * 15 + ((a & 7) - (b & 7) + 7)) * entry_stride + h * head_stride];
    return net_upload(net, bias.data(), bias.size() * sizeof(float), (void**)dev);
}

// The walk of a build over its fp32 blob: every method reads at the cursor `src`, uploads into allocations the net owns (weights first,
// then the bias: the order of the blob) and moves the cursor on.
struct BlobPacker {
    sdmi_net* net;
    const float* src;
    const float* end;
    using Map = std::function<int(int)>;
    static int ident(int v) { return v; }
    // one conv / linear: OIHW weight then (has_bias) the bias -> [n_pad][taps][cin_pad] fp16 + [n_pad] fp32, output row o at row_of(o),
    // input channel i at col_of(i), everything else zero; bias_add: a constant per REAL output row
    int conv(ConvW* c, int O, int I, int taps, int n_pad, int cin_pad, const Map& row_of = ident, const Map& col_of = ident,
             bool has_bias = true, const float* bias_add = nullptr) {
        std::vector<half_t> w((size_t)n_pad * taps * cin_pad, (half_t)0.f);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < taps; ++t)
                    w[((size_t)row_of(o) * taps + t) * cin_pad + col_of(i)] = (half_t)src[((size_t)o * I + i) * taps + t];
        src += (size_t)O * I * taps;
        c->cin = I; c->cin_pad = cin_pad; c->cout = O; c->n_pad = n_pad; c->taps = taps;
        TRY(net_upload(net, w.data(), w.size() * sizeof(half_t), (void**)&c->w));
        if (!has_bias) return 0;
        std::vector<float> b((size_t)n_pad, 0.f);
        for (int o = 0; o < O; ++o) b[(size_t)row_of(o)] = src[o] + (bias_add ? bias_add[o] : 0.f);
        src += O;
        return net_upload(net, b.data(), b.size() * sizeof(float), (void**)&c->b);
    }
    int norm(NormW* n, int C) { return net_norm(net, src, C, n); }
    int raw(float** dev, size_t count) {
        TRY(net_upload(net, src, count * sizeof(float), (void**)dev));
        src += count;
        return 0;
    }
    // an fp32 matrix [rows][cols] -> [rows_pad][cols_pad] with row r at row_of(r), column c at col_of(c); transposed: the blob holds
    // [cols][rows] (a depthwise weight [C][9] -> [9][C])
    int mat(float** dev, int rows, int cols, int rows_pad, int cols_pad, const Map& row_of = ident, const Map& col_of = ident, bool transposed = false) {
        std::vector<float> m((size_t)rows_pad * cols_pad, 0.f);
        for (int rr = 0; rr < rows; ++rr)
            for (int cc = 0; cc < cols; ++cc)
                m[(size_t)row_of(rr) * cols_pad + col_of(cc)] = transposed ? src[(size_t)cc * rows + rr] : src[(size_t)rr * cols + cc];
        src += (size_t)rows * cols;
        return net_upload(net, m.data(), m.size() * sizeof(float), (void**)dev);
    }
    float scalar() { return *src++; }
    // conv_last of the 64-channel tails on rrdb_conv: 3 outputs of a 32-wide tile, y / img_range + mean folded into the bias
    int conv_last(ConvW* c) {
        static const float mean[3] = {0.4488f, 0.4371f, 0.4040f};
        return conv(c, 3, 64, 9, 32, 64, ident, ident, true, mean);
    }
    // the pixelshuffle tail (Swin2SR's upsampler 1, DAT, HAT): conv_before_upsample, per step (one, two at scale 4) a conv 64 -> f^2 64 with
    // torch's output channel c f^2 + (i f + j) at row (i f + j) * 64 + c, conv_last
    int ps_tail(ConvW* before, ConvW* ps, ConvW* last, int C, int Cp, int scale) {
        const int f2 = scale == 3 ? 9 : 4;
        TRY(conv(before, 64, C, 9, 64, Cp));
        for (int k = 0; k < (scale == 4 ? 2 : 1); ++k) TRY(conv(&ps[k], f2 * 64, 64, 9, f2 * 64, 64, [&](int o) { return (o % f2) * 64 + o / f2; }));
        return conv_last(last);
    }
    int done() {
        SDMI_REQUIRE(src == end, "internal: blob walk does not end at its length");
        SDMI_CHECK_HIP(hipDeviceSynchronize());
        return 0;
    }
};

// The launches of a pass on its grid: B images of H x W tokens / pixels (dry: the arena layout alone)
struct Grid {
    Run& r;
    int B, H, W;
    // 3x3 pad 1 / 1x1 / linear on the grid x f; rows of a, resid and o as wide as the weight's unless lda / ldr / ldo say otherwise
    int conv(const ConvW& w, const half_t* a, const half_t* resid, half_t* o, int flags = 0, int f = 1, int lda = 0, int ldr = 0, int ldo = 0) {
        ConvArgs c;
        c.a0 = a; c.c0 = w.cin_pad; c.lda0 = lda; c.B = B; c.Hi = c.Ho = H * f; c.Wi = c.Wo = W * f; c.pad = w.taps == 9 ? 1 : 0;
        c.resid = resid; c.ldr = ldr ? ldr : w.n_pad; c.out = o; c.ldo = ldo ? ldo : w.n_pad; c.flags = flags;
        const size_t mark = r.ar->mark();                     // a split-K workspace lives for its launch only
        const int rc = run_conv(r, w, c);
        r.ar->rewind(mark);
        return rc;
    }
    // LayerNorm over the norm's columns of every row: a and o [B H W][ld]
    int lnorm(const NormW& w, const half_t* a, half_t* o, int ld) {
        return r.dry ? 0 : launch_swin_layernorm(a, w.g, w.b, o, (int64_t)B * H * W, w.c, ld, 1e-5f, r.s);
    }
    int lrelu(half_t* a, size_t cnt, float slope) { return r.dry ? 0 : launch_swin_lrelu(a, (int64_t)cnt, slope, r.s); }
    // a packed 3x3 conv (n_pad 32 / 64) on rrdb_conv (rrdb.hip), output grid x f: the first cin columns of src's lda-wide rows -> dst
    int rrdb(const ConvW& w, const half_t* src, int cin, int lda, int f, int up, void* dst, int ldo, int ep, int store = RRDB_ST_F16,
             const half_t* r1 = nullptr, int ldr1 = 0) {
        if (r.dry) return 0;
        RrdbP p{};
        p.in = src; p.w = w.w; p.bias = w.b; p.r1 = r1; p.out = dst;     // w.b: null for a pack without a bias (ConvW's default)
        p.B = B; p.H = H * f; p.W = W * f; p.cin = cin; p.lda = lda; p.up = up; p.ldo = ldo; p.n_real = w.cout; p.ldr1 = ldr1; p.ep = ep; p.store = store;
        p.alpha = 1.f; p.beta = 1.f;
        return launch_rrdb_conv(p, w.n_pad, r.s);
    }
};

// The pixelshuffle tail of a forward (Swin2SR's upsampler 1, DAT) on the grid g: conv_before_upsample, LeakyReLU 0.01, per step the conv
// 64 -> f^2 64 (GEMM) and the shuffle, conv_last on rrdb_conv onto `full`, which swin_output crops to the H x W image (x sc).  c1: [M][64];
// up[0], up[1]: [M sc^2][64], the step convs' outputs and their shuffles
static int pixelshuffle_tail(Grid& g, const ConvW& before, const ConvW* ps, const ConvW& last, int sc, const half_t* trunk, half_t* c1,
                             half_t* const* up, float* full, void* out, int out_u8, int H, int W) {
    Run& r = g.r;
    TRY(g.conv(before, trunk, nullptr, c1));
    TRY(g.lrelu(c1, (size_t)g.B * g.H * g.W * 64, 0.01f));
    const int f = sc == 3 ? 3 : 2;
    const half_t* t = c1;
    int m = 1;                                                // the grid so far: (g.H m) x (g.W m)
    for (int k = 0; k < (sc == 4 ? 2 : 1); ++k) {
        TRY(g.conv(ps[k], t, nullptr, up[0], 0, m));
        if (!r.dry) TRY(launch_swin2_pixel_shuffle(up[0], up[1], g.B, g.H * m, g.W * m, f, r.s));
        t = up[1];
        m *= f;
    }
    TRY(g.rrdb(last, up[1], 64, 64, sc, 0, full, 0, RRDB_EP_NONE, RRDB_ST_F32_NCHW));
    return r.dry ? 0 : launch_swin_output(full, out, out_u8, g.B, H * sc, W * sc, g.H * sc, g.W * sc, r.s);
}

// Every family's two entries over its walk pass(r, net, in, in_u8, B, H, W, out, out_u8), which is one pass over an arena.  The arena bytes
// of a run: what a dry walk takes from a private arena, 0 for a size that size_ok(net, B, H, W) refuses ...
template <class Net, class SizeOk, class Pass>
static int64_t net_scratch_bytes(const Net* n, int B, int H, int W, SizeOk size_ok, Pass pass) {
    if (!n || !size_ok(*n, B, H, W)) return 0;
    Arena ar;
    ar.dry = true;
    Run dry(n->e, nullptr, true, &ar);
    if (pass(dry, *n, nullptr, 0, B, H, W, nullptr, 0) != 0) return 0;
    return (int64_t)ar.high;
}
// ... and the run, out of the engine's arena, after the family's requirements on the size, size_check(n, B, H, W)
template <class Net, class SizeCheck, class Pass>
static int net_run(Net* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s, SizeCheck size_check, Pass pass) {
    SDMI_REQUIRE(n && in && out, "null argument");
    TRY(size_check(n, B, H, W));
    sdmi_engine* e = n->e;
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    const bool tiling = e->tiling;                            // p.tiling belongs to the diffusion model's convs, not to an upscaler's
    e->tiling = false;
    struct Restore { sdmi_engine* e; bool v; ~Restore() { e->tiling = v; } } restore{e, tiling};
    return two_pass(e->arena, s, [&](bool dry) {
        Run r(e, s, dry);
        return pass(r, *n, in, in_u8, B, H, W, out, out_u8);
    });
}
static bool nonempty(const sdmi_net&, int B, int H, int W) { return B > 0 && H > 0 && W > 0; }

// the floats of one conv / linear in a blob: the OIHW weight and the bias
static int64_t lin(int64_t o, int64_t i, int64_t taps = 1) { return o * i * taps + o; }

// the range checks on a config's list of layers: what is wrong with it, or null
static const char* depths_wrong(int num_layers, const int* depths) {
    if (num_layers < 1 || num_layers > 16) return "num_layers in 1..16";
    for (int i = 0; i < num_layers; ++i)
        if (depths[i] < 1 || depths[i] > 64) return "depths[i] in 1..64";
    return nullptr;
}

// ------------------------------------------------------------------------------------------------------------
// RRDBNet upscalers (ESRGAN / Real-ESRGAN): BasicSR's RRDBNet.forward (basicsr/archs/rrdbnet_arch.py) as rrdb_conv launches
// ------------------------------------------------------------------------------------------------------------
// blob: fp32, for every conv in checkpoint order (conv_first, body.{i}.rdb{1..3}.conv{1..5}, conv_body, conv_up1, conv_up2, conv_hr,
// conv_last) the OIHW weight followed by the bias.
int64_t esrgan_blob_floats(int num_block, int in_ch) {
    int64_t n = lin(64, in_ch, 9);
    for (int k = 0; k < 5; ++k) n += (int64_t)num_block * 3 * lin(k < 4 ? 32 : 64, 64 + 32 * k, 9);
    return n + 4 * lin(64, 64, 9) + lin(3, 64, 9);
}

int esrgan_create(sdmi_engine* e, const float* blob, int64_t blob_floats, int num_block, int in_ch, int scale, sdmi_esrgan** out) {
    SDMI_REQUIRE(e && blob && out, "null argument");
    SDMI_REQUIRE(num_block >= 1 && num_block <= 64, "num_block");
    SDMI_REQUIRE((scale == 4 && in_ch == 3) || (scale == 2 && in_ch == 12) || (scale == 1 && in_ch == 48),
                 "RRDBNet: scale 4 / 2 / 1 with 3 / 12 / 48 input channels (pixel-unshuffle in front of conv_first)");
    SDMI_REQUIRE(blob_floats == esrgan_blob_floats(num_block, in_ch), "weight blob size does not match num_block / in_ch");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_esrgan> net(new sdmi_esrgan);
    net->e = e; net->num_block = num_block; net->in_ch = in_ch; net->scale = scale; net->unshuffle = 4 / scale;
    net->cin0 = rup(in_ch, 32);
    StagedBlob dblob;
    TRY(dblob.stage(blob, blob_floats));
    int64_t off = 0;
    auto pack = [&](sdmi_esrgan::Conv* c, int O, int I) -> int {
        c->cin = rup(I, 32); c->nout = O <= 32 ? 32 : 64; c->n_real = O;
        const size_t wb = (size_t)c->nout * 9 * c->cin * sizeof(half_t), bb = (size_t)c->nout * sizeof(float);
        TRY(net_upload(net.get(), nullptr, wb, (void**)&c->w));
        TRY(net_upload(net.get(), nullptr, bb, (void**)&c->b));
        TRY(launch_pack_conv_weight(dblob.p + off, 1, c->w, O, I, 3, 3, c->nout, c->cin, 0, nullptr));
        off += (int64_t)O * I * 9;
        SDMI_CHECK_HIP(hipMemset(c->b, 0, bb));
        SDMI_CHECK_HIP(hipMemcpy(c->b, dblob.p + off, (size_t)O * sizeof(float), hipMemcpyDeviceToDevice));
        off += O;
        return 0;
    };
    TRY(pack(&net->first, 64, in_ch));
    net->rdb.resize((size_t)num_block * 15);
    for (int i = 0; i < num_block * 3; ++i)
        for (int k = 0; k < 5; ++k) TRY(pack(&net->rdb[(size_t)i * 5 + k], k < 4 ? 32 : 64, 64 + 32 * k));
    TRY(pack(&net->body, 64, 64));
    TRY(pack(&net->up1, 64, 64));
    TRY(pack(&net->up2, 64, 64));
    TRY(pack(&net->hr, 64, 64));
    TRY(pack(&net->last, 3, 64));
    SDMI_CHECK_HIP(hipDeviceSynchronize());
    *out = net.release();
    return 0;
}

// One pass over the network (dry: the arena layout alone).  M = B * h * w low-resolution pixels
static int esrgan_pass(Run& r, const sdmi_esrgan& n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8) {
    const int f = n.unshuffle, h = H / f, w = W / f;
    const size_t M = (size_t)B * h * w;
    r.ar->reset();
    half_t* xin = r.H(M * n.cin0);
    half_t* x[3];
    for (half_t*& p : x) p = r.H(M * 192);
    half_t* feat = r.H(M * 64);
    half_t* trunk = r.H(M * 64);
    half_t* u1 = r.H(4 * M * 64);
    half_t* u2 = r.H(16 * M * 64);
    half_t* u3 = r.H(16 * M * 64);
    if (r.dry) return 0;

    auto conv = [&](const sdmi_esrgan::Conv& c, const half_t* src, int lda, int hh, int ww, int up, void* dst, int ldo, int ep,
                    float alpha = 1.f, const half_t* r1 = nullptr, int ldr1 = 0, float beta = 1.f, const half_t* r2 = nullptr, int ldr2 = 0,
                    int store = RRDB_ST_F16) -> int {
        RrdbP p{};
        p.in = src; p.w = c.w; p.bias = c.b; p.r1 = r1; p.r2 = r2; p.out = dst;
        p.B = B; p.H = hh; p.W = ww; p.cin = c.cin; p.lda = lda; p.up = up;
        p.ldo = ldo; p.n_real = c.n_real; p.ldr1 = ldr1; p.ldr2 = ldr2; p.ep = ep; p.store = store; p.alpha = alpha; p.beta = beta;
        return launch_rrdb_conv(p, c.nout, r.s);
    };

    TRY(launch_rrdb_input(in, in_u8, xin, B, 3, H, W, f, n.cin0, r.s));
    // conv_first twice (K = 288: 0.4 % of the network's work): once into `feat`, the trunk's skip tensor that conv_body's epilogue adds,
    // once into channels 0..63 of the first dense buffer.  conv_body cannot read that skip from x[0]: the third RDB of every RRDB writes
    // its result over x[0], so by then x[0] holds the body's output, not conv_first's.
    TRY(conv(n.first, xin, n.cin0, h, w, 0, feat, 64, RRDB_EP_NONE));
    TRY(conv(n.first, xin, n.cin0, h, w, 0, x[0], 192, RRDB_EP_NONE));
    // Dense blocks on three rotating 192-wide buffers: RDB j of an RRDB reads x[j] and writes channels 0..63 of x[(j + 1) % 3], so the
    // third one lands on x[0] — the RRDB's own input, which its epilogue reads as r2 (same element, same lane, before the store).
    for (int i = 0; i < n.num_block; ++i)
        for (int j = 0; j < 3; ++j) {
            const sdmi_esrgan::Conv* c = &n.rdb[((size_t)i * 3 + j) * 5];
            half_t* src = x[j];
            half_t* dst = x[(j + 1) % 3];
            for (int k = 0; k < 4; ++k) TRY(conv(c[k], src, 192, h, w, 0, src + 64 + 32 * k, 192, RRDB_EP_LRELU));
            if (j < 2) TRY(conv(c[4], src, 192, h, w, 0, dst, 192, RRDB_EP_RES1, 0.2f, src, 192));
            else TRY(conv(c[4], src, 192, h, w, 0, dst, 192, RRDB_EP_RES2, 0.2f, src, 192, 0.2f, dst, 192));
        }
    TRY(conv(n.body, x[0], 192, h, w, 0, trunk, 64, RRDB_EP_RES1, 1.f, feat, 64));
    TRY(conv(n.up1, trunk, 64, 2 * h, 2 * w, 1, u1, 64, RRDB_EP_LRELU));
    TRY(conv(n.up2, u1, 64, 4 * h, 4 * w, 1, u2, 64, RRDB_EP_LRELU));
    TRY(conv(n.hr, u2, 64, 4 * h, 4 * w, 0, u3, 64, RRDB_EP_LRELU));
    TRY(conv(n.last, u3, 64, 4 * h, 4 * w, 0, out, 0, RRDB_EP_NONE, 1.f, nullptr, 0, 1.f, nullptr, 0,
             out_u8 ? RRDB_ST_U8_HWC : RRDB_ST_F32_NCHW));
    return 0;
}

static int esrgan_size_check(const sdmi_esrgan* n, int B, int H, int W) {
    const int f = n->unshuffle;
    SDMI_REQUIRE(B > 0 && H > 0 && W > 0 && H % f == 0 && W % f == 0, "image sides must be multiples of the model's pixel-unshuffle factor");
    const int h = H / f, w = W / f;
    SDMI_REQUIRE((long long)B * h * w * 16 < (1ll << 31) - 256, "image too large: B*H*W*16 output pixels must stay below 2^31");
    return 0;
}
int64_t esrgan_scratch_bytes(const sdmi_esrgan* n, int B, int H, int W) { return net_scratch_bytes(n, B, H, W, nonempty, esrgan_pass); }
int esrgan_run(sdmi_esrgan* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s) {
    return net_run(n, in, in_u8, B, H, W, out, out_u8, s, esrgan_size_check, esrgan_pass);
}

// ------------------------------------------------------------------------------------------------------------
// Compact Real-ESRGAN upscalers: SRVGGNetCompact.forward (realesrgan/archs/srvgg_arch.py) as compact_conv launches
// ------------------------------------------------------------------------------------------------------------
// blob: fp32, for every conv in checkpoint order (body.0, body.2, ..., body.{2 (num_conv + 1)}) the OIHW weight, the bias, then (all
// but the last conv) the 64 PReLU slopes.
int64_t compact_blob_floats(int num_conv, int scale) {
    return (64 * 3 * 9 + 64 + 64) + (int64_t)num_conv * (64 * 64 * 9 + 64 + 64) + (3 * scale * scale * 64 * 9 + 3 * scale * scale);
}

int compact_create(sdmi_engine* e, const float* blob, int64_t blob_floats, int num_conv, int scale, sdmi_compact** out) {
    SDMI_REQUIRE(e && blob && out, "null argument");
    SDMI_REQUIRE(num_conv >= 1 && num_conv <= 256, "num_conv");
    SDMI_REQUIRE(scale >= 1 && scale <= 4, "SRVGGNetCompact: scale 1..4 (3 scale^2 <= 64 channels to shuffle)");
    SDMI_REQUIRE(blob_floats == compact_blob_floats(num_conv, scale), "weight blob size does not match num_conv / scale");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_compact> net(new sdmi_compact);
    net->e = e; net->num_conv = num_conv; net->scale = scale;
    StagedBlob dblob;
    TRY(dblob.stage(blob, blob_floats));
    int64_t off = 0;
    net->convs.resize((size_t)num_conv + 2);
    for (int i = 0; i < num_conv + 2; ++i) {
        sdmi_compact::Conv* c = &net->convs[(size_t)i];
        const int O = i == num_conv + 1 ? 3 * scale * scale : 64, I = i == 0 ? 3 : 64, cin = i == 0 ? 32 : 64;
        TRY(net_upload(net.get(), nullptr, (size_t)64 * 9 * cin * sizeof(half_t), (void**)&c->w));
        TRY(net_upload(net.get(), nullptr, 2 * 64 * sizeof(float), (void**)&c->b));
        c->slope = c->b + 64;
        TRY(launch_pack_conv_weight(dblob.p + off, 1, c->w, O, I, 3, 3, 64, cin, 0, nullptr));
        off += (int64_t)O * I * 9;
        SDMI_CHECK_HIP(hipMemset(c->b, 0, 2 * 64 * sizeof(float)));
        SDMI_CHECK_HIP(hipMemcpy(c->b, dblob.p + off, (size_t)O * sizeof(float), hipMemcpyDeviceToDevice));
        off += O;
        if (i <= num_conv) {
            SDMI_CHECK_HIP(hipMemcpy(c->slope, dblob.p + off, 64 * sizeof(float), hipMemcpyDeviceToDevice));
            off += 64;
        }
    }
    SDMI_CHECK_HIP(hipDeviceSynchronize());
    *out = net.release();
    return 0;
}

// One pass over the network (dry: the arena layout alone).  M = B * H * W pixels: every activation is at the input's resolution
static int compact_pass(Run& r, const sdmi_compact& n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8) {
    const size_t M = (size_t)B * H * W;
    r.ar->reset();
    half_t* xin = r.H(M * 32);
    half_t* x[2];
    for (half_t*& p : x) p = r.H(M * 64);
    if (r.dry) return 0;

    TRY(launch_rrdb_input(in, in_u8, xin, B, 3, H, W, 1, 32, r.s));
    const half_t* src = xin;
    for (int i = 0; i < n.num_conv + 2; ++i) {
        const sdmi_compact::Conv& c = n.convs[(size_t)i];
        const bool last = i == n.num_conv + 1;
        CompactP p{};
        p.in = src; p.w = c.w; p.bias = c.b; p.slope = c.slope;
        p.B = B; p.H = H; p.W = W; p.cin = i == 0 ? 32 : 64; p.lda = p.cin;
        if (last) {                                   // the activations never see a high-resolution tensor
            p.ep = COMPACT_EP_TAIL; p.r = n.scale; p.n_real = 3 * n.scale * n.scale;
            p.base = in; p.base_u8 = in_u8; p.out = out; p.out_u8 = out_u8;
        } else {
            p.ep = COMPACT_EP_PRELU; p.n_real = 64; p.out = x[i & 1]; p.ldo = 64;
            src = x[i & 1];
        }
        TRY(launch_compact_conv(p, r.s));
    }
    return 0;
}

static int compact_size_check(const sdmi_compact* n, int B, int H, int W) {
    SDMI_REQUIRE(B > 0 && H > 0 && W > 0, "empty image");
    SDMI_REQUIRE((long long)B * H * W * n->scale * n->scale < (1ll << 31) - 256, "image too large: the output must stay below 2^31 pixels");
    return 0;
}
int64_t compact_scratch_bytes(const sdmi_compact* n, int B, int H, int W) { return net_scratch_bytes(n, B, H, W, nonempty, compact_pass); }
int compact_run(sdmi_compact* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s) {
    return net_run(n, in, in_u8, B, H, W, out, out_u8, s, compact_size_check, compact_pass);
}

// ------------------------------------------------------------------------------------------------------------
// SwinIR upscalers (nearest+conv upsampler): SwinIR.forward as GEMM launches (gemm.hip), swin_window_attn / swin_layernorm (swinir.hip)
// and the 64-channel tail on rrdb_conv (rrdb.hip)
// ------------------------------------------------------------------------------------------------------------
// blob: fp32, in the order include/sdmi.h documents at sdmi_swinir_config.
static bool swinir_config_ok(const sdmi_swinir_config& c, std::string* why) {
    auto fail = [&](const char* m) { if (why) *why = m; return false; };
    if (c.embed_dim < 1 || c.num_heads < 1 || c.embed_dim % c.num_heads) return fail("embed_dim must be a positive multiple of num_heads");
    if (c.num_heads * 32 < c.embed_dim) return fail("head dim = embed_dim / num_heads must be <= 32 (num_heads * 32 >= embed_dim)");
    if (const char* m = depths_wrong(c.num_layers, c.depths)) return fail(m);
    if (c.mlp_hidden < 1) return fail("mlp_hidden");
    if (c.scale != 2 && c.scale != 4) return fail("scale 4 (conv_up1, conv_up2) or 2 (conv_up1)");
    if (c.resi_3conv != 0 && c.resi_3conv != 1) return fail("resi_3conv 0 | 1");
    if (c.resi_3conv && (c.embed_dim % 4 || c.embed_dim / 4 > 64)) return fail("3conv: embed_dim / 4 must be an integer <= 64");
    return true;
}

int64_t swinir_blob_floats(const sdmi_swinir_config* c) {
    if (!c || !swinir_config_ok(*c, nullptr)) return 0;
    const int64_t C = c->embed_dim, Hd = c->mlp_hidden, q = C / 4;
    const int64_t resi = c->resi_3conv ? lin(q, C, 9) + lin(q, q) + lin(C, q, 9) : lin(C, C, 9);
    const int64_t block = 2 * C + 225 * c->num_heads + lin(3 * C, C) + lin(C, C) + 2 * C + lin(Hd, C) + lin(C, Hd);
    int64_t n = lin(C, 3, 9) + 2 * C;
    for (int i = 0; i < c->num_layers; ++i) n += c->depths[i] * block + resi;
    n += 2 * C + resi + lin(64, C, 9) + (c->scale == 4 ? 3 : 2) * lin(64, 64, 9) + lin(3, 64, 9);
    return n;
}

// Swin2SR: the SwinIR config its trunk shares (scale 3 and the pixel-shuffle tails are checked here, the rest by swinir_config_ok)
static bool swin2sr_config_ok(const sdmi_swin2sr_config& c, sdmi_swinir_config* base, std::string* why) {
    auto fail = [&](const char* m) { if (why) *why = m; return false; };
    if (c.upsampler < 0 || c.upsampler > 2) return fail("upsampler 0 (nearest+conv) | 1 (pixelshuffle) | 2 (pixelshuffledirect)");
    if (c.upsampler == 0 ? c.scale != 4 : (c.scale != 2 && c.scale != 3 && c.scale != 4))
        return fail("scale 4 with the nearest+conv upsampler, 2 | 3 | 4 with pixelshuffle / pixelshuffledirect");
    sdmi_swinir_config b{};
    b.embed_dim = c.embed_dim; b.num_layers = c.num_layers; b.num_heads = c.num_heads; b.mlp_hidden = c.mlp_hidden;
    b.resi_3conv = c.resi_3conv; b.scale = c.scale == 3 ? 4 : c.scale;
    for (int i = 0; i < 16; ++i) b.depths[i] = c.depths[i];
    if (!swinir_config_ok(b, why)) return false;
    b.scale = c.scale;
    if (base) *base = b;
    return true;
}

int64_t swin2sr_blob_floats(const sdmi_swin2sr_config* c) {
    sdmi_swinir_config b{};
    if (!c || !swin2sr_config_ok(*c, &b, nullptr)) return 0;
    const int64_t C = c->embed_dim, Hd = c->mlp_hidden, q = C / 4, s2 = c->scale == 3 ? 9 : 4;
    const int64_t resi = c->resi_3conv ? lin(q, C, 9) + lin(q, q) + lin(C, q, 9) : lin(C, C, 9);
    const int64_t block = lin(3 * C, C) + 226 * c->num_heads + lin(C, C) + 2 * C + lin(Hd, C) + lin(C, Hd) + 2 * C;
    int64_t n = lin(C, 3, 9) + lin(C, C) + 2 * C;
    for (int i = 0; i < c->num_layers; ++i) n += c->depths[i] * block + resi;
    n += 2 * C + resi;
    if (c->upsampler == 0) n += lin(64, C, 9) + 3 * lin(64, 64, 9) + lin(3, 64, 9);
    else if (c->upsampler == 1) n += lin(64, C, 9) + (c->scale == 4 ? 2 : 1) * lin(s2 * 64, 64, 9) + lin(3, 64, 9);
    else n += lin(3 * c->scale * c->scale, C, 9);
    return n;
}

// Uploads and packs the weights of a SwinIR (net->v2 == 0) or Swin2SR network off its blob; net->cfg, v2 and upsampler are set
static int swin_net_build(sdmi_swinir* net, const float* blob, int64_t blob_floats);

int swinir_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_swinir_config* cfg, sdmi_swinir** out) {
    SDMI_REQUIRE(e && blob && cfg && out, "null argument");
    std::string why;
    SDMI_REQUIRE(swinir_config_ok(*cfg, &why), "SwinIR config: " + why);
    SDMI_REQUIRE(blob_floats == swinir_blob_floats(cfg), "weight blob size does not match the config");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_swinir> net(new sdmi_swinir);
    net->e = e; net->cfg = *cfg;
    TRY(swin_net_build(net.get(), blob, blob_floats));
    *out = net.release();
    return 0;
}

int swin2sr_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_swin2sr_config* cfg, sdmi_swin2sr** out) {
    SDMI_REQUIRE(e && blob && cfg && out, "null argument");
    std::string why;
    sdmi_swinir_config base{};
    SDMI_REQUIRE(swin2sr_config_ok(*cfg, &base, &why), "Swin2SR config: " + why);
    SDMI_REQUIRE(blob_floats == swin2sr_blob_floats(cfg), "weight blob size does not match the config");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_swin2sr> net(new sdmi_swin2sr);
    net->e = e; net->cfg = base; net->cfg2 = *cfg; net->v2 = 1; net->upsampler = cfg->upsampler;
    TRY(swin_net_build(net.get(), blob, blob_floats));
    *out = net.release();
    return 0;
}

static int swin_net_build(sdmi_swinir* net, const float* blob, int64_t blob_floats) {
    const sdmi_swinir_config* cfg = &net->cfg;
    const bool v2 = net->v2 != 0;
    const int C = cfg->embed_dim, heads = cfg->num_heads, D = C / heads, Hd = cfg->mlp_hidden, Cq = C / 4;
    const int Cp = rup(C, 64), hid_pad = rup(Hd, 64), ldq = rup(96 * heads, 64), lda = rup(32 * heads, 64);
    net->C = C; net->Cp = Cp; net->D = D; net->ldq = ldq; net->lda = lda; net->hid_pad = hid_pad;
    BlobPacker bp{net, blob, blob + blob_floats};
    auto ident = BlobPacker::ident;
    auto norm = [&](NormW* n) { return bp.norm(n, C); };
    // the conv that closes a layer / the trunk: 1conv, or 3conv with C / 4 padded to 64
    auto resi = [&](ConvW* c) -> int {
        if (!cfg->resi_3conv) return bp.conv(&c[0], C, C, 9, Cp, Cp);
        TRY(bp.conv(&c[0], Cq, C, 9, 64, Cp));
        TRY(bp.conv(&c[1], Cq, Cq, 1, 64, 64));
        return bp.conv(&c[2], C, Cq, 9, Cp, 64);
    };
    auto slot = [&](int v) { return (v / D) * 32 + v % D; };          // feature h * D + d -> column h * 32 + d

    TRY(bp.conv(&net->first, C, 3, 9, Cp, 64));
    if (v2) TRY(bp.conv(&net->pe_proj, C, C, 1, Cp, Cp));
    TRY(norm(&net->pe_norm));
    net->layers.resize((size_t)cfg->num_layers);
    for (int i = 0; i < cfg->num_layers; ++i) {
        sdmi_swinir::Layer& L = net->layers[(size_t)i];
        L.blocks.resize((size_t)cfg->depths[i]);
        for (sdmi_swinir::Block& bk : L.blocks) {
            auto table = [&]() -> int {                                // [225][heads]
                const float* t = bp.src;
                bp.src += 225 * heads;
                return net_rel_bias(net, t, heads, (size_t)heads, 1, &bk.bias);
            };
            auto qkv = [&]() { return bp.conv(&bk.qkv, 3 * C, C, 1, ldq, Cp, [&](int o) { return (o / C) * heads * 32 + slot(o % C); }); };
            if (!v2) {
                TRY(norm(&bk.n1));
                TRY(table());
                TRY(qkv());
                TRY(bp.conv(&bk.proj, C, C, 1, Cp, lda, ident, slot));
                TRY(norm(&bk.n2));
            } else {
                TRY(qkv());
                TRY(table());
                TRY(bp.raw(&bk.head_scale, (size_t)heads));
                TRY(bp.conv(&bk.proj, C, C, 1, Cp, lda, ident, slot));
                TRY(norm(&bk.n1));
            }
            TRY(bp.conv(&bk.fc1, Hd, C, 1, hid_pad, Cp));
            TRY(bp.conv(&bk.fc2, C, Hd, 1, Cp, hid_pad));
            if (v2) TRY(norm(&bk.n2));
        }
        TRY(resi(L.conv));
    }
    TRY(norm(&net->norm));
    TRY(resi(net->after));
    if (net->upsampler == 0) {
        TRY(bp.conv(&net->before, 64, C, 9, 64, Cp));
        TRY(bp.conv(&net->up1, 64, 64, 9, 64, 64));
        if (cfg->scale == 4) TRY(bp.conv(&net->up2, 64, 64, 9, 64, 64));
        TRY(bp.conv(&net->hr, 64, 64, 9, 64, 64));
        TRY(bp.conv_last(&net->last));
    } else if (net->upsampler == 1) {
        TRY(bp.ps_tail(&net->before, net->ps, &net->last, C, Cp, cfg->scale));
    } else {
        TRY(bp.conv(&net->direct, 3 * cfg->scale * cfg->scale, C, 9, 64, Cp));
    }
    return bp.done();
}

// One pass over the network (dry: the arena layout alone).  M tokens = B * Hp * Wp on the padded grid; every token tensor is Cp wide with
// zeros in columns C .. Cp - 1 (zero weight rows / bias entries and swin_layernorm keep them so).
static int swinir_pass(Run& r, const sdmi_swinir& n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8) {
    const int Hp = rup(H, 8), Wp = rup(W, 8), sc = n.cfg.scale, Cp = n.Cp;
    const size_t M = (size_t)B * Hp * Wp;
    r.ar->reset();
    half_t* x0 = r.H(M * 64);                                 // the padded, mean-subtracted input
    half_t* feat = r.H(M * Cp);                               // conv_first's output: the trunk's skip tensor
    half_t* pool[4];                                          // token tensors: a layer's input and the blocks' ping-pong
    for (half_t*& p : pool) p = r.H(M * Cp);
    half_t* ln = r.H(M * Cp);
    half_t* qkv = r.H(M * n.ldq);
    half_t* att = r.H(M * n.lda);
    half_t* hid = r.H(M * n.hid_pad);
    half_t* c1 = r.H(M * 64);
    half_t* c2 = r.H(M * 64);
    half_t* up[3] = {nullptr, nullptr, nullptr};
    float* full = nullptr;
    if (n.upsampler == 0) {
        up[0] = r.H(M * 4 * 64); up[1] = sc == 4 ? r.H(M * 16 * 64) : nullptr; up[2] = r.H(M * sc * sc * 64);
    } else if (n.upsampler == 1) {                            // the step convs' outputs and their shuffles, ping-pong
        up[0] = r.H(M * sc * sc * 64); up[1] = r.H(M * sc * sc * 64);
    }
    if (n.upsampler != 2) full = r.F(M * sc * sc * 3);        // conv_last on the padded grid, cropped by swin_output

    Grid g{r, B, Hp, Wp};
    // conv(x) + resid with the layer-closing conv (1conv | 3conv)
    auto resi = [&](const ConvW* w, const half_t* a, const half_t* resid, half_t* o) -> int {
        if (!n.cfg.resi_3conv) return g.conv(w[0], a, resid, o);
        TRY(g.conv(w[0], a, nullptr, c1));
        TRY(g.lrelu(c1, M * 64, 0.2f));
        TRY(g.conv(w[1], c1, nullptr, c2));
        TRY(g.lrelu(c2, M * 64, 0.2f));
        return g.conv(w[2], c2, resid, o);
    };

    if (!r.dry) {
        TRY(launch_swin_input(in, in_u8, x0, B, H, W, Hp, Wp, 64, r.s));
        if (n.lda > 32 * n.cfg.num_heads)                     // an odd head count: proj reads 32 columns the attention never writes (zero weights, but not NaN x 0)
            SDMI_CHECK_HIP(hipMemsetAsync(att, 0, M * n.lda * sizeof(half_t), r.s));
    }
    TRY(g.conv(n.first, x0, nullptr, feat));
    half_t* x = pool[0];
    std::vector<half_t*> free_ = {pool[1], pool[2], pool[3]};
    if (n.v2) {                                               // Swin2SR's PatchEmbed has a 1x1 projection in front of its norm; the skip stays conv_first's output
        TRY(g.conv(n.pe_proj, feat, nullptr, ln));
        TRY(g.lnorm(n.pe_norm, ln, x, Cp));
    } else {
        TRY(g.lnorm(n.pe_norm, feat, x, Cp));
    }
    auto attention = [&](const sdmi_swinir::Block& bk, size_t j) -> int {    // qkv -> att
        if (r.dry) return 0;
        SwinAttnP a{};
        a.qkv = qkv; a.bias = bk.bias; a.out = att; a.B = B; a.H = Hp; a.W = Wp; a.heads = n.cfg.num_heads; a.D = n.D;
        a.ldq = n.ldq; a.ldo = n.lda; a.shift = (j & 1) ? 4 : 0;
        if (n.v2) { a.cosine = 1; a.head_scale = bk.head_scale; }
        else a.scale = 1.0f / sqrtf((float)n.D);
        return launch_swin_attention(a, r.s);
    };
    for (const sdmi_swinir::Layer& L : n.layers) {
        half_t* cur = x;
        for (size_t j = 0; j < L.blocks.size(); ++j) {
            const sdmi_swinir::Block& bk = L.blocks[j];
            if (n.v2) {
                // res-post-norm: no norm in front of qkv / fc1; the stream is updated in place by swin2_layernorm_add (the layer's
                // first block writes a fresh buffer: x stays the skip of the layer's closing conv); `ln` holds the branch outputs
                half_t* dst = cur;
                if (cur == x) { dst = free_.back(); free_.pop_back(); }
                auto lnadd = [&](const NormW& w, const half_t* resid, half_t* o) -> int {
                    return r.dry ? 0 : launch_swin2_layernorm_add(ln, w.g, w.b, resid, o, (int64_t)M, n.C, Cp, 1e-5f, r.s);
                };
                TRY(g.conv(bk.qkv, cur, nullptr, qkv));
                TRY(attention(bk, j));
                TRY(g.conv(bk.proj, att, nullptr, ln));
                TRY(lnadd(bk.n1, cur, dst));
                TRY(g.conv(bk.fc1, dst, nullptr, hid, EP_GELU));
                TRY(g.conv(bk.fc2, hid, nullptr, ln));
                TRY(lnadd(bk.n2, dst, dst));
                cur = dst;
                continue;
            }
            half_t* mid = free_.back(); free_.pop_back();
            half_t* nxt = free_.back(); free_.pop_back();
            TRY(g.lnorm(bk.n1, cur, ln, Cp));
            TRY(g.conv(bk.qkv, ln, nullptr, qkv));
            TRY(attention(bk, j));
            TRY(g.conv(bk.proj, att, cur, mid));
            TRY(g.lnorm(bk.n2, mid, ln, Cp));
            TRY(g.conv(bk.fc1, ln, nullptr, hid, EP_GELU));
            TRY(g.conv(bk.fc2, hid, mid, nxt));
            free_.push_back(mid);
            if (cur != x) free_.push_back(cur);
            cur = nxt;
        }
        half_t* y = free_.back(); free_.pop_back();
        TRY(resi(L.conv, cur, x, y));
        free_.push_back(x);
        if (cur != x) free_.push_back(cur);
        x = y;
    }
    TRY(g.lnorm(n.norm, x, ln, Cp));
    half_t* trunk = free_.back();
    TRY(resi(n.after, ln, feat, trunk));
    if (n.upsampler == 2) {                                   // pixelshuffledirect: one conv C -> 3 sc^2, the shuffle folded into the output pass
        TRY(g.conv(n.direct, trunk, nullptr, c1));
        return r.dry ? 0 : launch_swin2_output_shuffle(c1, out, out_u8, B, H, W, Hp, Wp, sc, 64, r.s);
    }
    if (n.upsampler == 1) return pixelshuffle_tail(g, n.before, n.ps, n.last, sc, trunk, c1, up, full, out, out_u8, H, W);
    TRY(g.conv(n.before, trunk, nullptr, c1));
    TRY(g.lrelu(c1, M * 64, 0.01f));
    // nearest+conv: the 64-channel convs on rrdb_conv, the 2x nearest upsampling in the gather of conv_up1 / conv_up2
    TRY(g.rrdb(n.up1, c1, 64, 64, 2, 1, up[0], 64, RRDB_EP_LRELU));
    const half_t* t = up[0];
    if (sc == 4) { TRY(g.rrdb(n.up2, t, 64, 64, 4, 1, up[1], 64, RRDB_EP_LRELU)); t = up[1]; }
    TRY(g.rrdb(n.hr, t, 64, 64, sc, 0, up[2], 64, RRDB_EP_LRELU));
    TRY(g.rrdb(n.last, up[2], 64, 64, sc, 0, full, 0, RRDB_EP_NONE, RRDB_ST_F32_NCHW));
    return r.dry ? 0 : launch_swin_output(full, out, out_u8, B, H * sc, W * sc, Hp * sc, Wp * sc, r.s);
}

static bool swinir_size_ok(const sdmi_swinir& n, int B, int H, int W) {
    if (B <= 0 || H < 8 || W < 8) return false;
    const long long M = (long long)B * rup(H, 8) * rup(W, 8);
    const long long widest = std::max<long long>({(long long)n.ldq, (long long)n.hid_pad, (long long)n.Cp, 64ll * n.cfg.scale * n.cfg.scale});
    return M * widest < (1ll << 31) - 256;
}

static int swinir_size_check(const sdmi_swinir* n, int B, int H, int W) {
    SDMI_REQUIRE(B > 0 && H >= 8 && W >= 8, "image sides must be at least 8 (a smaller side cannot be reflect-padded to a window)");
    SDMI_REQUIRE(swinir_size_ok(*n, B, H, W), "image too large: every intermediate tensor must stay below 2^31 elements");
    return 0;
}
int64_t swinir_scratch_bytes(const sdmi_swinir* n, int B, int H, int W) { return net_scratch_bytes(n, B, H, W, swinir_size_ok, swinir_pass); }
int swinir_run(sdmi_swinir* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s) {
    return net_run(n, in, in_u8, B, H, W, out, out_u8, s, swinir_size_check, swinir_pass);
}

// ------------------------------------------------------------------------------------------------------------
// ScuNET (SCUNet.forward of network_scunet.py, dim 64): the transformer Block of the 32- and 64-wide levels as scu_block launches
// (scunet.hip), of the 128- and 256-wide levels as swin_layernorm + GEMMs + swin_window_attn, the 1x1 convs and the 2x2 stride-2 /
// transposed convs as GEMMs (the latter through scu_patch2), the 3x3 pairs on rrdb_conv (32 / 64) or the GEMMs (128 / 256)
// ------------------------------------------------------------------------------------------------------------
// blob: fp32, in the order include/sdmi.h documents at sdmi_scunet_config.
static bool scunet_config_ok(const sdmi_scunet_config& c, std::string* why) {
    const char* m = depths_wrong(7, c.depths);
    if (m && why) *why = m;
    return !m;
}
static int scunet_stage_c(int st) { return 32 << (st < 4 ? st : 6 - st); }       // conv_dim = trans_dim of m_down1 .. m_body .. m_up1

int64_t scunet_blob_floats(const sdmi_scunet_config* c) {
    if (!c || !scunet_config_ok(*c, nullptr)) return 0;
    int64_t n = 64 * 3 * 9 + 3 * 64 * 9;
    for (int st = 0; st < 7; ++st) {
        const int64_t t = scunet_stage_c(st), D = 2 * t;
        const int64_t block = 2 * t + 225 * (t / 32) + (3 * t * t + 3 * t) + (t * t + t) + 2 * t + (4 * t * t + 4 * t) + (4 * t * t + t) +
                              2 * (D * D + D) + 2 * (t * t * 9);
        n += c->depths[st] * block;
        if (st < 3) n += 2 * D * D * 4;                     // Conv2d(D, 2 D, 2, 2)
        if (st > 3) n += 2 * D * D * 4;                     // ConvTranspose2d(2 D, D, 2, 2)
    }
    return n;
}

int scunet_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_scunet_config* cfg, sdmi_scunet** out) {
    SDMI_REQUIRE(e && blob && cfg && out, "null argument");
    std::string why;
    SDMI_REQUIRE(scunet_config_ok(*cfg, &why), "ScuNET config: " + why);
    SDMI_REQUIRE(blob_floats == scunet_blob_floats(cfg), "weight blob size does not match the config");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_scunet> net(new sdmi_scunet);
    net->e = e; net->cfg = *cfg;
    BlobPacker bp{net.get(), blob, blob + blob_floats};
    const float*& src = bp.src;
    // one conv / linear off the blob -> [O][taps][I] fp16 (+ [O] fp32 bias), no padding.  at(o, i, t): where the checkpoint keeps that
    // weight — the resampling convs gather across (o, i, t), which BlobPacker::conv's row and column maps cannot say
    auto pack = [&](ConvW* c, int O, int I, int taps, bool bias, const std::function<size_t(int, int, int)>& at) -> int {
        std::vector<half_t> w((size_t)O * taps * I);
        for (int o = 0; o < O; ++o)
            for (int t = 0; t < taps; ++t)
                for (int i = 0; i < I; ++i) w[((size_t)o * taps + t) * I + i] = (half_t)src[at(o, i, t)];
        src += (size_t)O * I * taps;
        c->cin = c->cin_pad = I; c->cout = c->n_pad = O; c->taps = taps;
        TRY(net_upload(net.get(), w.data(), w.size() * sizeof(half_t), (void**)&c->w));
        if (!bias) return 0;
        TRY(net_upload(net.get(), src, (size_t)O * sizeof(float), (void**)&c->b));
        src += O;
        return 0;
    };
    auto oihw = [](int I, int taps) { return [=](int o, int i, int t) { return ((size_t)o * I + i) * taps + t; }; };
    // m_head / m_tail on rrdb_conv, no bias: 3 input channels in a 32-wide row, 3 output channels of a 32-wide tile
    TRY(bp.conv(&net->head, 64, 3, 9, 64, 32, BlobPacker::ident, BlobPacker::ident, false));
    for (int st = 0; st < 7; ++st) {
        const int t = scunet_stage_c(st), D = 2 * t, heads = t / 32;
        if (st > 3)     // ConvTranspose2d(2 D, D, 2, 2) [2 D][D][2][2]: GEMM row (dy * 2 + dx) * D + o, column i
            TRY(pack(&net->up[6 - st], 4 * D, 2 * D, 1, false, [=](int n, int i, int) { return ((size_t)i * D + n % D) * 4 + n / D; }));
        net->stage[st].resize((size_t)cfg->depths[st]);
        for (sdmi_scunet::Block& bk : net->stage[st]) {
            bk.c = t;
            const float* ln1 = src;
            src += 2 * t;
            TRY(net_rel_bias(net.get(), src, heads, 1, 225, &bk.bias));      // relative_position_params [heads][15][15]
            src += 225 * heads;
            if (t <= 64) {
                // the Block's tensors as the pack kernel wants them: fp16 matrices, fp32 vectors, all temporaries
                std::vector<void*> tmp;
                auto up16 = [&](int n, const half_t** dev) -> int {
                    std::vector<half_t> w((size_t)n);
                    for (int i = 0; i < n; ++i) w[(size_t)i] = (half_t)src[i];
                    src += n;
                    void* d = nullptr;
                    SDMI_CHECK_HIP(hipMalloc(&d, std::max<size_t>((size_t)n * 2, 256)));
                    tmp.push_back(d);
                    SDMI_CHECK_HIP(hipMemcpy(d, w.data(), (size_t)n * 2, hipMemcpyHostToDevice));
                    *dev = (const half_t*)d;
                    return 0;
                };
                auto up32 = [&](const float* host, int n, const float** dev) -> int {
                    void* d = nullptr;
                    SDMI_CHECK_HIP(hipMalloc(&d, std::max<size_t>((size_t)n * 4, 256)));
                    tmp.push_back(d);
                    SDMI_CHECK_HIP(hipMemcpy(d, host, (size_t)n * 4, hipMemcpyHostToDevice));
                    *dev = (const float*)d;
                    return 0;
                };
                ScuPackP pp{};
                int rc = up32(ln1, t, &pp.ln1_g) || up32(ln1 + t, t, &pp.ln1_b);
                rc = rc || up16(3 * t * t, &pp.wqkv) || up32(src, 3 * t, &pp.bqkv); src += 3 * t;
                rc = rc || up16(t * t, &pp.wproj) || up32(src, t, &pp.bproj); src += t;
                rc = rc || up32(src, t, &pp.ln2_g) || up32(src + t, t, &pp.ln2_b); src += 2 * t;
                rc = rc || up16(4 * t * t, &pp.w1) || up32(src, 4 * t, &pp.b1); src += 4 * t;
                rc = rc || up16(4 * t * t, &pp.w2) || up32(src, t, &pp.b2); src += t;
                if (!rc) {
                    rc = net_upload(net.get(), nullptr, scu_block_pack_bytes(t), &bk.packs);
                    if (!rc) {
                        pp.packs = bk.packs;
                        rc = launch_scu_block_pack(pp, t, nullptr) || hipDeviceSynchronize() != hipSuccess;
                    }
                }
                for (void* d : tmp) (void)hipFree(d);
                SDMI_REQUIRE(!rc, "packing a Block's weights failed");
            } else {
                TRY(net_norm(net.get(), ln1, t, &bk.n1));
                TRY(pack(&bk.qkv, 3 * t, t, 1, true, oihw(t, 1)));
                TRY(pack(&bk.proj, t, t, 1, true, oihw(t, 1)));
                TRY(net_norm(net.get(), src, t, &bk.n2));
                TRY(pack(&bk.fc1, 4 * t, t, 1, true, oihw(t, 1)));
                TRY(pack(&bk.fc2, t, 4 * t, 1, true, oihw(4 * t, 1)));
            }
            TRY(pack(&bk.c11, D, D, 1, true, oihw(D, 1)));
            TRY(pack(&bk.c12, D, D, 1, true, oihw(D, 1)));
            TRY(pack(&bk.cb0, t, t, 9, false, oihw(t, 9)));
            TRY(pack(&bk.cb2, t, t, 9, false, oihw(t, 9)));
        }
        if (st < 3)     // Conv2d(D, 2 D, 2, 2) [2 D][D][2][2]: GEMM column (dy * 2 + dx) * D + i
            TRY(pack(&net->down[st], 2 * D, 4 * D, 1, false, [=](int o, int k, int) { return ((size_t)o * D + k % D) * 4 + k / D; }));
    }
    TRY(bp.conv(&net->tail, 3, 64, 9, 32, 64, BlobPacker::ident, BlobPacker::ident, false));
    TRY(bp.done());
    *out = net.release();
    return 0;
}

// One pass over the network (dry: the arena layout alone).  A fixed set of buffers whatever the depths: the four skip tensors, and
// level-1-sized work buffers that every level reuses (a level's tensors are half the size of the level above).
static int scunet_pass(Run& r, const sdmi_scunet& n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8) {
    const int Hp = rup(H, 64), Wp = rup(W, 64);
    const size_t M1 = (size_t)B * Hp * Wp;
    r.ar->reset();
    half_t* in0 = r.H(M1 * 32);
    half_t* skip[4] = {r.H(M1 * 64), r.H(M1 * 32), r.H(M1 * 16), r.H(M1 * 8)};      // x1 .. x4: [M1 / 4^l][64 << l]
    half_t* pool[2] = {r.H(M1 * 64), r.H(M1 * 64)};          // a stage's ping-pong
    half_t* Y = r.H(M1 * 64);                                 // conv1_1's output: conv_x | trans_x
    half_t* Z = r.H(M1 * 64);                                 // cat(conv_x, trans_x) that conv1_2 reads; the 2x2 patches of the resampling convs
    half_t* T = r.H(M1 * 32);                                 // between the two 3x3 convs
    // the Block at trans_dim 128 / 256 (levels 3 and 4; sized for level 3, M1 / 16 rows)
    half_t* lnb = r.H(M1 * 16);                               // [M][2 t]: swin_layernorm writes rows as wide as it reads
    half_t* qkv = r.H(M1 * 24);
    half_t* att = r.H(M1 * 8);
    half_t* mid = r.H(M1 * 8);
    half_t* hid = r.H(M1 * 32);
    float* full = r.F(M1 * 3);                                // m_tail on the padded grid, cropped by swin_output

    // one ConvTransBlock: x [M][D] -> o [M][D].  The GEMMs name their row strides (lda, ldr, ldo): most tensors here are halves of wider rows
    auto ctb = [&](const sdmi_scunet::Block& bk, int type_sw, const half_t* x, half_t* o, int h, int wd) -> int {
        const int t = bk.c, D = 2 * t;
        const size_t M = (size_t)B * h * wd;
        Grid g{r, B, h, wd};
        TRY(g.conv(bk.c11, x, nullptr, Y, 0, 1, D, 0, D));
        if (t <= 64) {
            TRY(g.rrdb(bk.cb0, Y, t, D, 1, 0, T, t, RRDB_EP_RELU));
            TRY(g.rrdb(bk.cb2, T, t, t, 1, 0, Z, D, RRDB_EP_RES1, RRDB_ST_F16, Y, D));
            if (!r.dry) {
                ScuBlockP p{};
                p.x = Y + t; p.out = Z + t; p.packs = bk.packs; p.bias = bk.bias; p.B = B; p.H = h; p.W = wd; p.ldx = D; p.ldo = D;
                p.shift = type_sw ? 4 : 0;
                TRY(launch_scu_block(p, t, r.s));
            }
        } else {
            TRY(g.conv(bk.cb0, Y, nullptr, T, 0, 1, D, 0, t));
            TRY(g.lrelu(T, M * t, 0.f));                      // slope 0: ReLU
            TRY(g.conv(bk.cb2, T, Y, Z, 0, 1, t, D, D));
            TRY(g.lnorm(bk.n1, Y + t, lnb, D));
            TRY(g.conv(bk.qkv, lnb, nullptr, qkv, 0, 1, D, 0, 3 * t));
            if (!r.dry) {
                SwinAttnP a{};                                // -100 where the reference has -inf: the same probabilities after an fp32 softmax
                a.qkv = qkv; a.bias = bk.bias; a.out = att; a.B = B; a.H = h; a.W = wd; a.heads = t / 32; a.D = 32;
                a.ldq = 3 * t; a.ldo = t; a.shift = type_sw ? 4 : 0; a.scale = 0.17677669529663689f;
                TRY(launch_swin_attention(a, r.s));
            }
            TRY(g.conv(bk.proj, att, Y + t, mid, 0, 1, t, D, t));
            TRY(g.lnorm(bk.n2, mid, att, t));
            TRY(g.conv(bk.fc1, att, nullptr, hid, EP_GELU, 1, t, 0, 4 * t));
            TRY(g.conv(bk.fc2, hid, mid, Z + t, 0, 1, 4 * t, t, D));
        }
        return g.conv(bk.c12, Z, x, o, 0, 1, D, D, D);
    };
    // the blocks of a stage through the ping-pong, block i into pool[(first + i) % 2] (the caller keeps `x` out of pool[first]);
    // *res: the buffer the result is in
    auto stage = [&](int st, const half_t* x, int h, int wd, int first, half_t** res) -> int {
        const half_t* cur = x;
        for (size_t i = 0; i < n.stage[st].size(); ++i) {
            half_t* o = pool[(first + i) & 1];
            TRY(ctb(n.stage[st][i], (int)(i & 1), cur, o, h, wd));
            cur = o;
        }
        *res = const_cast<half_t*>(cur);
        return 0;
    };

    Grid full_res{r, B, Hp, Wp};
    if (!r.dry) TRY(launch_scu_input(in, in_u8, in0, B, H, W, Hp, Wp, 32, r.s));
    TRY(full_res.rrdb(n.head, in0, 32, 32, 1, 0, skip[0], 64, RRDB_EP_NONE));
    half_t* x = nullptr;
    for (int l = 0; l < 3; ++l) {                             // m_down1 .. m_down3
        const int h = Hp >> l, wd = Wp >> l, D = 64 << l;
        TRY(stage(l, skip[l], h, wd, 0, &x));
        if (!r.dry) TRY(launch_scu_patch2(x, Z, B, h / 2, wd / 2, D, 1, r.s));
        Grid below{r, B, h / 2, wd / 2};
        TRY(below.conv(n.down[l], Z, nullptr, skip[l + 1]));
    }
    TRY(stage(3, skip[3], Hp >> 3, Wp >> 3, 0, &x));
    for (int l = 2; l >= 0; --l) {                            // m_up3 .. m_up1 at level l: x + skip, the transposed conv, the blocks
        const int h = Hp >> l, wd = Wp >> l, D = 64 << l;
        if (!r.dry) TRY(launch_scu_add(x, skip[l + 1], (int64_t)B * (h / 2) * (wd / 2) * 2 * D, r.s));
        Grid below{r, B, h / 2, wd / 2};
        TRY(below.conv(n.up[l], x, nullptr, Z));
        if (!r.dry) TRY(launch_scu_patch2(Z, x, B, h / 2, wd / 2, D, 0, r.s));       // over the GEMM's input: it is dead
        TRY(stage(6 - l, x, h, wd, x == pool[0] ? 1 : 0, &x));
    }
    if (r.dry) return 0;
    TRY(launch_scu_add(x, skip[0], (int64_t)M1 * 64, r.s));
    TRY(full_res.rrdb(n.tail, x, 64, 64, 1, 0, full, 0, RRDB_EP_NONE, RRDB_ST_F32_NCHW));
    return launch_swin_output(full, out, out_u8, B, H, W, Hp, Wp, r.s);
}

static bool scunet_size_ok(const sdmi_scunet&, int B, int H, int W) {
    if (B <= 0 || H < 1 || W < 1) return false;
    return (long long)B * rup(H, 64) * rup(W, 64) * 64 < (1ll << 31) - 256;
}

static int scunet_size_check(const sdmi_scunet* n, int B, int H, int W) {
    SDMI_REQUIRE(B > 0 && H >= 1 && W >= 1, "empty image");
    SDMI_REQUIRE(scunet_size_ok(*n, B, H, W), "image too large: every intermediate tensor must stay below 2^31 elements");
    return 0;
}
int64_t scunet_scratch_bytes(const sdmi_scunet* n, int B, int H, int W) { return net_scratch_bytes(n, B, H, W, scunet_size_ok, scunet_pass); }
int scunet_run(sdmi_scunet* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s) {
    return net_run(n, in, in_u8, B, H, W, out, out_u8, s, scunet_size_check, scunet_pass);
}

// ------------------------------------------------------------------------------------------------------------
// DAT upscalers (pixelshuffle, 1conv): DAT.forward as GEMM launches (gemm.hip), swin_layernorm and Swin2SR's tail passes (swinir.hip),
// the window / channel attention, depthwise convs and AIM gates of dat.hip, conv_last on rrdb_conv (rrdb.hip)
// ------------------------------------------------------------------------------------------------------------
// blob: fp32, in the order include/sdmi.h documents at sdmi_dat_config.
static bool dat_config_ok(const sdmi_dat_config& c, std::string* why) {
    auto fail = [&](const char* m) { if (why) *why = m; return false; };
    if (c.embed_dim < 16 || c.num_heads < 2 || c.embed_dim % c.num_heads) return fail("embed_dim must be at least 16 and a multiple of num_heads");
    if (c.num_heads % 2) return fail("num_heads must be even (half of the heads per window branch)");
    if (c.num_heads * 32 < c.embed_dim) return fail("head dim = embed_dim / num_heads must be <= 32 (num_heads * 32 >= embed_dim)");
    if (c.num_heads * 32 > 512 || (c.embed_dim / 16) * c.num_heads * 32 > 8192) return fail("num_heads * 32 must be <= 512 (the AIM pass holds a row per wave)");
    if (c.split0 != 8 || (c.split1 != 16 && c.split1 != 32)) return fail("split must be (8, 16) or (8, 32)");
    if (const char* m = depths_wrong(c.num_layers, c.depths)) return fail(m);
    if (c.ffn_hidden < 2 || c.ffn_hidden % 2) return fail("ffn_hidden must be even (the feed-forward gate splits it in two)");
    if (c.scale != 2 && c.scale != 3 && c.scale != 4) return fail("scale 2 | 3 | 4");
    return true;
}

int64_t dat_blob_floats(const sdmi_dat_config* c) {
    if (!c || !dat_config_ok(*c, nullptr)) return 0;
    const int64_t C = c->embed_dim, E = c->ffn_hidden, hf = E / 2, C8 = C / 8, C16 = C / 16, hh = c->num_heads / 2;
    const int64_t tab = (2 * c->split0 - 1) * (2 * c->split1 - 1) * hh, s2 = c->scale == 3 ? 9 : 4;
    const int64_t common = 2 * C + lin(3 * C, C) + 10 * C + (C8 * C + C8 + C * C8 + C) + (C16 * C + 2 * C16 + 1) + lin(C, C) + 2 * C + lin(E, C) +
                           2 * hf + 10 * hf + lin(C, hf);
    int64_t n = lin(C, 3, 9) + 2 * C;
    for (int i = 0; i < c->num_layers; ++i) {
        const int64_t d = c->depths[i], spatial = (d + 1) / 2;
        n += d * common + spatial * 2 * tab + (d - spatial) * c->num_heads + lin(C, C, 9);
    }
    return n + 2 * C + lin(C, C, 9) + lin(64, C, 9) + (c->scale == 4 ? 2 : 1) * lin(s2 * 64, 64, 9) + lin(3, 64, 9);
}

int dat_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_dat_config* cfg, sdmi_dat** out) {
    SDMI_REQUIRE(e && blob && cfg && out, "null argument");
    std::string why;
    SDMI_REQUIRE(dat_config_ok(*cfg, &why), "DAT config: " + why);
    SDMI_REQUIRE(blob_floats == dat_blob_floats(cfg), "weight blob size does not match the config");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_dat> holder(new sdmi_dat);
    sdmi_dat* net = holder.get();
    net->e = e; net->cfg = *cfg;
    const int C = cfg->embed_dim, heads = cfg->num_heads, D = C / heads, E = cfg->ffn_hidden, hf = E / 2, C8 = C / 8, C16 = C / 16;
    const int Cp = rup(C, 64), Sp = 32 * heads, Hh = rup(hf, 64);
    net->C = C; net->Cp = Cp; net->D = D; net->Sp = Sp; net->half = hf; net->Hh = Hh; net->C8 = C8; net->C16 = C16;
    BlobPacker bp{net, blob, blob + blob_floats};
    auto ident = BlobPacker::ident;
    auto slot = [&](int v) { return (v / D) * 32 + v % D; };            // channel h * D + d -> column h * 32 + d
    const size_t tab = (size_t)(2 * cfg->split0 - 1) * (2 * cfg->split1 - 1) * (heads / 2);

    TRY(bp.conv(&net->first, C, 3, 9, Cp, 64));
    TRY(bp.norm(&net->rg_norm, C));
    net->layers.resize((size_t)cfg->num_layers);
    for (int i = 0; i < cfg->num_layers; ++i) {
        sdmi_dat::Layer& L = net->layers[(size_t)i];
        L.blocks.resize((size_t)cfg->depths[i]);
        for (int j = 0; j < cfg->depths[i]; ++j) {
            sdmi_dat::Block& bk = L.blocks[(size_t)j];
            bk.spatial = j % 2 == 0;
            bk.shifted = bk.spatial && ((i % 2 == 0 && j > 0 && (j - 2) % 4 == 0) || (i % 2 == 1 && j % 4 == 0));
            TRY(bp.norm(&bk.n1, C));
            TRY(bp.conv(&bk.qkv, 3 * C, C, 1, 3 * Sp, Cp, [&](int o) { return (o / C) * Sp + slot(o % C); }));
            if (bk.spatial) {
                TRY(bp.raw(&bk.tab0, tab));
                TRY(bp.raw(&bk.tab1, tab));
            } else {
                TRY(bp.raw(&bk.temperature, (size_t)heads));
            }
            TRY(bp.mat(&bk.dw_w, 9, C, 9, Sp, ident, slot, true));
            TRY(bp.mat(&bk.dw_b, 1, C, 1, Sp, ident, slot));
            TRY(bp.mat(&bk.ci_w1, C8, C, C8, Sp, ident, slot));
            TRY(bp.raw(&bk.ci_b1, (size_t)C8));
            TRY(bp.mat(&bk.ci_w2, C, C8, Sp, C8, slot, ident));
            TRY(bp.mat(&bk.ci_b2, 1, C, 1, Sp, ident, slot));
            TRY(bp.mat(&bk.si_w1, C16, C, C16, Sp, ident, slot));
            TRY(bp.raw(&bk.si_b1, (size_t)C16));
            TRY(bp.raw(&bk.si_w2, (size_t)C16));
            bk.si_b2 = bp.scalar();
            TRY(bp.conv(&bk.proj, C, C, 1, Cp, Sp, ident, slot));
            TRY(bp.norm(&bk.n2, C));
            TRY(bp.conv(&bk.fc1, E, C, 1, 2 * Hh, Cp, [&](int o) { return o < hf ? o : Hh + o - hf; }));     // x1 | x2 in two 64-multiple halves
            TRY(bp.norm(&bk.sgn, hf));
            TRY(bp.mat(&bk.sg_w, 9, hf, 9, Hh, ident, ident, true));
            TRY(bp.mat(&bk.sg_b, 1, hf, 1, Hh));
            TRY(bp.conv(&bk.fc2, C, hf, 1, Cp, Hh));
        }
        TRY(bp.conv(&L.conv, C, C, 9, Cp, Cp));
    }
    TRY(bp.norm(&net->norm, C));
    TRY(bp.conv(&net->after, C, C, 9, Cp, Cp));
    TRY(bp.ps_tail(&net->before, net->ps, &net->last, C, Cp, cfg->scale));
    TRY(bp.done());
    *out = holder.release();
    return 0;
}

// One pass over the network (dry: the arena layout alone).  M = B * H * W tokens, no padding of the grid (the window attention pads by
// index).  Stream tensors are Cp wide with zeros in columns C .. Cp - 1; q | k | v, att, the AIM conv and proj's input are Sp = 32 heads wide
// in head slots; fc1 writes x1 | x2 as two Hh-wide halves of one row.
static int dat_pass(Run& r, const sdmi_dat& n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8) {
    const int sc = n.cfg.scale, Cp = n.Cp, Sp = n.Sp, Hh = n.Hh, heads = n.cfg.num_heads, N = H * W;
    const size_t M = (size_t)B * N;
    r.ar->reset();
    half_t* x0 = r.H(M * 64);                                 // the mean-subtracted input
    half_t* feat = r.H(M * Cp);                               // conv_first's output: the trunk's skip tensor
    half_t* pool[4];                                          // token tensors: a group's input and the blocks' ping-pong
    for (half_t*& p : pool) p = r.H(M * Cp);
    half_t* ln = r.H(M * Cp);
    half_t* qkv = r.H(M * 3 * Sp);
    half_t* att = r.H(M * Sp);
    half_t* cv = r.H(M * Sp);                                 // GELU(BN(dwconv(v)))
    half_t* mix = r.H(M * Sp);                                // what proj reads
    half_t* hid = r.H(M * 2 * Hh);
    half_t* gated = r.H(M * Hh);                              // x1 * dwconv(norm(x2))
    float* gram = r.F((size_t)B * heads * cdiv(N, DAT_GRAM_TOKENS) * 1088);
    half_t* amat = r.H((size_t)B * Sp * Sp);
    float* pool_ws = r.F((size_t)B * cdiv(N, DAT_POOL_TOKENS) * Sp);
    float* cgate = r.F((size_t)B * Sp);
    half_t* c1 = r.H(M * 64);
    half_t* up[2] = {r.H(M * sc * sc * 64), r.H(M * sc * sc * 64)};      // the step convs' outputs and their shuffles, ping-pong
    float* full = r.F(M * sc * sc * 3);

    Grid g{r, B, H, W};
    // everything between qkv and proj
    auto attention = [&](const sdmi_dat::Block& bk) -> int {
        if (r.dry) return 0;
        const half_t* v = qkv + 2 * Sp;
        if (bk.spatial) {
            DatAttnP a{};
            a.qkv = qkv; a.bias0 = bk.tab0; a.bias1 = bk.tab1; a.out = att; a.B = B; a.H = H; a.W = W; a.heads = heads; a.D = n.D;
            a.ldq = 3 * Sp; a.ldo = Sp; a.s0 = n.cfg.split0; a.s1 = n.cfg.split1; a.shifted = bk.shifted ? 1 : 0; a.scale = 1.0f / sqrtf((float)n.D);
            TRY(launch_dat_window_attention(a, r.s));
        } else {
            TRY(launch_dat_channel_gram(qkv, gram, B, N, heads, 3 * Sp, r.s));
            TRY(launch_dat_channel_softmax(gram, bk.temperature, amat, B, N, heads, n.D, r.s));
            GemmP gp{};                                       // att[b] = v[b] A[b]^T: a batched 1x1 GEMM with per-image weights
            gp.a0 = v; gp.c0 = Sp; gp.cin = Sp; gp.lda0 = 3 * Sp;
            gp.w = amat; gp.ldw = Sp;
            gp.out = att;
            gp.Hi = N; gp.Wi = 1; gp.Ho = N; gp.Wo = 1; gp.taps = 1; gp.stride = 1;
            gp.M = N; gp.N = Sp; gp.K = Sp; gp.ldo = Sp; gp.rows_per_batch = N; gp.n_real = Sp;
            gp.alpha = 1.f;
            gp.a_bs = (long)N * 3 * Sp; gp.w_bs = (long)Sp * Sp; gp.o_bs = (long)N * Sp;
            TRY(launch_gemm(gp, B, r.e->force_generic, r.e->use_glds, r.s));
        }
        TRY(launch_dat_dwconv3x3(v, bk.dw_w, bk.dw_b, nullptr, cv, B, H, W, Sp, 3 * Sp, 0, Sp, 0, r.s));
        const half_t* sop = bk.spatial ? att : cv;            // the spatial MLP's operand; the channel gate is pooled from the other
        const half_t* top = bk.spatial ? cv : att;
        TRY(launch_dat_pool_gate(top, bk.ci_w1, bk.ci_b1, bk.ci_w2, bk.ci_b2, pool_ws, cgate, B, N, Sp, n.C8, Sp, r.s));
        DatAimP m{};
        m.s = sop; m.t = top; m.cg = cgate; m.w1 = bk.si_w1; m.b1 = bk.si_b1; m.w2 = bk.si_w2; m.b2 = bk.si_b2; m.out = mix;
        m.rows = (long long)M; m.rows_per_image = N; m.C = Sp; m.C16 = n.C16; m.lds = Sp; m.ldt = Sp; m.ldo = Sp;
        return launch_dat_aim_combine(m, r.s);
    };
    // x2 <- LayerNorm(x2) in place (a lane reads what it then writes), then x1 * dwconv(x2)
    auto gate = [&](const sdmi_dat::Block& bk) -> int {
        if (r.dry) return 0;
        TRY(g.lnorm(bk.sgn, hid + Hh, hid + Hh, 2 * Hh));
        return launch_dat_dwconv3x3(hid + Hh, bk.sg_w, bk.sg_b, hid, gated, B, H, W, Hh, 2 * Hh, 2 * Hh, Hh, 1, r.s);
    };

    if (!r.dry) TRY(launch_swin_input(in, in_u8, x0, B, H, W, H, W, 64, r.s));
    TRY(g.conv(n.first, x0, nullptr, feat));
    half_t* x = pool[0];
    std::vector<half_t*> free_ = {pool[1], pool[2], pool[3]};
    TRY(g.lnorm(n.rg_norm, feat, x, Cp));
    for (const sdmi_dat::Layer& L : n.layers) {
        half_t* cur = x;
        for (const sdmi_dat::Block& bk : L.blocks) {
            half_t* mid = free_.back(); free_.pop_back();
            half_t* nxt = free_.back(); free_.pop_back();
            TRY(g.lnorm(bk.n1, cur, ln, Cp));
            TRY(g.conv(bk.qkv, ln, nullptr, qkv));
            TRY(attention(bk));
            TRY(g.conv(bk.proj, mix, cur, mid));
            TRY(g.lnorm(bk.n2, mid, ln, Cp));
            TRY(g.conv(bk.fc1, ln, nullptr, hid, EP_GELU));
            TRY(gate(bk));
            TRY(g.conv(bk.fc2, gated, mid, nxt));
            free_.push_back(mid);
            if (cur != x) free_.push_back(cur);
            cur = nxt;
        }
        half_t* y = free_.back(); free_.pop_back();
        TRY(g.conv(L.conv, cur, x, y));
        free_.push_back(x);
        if (cur != x) free_.push_back(cur);
        x = y;
    }
    TRY(g.lnorm(n.norm, x, ln, Cp));
    half_t* trunk = free_.back();
    TRY(g.conv(n.after, ln, feat, trunk));
    return pixelshuffle_tail(g, n.before, n.ps, n.last, sc, trunk, c1, up, full, out, out_u8, H, W);
}

static bool dat_size_ok(const sdmi_dat& n, int B, int H, int W) {
    if (B <= 0 || H < 1 || W < 1) return false;
    const long long Mp = (long long)B * rup(H, n.cfg.split1) * rup(W, n.cfg.split1);      // the attention's padded grid
    const long long widest = std::max<long long>({3ll * n.Sp, 2ll * n.Hh, (long long)n.Cp, 64ll * n.cfg.scale * n.cfg.scale});
    return Mp * widest < (1ll << 31) - 256;
}

static int dat_size_check(const sdmi_dat* n, int B, int H, int W) {
    SDMI_REQUIRE(B > 0 && H >= 1 && W >= 1, "empty image");
    SDMI_REQUIRE(dat_size_ok(*n, B, H, W), "image too large: every intermediate tensor must stay below 2^31 elements");
    return 0;
}
int64_t dat_scratch_bytes(const sdmi_dat* n, int B, int H, int W) { return net_scratch_bytes(n, B, H, W, dat_size_ok, dat_pass); }
int dat_run(sdmi_dat* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s) {
    return net_run(n, in, in_u8, B, H, W, out, out_u8, s, dat_size_check, dat_pass);
}

// ------------------------------------------------------------------------------------------------------------
// HAT upscalers (pixelshuffle, 1conv, window 16, overlap ratio 0.5): HAT.forward as GEMM launches (gemm.hip; the two convs of the channel-
// attention branch as implicit GEMMs, the first with fc1's GELU epilogue), swin_layernorm and the input / output / shuffle passes
// (swinir.hip), the window attention, channel gate and branch sum of hat.hip, conv_last on rrdb_conv (rrdb.hip)
// ------------------------------------------------------------------------------------------------------------
// blob: fp32, in the order include/sdmi.h documents at sdmi_hat_config.
static bool hat_config_ok(const sdmi_hat_config& c, std::string* why) {
    auto fail = [&](const char* m) { if (why) *why = m; return false; };
    if (c.embed_dim < 1 || c.num_heads < 1 || c.embed_dim % c.num_heads) return fail("embed_dim must be a positive multiple of num_heads");
    if (c.num_heads * 32 < c.embed_dim) return fail("head dim = embed_dim / num_heads must be <= 32 (num_heads * 32 >= embed_dim)");
    if (c.embed_dim > 1024) return fail("embed_dim must be <= 1024 (the channel gate holds a row of means per workgroup)");
    if (const char* m = depths_wrong(c.num_layers, c.depths)) return fail(m);
    if (c.mlp_hidden < 1) return fail("mlp_hidden");
    if (c.cab_mid < 1 || c.cab_mid > 64) return fail("cab_mid in 1..64 (the conv branch's mid width is packed to 64 channels)");
    if (c.cab_squeeze < 1 || c.cab_squeeze > 128) return fail("cab_squeeze in 1..128");
    if (!std::isfinite(c.conv_scale)) return fail("conv_scale must be finite");
    if (c.scale != 2 && c.scale != 3 && c.scale != 4) return fail("scale 2 | 3 | 4");
    return true;
}

int64_t hat_blob_floats(const sdmi_hat_config* c) {
    if (!c || !hat_config_ok(*c, nullptr)) return 0;
    const int64_t C = c->embed_dim, Hd = c->mlp_hidden, mid = c->cab_mid, Cs = c->cab_squeeze, heads = c->num_heads, s2 = c->scale == 3 ? 9 : 4;
    const int64_t mlp = 2 * C + lin(Hd, C) + lin(C, Hd);
    const int64_t block = 2 * C + 961 * heads + lin(3 * C, C) + lin(C, C) + lin(mid, C, 9) + lin(C, mid, 9) + lin(Cs, C) + lin(C, Cs) + mlp;
    const int64_t overlap = 2 * C + lin(3 * C, C) + 1521 * heads + lin(C, C) + mlp;
    int64_t n = lin(C, 3, 9) + 2 * C;
    for (int i = 0; i < c->num_layers; ++i) n += c->depths[i] * block + overlap + lin(C, C, 9);
    return n + 2 * C + lin(C, C, 9) + lin(64, C, 9) + (c->scale == 4 ? 2 : 1) * lin(s2 * 64, 64, 9) + lin(3, 64, 9);
}

int hat_create(sdmi_engine* e, const float* blob, int64_t blob_floats, const sdmi_hat_config* cfg, sdmi_hat** out) {
    SDMI_REQUIRE(e && blob && cfg && out, "null argument");
    std::string why;
    SDMI_REQUIRE(hat_config_ok(*cfg, &why), "HAT config: " + why);
    SDMI_REQUIRE(blob_floats == hat_blob_floats(cfg), "weight blob size does not match the config");
    SDMI_CHECK_HIP(hipSetDevice(e->device));
    std::unique_ptr<sdmi_hat> holder(new sdmi_hat);
    sdmi_hat* net = holder.get();
    net->e = e; net->cfg = *cfg;
    const int C = cfg->embed_dim, heads = cfg->num_heads, D = C / heads, Hd = cfg->mlp_hidden, mid = cfg->cab_mid, Cs = cfg->cab_squeeze;
    const int Cp = rup(C, 64), hid_pad = rup(Hd, 64), ldq = rup(96 * heads, 64), lda = rup(32 * heads, 64), mid_pad = rup(mid, 64);
    net->C = C; net->Cp = Cp; net->D = D; net->ldq = ldq; net->lda = lda; net->hid_pad = hid_pad; net->mid_pad = mid_pad;
    BlobPacker bp{net, blob, blob + blob_floats};
    auto ident = BlobPacker::ident;
    auto slot = [&](int v) { return (v / D) * 32 + v % D; };            // feature h * D + d -> column h * 32 + d
    auto qkv = [&](sdmi_hat::Block& bk) { return bp.conv(&bk.qkv, 3 * C, C, 1, ldq, Cp, [&](int o) { return (o / C) * heads * 32 + slot(o % C); }); };
    auto proj = [&](sdmi_hat::Block& bk) { return bp.conv(&bk.proj, C, C, 1, Cp, lda, ident, slot); };
    auto mlp = [&](sdmi_hat::Block& bk) -> int {
        TRY(bp.norm(&bk.n2, C));
        TRY(bp.conv(&bk.fc1, Hd, C, 1, hid_pad, Cp));
        return bp.conv(&bk.fc2, C, Hd, 1, Cp, hid_pad);
    };

    TRY(bp.conv(&net->first, C, 3, 9, Cp, 64));
    TRY(bp.norm(&net->pe_norm, C));
    net->layers.resize((size_t)cfg->num_layers);
    for (int i = 0; i < cfg->num_layers; ++i) {
        sdmi_hat::Layer& L = net->layers[(size_t)i];
        L.blocks.resize((size_t)cfg->depths[i]);
        for (sdmi_hat::Block& bk : L.blocks) {
            TRY(bp.norm(&bk.n1, C));
            TRY(bp.raw(&bk.table, (size_t)961 * heads));
            TRY(qkv(bk));
            TRY(proj(bk));
            TRY(bp.conv(&bk.cab0, mid, C, 9, mid_pad, Cp));
            TRY(bp.conv(&bk.cab2, C, mid, 9, Cp, mid_pad));
            TRY(bp.mat(&bk.ca_w1, Cs, C, Cs, Cp));
            TRY(bp.raw(&bk.ca_b1, (size_t)Cs));
            TRY(bp.mat(&bk.ca_w3, C, Cs, Cp, Cs));
            TRY(bp.mat(&bk.ca_b3, 1, C, 1, Cp));
            TRY(mlp(bk));
        }
        sdmi_hat::Block& oc = L.overlap;
        TRY(bp.norm(&oc.n1, C));
        TRY(qkv(oc));
        TRY(bp.raw(&oc.table, (size_t)1521 * heads));
        TRY(proj(oc));
        TRY(mlp(oc));
        TRY(bp.conv(&L.conv, C, C, 9, Cp, Cp));
    }
    TRY(bp.norm(&net->norm, C));
    TRY(bp.conv(&net->after, C, C, 9, Cp, Cp));
    TRY(bp.ps_tail(&net->before, net->ps, &net->last, C, Cp, cfg->scale));
    TRY(bp.done());
    *out = holder.release();
    return 0;
}

// One pass over the network (dry: the arena layout alone).  M tokens = B * Hp * Wp on the grid reflect-padded to multiples of 16; every
// token tensor is Cp wide with zeros in columns C .. Cp - 1 (zero weight rows / bias entries and swin_layernorm keep them so; the channel
// gate's padded channels multiply a zero); the conv branch's mid tensor is mid_pad wide.
static int hat_pass(Run& r, const sdmi_hat& n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8) {
    const int Hp = rup(H, 16), Wp = rup(W, 16), sc = n.cfg.scale, Cp = n.Cp, heads = n.cfg.num_heads, N = Hp * Wp;
    const size_t M = (size_t)B * N;
    r.ar->reset();
    half_t* x0 = r.H(M * 64);                                 // the padded, mean-subtracted input
    half_t* feat = r.H(M * Cp);                               // conv_first's output: the trunk's skip tensor
    half_t* pool[4];                                          // token tensors: a group's input and the blocks' ping-pong
    for (half_t*& p : pool) p = r.H(M * Cp);
    half_t* ln = r.H(M * Cp);
    half_t* qkv = r.H(M * n.ldq);
    half_t* att = r.H(M * n.lda);
    half_t* hid = r.H(M * n.hid_pad);
    half_t* cm = r.H(M * n.mid_pad);                          // GELU(cab.0(norm1(t)))
    half_t* cv = r.H(M * Cp);                                 // cab.2 of it: what the gate pools and scales
    float* pool_ws = r.F((size_t)B * cdiv(N, HAT_POOL_TOKENS) * Cp);
    float* gate = r.F((size_t)B * Cp);
    half_t* c1 = r.H(M * 64);
    half_t* up[2] = {r.H(M * sc * sc * 64), r.H(M * sc * sc * 64)};      // the step convs' outputs and their shuffles, ping-pong
    float* full = r.F(M * sc * sc * 3);                       // conv_last on the padded grid, cropped by swin_output

    Grid g{r, B, Hp, Wp};
    auto attention = [&](const sdmi_hat::Block& bk, int mode, int shift) -> int {       // qkv -> att
        if (r.dry) return 0;
        HatAttnP a{};
        a.qkv = qkv; a.bias = bk.table; a.out = att; a.B = B; a.H = Hp; a.W = Wp; a.heads = heads; a.D = n.D; a.ldq = n.ldq; a.ldo = n.lda;
        a.mode = mode; a.shift = shift; a.scale = 1.0f / sqrtf((float)n.D);
        return launch_hat_window_attention(a, r.s);
    };
    // mid += conv_scale * cab(ln), ln = norm1 of the block's input on the unshifted grid
    auto conv_branch = [&](const sdmi_hat::Block& bk, half_t* mid) -> int {
        TRY(g.conv(bk.cab0, ln, nullptr, cm, EP_GELU));
        TRY(g.conv(bk.cab2, cm, nullptr, cv));
        if (r.dry) return 0;
        TRY(launch_hat_channel_gate(cv, bk.ca_w1, bk.ca_b1, bk.ca_w3, bk.ca_b3, pool_ws, gate, B, N, Cp, n.cfg.cab_squeeze, Cp, r.s));
        return launch_hat_cab_add(mid, cv, gate, mid, (long long)M, N, Cp, Cp, Cp, Cp, n.cfg.conv_scale, r.s);
    };

    if (!r.dry) {
        TRY(launch_swin_input(in, in_u8, x0, B, H, W, Hp, Wp, 64, r.s));
        if (n.lda > 32 * heads)                               // an odd head count: proj reads 32 columns the attention never writes (zero weights, but not NaN x 0)
            SDMI_CHECK_HIP(hipMemsetAsync(att, 0, M * n.lda * sizeof(half_t), r.s));
    }
    TRY(g.conv(n.first, x0, nullptr, feat));
    half_t* x = pool[0];
    std::vector<half_t*> free_ = {pool[1], pool[2], pool[3]};
    TRY(g.lnorm(n.pe_norm, feat, x, Cp));
    for (const sdmi_hat::Layer& L : n.layers) {
        half_t* cur = x;
        for (size_t j = 0; j <= L.blocks.size(); ++j) {       // the hybrid attention blocks, then the overlapping cross-attention block
            const bool overlap = j == L.blocks.size();
            const sdmi_hat::Block& bk = overlap ? L.overlap : L.blocks[j];
            half_t* mid = free_.back(); free_.pop_back();
            half_t* nxt = free_.back(); free_.pop_back();
            TRY(g.lnorm(bk.n1, cur, ln, Cp));
            TRY(g.conv(bk.qkv, ln, nullptr, qkv));
            TRY(attention(bk, overlap ? 1 : 0, !overlap && (j & 1) ? 8 : 0));
            TRY(g.conv(bk.proj, att, cur, mid));
            if (!overlap) TRY(conv_branch(bk, mid));
            TRY(g.lnorm(bk.n2, mid, ln, Cp));
            TRY(g.conv(bk.fc1, ln, nullptr, hid, EP_GELU));
            TRY(g.conv(bk.fc2, hid, mid, nxt));
            free_.push_back(mid);
            if (cur != x) free_.push_back(cur);
            cur = nxt;
        }
        half_t* y = free_.back(); free_.pop_back();
        TRY(g.conv(L.conv, cur, x, y));
        free_.push_back(x);
        if (cur != x) free_.push_back(cur);
        x = y;
    }
    TRY(g.lnorm(n.norm, x, ln, Cp));
    half_t* trunk = free_.back();
    TRY(g.conv(n.after, ln, feat, trunk));
    return pixelshuffle_tail(g, n.before, n.ps, n.last, sc, trunk, c1, up, full, out, out_u8, H, W);
}

static bool hat_size_ok(const sdmi_hat& n, int B, int H, int W) {
    if (B <= 0 || H < 9 || W < 9) return false;
    const long long M = (long long)B * rup(H, 16) * rup(W, 16);
    const long long widest = std::max<long long>({(long long)n.ldq, (long long)n.hid_pad, (long long)n.Cp, 64ll * n.cfg.scale * n.cfg.scale});
    return M * widest < (1ll << 31) - 256;
}

static int hat_size_check(const sdmi_hat* n, int B, int H, int W) {
    SDMI_REQUIRE(B > 0 && H >= 9 && W >= 9, "image sides must be at least 9 (a smaller side cannot be reflect-padded to a window of 16)");
    SDMI_REQUIRE(hat_size_ok(*n, B, H, W), "image too large: every intermediate tensor must stay below 2^31 elements");
    return 0;
}
int64_t hat_scratch_bytes(const sdmi_hat* n, int B, int H, int W) { return net_scratch_bytes(n, B, H, W, hat_size_ok, hat_pass); }
int hat_run(sdmi_hat* n, const void* in, int in_u8, int B, int H, int W, void* out, int out_u8, hipStream_t s) {
    return net_run(n, in, in_u8, B, H, W, out, out_u8, s, hat_size_check, hat_pass);
}

}  // namespace sdmi

sdmi_net::~sdmi_net() {
    for (void* p : owned) (void)hipFree(p);
}

// The host-emulated test build (plain C++ against a stand-in HIP runtime) compiles a fixed list of translation units, this file among
// them; there the upscalers' kernel files travel inside this one.  The GPU build compiles rrdb.hip, compact.hip, swinir.hip, scunet.hip,
// dat.hip and hat.hip on their own (build.sh).
#ifndef __HIP__
#include "rrdb.hip"
#include "compact.hip"
#include "swinir.hip"
#include "scunet.hip"
#include "dat.hip"
#include "hat.hip"
#endif
