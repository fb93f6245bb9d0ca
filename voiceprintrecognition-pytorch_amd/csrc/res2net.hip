// Res2Net forward orchestrated natively (mvector/models/res2net.py:89-174).
//
// create(): reads the reference-layout fp32 state_dict, folds every eval-mode BatchNorm (eps 1e-5) into the conv in front of it, pads channel counts
// to multiples of 16 and packs the weights for conv2ds_kernel, as eres2net.hip and resnet_se.hip do.  A Bottle2neck block (res2net.py:53-86) keeps the
// width-sized channel groups that torch.split / torch.cat move around as fixed slices of two buffers (eres2net.hip's grouped_map: slice i at i * wpad):
//   A  = relu(bn1(conv1(x)))   [.., scale * wpad] at the block's input size      slice i = spx[i]
//   Bc = the "cat" buffer      [.., scale * wpad] at the block's output size     slice i = relu(bns[i](convs[i](.))), i < nums
// A 3x3 conv (the block's stride) writes slice i of Bc; in a 'normal' block it also writes "its output + slice i + 1 of A" (sp + spx[i], res2net.py:65)
// as its second output, which the next 3x3 conv reads.  The last slice: a 'stage' block runs AvgPool2d(3, stride, 1) from A into Bc (avgpool3,
// res2net2d.hip), a 'normal' block passes it on untouched -- conv3 reads it from A through its concatenated input.  conv3 takes the residual (x, or
// the 1x1 strided downsample) in its epilogue and clamps to [0, inf).  The ReLU has no upper bound, so every launch that stores a map reports the
// largest value it wanted to store to the handle's peak word (s16map.h; MV_INFO_S16_*).
// Stem: conv7x7 stride 3 + bn1 + ReLU, MaxPool2d(3, 2, 1) (res2net2d.hip).  Head: the last map as fp16 rows [B, T', C * H] (x.reshape(B, -1, T'),
// res2net.py:167) -> Pooling (model.h) -> bn2 . linear . bn3 folded.
// forward(): a fixed sequence of launches on the caller's stream over the caller's workspace; no host synchronisation.
#include <memory>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "s16map.h"

namespace mv {

namespace {

struct R2Conv {
    half_t* w = nullptr;   // split-packed (conv2ds_pack_host)
    float* bias = nullptr;
    float oscale = 0.0f;
    int cin16 = 0, cout16 = 0, ks = 1, stride = 1;
    int cin = 0, cout = 0;
};

struct R2Block {
    R2Conv conv1, conv3, down;
    std::vector<R2Conv> convs;   // nums of them
    bool has_down = false, stage = false;
    int in_c = 0, out_c = 0, in_c16 = 0, out_c16 = 0, width = 0, wpad = 0, nums = 1, stride = 1;
};

struct R2Extra {   // what only some of the launches have
    const float* x2 = nullptr;   // the channels behind cin1 come from here
    int64_t ldx2 = 0;
    int cin1 = 0;
    const float* res = nullptr;
    int64_t ldres = 0;
    const float* add = nullptr;  // second output y2 = y + add
    int64_t ldadd = 0;
    float* y2 = nullptr;
    int64_t ldy2 = 0;
};

std::vector<int> r2_dense(int c) {
    std::vector<int> m(c);
    for (int i = 0; i < c; ++i) m[i] = i;
    return m;
}

// channel c of a [scale * width] tensor lives at (c / width) * wpad + c % width
std::vector<int> r2_grouped(int width, int scale, int wpad) {
    std::vector<int> m((size_t)width * scale);
    for (int c = 0; c < width * scale; ++c) m[c] = (c / width) * wpad + c % width;
    return m;
}

}  // namespace

struct Res2NetModel : MvModelBase {
    static constexpr int EXPANSION = 4;   // Bottle2neck.expansion (res2net.py:11)
    MvRes2NetCfg cfg;
    int pool_type = MV_POOL_ASP, scale = 2, m = 0;
    float* stem_w = nullptr;  // [m][49] BN folded
    float* stem_b = nullptr;
    std::vector<R2Block> layers[4];
    Pooling pool;
    float* fc_w = nullptr;
    float* fc_b = nullptr;
    unsigned* d_peak = nullptr;   // device word: largest |64 * value| a launch wanted to store (float bits; sticky, diagnostic only); null: MV_RES2NET_NO_PEAK
    int final_c = 0, final_h = 0;

    static int down(int n) { return (n - 1) / 2 + 1; }            // a 3x3 window with padding 1, or a 1x1 one, at stride 2
    static int stem(int n) { return (n - 5) / 3 + 1; }            // the 7x7 window with padding 1 at stride 3

    // conv (no bias) [cout][cin][ks][ks] followed by BatchNorm `bn`; out channel c -> row out_pos[c], in channel c -> column in_pos[c], zeros elsewhere
    int make_conv_bn(const Weights& w, const std::string& conv, const std::string& bn, int cout, int cin, int ks, int stride, const std::vector<int>& out_pos,
                     int cout16, const std::vector<int>& in_pos, int cin16, R2Conv* L) {
        std::vector<float> W, s, t;
        int rc;
        if ((rc = w.host(conv + ".weight", (int64_t)cout * cin * ks * ks, W)) || (rc = fold_bn(w, bn, cout, s, t, 1e-5f))) return rc;
        const int taps = ks * ks;
        std::vector<float> packed((size_t)cout16 * taps * cin16, 0.0f), bias((size_t)cout16, 0.0f);
        for (int co = 0; co < cout; ++co) {
            bias[out_pos[co]] = t[co];
            for (int ci = 0; ci < cin; ++ci)
                for (int tp = 0; tp < taps; ++tp)
                    packed[((size_t)out_pos[co] * taps + tp) * cin16 + in_pos[ci]] = W[((size_t)co * cin + ci) * taps + tp] * s[co];
        }
        std::vector<half_t> split((size_t)conv2ds_packed_floats(cout16, cin16, ks) * 2);
        L->oscale = conv2ds_pack_host(packed.data(), cout16, cin16, ks, split.data());
        L->w = static_cast<half_t*>(dev_alloc(split.size() * sizeof(half_t)));
        L->bias = upload(bias);
        if (L->w == nullptr || L->bias == nullptr) return fail(MV_ERR_HIP, "res2net create: out of device memory");
        MV_HIP_OK(hipMemcpy(L->w, split.data(), split.size() * sizeof(half_t), hipMemcpyHostToDevice));
        L->cin16 = cin16;
        L->cout16 = cout16;
        L->cin = cin;
        L->cout = cout;
        L->ks = ks;
        L->stride = stride;
        return MV_OK;
    }

    int make_block(const Weights& w, const std::string& p, int in_planes, int planes, int stride, bool stage, bool has_down, R2Block* b) {
        const int width = (int)((double)planes * ((double)cfg.base_width / 64.0));   // floor (res2net.py:26)
        MV_REQUIRE(width >= 4, "res2net: block width floor(planes * base_width / 64) below 4 in " + p);
        b->width = width;
        b->wpad = (int)round_up(width, 16);
        b->nums = scale == 1 ? 1 : scale - 1;   // res2net.py:30-33
        b->stride = stride;
        b->stage = stage;
        b->in_c = in_planes;
        b->out_c = planes * EXPANSION;
        b->in_c16 = (int)round_up(b->in_c, 16);
        b->out_c16 = (int)round_up(b->out_c, 16);
        const std::vector<int> gmap = r2_grouped(width, scale, b->wpad);
        int rc;
        if ((rc = make_conv_bn(w, p + ".conv1", p + ".bn1", width * scale, in_planes, 1, 1, gmap, scale * b->wpad, r2_dense(in_planes), b->in_c16, &b->conv1)))
            return rc;
        b->convs.resize(b->nums);
        for (int i = 0; i < b->nums; ++i)
            if ((rc = make_conv_bn(w, p + ".convs." + std::to_string(i), p + ".bns." + std::to_string(i), width, width, 3, stride, r2_dense(width), b->wpad,
                                   r2_dense(width), b->wpad, &b->convs[i])))
                return rc;
        if ((rc = make_conv_bn(w, p + ".conv3", p + ".bn3", b->out_c, width * scale, 1, 1, r2_dense(b->out_c), b->out_c16, gmap, scale * b->wpad, &b->conv3)))
            return rc;
        b->has_down = has_down;
        if (has_down)
            return make_conv_bn(w, p + ".downsample.0", p + ".downsample.1", b->out_c, in_planes, 1, stride, r2_dense(b->out_c), b->out_c16, r2_dense(in_planes),
                                b->in_c16, &b->down);
        return MV_OK;
    }

    int create(const MvRes2NetCfg& c, const Weights& w) {
        cfg = c;
        const bool track = c.pooling_type < 0 || (c.pooling_type & MV_RES2NET_NO_PEAK) == 0;
        pool_type = c.pooling_type < 0 ? c.pooling_type : c.pooling_type & ~MV_RES2NET_NO_PEAK;
        MV_REQUIRE(c.scale >= 1 && c.scale <= 8, "res2net: scale must be 1..8");
        MV_REQUIRE(c.m_channels >= 8 && c.m_channels % 8 == 0, "res2net: m_channels must be a multiple of 8");
        MV_REQUIRE(c.m_channels <= 256, "res2net: m_channels must be at most 256 (the stem kernel's limit)");
        for (int i = 0; i < 4; ++i) MV_REQUIRE(c.layers[i] >= 1, "res2net: every stage needs a block (stage " + std::to_string(i + 1) + ")");
        MV_REQUIRE(c.embd_dim > 0 && c.base_width > 0, "res2net: embd_dim and base_width must be positive");
        MV_REQUIRE(c.input_size >= 5, "res2net: input_size must be at least 5 (the 7x7 stem with padding 1)");
        if (pool_type < MV_POOL_ASP || pool_type > MV_POOL_TSP)
            return fail(MV_ERR_INVALID_ARGUMENT, "res2net: pooling_type " + std::to_string(pool_type) +
                                                     " is not MV_POOL_ASP (0), MV_POOL_SAP (1), MV_POOL_TAP (2) or MV_POOL_TSP (3)");
        // cat_channels = m * 8 * expansion * (input_size // base_width) (res2net.py:107) has to be what x.reshape(B, -1, T') finds
        int h = down(stem(c.input_size));
        for (int l = 1; l < 4; ++l) h = down(h);
        final_h = c.input_size / c.base_width;
        if (h != final_h)
            return fail(MV_ERR_INVALID_ARGUMENT, "res2net: input_size // base_width = " + std::to_string(final_h) + " differs from the frequency size " +
                                                     std::to_string(h) + " behind the four stages of input_size " + std::to_string(c.input_size) +
                                                     " (the reference's cat_channels does not fit its own forward)");
        m = c.m_channels;
        scale = c.scale;
        embd_dim = c.embd_dim;
        input_size = c.input_size;
        int rc;
        {   // conv1 + bn1 + relu (res2net.py:98-100, 157-159): fp32 weights for the VALU stem kernel
            std::vector<float> W, s, t;
            if ((rc = w.host("conv1.weight", (int64_t)m * 49, W)) || (rc = fold_bn(w, "bn1", m, s, t, 1e-5f))) return rc;
            for (int co = 0; co < m; ++co)
                for (int j = 0; j < 49; ++j) W[(size_t)co * 49 + j] *= s[co];
            stem_w = upload(W);
            stem_b = upload(t);
            if (stem_w == nullptr || stem_b == nullptr) return fail(MV_ERR_HIP, "res2net create: upload failed");
        }
        int in_planes = m;
        for (int l = 0; l < 4; ++l) {   // _make_layer (res2net.py:138-152): the first block of a stage is the 'stage' block and carries the downsample
            const int planes = m << l, stride = l == 0 ? 1 : 2;
            layers[l].resize(c.layers[l]);
            for (int j = 0; j < c.layers[l]; ++j) {
                const bool first = j == 0;
                if ((rc = make_block(w, "layer" + std::to_string(l + 1) + "." + std::to_string(j), in_planes, planes, first ? stride : 1, first,
                                     first && (stride != 1 || in_planes != planes * EXPANSION), &layers[l][j])))
                    return rc;
                in_planes = planes * EXPANSION;
            }
        }
        final_c = in_planes;
        if ((rc = pool.create(this, w, "pooling", pool_type, final_c * final_h, 128, true))) return rc;
        if ((rc = fold_final_linear(this, w, "linear.weight", "linear.bias", "bn2", "bn3", c.embd_dim, pool.width(), &fc_w, &fc_b))) return rc;
        if (track) {
            d_peak = static_cast<unsigned*>(dev_alloc(sizeof(unsigned)));
            if (d_peak == nullptr) return fail(MV_ERR_HIP, "res2net create: out of device memory");
            MV_HIP_OK(hipMemset(d_peak, 0, sizeof(unsigned)));
        }
        MV_HIP_OK(hipDeviceSynchronize());   // (the pooling head packs its weights on the device from temporaries of this call)
        return MV_OK;
    }

    int info(int key, float* value) const override {
        if (key == MV_INFO_S16_PEAK || key == MV_INFO_S16_SATURATED) {   // (waits for the device: a diagnostic, not a hot-path call)
            if (d_peak == nullptr) {
                *value = -1.0f;
                return MV_OK;
            }
            unsigned bits = 0;
            MV_HIP_OK(hipDeviceSynchronize());
            MV_HIP_OK(hipMemcpy(&bits, d_peak, sizeof(bits), hipMemcpyDeviceToHost));
            const float v = __builtin_bit_cast(float, bits);
            *value = key == MV_INFO_S16_PEAK ? v / CS_XSCALE : (v >= 65504.0f ? 1.0f : 0.0f);
            return MV_OK;
        }
        return MvModelBase::info(key, value);
    }

    // ---- workspace ---------------------------------------------------------------------------------------------
    struct Ws {
        float *ping[2], *a, *bc, *r, *t, *t2;   // maps: S16 form, 4 bytes per channel
        float *pooled, *asp_f, *lin_ws;
        half_t *rows, *h;
        size_t bytes, lin_ws_floats;
    };

    Ws carve(void* base, int B, int T) const {
        Carver cv(base);
        Ws s;
        const int m16 = (int)round_up(m, 16);
        int H = stem(cfg.input_size), W = stem(T);
        size_t max_io = (size_t)B * H * W * m16, max_a = 0, max_bc = 0, max_r = 0, max_t = 0;
        H = down(H);
        W = down(W);
        for (int l = 0; l < 4; ++l)
            for (const R2Block& k : layers[l]) {
                const int Ho = k.stride == 2 ? down(H) : H, Wo = k.stride == 2 ? down(W) : W;
                max_a = std::max(max_a, (size_t)B * H * W * scale * k.wpad);
                max_bc = std::max(max_bc, (size_t)B * Ho * Wo * scale * k.wpad);
                max_t = std::max(max_t, (size_t)B * Ho * Wo * k.wpad);
                max_r = std::max(max_r, (size_t)B * Ho * Wo * k.out_c16);
                max_io = std::max(max_io, (size_t)B * Ho * Wo * k.out_c16);
                H = Ho;
                W = Wo;
            }
        const size_t slack = 64;  // the conv loader reads whole 16-byte chunks
        s.ping[0] = cv.take<float>(max_io + slack);
        s.ping[1] = cv.take<float>(max_io + slack);
        s.a = cv.take<float>(max_a + slack);
        s.bc = cv.take<float>(max_bc + slack);
        s.r = cv.take<float>(max_r + slack);
        s.t = cv.take<float>(max_t + slack);
        s.t2 = cv.take<float>(max_t + slack);
        const int Cp = final_c * final_h;   // a multiple of 8 (final_c is one of 256)
        s.rows = cv.take<half_t>((size_t)B * W * Cp);
        s.h = cv.take<half_t>((size_t)B * W * pool.hidden_width());
        s.asp_f = cv.take<float>(pool.workspace_floats(B, W));
        s.pooled = cv.take<float>((size_t)B * pool.width());
        s.lin_ws_floats = linear_f32_splitk_floats(B, pool.width(), cfg.embd_dim);
        s.lin_ws = cv.take<float>(s.lin_ws_floats);
        s.bytes = cv.total();
        return s;
    }

    int workspace_bytes(int B, int T, size_t* bytes) const override {
        MV_REQUIRE(B > 0 && T >= 5 && bytes != nullptr, "res2net workspace: needs B > 0 and at least 5 frames");
        *bytes = carve(nullptr, B, T).bytes;
        return MV_OK;
    }

    // ---- launches ----------------------------------------------------------------------------------------------
    int conv(const R2Conv& L, const float* x, int64_t ldx, float* y, int64_t ldy, int B, int H, int W, float lo, hipStream_t st, const R2Extra& e = R2Extra()) const {
        MvConv2dsDesc d{};
        d.x = x; d.ldx = ldx; d.x2 = e.x2; d.ldx2 = e.ldx2; d.cin1 = e.cin1;
        d.w = L.w; d.bias = L.bias; d.oscale = L.oscale;
        d.res = e.res; d.ldres = e.ldres; d.add = e.add; d.ldadd = e.ldadd; d.y2 = e.y2; d.ldy2 = e.ldy2;
        d.y = y; d.ldy = ldy; d.B = B; d.H = H; d.W = W; d.cin16 = L.cin16; d.cout16 = L.cout16; d.ks = L.ks; d.stride = L.stride;
        d.epi = MV_EPI_CLAMP; d.lo = lo; d.hi = 3.0e38f;
        d.cin_alg = L.cin; d.cout_alg = L.cout;
        d.peak = d_peak;
        return conv2ds_launch(d, st);
    }

    int run_block(const R2Block& k, const float* x, float* y, const Ws& s, int B, int Hin, int Win, hipStream_t st) const {
        const float NEG = -3.0e38f;
        const int Ho = k.stride == 2 ? down(Hin) : Hin, Wo = k.stride == 2 ? down(Win) : Win;
        const int64_t lda = (int64_t)scale * k.wpad;
        int rc;
        // out = relu(bn1(conv1(x))); spx = split(out, width)   (res2net.py:56-60)
        if ((rc = conv(k.conv1, x, k.in_c16, s.a, lda, B, Hin, Win, 0.0f, st))) return rc;
        float* const sums[2] = {s.t, s.t2};
        for (int i = 0; i < k.nums; ++i) {   // sp = relu(bns[i](convs[i](sp)))   (res2net.py:61-71)
            const float* spx = s.a + (int64_t)i * k.wpad;
            float* dst = s.bc + (int64_t)i * k.wpad;
            if (k.stage) {   // every conv reads its own slice
                rc = conv(k.convs[i], spx, lda, dst, lda, B, Hin, Win, 0.0f, st);
            } else {         // sp + spx[i] was formed by the conv before as its second output; this one forms the next (stride 1: one size)
                R2Extra e;
                if (i + 1 < k.nums) {
                    e.add = spx + k.wpad;
                    e.ldadd = lda;
                    e.y2 = sums[i & 1];
                    e.ldy2 = k.wpad;
                }
                rc = conv(k.convs[i], i == 0 ? spx : sums[(i - 1) & 1], i == 0 ? lda : k.wpad, dst, lda, B, Hin, Win, 0.0f, st, e);
            }
            if (rc != MV_OK) return rc;
        }
        R2Extra e3;
        if (scale != 1) {
            const int64_t last = (int64_t)k.nums * k.wpad;
            if (k.stage) {   // cat(out, pool(spx[nums]))   (res2net.py:74-75): layer1's stride is 1 and it still averages
                if ((rc = avgpool3_s16_launch(reinterpret_cast<const half_t*>(s.a + last), lda, reinterpret_cast<half_t*>(s.bc + last), lda, B, Hin, Win, k.width,
                                              k.stride, st)))
                    return rc;
            } else {         // cat(out, spx[nums])   (res2net.py:72-73): read where it is
                e3.x2 = s.a + last;
                e3.ldx2 = lda;
                e3.cin1 = (int)last;
            }
        }
        e3.res = x;
        e3.ldres = k.in_c16;
        if (k.has_down) {   // downsample(x) (res2net.py:80-81)
            if ((rc = conv(k.down, x, k.in_c16, s.r, k.out_c16, B, Hin, Win, NEG, st))) return rc;
            e3.res = s.r;
            e3.ldres = k.out_c16;
        }
        // relu(bn3(conv3(out)) + residual)   (res2net.py:77-84)
        return conv(k.conv3, s.bc, lda, y, k.out_c16, B, Ho, Wo, 0.0f, st, e3);
    }

    int forward(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st) const override {
        MV_REQUIRE(feats != nullptr && emb != nullptr && ws != nullptr, "res2net forward: null buffer");
        MV_REQUIRE(B > 0 && T >= 5, "res2net forward: needs at least 5 frames (the 7x7 stem with padding 1)");
        const Ws s = carve(ws, B, T);
        if (s.bytes > ws_bytes) return fail(MV_ERR_WORKSPACE, "res2net forward: workspace too small");
        int rc;
        const int m16 = (int)round_up(m, 16);
        int H = stem(cfg.input_size), W = stem(T);
        // x.transpose(2, 1).unsqueeze(1) -> relu(bn1(conv1(x))) -> max_pool   (res2net.py:155-160)
        if ((rc = conv2d_stem7_s16_launch(feats, reinterpret_cast<half_t*>(s.ping[0]), stem_w, stem_b, B, T, cfg.input_size, m, st, d_peak)) ||
            (rc = maxpool3s2_s16_launch(reinterpret_cast<const half_t*>(s.ping[0]), m16, reinterpret_cast<half_t*>(s.ping[1]), m16, B, H, W, m, st)))
            return rc;
        H = down(H);
        W = down(W);
        const float* cur = s.ping[1];
        int pp = 0;
        for (int l = 0; l < 4; ++l)
            for (const R2Block& k : layers[l]) {
                if ((rc = run_block(k, cur, s.ping[pp], s, B, H, W, st))) return rc;
                if (k.stride == 2) {
                    H = down(H);
                    W = down(W);
                }
                cur = s.ping[pp];
                pp ^= 1;
            }
        MV_REQUIRE(H == final_h, "res2net forward: unexpected frequency size after the four stages");
        // x.reshape(B, -1, T') -> pooling -> bn2 -> linear -> bn3   (res2net.py:167-172)
        const int Cp = final_c * final_h;
        if ((rc = s16_map_to_rows_launch(reinterpret_cast<const half_t*>(cur), (int64_t)round_up(final_c, 16), B, H, W, final_c, s.rows, Cp, st)) ||
            (rc = pool.forward(s.rows, Cp, B, W, s.h, s.asp_f, s.pooled, st)))
            return rc;
        const int P = pool.width();
        return linear_f32_launch(s.pooled, P, fc_w, P, fc_b, MV_ACT_NONE, emb, cfg.embd_dim, B, P, cfg.embd_dim, 0, st, s.lin_ws, s.lin_ws_floats);
    }
};

}  // namespace mv

extern "C" {

int mv_res2net_create(const MvRes2NetCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out) {
    MV_REQUIRE(cfg != nullptr && out != nullptr, "mv_res2net_create: null argument");
    mv::Weights w;
    int rc = w.init(tensors, num_tensors);
    if (rc != MV_OK) return rc;
    auto m = std::make_unique<mv::Res2NetModel>();
    rc = m->create(*cfg, w);
    if (rc != MV_OK) return rc;
    *out = reinterpret_cast<MvModel*>(static_cast<mv::MvModelBase*>(m.release()));
    return MV_OK;
}

}  // extern "C"
