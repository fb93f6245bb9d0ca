// Res2Net forward orchestrated natively (mvector/models/res2net.py:89-174).
//
// create(): reads the reference-layout fp32 state_dict; every eval-mode BatchNorm folds into the conv in front of it, channel counts padded to
// multiples of 16 and packed for conv2ds_kernel (make_s16_conv_bn, s16model.h).  A Bottle2neck block (res2net.py:53-86) keeps the
// width-sized channel groups that torch.split / torch.cat move around as fixed slices of two buffers (s16_grouped_map: slice i at i * wpad):
//   A  = relu(bn1(conv1(x)))   [.., scale * wpad] at the block's input size      slice i = spx[i]
//   Bc = the "cat" buffer      [.., scale * wpad] at the block's output size     slice i = relu(bns[i](convs[i](.))), i < nums
// A 3x3 conv (the block's stride) writes slice i of Bc; in a 'normal' block it also writes "its output + slice i + 1 of A" (sp + spx[i], res2net.py:65)
// as its second output, which the next 3x3 conv reads.  The last slice: a 'stage' block runs AvgPool2d(3, stride, 1) from A into Bc (avgpool3,
// res2net2d.hip), a 'normal' block passes it on untouched -- conv3 reads it from A through its concatenated input.  conv3 takes the residual (x, or
// the 1x1 strided downsample) in its epilogue and clamps to [0, inf).  The ReLU has no upper bound, so every launch that stores a map reports the
// largest value it wanted to store to the handle's peak word (S16Peak; MV_INFO_S16_*).
// Stem: conv7x7 stride 3 + bn1 + ReLU, MaxPool2d(3, 2, 1) (res2net2d.hip).  Head: S16Head (s16model.h) on the last map (x.reshape(B, -1, T'), res2net.py:167).
// forward(): a fixed sequence of launches on the caller's stream over the caller's workspace; no host synchronisation.
#include "s16model.h"

namespace mv {

namespace {

struct R2Block {
    S16Conv conv1, conv3, down;
    std::vector<S16Conv> convs;   // nums of them
    bool has_down = false, stage = false;
    int in_c = 0, out_c = 0, in_c16 = 0, out_c16 = 0, width = 0, wpad = 0, nums = 1, stride = 1;
};

}  // namespace

struct Res2NetModel : MvModelBase {
    static constexpr int EXPANSION = 4;   // Bottle2neck.expansion (res2net.py:11)
    MvRes2NetCfg cfg;
    int pool_type = MV_POOL_ASP, scale = 2, m = 0;
    float* stem_w = nullptr;  // [m][49] BN folded
    float* stem_b = nullptr;
    std::vector<R2Block> layers[4];
    S16Peak peak;
    S16Head head;
    int final_h = 0;

    static int stem(int n) { return (n - 5) / 3 + 1; }            // the 7x7 window with padding 1 at stride 3

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
        const std::vector<int> gmap = s16_grouped_map(width, scale, b->wpad);
        int rc;
        const char* who = "res2net";
        if ((rc = make_s16_conv_bn(this, w, who, p + ".conv1", p + ".bn1", width * scale, in_planes, 1, 1, gmap, scale * b->wpad, s16_dense_map(in_planes),
                                   b->in_c16, &b->conv1)))
            return rc;
        b->convs.resize(b->nums);
        for (int i = 0; i < b->nums; ++i)
            if ((rc = make_s16_conv_bn(this, w, who, p + ".convs." + std::to_string(i), p + ".bns." + std::to_string(i), width, width, 3, stride, &b->convs[i])))
                return rc;
        if ((rc = make_s16_conv_bn(this, w, who, p + ".conv3", p + ".bn3", b->out_c, width * scale, 1, 1, s16_dense_map(b->out_c), b->out_c16, gmap,
                                   scale * b->wpad, &b->conv3)))
            return rc;
        b->has_down = has_down;
        if (has_down) return make_s16_conv_bn(this, w, who, p + ".downsample.0", p + ".downsample.1", b->out_c, in_planes, 1, stride, &b->down);
        return MV_OK;
    }

    int create(const MvRes2NetCfg& c, const Weights& w) {
        cfg = c;
        MV_REQUIRE(c.scale >= 1 && c.scale <= 8, "res2net: scale must be 1..8");
        MV_REQUIRE(c.m_channels >= 8 && c.m_channels % 8 == 0, "res2net: m_channels must be a multiple of 8");
        MV_REQUIRE(c.m_channels <= 256, "res2net: m_channels must be at most 256 (the stem kernel's limit)");
        for (int i = 0; i < 4; ++i) MV_REQUIRE(c.layers[i] >= 1, "res2net: every stage needs a block (stage " + std::to_string(i + 1) + ")");
        MV_REQUIRE(c.embd_dim > 0 && c.base_width > 0, "res2net: embd_dim and base_width must be positive");
        MV_REQUIRE(c.input_size >= 5, "res2net: input_size must be at least 5 (the 7x7 stem with padding 1)");
        int rc;
        if ((rc = peak.create(this, c.pooling_type, "res2net", &pool_type))) return rc;
        // cat_channels = m * 8 * expansion * (input_size // base_width) (res2net.py:107) has to be what x.reshape(B, -1, T') finds
        int h = s16_down(stem(c.input_size));
        for (int l = 1; l < 4; ++l) h = s16_down(h);
        final_h = c.input_size / c.base_width;
        if (h != final_h)
            return fail(MV_ERR_INVALID_ARGUMENT, "res2net: input_size // base_width = " + std::to_string(final_h) + " differs from the frequency size " +
                                                     std::to_string(h) + " behind the four stages of input_size " + std::to_string(c.input_size) +
                                                     " (the reference's cat_channels does not fit its own forward)");
        m = c.m_channels;
        scale = c.scale;
        embd_dim = c.embd_dim;
        input_size = c.input_size;
        // conv1 + bn1 + relu (res2net.py:98-100, 157-159): fp32 weights for the VALU stem kernel
        if ((rc = fold_s16_stem(this, w, "res2net", m, 49, &stem_w, &stem_b))) return rc;
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
        return head.create(this, w, pool_type, in_planes, final_h, c.embd_dim);
    }

    int info(int key, float* value) const override {
        int rc;
        return peak.info(key, value, &rc) ? rc : MvModelBase::info(key, value);
    }

    // ---- workspace ---------------------------------------------------------------------------------------------
    struct Ws {
        float *ping[2], *a, *bc, *r, *t, *t2;   // maps: S16 form, 4 bytes per channel
        S16Head::Ws head;
        size_t bytes;
    };

    Ws carve(void* base, int B, int T) const {
        Carver cv(base);
        Ws s;
        const int m16 = (int)round_up(m, 16);
        int H = stem(cfg.input_size), W = stem(T);
        size_t max_io = (size_t)B * H * W * m16, max_a = 0, max_bc = 0, max_r = 0, max_t = 0;
        H = s16_down(H);
        W = s16_down(W);
        for (int l = 0; l < 4; ++l)
            for (const R2Block& k : layers[l]) {
                const int Ho = k.stride == 2 ? s16_down(H) : H, Wo = k.stride == 2 ? s16_down(W) : W;
                max_a = std::max(max_a, (size_t)B * H * W * scale * k.wpad);
                max_bc = std::max(max_bc, (size_t)B * Ho * Wo * scale * k.wpad);
                max_t = std::max(max_t, (size_t)B * Ho * Wo * k.wpad);
                max_r = std::max(max_r, (size_t)B * Ho * Wo * k.out_c16);
                max_io = std::max(max_io, (size_t)B * Ho * Wo * k.out_c16);
                H = Ho;
                W = Wo;
            }
        s.ping[0] = cv.take<float>(max_io + S16_SLACK);
        s.ping[1] = cv.take<float>(max_io + S16_SLACK);
        s.a = cv.take<float>(max_a + S16_SLACK);
        s.bc = cv.take<float>(max_bc + S16_SLACK);
        s.r = cv.take<float>(max_r + S16_SLACK);
        s.t = cv.take<float>(max_t + S16_SLACK);
        s.t2 = cv.take<float>(max_t + S16_SLACK);
        s.head = head.carve(cv, B, W);
        s.bytes = cv.total();
        return s;
    }

    int workspace_bytes(int B, int T, size_t* bytes) const override {
        MV_REQUIRE(B > 0 && T >= 5 && bytes != nullptr, "res2net workspace: needs B > 0 and at least 5 frames");
        *bytes = carve(nullptr, B, T).bytes;
        return MV_OK;
    }

    // ---- launches ----------------------------------------------------------------------------------------------
    int run_block(const R2Block& k, const float* x, float* y, const Ws& s, int B, int Hin, int Win, hipStream_t st) const {
        const float NEG = -3.0e38f, POS = 3.0e38f;
        const int Ho = k.stride == 2 ? s16_down(Hin) : Hin, Wo = k.stride == 2 ? s16_down(Win) : Win;
        const int64_t lda = (int64_t)scale * k.wpad;
        int rc;
        // out = relu(bn1(conv1(x))); spx = split(out, width)   (res2net.py:56-60)
        MvConv2dsDesc d = s16_conv_desc(k.conv1, x, k.in_c16, s.a, lda, B, Hin, Win);
        d.lo = 0.0f; d.hi = POS; d.peak = peak.word();
        if ((rc = conv2ds_launch(d, st))) return rc;
        float* const sums[2] = {s.t, s.t2};
        for (int i = 0; i < k.nums; ++i) {   // sp = relu(bns[i](convs[i](sp)))   (res2net.py:61-71)
            const float* spx = s.a + (int64_t)i * k.wpad;
            float* dst = s.bc + (int64_t)i * k.wpad;
            if (k.stage) {   // every conv reads its own slice
                d = s16_conv_desc(k.convs[i], spx, lda, dst, lda, B, Hin, Win);
            } else {         // sp + spx[i] was formed by the conv before as its second output; this one forms the next (stride 1: one size)
                d = s16_conv_desc(k.convs[i], i == 0 ? spx : sums[(i - 1) & 1], i == 0 ? lda : k.wpad, dst, lda, B, Hin, Win);
                if (i + 1 < k.nums) {
                    d.add = spx + k.wpad; d.ldadd = lda; d.y2 = sums[i & 1]; d.ldy2 = k.wpad;
                }
            }
            d.lo = 0.0f; d.hi = POS; d.peak = peak.word();
            if ((rc = conv2ds_launch(d, st))) return rc;
        }
        // relu(bn3(conv3(out)) + residual)   (res2net.py:77-84)
        MvConv2dsDesc d3 = s16_conv_desc(k.conv3, s.bc, lda, y, k.out_c16, B, Ho, Wo);
        if (scale != 1) {
            const int64_t last = (int64_t)k.nums * k.wpad;
            if (k.stage) {   // cat(out, pool(spx[nums]))   (res2net.py:74-75): layer1's stride is 1 and it still averages
                if ((rc = avgpool3_s16_launch(reinterpret_cast<const half_t*>(s.a + last), lda, reinterpret_cast<half_t*>(s.bc + last), lda, B, Hin, Win, k.width,
                                              k.stride, st)))
                    return rc;
            } else {         // cat(out, spx[nums])   (res2net.py:72-73): read where it is
                d3.x2 = s.a + last; d3.ldx2 = lda; d3.cin1 = (int)last;
            }
        }
        d3.res = x; d3.ldres = k.in_c16;
        if (k.has_down) {   // downsample(x) (res2net.py:80-81)
            d = s16_conv_desc(k.down, x, k.in_c16, s.r, k.out_c16, B, Hin, Win);
            d.lo = NEG; d.hi = POS; d.peak = peak.word();
            if ((rc = conv2ds_launch(d, st))) return rc;
            d3.res = s.r; d3.ldres = k.out_c16;
        }
        d3.lo = 0.0f; d3.hi = POS; d3.peak = peak.word();
        return conv2ds_launch(d3, st);
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
        if ((rc = conv2d_stem7_s16_launch(feats, reinterpret_cast<half_t*>(s.ping[0]), stem_w, stem_b, B, T, cfg.input_size, m, st, peak.word())) ||
            (rc = maxpool3s2_s16_launch(reinterpret_cast<const half_t*>(s.ping[0]), m16, reinterpret_cast<half_t*>(s.ping[1]), m16, B, H, W, m, st)))
            return rc;
        H = s16_down(H);
        W = s16_down(W);
        const float* cur = s.ping[1];
        int pp = 0;
        for (int l = 0; l < 4; ++l)
            for (const R2Block& k : layers[l]) {
                if ((rc = run_block(k, cur, s.ping[pp], s, B, H, W, st))) return rc;
                if (k.stride == 2) {
                    H = s16_down(H);
                    W = s16_down(W);
                }
                cur = s.ping[pp];
                pp ^= 1;
            }
        MV_REQUIRE(H == final_h, "res2net forward: unexpected frequency size after the four stages");
        // x.reshape(B, -1, T') -> pooling -> bn2 -> linear -> bn3   (res2net.py:167-172)
        return head.forward(s.head, cur, B, H, W, emb, st);
    }
};

}  // namespace mv

extern "C" {

int mv_res2net_create(const MvRes2NetCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out) {
    return mv::create_model<mv::Res2NetModel>("mv_res2net_create", cfg, tensors, num_tensors, out);
}

}  // extern "C"
