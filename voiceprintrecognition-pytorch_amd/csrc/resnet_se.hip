// ResNetSE forward orchestrated natively (mvector/models/resnet_se.py:65-145).
//
// create(): reads the reference-layout fp32 state_dict; every eval-mode BatchNorm folds into the conv in front of it (BN follows each conv directly:
// resnet_se.py:26-35, 114-118), channel counts padded to multiples of 16 and packed for conv2ds_kernel (make_s16_conv_bn, s16model.h).
// A bottleneck block is   conv1 1x1 + ReLU -> conv2 3x3 (stride) + ReLU -> conv3 1x1 -> SE gate -> + residual -> ReLU   (resnet_se.py:23-44):
// three (four with a downsample) conv2ds launches and the three passes of se2d.hip.  The ReLU has no upper bound, so every launch that stores a map
// reports the largest value it wanted to store to the handle's peak word (S16Peak; MV_INFO_S16_*).
// Head: S16Head (s16model.h) on the last map (x.reshape(B, -1, T'), resnet_se.py:139).
// forward(): a fixed sequence of launches on the caller's stream over the caller's workspace; no host synchronisation.
#include "s16model.h"

namespace mv {

namespace {

struct SeBlock {
    S16Conv conv1, conv2, conv3, down;
    bool has_down = false;
    float *fc1_w = nullptr, *fc1_b = nullptr, *fc2_w = nullptr, *fc2_b = nullptr;   // SELayer.fc.0 [R, C], fc.2 [C, R]
    int in_c = 0, planes = 0, out_c = 0, hidden = 0, stride = 1;
    int in_c16 = 0, planes16 = 0, out_c16 = 0;
};

}  // namespace

struct ResNetSeModel : MvModelBase {
    MvResNetSeCfg cfg;
    int pool_type = MV_POOL_ASP;
    float* stem_w = nullptr;  // [nf0][9] BN folded
    float* stem_b = nullptr;
    std::vector<SeBlock> layers[4];
    S16Peak peak;
    S16Head head;
    int final_h = 0;

    int make_block(const Weights& w, const std::string& p, int in_planes, int planes, int stride, SeBlock* b) {
        b->in_c = in_planes;
        b->planes = planes;
        b->out_c = 2 * planes;   // SEBottleneck.expansion (resnet_se.py:8)
        b->hidden = b->out_c / cfg.reduction;
        b->stride = stride;
        b->in_c16 = (int)round_up(b->in_c, 16);
        b->planes16 = (int)round_up(planes, 16);
        b->out_c16 = (int)round_up(b->out_c, 16);
        MV_REQUIRE(b->hidden >= 1, "resnet_se: the reduction leaves the SE layer of " + p + " without a hidden unit");
        int rc;
        if ((rc = make_s16_conv_bn(this, w, "resnet_se", p + ".conv1", p + ".bn1", planes, in_planes, 1, 1, &b->conv1)) ||
            (rc = make_s16_conv_bn(this, w, "resnet_se", p + ".conv2", p + ".bn2", planes, planes, 3, stride, &b->conv2)) ||
            (rc = make_s16_conv_bn(this, w, "resnet_se", p + ".conv3", p + ".bn3", b->out_c, planes, 1, 1, &b->conv3)))
            return rc;
        std::vector<float> v;
        if ((rc = w.host(p + ".se.fc.0.weight", (int64_t)b->hidden * b->out_c, v))) return rc;
        b->fc1_w = upload(v);
        if ((rc = w.host(p + ".se.fc.0.bias", b->hidden, v))) return rc;
        b->fc1_b = upload(v);
        if ((rc = w.host(p + ".se.fc.2.weight", (int64_t)b->out_c * b->hidden, v))) return rc;
        b->fc2_w = upload(v);
        if ((rc = w.host(p + ".se.fc.2.bias", b->out_c, v))) return rc;
        b->fc2_b = upload(v);
        if (b->fc1_w == nullptr || b->fc1_b == nullptr || b->fc2_w == nullptr || b->fc2_b == nullptr)
            return fail(MV_ERR_HIP, "resnet_se create: out of device memory");
        b->has_down = stride != 1 || in_planes != b->out_c;   // resnet_se.py:113
        if (b->has_down) return make_s16_conv_bn(this, w, "resnet_se", p + ".downsample.0", p + ".downsample.1", b->out_c, in_planes, 1, stride, &b->down);
        return MV_OK;
    }

    int create(const MvResNetSeCfg& c, const Weights& w) {
        cfg = c;
        MV_REQUIRE(c.input_size >= 8 && c.input_size % 8 == 0, "resnet_se: input_size must be a multiple of 8");
        for (int i = 0; i < 4; ++i) {
            MV_REQUIRE(c.num_filters[i] >= 16 && c.num_filters[i] % 16 == 0 && c.num_filters[i] <= 512,
                       "resnet_se: num_filters must be multiples of 16, at most 512 (entry " + std::to_string(i) + ")");
            MV_REQUIRE(c.layers[i] >= 1, "resnet_se: every stage needs a block (stage " + std::to_string(i + 1) + ")");
        }
        MV_REQUIRE(c.embd_dim > 0 && c.reduction >= 1, "resnet_se: embd_dim and reduction must be positive");
        int rc;
        if ((rc = peak.create(this, c.pooling_type, "resnet_se", &pool_type))) return rc;
        embd_dim = c.embd_dim;
        input_size = c.input_size;
        // conv1 + bn1 + relu (resnet_se.py:71-73, 130-132): fp32 weights for the VALU stem kernel
        if ((rc = fold_s16_stem(this, w, "resnet_se", c.num_filters[0], 9, &stem_w, &stem_b))) return rc;
        int in_planes = c.num_filters[0];
        for (int l = 0; l < 4; ++l) {
            const int planes = c.num_filters[l];
            layers[l].resize(c.layers[l]);
            for (int j = 0; j < c.layers[l]; ++j) {
                const int stride = (j == 0 && l > 0) ? 2 : 1;
                if ((rc = make_block(w, "layer" + std::to_string(l + 1) + "." + std::to_string(j), in_planes, planes, stride, &layers[l][j])))
                    return rc;
                in_planes = 2 * planes;
            }
        }
        final_h = c.input_size / 8;
        return head.create(this, w, pool_type, in_planes, final_h, c.embd_dim);
    }

    int info(int key, float* value) const override {
        int rc;
        return peak.info(key, value, &rc) ? rc : MvModelBase::info(key, value);
    }

    // ---- workspace ---------------------------------------------------------------------------------------------
    struct Ws {
        float *ping[2], *a, *b, *c, *r;   // maps: S16 form, 4 bytes per channel
        float *sq, *gate, *sq_ws;
        S16Head::Ws head;
        size_t bytes, sq_ws_floats;
    };

    Ws carve(void* base, int B, int T) const {
        Carver cv(base);
        Ws s;
        size_t max_io = 0, max_a = 0, max_b = 0, max_c = 0, max_sq = 0;
        int H = cfg.input_size, W = T, maxc = 0;
        max_io = (size_t)B * H * W * (size_t)round_up(cfg.num_filters[0], 16);
        for (int l = 0; l < 4; ++l)
            for (const SeBlock& k : layers[l]) {
                const int Ho = k.stride == 2 ? s16_down(H) : H, Wo = k.stride == 2 ? s16_down(W) : W;
                max_a = std::max(max_a, (size_t)B * H * W * k.planes16);
                max_b = std::max(max_b, (size_t)B * Ho * Wo * k.planes16);
                max_c = std::max(max_c, (size_t)B * Ho * Wo * k.out_c16);
                max_io = std::max(max_io, (size_t)B * Ho * Wo * k.out_c16);
                max_sq = std::max(max_sq, se2d_squeeze_ws_floats(B, Ho, Wo, k.out_c));
                maxc = std::max(maxc, k.out_c);
                H = Ho;
                W = Wo;
            }
        s.ping[0] = cv.take<float>(max_io + S16_SLACK);
        s.ping[1] = cv.take<float>(max_io + S16_SLACK);
        s.a = cv.take<float>(max_a + S16_SLACK);
        s.b = cv.take<float>(max_b + S16_SLACK);
        s.c = cv.take<float>(max_c + S16_SLACK);
        s.r = cv.take<float>(max_c + S16_SLACK);
        s.sq = cv.take<float>((size_t)B * maxc);
        s.gate = cv.take<float>((size_t)B * maxc);
        s.sq_ws_floats = max_sq;
        s.sq_ws = cv.take<float>(max_sq);
        s.head = head.carve(cv, B, W);
        s.bytes = cv.total();
        return s;
    }

    int workspace_bytes(int B, int T, size_t* bytes) const override {
        MV_REQUIRE(B > 0 && T >= 9 && bytes != nullptr, "resnet_se workspace: needs B > 0 and at least 9 frames");
        *bytes = carve(nullptr, B, T).bytes;
        return MV_OK;
    }

    // ---- launches ----------------------------------------------------------------------------------------------
    int run_block(const SeBlock& k, const float* x, float* y, const Ws& s, int B, int Hin, int Win, hipStream_t st) const {
        const float NEG = -3.0e38f, POS = 3.0e38f;
        const int Ho = k.stride == 2 ? s16_down(Hin) : Hin, Wo = k.stride == 2 ? s16_down(Win) : Win;
        int rc;
        // relu(bn1(conv1(x))), relu(bn2(conv2(.))), bn3(conv3(.))   (resnet_se.py:26-35)
        MvConv2dsDesc d = s16_conv_desc(k.conv1, x, k.in_c16, s.a, k.planes16, B, Hin, Win);
        d.lo = 0.0f; d.hi = POS; d.peak = peak.word();
        if ((rc = conv2ds_launch(d, st))) return rc;
        d = s16_conv_desc(k.conv2, s.a, k.planes16, s.b, k.planes16, B, Hin, Win);
        d.lo = 0.0f; d.hi = POS; d.peak = peak.word();
        if ((rc = conv2ds_launch(d, st))) return rc;
        d = s16_conv_desc(k.conv3, s.b, k.planes16, s.c, k.out_c16, B, Ho, Wo);
        d.lo = NEG; d.hi = POS; d.peak = peak.word();
        if ((rc = conv2ds_launch(d, st))) return rc;
        // SELayer (resnet_se.py:58-62): y = fc(avg_pool(out))
        const half_t* c16 = reinterpret_cast<const half_t*>(s.c);
        if ((rc = se2d_squeeze_launch(c16, k.out_c16, B, Ho, Wo, k.out_c, s.sq, s.sq_ws, s.sq_ws_floats, st)) ||
            (rc = se2d_excite_launch(s.sq, k.fc1_w, k.fc1_b, k.fc2_w, k.fc2_b, s.gate, B, k.out_c, k.hidden, st)))
            return rc;
        const float* resid = x;
        int64_t ldr = k.in_c16;
        if (k.has_down) {   // downsample(x) (resnet_se.py:38-39)
            d = s16_conv_desc(k.down, x, k.in_c16, s.r, k.out_c16, B, Hin, Win);
            d.lo = NEG; d.hi = POS; d.peak = peak.word();
            if ((rc = conv2ds_launch(d, st))) return rc;
            resid = s.r;
            ldr = k.out_c16;
        }
        // relu(out * y + residual)   (resnet_se.py:62, 41-42)
        return se2d_gate_res_relu_launch(c16, k.out_c16, s.gate, reinterpret_cast<const half_t*>(resid), ldr, reinterpret_cast<half_t*>(y), k.out_c16, B, Ho, Wo,
                                         k.out_c, st, peak.word());
    }

    int forward(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st) const override {
        MV_REQUIRE(feats != nullptr && emb != nullptr && ws != nullptr, "resnet_se forward: null buffer");
        MV_REQUIRE(B > 0 && T >= 9, "resnet_se forward: needs at least 9 frames (two time steps after three stride-2 stages)");
        const Ws s = carve(ws, B, T);
        if (s.bytes > ws_bytes) return fail(MV_ERR_WORKSPACE, "resnet_se forward: workspace too small");
        int rc;
        int H = cfg.input_size, W = T;
        // x.transpose(2, 1).unsqueeze(1) -> relu(bn1(conv1(x)))   (resnet_se.py:128-132)
        if ((rc = conv2d_first_s16_launch(feats, reinterpret_cast<half_t*>(s.ping[0]), stem_w, stem_b, B, T, cfg.input_size, cfg.num_filters[0], st, peak.word())))
            return rc;
        const float* cur = s.ping[0];
        int pp = 1;
        for (int l = 0; l < 4; ++l)
            for (const SeBlock& k : layers[l]) {
                if ((rc = run_block(k, cur, s.ping[pp], s, B, H, W, st))) return rc;
                if (k.stride == 2) {
                    H = s16_down(H);
                    W = s16_down(W);
                }
                cur = s.ping[pp];
                pp ^= 1;
            }
        MV_REQUIRE(H == final_h, "resnet_se forward: unexpected frequency size after the four stages");
        // x.reshape(B, -1, T') -> pooling -> bn2 -> linear -> bn3   (resnet_se.py:139-144)
        return head.forward(s.head, cur, B, H, W, emb, st);
    }
};

}  // namespace mv

extern "C" {

int mv_resnetse_create(const MvResNetSeCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out) {
    return mv::create_model<mv::ResNetSeModel>("mv_resnetse_create", cfg, tensors, num_tensors, out);
}

}  // extern "C"
