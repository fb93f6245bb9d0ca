// ResNetSE forward orchestrated natively (mvector/models/resnet_se.py:65-145).
//
// create(): reads the reference-layout fp32 state_dict, folds every eval-mode BatchNorm (eps 1e-5) into the conv in front of it (BN follows each conv
// directly: resnet_se.py:26-35, 114-118), pads channel counts to multiples of 16 and packs the weights for conv2ds_kernel, as eres2net.hip does.
// A bottleneck block is   conv1 1x1 + ReLU -> conv2 3x3 (stride) + ReLU -> conv3 1x1 -> SE gate -> + residual -> ReLU   (resnet_se.py:23-44):
// three (four with a downsample) conv2ds launches and the three passes of se2d.hip.  The ReLU has no upper bound, so every launch that stores a map
// reports the largest value it wanted to store to the handle's peak word (s16map.h; MV_INFO_RESNETSE_*).
// Head: the last map as fp16 rows [B, T', C * H] (x.reshape(B, -1, T'), resnet_se.py:139) -> Pooling (model.h) -> bn2 . linear . bn3 folded.
// forward(): a fixed sequence of launches on the caller's stream over the caller's workspace; no host synchronisation.
#include <memory>
#include <vector>

#include "kernels.h"
#include "model.h"
#include "s16map.h"

namespace mv {

namespace {

struct SeConv {
    half_t* w = nullptr;   // split-packed (conv2ds_pack_host)
    float* bias = nullptr;
    float oscale = 0.0f;
    int cin16 = 0, cout16 = 0, ks = 1, stride = 1;
    int cin = 0, cout = 0;
};

struct SeBlock {
    SeConv conv1, conv2, conv3, down;
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
    Pooling pool;
    float* fc_w = nullptr;
    float* fc_b = nullptr;
    unsigned* d_peak = nullptr;   // device word: largest |64 * value| a launch wanted to store (float bits; sticky, diagnostic only); null: MV_RESNETSE_NO_PEAK
    int final_c = 0, final_h = 0;

    // conv (no bias) [cout][cin][ks][ks] followed by BatchNorm `bn`, channels in their own order, zero rows / columns up to the padded counts
    int make_conv_bn(const Weights& w, const std::string& conv, const std::string& bn, int cout, int cin, int ks, int stride, SeConv* L) {
        std::vector<float> W, s, t;
        int rc;
        if ((rc = w.host(conv + ".weight", (int64_t)cout * cin * ks * ks, W)) || (rc = fold_bn(w, bn, cout, s, t, 1e-5f))) return rc;
        const int taps = ks * ks, cout16 = (int)round_up(cout, 16), cin16 = (int)round_up(cin, 16);
        std::vector<float> packed((size_t)cout16 * taps * cin16, 0.0f), bias((size_t)cout16, 0.0f);
        for (int co = 0; co < cout; ++co) {
            bias[co] = t[co];
            for (int ci = 0; ci < cin; ++ci)
                for (int tp = 0; tp < taps; ++tp) packed[((size_t)co * taps + tp) * cin16 + ci] = W[((size_t)co * cin + ci) * taps + tp] * s[co];
        }
        std::vector<half_t> split((size_t)conv2ds_packed_floats(cout16, cin16, ks) * 2);
        L->oscale = conv2ds_pack_host(packed.data(), cout16, cin16, ks, split.data());
        L->w = static_cast<half_t*>(dev_alloc(split.size() * sizeof(half_t)));
        L->bias = upload(bias);
        if (L->w == nullptr || L->bias == nullptr) return fail(MV_ERR_HIP, "resnet_se create: out of device memory");
        MV_HIP_OK(hipMemcpy(L->w, split.data(), split.size() * sizeof(half_t), hipMemcpyHostToDevice));
        L->cin16 = cin16;
        L->cout16 = cout16;
        L->cin = cin;
        L->cout = cout;
        L->ks = ks;
        L->stride = stride;
        return MV_OK;
    }

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
        if ((rc = make_conv_bn(w, p + ".conv1", p + ".bn1", planes, in_planes, 1, 1, &b->conv1)) ||
            (rc = make_conv_bn(w, p + ".conv2", p + ".bn2", planes, planes, 3, stride, &b->conv2)) ||
            (rc = make_conv_bn(w, p + ".conv3", p + ".bn3", b->out_c, planes, 1, 1, &b->conv3)))
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
        if (b->has_down) return make_conv_bn(w, p + ".downsample.0", p + ".downsample.1", b->out_c, in_planes, 1, stride, &b->down);
        return MV_OK;
    }

    int create(const MvResNetSeCfg& c, const Weights& w) {
        cfg = c;
        const bool track = c.pooling_type < 0 || (c.pooling_type & MV_RESNETSE_NO_PEAK) == 0;
        pool_type = c.pooling_type < 0 ? c.pooling_type : c.pooling_type & ~MV_RESNETSE_NO_PEAK;
        MV_REQUIRE(c.input_size >= 8 && c.input_size % 8 == 0, "resnet_se: input_size must be a multiple of 8");
        for (int i = 0; i < 4; ++i) {
            MV_REQUIRE(c.num_filters[i] >= 16 && c.num_filters[i] % 16 == 0 && c.num_filters[i] <= 512,
                       "resnet_se: num_filters must be multiples of 16, at most 512 (entry " + std::to_string(i) + ")");
            MV_REQUIRE(c.layers[i] >= 1, "resnet_se: every stage needs a block (stage " + std::to_string(i + 1) + ")");
        }
        MV_REQUIRE(c.embd_dim > 0 && c.reduction >= 1, "resnet_se: embd_dim and reduction must be positive");
        if (pool_type < MV_POOL_ASP || pool_type > MV_POOL_TSP)
            return fail(MV_ERR_INVALID_ARGUMENT, "resnet_se: pooling_type " + std::to_string(pool_type) +
                                                     " is not MV_POOL_ASP (0), MV_POOL_SAP (1), MV_POOL_TAP (2) or MV_POOL_TSP (3)");
        embd_dim = c.embd_dim;
        input_size = c.input_size;
        int rc;
        const int m = c.num_filters[0];
        {   // conv1 + bn1 + relu (resnet_se.py:71-73, 130-132): fp32 weights for the VALU stem kernel
            std::vector<float> W, s, t;
            if ((rc = w.host("conv1.weight", (int64_t)m * 9, W)) || (rc = fold_bn(w, "bn1", m, s, t, 1e-5f))) return rc;
            for (int co = 0; co < m; ++co)
                for (int j = 0; j < 9; ++j) W[(size_t)co * 9 + j] *= s[co];
            stem_w = upload(W);
            stem_b = upload(t);
            if (stem_w == nullptr || stem_b == nullptr) return fail(MV_ERR_HIP, "resnet_se create: upload failed");
        }
        int in_planes = m;
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
        final_c = in_planes;
        final_h = c.input_size / 8;
        if ((rc = pool.create(this, w, "pooling", pool_type, final_c * final_h, 128, true))) return rc;
        if ((rc = fold_final_linear(this, w, "linear.weight", "linear.bias", "bn2", "bn3", c.embd_dim, pool.width(), &fc_w, &fc_b))) return rc;
        if (track) {
            d_peak = static_cast<unsigned*>(dev_alloc(sizeof(unsigned)));
            if (d_peak == nullptr) return fail(MV_ERR_HIP, "resnet_se create: out of device memory");
            MV_HIP_OK(hipMemset(d_peak, 0, sizeof(unsigned)));
        }
        MV_HIP_OK(hipDeviceSynchronize());   // (the pooling head packs its weights on the device from temporaries of this call)
        return MV_OK;
    }

    int info(int key, float* value) const override {
        if (key == MV_INFO_RESNETSE_PEAK || key == MV_INFO_RESNETSE_SATURATED) {   // (waits for the device: a diagnostic, not a hot-path call)
            if (d_peak == nullptr) {
                *value = -1.0f;
                return MV_OK;
            }
            unsigned bits = 0;
            MV_HIP_OK(hipDeviceSynchronize());
            MV_HIP_OK(hipMemcpy(&bits, d_peak, sizeof(bits), hipMemcpyDeviceToHost));
            const float v = __builtin_bit_cast(float, bits);
            *value = key == MV_INFO_RESNETSE_PEAK ? v / CS_XSCALE : (v >= 65504.0f ? 1.0f : 0.0f);
            return MV_OK;
        }
        return MvModelBase::info(key, value);
    }

    // ---- workspace ---------------------------------------------------------------------------------------------
    struct Ws {
        float *ping[2], *a, *b, *c, *r;   // maps: S16 form, 4 bytes per channel
        float *sq, *gate, *sq_ws, *pooled, *asp_f, *lin_ws;
        half_t *rows, *h;
        size_t bytes, sq_ws_floats, lin_ws_floats;
    };
    static int down(int n) { return (n - 1) / 2 + 1; }

    Ws carve(void* base, int B, int T) const {
        Carver cv(base);
        Ws s;
        size_t max_io = 0, max_a = 0, max_b = 0, max_c = 0, max_sq = 0;
        int H = cfg.input_size, W = T, maxc = 0;
        max_io = (size_t)B * H * W * (size_t)round_up(cfg.num_filters[0], 16);
        for (int l = 0; l < 4; ++l)
            for (const SeBlock& k : layers[l]) {
                const int Ho = k.stride == 2 ? down(H) : H, Wo = k.stride == 2 ? down(W) : W;
                max_a = std::max(max_a, (size_t)B * H * W * k.planes16);
                max_b = std::max(max_b, (size_t)B * Ho * Wo * k.planes16);
                max_c = std::max(max_c, (size_t)B * Ho * Wo * k.out_c16);
                max_io = std::max(max_io, (size_t)B * Ho * Wo * k.out_c16);
                max_sq = std::max(max_sq, se2d_squeeze_ws_floats(B, Ho, Wo, k.out_c));
                maxc = std::max(maxc, k.out_c);
                H = Ho;
                W = Wo;
            }
        const size_t slack = 64;  // the conv loader reads whole 16-byte chunks
        s.ping[0] = cv.take<float>(max_io + slack);
        s.ping[1] = cv.take<float>(max_io + slack);
        s.a = cv.take<float>(max_a + slack);
        s.b = cv.take<float>(max_b + slack);
        s.c = cv.take<float>(max_c + slack);
        s.r = cv.take<float>(max_c + slack);
        s.sq = cv.take<float>((size_t)B * maxc);
        s.gate = cv.take<float>((size_t)B * maxc);
        s.sq_ws_floats = max_sq;
        s.sq_ws = cv.take<float>(max_sq);
        const int Cp = final_c * final_h;   // a multiple of 8 (final_c is one of 32)
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
        MV_REQUIRE(B > 0 && T >= 9 && bytes != nullptr, "resnet_se workspace: needs B > 0 and at least 9 frames");
        *bytes = carve(nullptr, B, T).bytes;
        return MV_OK;
    }

    // ---- launches ----------------------------------------------------------------------------------------------
    int conv(const SeConv& L, const float* x, int64_t ldx, float* y, int64_t ldy, int B, int H, int W, float lo, float hi, hipStream_t st) const {
        MvConv2dsDesc d{};
        d.x = x; d.ldx = ldx; d.w = L.w; d.bias = L.bias; d.oscale = L.oscale;
        d.y = y; d.ldy = ldy; d.B = B; d.H = H; d.W = W; d.cin16 = L.cin16; d.cout16 = L.cout16; d.ks = L.ks; d.stride = L.stride;
        d.epi = MV_EPI_CLAMP; d.lo = lo; d.hi = hi;
        d.cin_alg = L.cin; d.cout_alg = L.cout;
        d.peak = d_peak;
        return conv2ds_launch(d, st);
    }

    int run_block(const SeBlock& k, const float* x, float* y, const Ws& s, int B, int Hin, int Win, hipStream_t st) const {
        const float NEG = -3.0e38f, POS = 3.0e38f;
        const int Ho = k.stride == 2 ? down(Hin) : Hin, Wo = k.stride == 2 ? down(Win) : Win;
        int rc;
        // relu(bn1(conv1(x))), relu(bn2(conv2(.))), bn3(conv3(.))   (resnet_se.py:26-35)
        if ((rc = conv(k.conv1, x, k.in_c16, s.a, k.planes16, B, Hin, Win, 0.0f, POS, st)) ||
            (rc = conv(k.conv2, s.a, k.planes16, s.b, k.planes16, B, Hin, Win, 0.0f, POS, st)) ||
            (rc = conv(k.conv3, s.b, k.planes16, s.c, k.out_c16, B, Ho, Wo, NEG, POS, st)))
            return rc;
        // SELayer (resnet_se.py:58-62): y = fc(avg_pool(out))
        const half_t* c16 = reinterpret_cast<const half_t*>(s.c);
        if ((rc = se2d_squeeze_launch(c16, k.out_c16, B, Ho, Wo, k.out_c, s.sq, s.sq_ws, s.sq_ws_floats, st)) ||
            (rc = se2d_excite_launch(s.sq, k.fc1_w, k.fc1_b, k.fc2_w, k.fc2_b, s.gate, B, k.out_c, k.hidden, st)))
            return rc;
        const float* resid = x;
        int64_t ldr = k.in_c16;
        if (k.has_down) {   // downsample(x) (resnet_se.py:38-39)
            if ((rc = conv(k.down, x, k.in_c16, s.r, k.out_c16, B, Hin, Win, NEG, POS, st))) return rc;
            resid = s.r;
            ldr = k.out_c16;
        }
        // relu(out * y + residual)   (resnet_se.py:62, 41-42)
        return se2d_gate_res_relu_launch(c16, k.out_c16, s.gate, reinterpret_cast<const half_t*>(resid), ldr, reinterpret_cast<half_t*>(y), k.out_c16, B, Ho, Wo,
                                         k.out_c, st, d_peak);
    }

    int forward(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st) const override {
        MV_REQUIRE(feats != nullptr && emb != nullptr && ws != nullptr, "resnet_se forward: null buffer");
        MV_REQUIRE(B > 0 && T >= 9, "resnet_se forward: needs at least 9 frames (two time steps after three stride-2 stages)");
        const Ws s = carve(ws, B, T);
        if (s.bytes > ws_bytes) return fail(MV_ERR_WORKSPACE, "resnet_se forward: workspace too small");
        int rc;
        int H = cfg.input_size, W = T;
        // x.transpose(2, 1).unsqueeze(1) -> relu(bn1(conv1(x)))   (resnet_se.py:128-132)
        if ((rc = conv2d_first_s16_launch(feats, reinterpret_cast<half_t*>(s.ping[0]), stem_w, stem_b, B, T, cfg.input_size, cfg.num_filters[0], st, d_peak)))
            return rc;
        const float* cur = s.ping[0];
        int pp = 1;
        for (int l = 0; l < 4; ++l)
            for (const SeBlock& k : layers[l]) {
                if ((rc = run_block(k, cur, s.ping[pp], s, B, H, W, st))) return rc;
                if (k.stride == 2) {
                    H = down(H);
                    W = down(W);
                }
                cur = s.ping[pp];
                pp ^= 1;
            }
        MV_REQUIRE(H == final_h, "resnet_se forward: unexpected frequency size after the four stages");
        // x.reshape(B, -1, T') -> pooling -> bn2 -> linear -> bn3   (resnet_se.py:139-144)
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

int mv_resnetse_create(const MvResNetSeCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out) {
    MV_REQUIRE(cfg != nullptr && out != nullptr, "mv_resnetse_create: null argument");
    mv::Weights w;
    int rc = w.init(tensors, num_tensors);
    if (rc != MV_OK) return rc;
    auto m = std::make_unique<mv::ResNetSeModel>();
    rc = m->create(*cfg, w);
    if (rc != MV_OK) return rc;
    *out = reinterpret_cast<MvModel*>(static_cast<mv::MvModelBase*>(m.release()));
    return MV_OK;
}

}  // extern "C"
