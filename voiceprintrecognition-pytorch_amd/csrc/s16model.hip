// What the S16 backbones share on the host (s16model.h): weight packing at create time, the launch descriptor, the peak word, the pooling head.
#include "s16model.h"

#include "s16map.h"

namespace mv {

std::vector<int> s16_dense_map(int c) {
    std::vector<int> m(c);
    for (int i = 0; i < c; ++i) m[i] = i;
    return m;
}

std::vector<int> s16_grouped_map(int width, int scale, int wpad) {
    std::vector<int> m((size_t)width * scale);
    for (int c = 0; c < width * scale; ++c) m[c] = (c / width) * wpad + c % width;
    return m;
}

int make_s16_conv_bn(MvModelBase* m, const Weights& w, const char* who, const std::string& conv, const std::string& bn, int cout, int cin, int ks,
                     int stride, const std::vector<int>& out_pos, int cout16, const std::vector<int>& in_pos, int cin16, S16Conv* L,
                     std::vector<float>* bias_host) {
    std::vector<float> W, s, t, cb;
    int rc;
    if ((rc = w.host(conv + ".weight", (int64_t)cout * cin * ks * ks, W))) return rc;
    if (w.has(conv + ".bias") && (rc = w.host(conv + ".bias", cout, cb))) return rc;
    if (!bn.empty()) {
        if ((rc = fold_bn(w, bn, cout, s, t, 1e-5f))) return rc;
        if (!cb.empty())
            for (int c = 0; c < cout; ++c) t[c] += cb[c] * s[c];
    } else if (!cb.empty()) {
        t = cb;
    }
    // dense [cout16][taps][cin16]: row out_pos[co] scaled by s[co], column in_pos[ci]
    const int taps = ks * ks;
    std::vector<float> packed((size_t)cout16 * taps * cin16, 0.0f), bias((size_t)cout16, 0.0f);
    for (int co = 0; co < cout; ++co) {
        const float sc = s.empty() ? 1.0f : s[co];
        bias[out_pos[co]] = t.empty() ? 0.0f : t[co];
        for (int ci = 0; ci < cin; ++ci)
            for (int tp = 0; tp < taps; ++tp)
                packed[((size_t)out_pos[co] * taps + tp) * cin16 + in_pos[ci]] = W[((size_t)co * cin + ci) * taps + tp] * sc;
    }
    std::vector<half_t> split((size_t)conv2ds_packed_floats(cout16, cin16, ks) * 2);
    L->oscale = conv2ds_pack_host(packed.data(), cout16, cin16, ks, split.data());
    L->w = static_cast<half_t*>(m->dev_alloc(split.size() * sizeof(half_t)));
    L->bias = m->upload(bias);
    if (L->w == nullptr || L->bias == nullptr) return fail(MV_ERR_HIP, std::string(who) + " create: out of device memory");
    MV_HIP_OK(hipMemcpy(L->w, split.data(), split.size() * sizeof(half_t), hipMemcpyHostToDevice));
    L->cin16 = cin16;
    L->cout16 = cout16;
    L->cin = cin;
    L->cout = cout;
    L->ks = ks;
    L->stride = stride;
    if (bias_host != nullptr) *bias_host = bias;
    return MV_OK;
}

int fold_s16_stem(MvModelBase* m, const Weights& w, const char* who, int C, int taps, float** stem_w, float** stem_b) {
    std::vector<float> W, s, t;
    int rc;
    if ((rc = w.host("conv1.weight", (int64_t)C * taps, W)) || (rc = fold_bn(w, "bn1", C, s, t, 1e-5f))) return rc;
    for (int co = 0; co < C; ++co)
        for (int j = 0; j < taps; ++j) W[(size_t)co * taps + j] *= s[co];
    *stem_w = m->upload(W);
    *stem_b = m->upload(t);
    if (*stem_w == nullptr || *stem_b == nullptr) return fail(MV_ERR_HIP, std::string(who) + " create: upload failed");
    return MV_OK;
}

MvConv2dsDesc s16_conv_desc(const S16Conv& L, const float* x, int64_t ldx, float* y, int64_t ldy, int B, int H, int W) {
    MvConv2dsDesc d{};
    d.x = x;
    d.ldx = ldx;
    d.y = y;
    d.ldy = ldy;
    d.w = L.w;
    d.bias = L.bias;
    d.oscale = L.oscale;
    d.B = B;
    d.H = H;
    d.W = W;
    d.cin16 = L.cin16;
    d.cout16 = L.cout16;
    d.ks = L.ks;
    d.stride = L.stride;
    d.epi = MV_EPI_CLAMP;
    d.cin_alg = L.cin;
    d.cout_alg = L.cout;
    return d;
}

int S16Peak::create(MvModelBase* m, int cfg_pooling_type, const char* who, int* pool_type) {
    static_assert(MV_RESNETSE_NO_PEAK == MV_RES2NET_NO_PEAK, "one flag bit for every S16 backbone");
    const int NO_PEAK = MV_RES2NET_NO_PEAK;
    const bool track = cfg_pooling_type < 0 || (cfg_pooling_type & NO_PEAK) == 0;
    *pool_type = cfg_pooling_type < 0 ? cfg_pooling_type : cfg_pooling_type & ~NO_PEAK;
    if (*pool_type < MV_POOL_ASP || *pool_type > MV_POOL_TSP)
        return fail(MV_ERR_INVALID_ARGUMENT, std::string(who) + ": pooling_type " + std::to_string(*pool_type) +
                                                 " is not MV_POOL_ASP (0), MV_POOL_SAP (1), MV_POOL_TAP (2) or MV_POOL_TSP (3)");
    return track ? alloc(m, who) : MV_OK;
}

int S16Peak::alloc(MvModelBase* m, const char* who) {
    d_peak = static_cast<unsigned*>(m->dev_alloc(sizeof(unsigned)));
    if (d_peak == nullptr) return fail(MV_ERR_HIP, std::string(who) + " create: out of device memory");
    return clear();
}

int S16Peak::read(int key, float* value) const {
    if (d_peak == nullptr) {
        *value = -1.0f;
        return MV_OK;
    }
    float v = 0.0f;
    MV_HIP_OK(hipDeviceSynchronize());
    if (const int rc = raw(&v)) return rc;
    *value = key == MV_INFO_S16_PEAK ? v / CS_XSCALE : (v >= 65504.0f ? 1.0f : 0.0f);
    return MV_OK;
}

bool S16Peak::info(int key, float* value, int* rc) const {
    if (key != MV_INFO_S16_PEAK && key != MV_INFO_S16_SATURATED) return false;
    *rc = read(key, value);
    return true;
}

int S16Head::create(MvModelBase* m, const Weights& w, int pool_type, int final_c_, int final_h_, int embd_dim_) {
    final_c = final_c_;
    final_h = final_h_;
    embd_dim = embd_dim_;
    int rc;
    if ((rc = pool.create(m, w, "pooling", pool_type, final_c * final_h, 128, true))) return rc;
    if ((rc = fold_final_linear(m, w, "linear.weight", "linear.bias", "bn2", "bn3", embd_dim, pool.width(), &fc_w, &fc_b))) return rc;
    MV_HIP_OK(hipDeviceSynchronize());   // (the pooling head packs its weights on the device from temporaries of this call)
    return MV_OK;
}

S16Head::Ws S16Head::carve(Carver& cv, int B, int W) const {
    Ws s;
    const int Cp = final_c * final_h;   // a multiple of 8 (final_c is one of 32 or more)
    s.rows = cv.take<half_t>((size_t)B * W * Cp);
    s.h = cv.take<half_t>((size_t)B * W * pool.hidden_width());
    s.asp_f = cv.take<float>(pool.workspace_floats(B, W));
    s.pooled = cv.take<float>((size_t)B * pool.width());
    s.lin_ws_floats = linear_f32_splitk_floats(B, pool.width(), embd_dim);
    s.lin_ws = cv.take<float>(s.lin_ws_floats);
    return s;
}

int S16Head::forward(const Ws& s, const float* map, int B, int H, int W, float* emb, hipStream_t st) const {
    const int Cp = final_c * final_h, P = pool.width();
    int rc;
    if ((rc = s16_map_to_rows_launch(reinterpret_cast<const half_t*>(map), (int64_t)round_up(final_c, 16), B, H, W, final_c, s.rows, Cp, st)) ||
        (rc = pool.forward(s.rows, Cp, B, W, s.h, s.asp_f, s.pooled, st)))
        return rc;
    return linear_f32_launch(s.pooled, P, fc_w, P, fc_b, MV_ACT_NONE, emb, embd_dim, B, P, embd_dim, 0, st, s.lin_ws, s.lin_ws_floats);
}

}  // namespace mv
