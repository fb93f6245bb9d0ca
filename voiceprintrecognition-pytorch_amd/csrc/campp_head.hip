// The FCM head of CAM++ (campplus.hip) in both forms: conv3x3(1->32)+BN+ReLU, 2 x [BasicResBlock(stride (2,1)), BasicResBlock], conv3x3 stride (2,1)
// +BN+ReLU on channel-last maps [B, F, T, 32]; the last conv writes the rows [B, T, F/8, 32] the TDNN reads.
//
// Head precision.  The fp16 head (fp16 maps and tap matrices, fp32 accumulation) reproduces trained-like checkpoints to 6e-8, but a head
// with large BatchNorm gains amplifies the 2^-11 operand rounding of its ~20 sites ~100 x (tests/budget_campp.py: the stress golden
// lands at 4e-4, no single site owning it).  So the handle also carries the head in an EXACT form -- the "fp32 head" of the interface: since
// round 4 the split-operand kernels of the ERes2Net family (conv2ds.hip: maps and weights as hi + lo fp16 pairs = 22 bits, three fp16 MFMA
// passes, the frequency-only stride through MvConv2dsDesc.stride_w; rounds 2-3: fp32 maps on v_mfma_f32_16x16x4_f32, conv2d.hip) -- and
// DECIDES AT CREATION which one it runs: both heads embed THREE fixed probe utterances (white uniform, white bell-shaped with the time mean
// removed, smooth voiced-like); if the embeddings of any probe differ by more than 5e-6 in 1 - cos the checkpoint is ill-conditioned for fp16
// maps and the handle takes the exact head (a multiple of the step time: bench leg config3_campp_fp32_head), otherwise the fp16 head.  How far such a figure is from the miss on a given input
// depends on the input (tests/budget_campp.py + profiles/r12_campp_head_probes.log: on the BatchNorm-calibrated family of the stress
// golden one white probe alone under-reads the miss on the test input by 2-40 x, the bell-shaped probe -- the test input's own statistics
// -- tracks it within 2 x), hence several probes with different statistics and the largest figure.
// MvCamppCfg.head_precision pins the head (measurements, tests, one numerics on every rank); mv_model_info reports the choice and the figures.
// The probes, the gain search and the choice: campp_probe.hip.
#include <array>
#include <cfloat>

#include "campplus.h"

namespace mv {

namespace {

// fp16 head: conv 3x3 (+ its BatchNorm) as nine tap matrices [tap][co][ci], the block's shortcut conv (+ BatchNorm; sc_conv empty: none) as a tenth
int fold_fcm_conv(MvModelBase* m, const Weights& w, const std::string& conv, const std::string& bn, const std::string& sc_conv, const std::string& sc_bn,
                  CamppHead::FcmConv* out) {
    std::vector<float> W, s, t, Ws, ss, ts;
    int rc;
    if ((rc = w.host(conv + ".weight", 32 * 32 * 9, W)) || (rc = fold_bn(w, bn, 32, s, t, 1e-5f))) return rc;
    const bool sc = !sc_conv.empty();
    if (sc)
        if ((rc = w.host(sc_conv + ".weight", 32 * 32, Ws)) || (rc = fold_bn(w, sc_bn, 32, ss, ts, 1e-5f))) return rc;
    out->ntaps = sc ? 10 : 9;
    std::vector<float> bias(32);
    std::vector<half_t> ph((size_t)out->ntaps * 32 * 32);   // fp32 -> fp16 on the host (round-to-nearest-even via _Float16)
    for (int co = 0; co < 32; ++co) {
        bias[co] = t[co] + (sc ? ts[co] : 0.0f);
        for (int ci = 0; ci < 32; ++ci) {
            for (int tap = 0; tap < 9; ++tap) ph[((size_t)tap * 32 + co) * 32 + ci] = (half_t)(W[((size_t)co * 32 + ci) * 9 + tap] * s[co]);
            if (sc) ph[((size_t)9 * 32 + co) * 32 + ci] = (half_t)(Ws[(size_t)co * 32 + ci] * ss[co]);
        }
    }
    out->w = static_cast<half_t*>(m->dev_alloc(ph.size() * sizeof(half_t)));
    if (out->w == nullptr) return fail(MV_ERR_HIP, "campp create: out of device memory");
    MV_HIP_OK(hipMemcpy(out->w, ph.data(), ph.size() * sizeof(half_t), hipMemcpyHostToDevice));
    out->bias = m->upload(bias);
    return out->bias ? MV_OK : fail(MV_ERR_HIP, "campp create: upload failed");
}

}  // namespace

int CamppHead::create(MvModelBase* m, const Weights& w, int input_size) {
    F = input_size;
    F8 = (F + 7) / 8;
    int rc;
    {  // head.conv1 + bn1 (one input map)
        std::vector<float> W, s, t;
        if ((rc = w.host("head.conv1.weight", 32 * 9, W)) || (rc = fold_bn(w, "head.bn1", 32, s, t, 1e-5f))) return rc;
        for (int co = 0; co < 32; ++co)
            for (int j = 0; j < 9; ++j) W[co * 9 + j] *= s[co];
        c1_w = m->upload(W);
        c1_b = m->upload(t);
        c1_wx = m->upload(W);
        c1_bx = m->upload(t);
        gained.push_back({c1_wx, W});
        gained.push_back({c1_bx, t});
        if (c1_wx == nullptr || c1_bx == nullptr) return fail(MV_ERR_HIP, "campp create: out of device memory");
        if ((rc = peak.alloc(m, "campp"))) return rc;
        std::vector<half_t> frag(2 * 64 * 8);
        fcm_c1_pack(W.data(), frag.data());
        c1_a = static_cast<half_t*>(m->dev_alloc(frag.size() * sizeof(half_t)));
        if (c1_a == nullptr) return fail(MV_ERR_HIP, "campp create: out of device memory");
        MV_HIP_OK(hipMemcpy(c1_a, frag.data(), frag.size() * sizeof(half_t), hipMemcpyHostToDevice));
    }
    // exact head: the same arithmetic (W * s[co] in fp32, the BN shift as bias) packed for conv2ds_kernel; the bias carries the gain
    auto exact = [&](const std::string& conv, const std::string& bn, int ks, int stride, S16Conv* L) {
        gained.emplace_back();
        const int rc = make_s16_conv_bn(m, w, "campp", conv, bn, 32, 32, ks, stride, L, &gained.back().host);
        gained.back().dev = L->bias;
        return rc;
    };
    const char* names[4] = {"head.layer1.0", "head.layer1.1", "head.layer2.0", "head.layer2.1"};
    for (int i = 0; i < 4; ++i) {
        const std::string p = names[i];
        ResBlock& r = res[i];
        r.has_shortcut = (i % 2 == 0);
        r.stride = r.has_shortcut ? 2 : 1;
        const std::string sc0 = r.has_shortcut ? p + ".shortcut.0" : "", sc1 = r.has_shortcut ? p + ".shortcut.1" : "";
        if ((rc = fold_fcm_conv(m, w, p + ".conv1", p + ".bn1", "", "", &r.conv1)) || (rc = exact(p + ".conv1", p + ".bn1", 3, r.stride, &r.x1)) ||
            (rc = fold_fcm_conv(m, w, p + ".conv2", p + ".bn2", sc0, sc1, &r.conv2)) || (rc = exact(p + ".conv2", p + ".bn2", 3, 1, &r.x2)))
            return rc;
        if (r.has_shortcut && (rc = exact(sc0, sc1, 1, r.stride, &r.xsc))) return rc;
    }
    if ((rc = fold_fcm_conv(m, w, "head.conv2", "head.bn2", "", "", &out))) return rc;
    return exact("head.conv2", "head.bn2", 3, 2, &outx);
}

int CamppHead::set_gain(int k) {
    gain_k = k;
    const float g = ldexpf(1.0f, -k);
    for (const Gained& e : gained) {
        std::vector<float> v(e.host);
        for (float& x : v) x *= g;
        MV_HIP_OK(hipMemcpy(e.dev, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return MV_OK;
}

// exact FCM head: S16 maps [B, F, T, 32] (hi + lo fp16 pairs, 4 bytes per channel) through the split-operand conv2ds kernels (header comment)
int CamppHead::forward_exact(const float* feats, int B, int T, const Maps& s, half_t* rows, hipStream_t st) const {
    int rc;
    if ((rc = conv2d_first_s16_launch(feats, reinterpret_cast<half_t*>(s.f0), c1_wx, c1_bx, B, T, F, 32, st, peak.word()))) return rc;
    // what every conv of this head adds to its record's descriptor: the stride along the frequency axis only, the residual, ReLU or none
    auto run = [&](MvConv2dsDesc d, const float* resid, bool relu) {
        d.stride_w = 1;
        d.res = resid;
        d.ldres = 32;
        d.lo = relu ? 0.0f : -FLT_MAX;
        d.hi = FLT_MAX;
        d.peak = peak.word();
        return conv2ds_launch(d, st);
    };
    const float* cur = s.f0;
    int Fc = F;
    for (int i = 0; i < 4; ++i) {
        const ResBlock& r = res[i];
        const int Fo = (Fc - 1) / r.stride + 1;
        // buffers: block 0 f0 -> fc, block 1 fc -> fb, block 2 fb -> f0, block 3 f0 -> fb (conv1 output always in fa; shortcut of
        // block 0 in fb, of block 2 in fc)
        float* y = i == 0 ? s.fc : (i == 2 ? s.f0 : s.fb);
        float* scb = i == 0 ? s.fb : s.fc;
        if ((rc = run(s16_conv_desc(r.x1, cur, 32, s.fa, 32, B, Fc, T), nullptr, true))) return rc;
        const float* resid = cur;
        if (r.has_shortcut) {
            if ((rc = run(s16_conv_desc(r.xsc, cur, 32, scb, 32, B, Fc, T), nullptr, false))) return rc;
            resid = scb;
        }
        if ((rc = run(s16_conv_desc(r.x2, s.fa, 32, y, 32, B, Fo, T), resid, true))) return rc;
        cur = y;
        Fc = Fo;
    }
    MV_REQUIRE((Fc - 1) / 2 + 1 == F8, "campp forward: unexpected frequency size after the head");
    if ((rc = run(s16_conv_desc(outx, cur, 32, s.fa, 32, B, Fc, T), nullptr, true))) return rc;
    return fcm_rows_from_s16_launch(reinterpret_cast<const half_t*>(s.fa), rows, B, T, F8, st, ldexpf(1.0f, gain_k));
}

int CamppHead::forward_f16(const float* feats, int B, int T, const Maps& s, half_t* rows, hipStream_t st) const {
    int rc;
    auto plain = [&](int Fd) { return std::array<int64_t, 3>{(int64_t)Fd * T * 32, (int64_t)T * 32, 32}; };
    const half_t* cur = s.m0;
    int Fc = F;
    half_t* pp[2] = {s.m1, s.m2};
    // head.conv1 is evaluated inside the first block's kernel (no [B, F, T, 32] image of the features in HBM) whenever the block has the
    // reference's shape (strided, with its shortcut conv); fcm_conv1_kernel (fp32 weights on the vector pipe) covers the rest
    const bool c1_inside = res[0].stride == 2 && res[0].has_shortcut && F >= 3 && (int64_t)B * T * F < ((int64_t)1 << 31);
    if (!c1_inside)
        if ((rc = fcm_conv1_launch(feats, s.m0, c1_w, c1_b, B, T, F, st))) return rc;
    for (int i = 0; i < 4; ++i) {
        // one launch per BasicResBlock (fcmblock.hip): x read once, mid map in LDS, output written once
        const ResBlock& r = res[i];
        const int Fo = (Fc - 1) / r.stride + 1;
        auto so = plain(Fo);
        half_t* t2 = (cur == pp[0]) ? pp[1] : pp[0];
        if (!fcm_block_supported(t2, so[0], so[1], so[2], T, Fc))
            return fail(MV_ERR_UNSUPPORTED, "campp forward: utterance too long for the FCM head (T * 32 * F must stay below 2^31 elements)");
        const bool c1 = i == 0 && c1_inside;  // the block's input rows are made from the features inside the kernel
        if ((rc = fcm_block_launch(c1 ? nullptr : cur, Fc, r.stride, r.conv1.w, r.conv1.bias, r.conv2.w, r.conv2.bias, r.has_shortcut ? 1 : 0,
                                   t2, so[0], so[1], so[2], B, T, st, c1 ? feats : nullptr, c1_a, c1_b)))
            return rc;
        cur = t2;
        Fc = Fo;
    }
    // head.conv2 (stride 2 in frequency) -> rows [B, T, F8, 32]
    const int Fo = (Fc - 1) / 2 + 1;
    MV_REQUIRE(Fo == F8, "campp forward: unexpected frequency size after the head");
    return fcm_conv3x3_launch(cur, Fc, 2, nullptr, 0, 1, 0, out.w, out.bias, rows, (int64_t)T * F8 * 32, 32, (int64_t)F8 * 32, B, T, Fo, st);
}

}  // namespace mv
