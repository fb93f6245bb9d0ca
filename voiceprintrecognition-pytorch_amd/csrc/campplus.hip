// CAM++ forward orchestrated natively (mvector/models/campplus.py:295-357).
//
//   head      FCM: conv3x3(1->32)+BN+ReLU, 2 x [BasicResBlock(stride (2,1)), BasicResBlock], conv3x3 stride (2,1)+BN+ReLU
//             on channel-last maps [B, F, T, 32] (fcm.hip); the last conv writes [B, T, F/8, 32], i.e. the 320-channel
//             row the TDNN reads (the reference's reshape order c*10+f is absorbed into the packed TDNN weight).
//   xvector   tdnn (k=5, stride 2, BN, ReLU) -> three CAM dense-TDNN blocks.  A block owns ONE [B, T2, C_final] buffer and
//             every layer writes its 32 new channels into its slice (the reference re-copies the growing tensor with
//             torch.cat on each of the 52 layers, campplus.py:178-181).  Per layer:
//                 h   = ReLU(BN2(W1 . ReLU(BN1(x))))           1x1 conv, BN1/ReLU applied on load, BN2/ReLU in the epilogue
//                 ctx = mean_T(h) + segmean_100(h)             (campplus.py:94-111) -> [B, nseg, 128]
//                 m   = sigmoid(W_b . ReLU(W_a . ctx + b_a) + b_b)   evaluated once per segment, not per frame
//                 y   = conv_k3(h) * m                          gate multiplied in the conv epilogue
//             (one launch per block / layer for utterances of up to 160 strided frames: camblock.hip, camdense.hip; two launches per layer over
//             160-frame chunks beyond: camdense.hip "long utterances"; five launches per layer only where neither form applies)
//             transit: 1x1 conv with BN/ReLU on load; out_nonlinear + StatsPool (unbiased std) fused into one reduction;
//             dense + BN(affine=False) folded into one fp32 linear layer.
//
// The head in its two forms and which one a handle runs: campp_head.hip ("Head precision").  What create() measures on its probe utterances
// (the exact head's gain, the head choice, the x-vector sensitivity): campp_probe.hip.  Struct declarations: campplus.h.
#include <functional>

#include "campplus.h"
#include "s16map.h"

namespace mv {

int CamppModel::create(const MvCamppCfg& c, const Weights& w) {
    cfg = c;
    input_size = c.input_size;
    embd_dim = c.embd_dim;
    MV_REQUIRE(c.input_size >= 8, "campp: input_size must be at least 8");
    MV_REQUIRE(c.growth_rate == 32 && c.bn_size * c.growth_rate == 128 && c.init_channels % 64 == 0,
               "campp: only growth_rate=32, bn_size=4 and init_channels multiple of 64 are implemented");
    F8 = (c.input_size + 7) / 8;
    bn_ch = c.bn_size * c.growth_rate;
    int rc;
    if ((rc = head.create(this, w, c.input_size))) return rc;
    {  // xvector.tdnn: weight [init, 32*F8, 5] with input channel c*F8+f  ->  our row layout f*32+c
        const int cin = 32 * F8;
        std::vector<float> W;
        if ((rc = w.host("xvector.tdnn.linear.weight", (int64_t)c.init_channels * cin * 5, W))) return rc;
        std::vector<float> P(W.size());
        for (int co = 0; co < c.init_channels; ++co)
            for (int ch = 0; ch < 32; ++ch)
                for (int f = 0; f < F8; ++f)
                    for (int j = 0; j < 5; ++j)
                        P[((size_t)co * cin + (f * 32 + ch)) * 5 + j] = W[((size_t)co * cin + (ch * F8 + f)) * 5 + j];
        float* tmp = upload(P);
        if (tmp == nullptr) return fail(MV_ERR_HIP, "campp create: upload failed");
        if ((rc = make_conv_from(tmp, nullptr, "", c.init_channels, cin, 5, &tdnn))) return rc;
        if ((rc = make_bn(w, "xvector.tdnn.nonlinear.batchnorm", c.init_channels, &tdnn_scale, &tdnn_shift))) return rc;
    }
    const int nlayers[3] = {12, 24, 16};
    const int dils[3] = {1, 2, 2};
    int channels = c.init_channels;
    for (int bi = 0; bi < 3; ++bi) {
        Block& B = blocks[bi];
        B.c_in = channels;
        B.dil = dils[bi];
        B.layers.resize(nlayers[bi]);
        for (int li = 0; li < nlayers[bi]; ++li) {
            DenseLayer& L = B.layers[li];
            L.cin = channels + li * c.growth_rate;
            const std::string p = "xvector.block" + std::to_string(bi + 1) + ".tdnnd" + std::to_string(li + 1);
            if ((rc = make_bn(w, p + ".nonlinear1.batchnorm", L.cin, &L.bn1_s, &L.bn1_t))) return rc;
            if ((rc = make_conv(w, p + ".linear1.weight", "", bn_ch, L.cin, 1, &L.lin1))) return rc;
            if ((rc = make_bn(w, p + ".nonlinear2.batchnorm", bn_ch, &L.bn2_s, &L.bn2_t))) return rc;
            if ((rc = make_conv(w, p + ".cam_layer.linear_local.weight", "", c.growth_rate, bn_ch, 3, &L.local))) return rc;
            std::vector<float> t;
            if ((rc = w.host(p + ".cam_layer.linear1.weight", (int64_t)(bn_ch / 2) * bn_ch, t))) return rc;
            L.wa = upload(t);
            if ((rc = w.host(p + ".cam_layer.linear1.bias", bn_ch / 2, t))) return rc;
            L.ba = upload(t);
            if ((rc = w.host(p + ".cam_layer.linear2.weight", (int64_t)c.growth_rate * (bn_ch / 2), t))) return rc;
            L.wb = upload(t);
            if ((rc = w.host(p + ".cam_layer.linear2.bias", c.growth_rate, t))) return rc;
            L.bb = upload(t);
        }
        {   // the block's layers as one device array (camblock.hip)
            std::vector<MvCamLayerDesc>& hd = B.hdescs;
            hd.resize(B.layers.size());
            for (size_t li = 0; li < B.layers.size(); ++li) {
                const DenseLayer& L = B.layers[li];
                hd[li] = MvCamLayerDesc{L.lin1.w, L.bn1_s, L.bn1_t, L.bn2_s, L.bn2_t, L.local.w, L.wa, L.ba, L.wb, L.bb, L.cin, conv1d_cin_pad(L.cin)};
            }
            B.descs = static_cast<MvCamLayerDesc*>(dev_alloc(hd.size() * sizeof(MvCamLayerDesc)));
            if (B.descs == nullptr) return fail(MV_ERR_HIP, "campp create: out of device memory");
            MV_HIP_OK(hipMemcpy(B.descs, hd.data(), hd.size() * sizeof(MvCamLayerDesc), hipMemcpyHostToDevice));
        }
        channels += nlayers[bi] * c.growth_rate;
        B.c_out = channels;
        const std::string tp = "xvector.transit" + std::to_string(bi + 1);
        if ((rc = make_bn(w, tp + ".nonlinear.batchnorm", channels, &B.tr_s, &B.tr_t))) return rc;
        if ((rc = make_conv(w, tp + ".linear.weight", tp + ".linear.bias", channels / 2, channels, 1, &B.transit))) return rc;
        channels /= 2;
    }
    cfin = channels;
    if ((rc = make_bn(w, "xvector.out_nonlinear.batchnorm", cfin, &out_s, &out_t))) return rc;
    if ((rc = fold_final_linear(this, w, "xvector.dense.linear.weight", "xvector.dense.linear.bias", "",
                                "xvector.dense.nonlinear.batchnorm", c.embd_dim, 2 * cfin, &dense_w, &dense_b)))
        return rc;
    MV_HIP_OK(hipDeviceSynchronize());
    if ((rc = choose_head())) return rc;
    return c.xvector_probe == MV_CAMPP_XVEC_PROBE_OFF ? MV_OK : probe_xvector(w);
}

int CamppModel::info(int key, float* value) const {
    switch (key) {
        case MV_INFO_CAMPP_HEAD_F32: *value = head_f32 ? 1.0f : 0.0f; return MV_OK;
        case MV_INFO_CAMPP_CALIBRATION: *value = calibration; return MV_OK;
        case MV_INFO_CAMPP_PROBE0: case MV_INFO_CAMPP_PROBE0 + 1: case MV_INFO_CAMPP_PROBE0 + 2:
            *value = probe_calibration[key - MV_INFO_CAMPP_PROBE0];
            return MV_OK;
        case MV_INFO_CAMPP_HEAD_GAIN_LOG2: *value = (float)-head.gain_k; return MV_OK;
        case MV_INFO_CAMPP_PROBE_PEAK: *value = probe_peak; return MV_OK;
        case MV_INFO_CAMPP_XVEC_SENSITIVITY: *value = xvec_sensitivity; return MV_OK;
        case MV_INFO_CAMPP_XVEC_PROBE0: case MV_INFO_CAMPP_XVEC_PROBE0 + 1: case MV_INFO_CAMPP_XVEC_PROBE0 + 2:
            *value = xvec_probe[key - MV_INFO_CAMPP_XVEC_PROBE0];
            return MV_OK;
        case MV_INFO_CAMPP_HEAD_PEAK: case MV_INFO_CAMPP_HEAD_SATURATED: {   // (waits for the device: a diagnostic, not a hot-path call)
            float v = 0.0f;   // largest scaled value the exact head wanted to store since the word was last cleared
            MV_HIP_OK(hipDeviceSynchronize());
            if (head.peak.raw(&v) != MV_OK) return MV_ERR_HIP;
            *value = key == MV_INFO_CAMPP_HEAD_PEAK ? ldexpf(v, head.gain_k) / CS_XSCALE : (v >= 65504.0f ? 1.0f : 0.0f);
            return MV_OK;
        }
    }
    return MvModelBase::info(key, value);
}

CamppModel::Ws CamppModel::carve(void* base, int B, int T, bool f32) const {
    Carver c(base);
    Ws s;
    const int F = cfg.input_size;
    s.T2 = (T - 1) / 2 + 1;
    s.nseg = (s.T2 + 99) / 100;
    const size_t full = (size_t)B * F * T * 32;
    const size_t half = (size_t)B * ((F + 1) / 2) * T * 32;
    CamppHead::Maps& m = s.maps;
    m.f0 = m.fa = m.fb = m.fc = nullptr;
    m.m0 = m.m1 = m.m2 = nullptr;
    if (f32) {
        m.f0 = c.take<float>(full);
        m.fa = c.take<float>(half);
        m.fb = c.take<float>(half);
        m.fc = c.take<float>(half);
    } else {
        m.m0 = c.take<half_t>(full);
        m.m1 = c.take<half_t>(half);
        m.m2 = c.take<half_t>(half);
    }
    s.rows = c.take<half_t>((size_t)B * T * 32 * F8);
    const size_t N2 = (size_t)B * s.T2;
    for (int i = 0; i < 3; ++i) s.xb[i] = c.take<half_t>(N2 * blocks[i].c_out);
    s.last = c.take<half_t>(N2 * cfin);
    s.h = c.take<half_t>(N2 * bn_ch);
    {
        size_t widest = 0;
        for (int i = 0; i < 3; ++i) widest = (size_t)blocks[i].c_out > widest ? (size_t)blocks[i].c_out : widest;
        s.act = c.take<half_t>(N2 * widest);
    }
    s.ctx = c.take<float>((size_t)B * s.nseg * bn_ch);
    s.hpart = c.take<float>((size_t)cam_dense_long_part_floats(B, s.T2));
    s.g1 = c.take<float>((size_t)B * s.nseg * (bn_ch / 2));
    s.gate = c.take<float>((size_t)B * s.nseg * cfg.growth_rate);
    s.stats = c.take<float>((size_t)B * 2 * cfin);
    s.bytes = c.total();
    return s;
}

int CamppModel::workspace_bytes(int B, int T, size_t* bytes) const {
    MV_REQUIRE(B > 0 && T > 0 && bytes != nullptr, "workspace_bytes: bad argument");
    *bytes = carve(nullptr, B, T, head_f32).bytes;
    return MV_OK;
}

// layer li of a dense block on X [B, T2, c_out] as five launches: every other geometry (bottleneck / growth widths the fused kernels are not built for)
int CamppModel::five_launches(const Block& Bk, half_t* X, const Ws& s, int B, int li, hipStream_t st) const {
    const DenseLayer& L = Bk.layers[li];
    const int T2 = s.T2, G = cfg.growth_rate;
    const int64_t ld = Bk.c_out;
    int rc;
    MvConv1dDesc d = conv_desc(L.lin1, X, ld, s.h, bn_ch, B, T2, T2);
    d.in_scale = L.bn1_s;
    d.in_shift = L.bn1_t;
    d.scale = L.bn2_s;
    d.shift = L.bn2_t;
    d.post_act = MV_ACT_RELU;
    d.pad_mode = MV_PAD_ZERO;
    if ((rc = conv1d_launch(d, st))) return rc;
    if ((rc = seg_mean_launch(s.h, bn_ch, B, T2, bn_ch, 100, s.ctx, st))) return rc;
    const int rows = B * s.nseg;
    if ((rc = linear_f32_launch(s.ctx, bn_ch, L.wa, bn_ch, L.ba, MV_ACT_RELU, s.g1, bn_ch / 2, rows, bn_ch, bn_ch / 2, 0, st)))
        return rc;
    if ((rc = linear_f32_launch(s.g1, bn_ch / 2, L.wb, bn_ch / 2, L.bb, MV_ACT_SIGMOID, s.gate, G, rows, bn_ch / 2, G, 0, st)))
        return rc;
    d = conv_desc(L.local, s.h, bn_ch, X + L.cin, ld, B, T2, T2);
    d.gate = s.gate;
    d.gate_seg_len = 100;
    d.dilation = Bk.dil;
    d.pad = Bk.dil;
    d.pad_mode = MV_PAD_ZERO;
    return conv1d_launch(d, st);
}

int CamppModel::forward_impl(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st, bool f32) const {
    MV_REQUIRE(feats != nullptr && emb != nullptr && ws != nullptr, "campp forward: null buffer");
    MV_REQUIRE(B > 0 && T >= 3, "campp forward: needs at least 3 frames (unbiased std over the strided time axis)");
    const Ws s = carve(ws, B, T, f32);
    if (s.bytes > ws_bytes) return fail(MV_ERR_WORKSPACE, "campp forward: workspace too small");
    int rc;
    // ---- head: features -> rows [B, T, F8, 32] ----
    if ((rc = f32 ? head.forward_exact(feats, B, T, s.maps, s.rows, st) : head.forward_f16(feats, B, T, s.maps, s.rows, st))) return rc;
    // ---- xvector.tdnn: k=5, stride 2, zero pad 2, BN, ReLU -> first slice of block 1's buffer ----
    const int T2 = s.T2;
    {
        MvConv1dDesc d = conv_desc(tdnn, s.rows, 32 * F8, s.xb[0], blocks[0].c_out, B, T, T2);
        d.scale = tdnn_scale;
        d.shift = tdnn_shift;
        d.post_act = MV_ACT_RELU;
        d.stride = 2;
        d.pad = 2;
        d.pad_mode = MV_PAD_ZERO;
        if ((rc = conv1d_launch(d, st))) return rc;
    }
    const int G = cfg.growth_rate;
    for (int bi = 0; bi < 3; ++bi) {
        const Block& Bk = blocks[bi];
        half_t* X = s.xb[bi];
        const int64_t ld = Bk.c_out;
        // all layers of the block in one launch, the next layer's first operands requested under the current layer's tail (camblock.hip);
        // geometries it does not take fall through to one launch per layer, long utterances to two (cam_dense_block_run: the choice
        // mv_cam_dense_block_f16 exposes as form 0), anything else to five_launches
        const std::function<int(int)> fallback = [&](int li) { return five_launches(Bk, X, s, B, li, st); };
        if ((rc = cam_dense_block_run(X, ld, B, T2, Bk.c_in, Bk.hdescs.data(), Bk.descs, (int)Bk.layers.size(), bn_ch, G, Bk.dil, 100,
                                      MV_CAM_FORM_AUTO, s.h, s.hpart, nullptr, &fallback, st)))
            return rc;
        // transit: BN + ReLU, then a 1x1 conv that halves the channels into the next block's buffer.  The pre-activation is written out once
        // (bn_relu_rows_kernel) and the conv runs on the direct global -> LDS path (ring kernel, 256 x 256 tiles) instead of transforming on
        // load through registers: 124 -> 83 us for the two 1024-channel blocks, 60 -> ~35 for the 512-channel one (r10d, r10i).
        // The 512-channel block (c_out 256 after it) keeps transform-on-load (measured equal).
        const bool pre = Bk.c_out >= 512;
        if (pre && (rc = bn_relu_rows_launch(X, ld, Bk.tr_s, Bk.tr_t, s.act, Bk.c_out, (int64_t)B * T2, Bk.c_out, st))) return rc;
        // (the pre-activated copy keeps the block buffer's leading dimension)
        MvConv1dDesc d = conv_desc(Bk.transit, pre ? s.act : X, ld, bi < 2 ? s.xb[bi + 1] : s.last, bi < 2 ? blocks[bi + 1].c_out : cfin, B, T2, T2);
        if (pre && (Bk.c_out / 2) % 256 == 0 && (int64_t)B * T2 >= 16384) d.tile = 256;  // 256 x 256 tiles on the ring kernel even where they do not fill the chip (149 tiles for the first transit: r10i)
        d.in_scale = pre ? nullptr : Bk.tr_s;
        d.in_shift = pre ? nullptr : Bk.tr_t;
        d.pad_mode = MV_PAD_ZERO;
        if ((rc = conv1d_launch(d, st))) return rc;
    }
    // out_nonlinear (BN+ReLU) + StatsPool (mean, unbiased std) in one reduction, then dense + BN(affine=False)
    if ((rc = time_stats_launch(s.last, cfin, B, T2, cfin, s.stats, s.stats + cfin, 2 * cfin, 1, 0.0f, st, out_s, out_t)))
        return rc;
    return linear_f32_launch(s.stats, 2 * cfin, dense_w, 2 * cfin, dense_b, MV_ACT_NONE, emb, cfg.embd_dim, B, 2 * cfin,
                             cfg.embd_dim, 0, st);
}

}  // namespace mv

extern "C" {

int mv_campp_create(const MvCamppCfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out) {
    return mv::create_model<mv::CamppModel>("mv_campp_create", cfg, tensors, num_tensors, out);
}

}  // extern "C"
