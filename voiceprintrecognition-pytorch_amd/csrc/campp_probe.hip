// What CamppModel::create runs once per handle, after the weights are in place (campplus.h): three fixed probe utterances set the exact head's gain,
// decide which head forward() runs (campp_head.hip, "Head precision") and measure the x-vector part's sensitivity to its fp16 operands.
#include "campplus.h"
#include "s16map.h"

namespace mv {

namespace {

constexpr int NPROBE = CamppModel::NPROBE;

void make_probes(int F, std::vector<float> (&feats)[NPROBE]) {
    const int* probe_T = CamppModel::probe_T;
    uint32_t lcg = 0x2545F491u;
    auto uni = [&]() {  // uniform in [-0.5, 0.5)
        lcg = lcg * 1664525u + 1013904223u;
        return (float)(lcg >> 8) / 16777216.0f - 0.5f;
    };
    // probe 0: white, uniform in [-3, 3) -- the scale of mean-normalised log-mel features
    feats[0].resize((size_t)probe_T[0] * F);
    for (float& v : feats[0]) v = uni() * 6.0f;
    // probe 1: white, bell-shaped (sum of four uniforms), standard deviation 2, time mean removed -- what a noise-like recording gives
    feats[1].resize((size_t)probe_T[1] * F);
    for (float& v : feats[1]) v = (uni() + uni() + uni() + uni()) * (2.0f / 0.57735f);
    // probe 2: smooth in time and frequency like voiced audio -- drifting harmonics, a spectral tilt, a voiced / silent alternation, a
    // little noise; standard deviation ~2, time mean removed
    feats[2].resize((size_t)probe_T[2] * F);
    for (int t = 0; t < probe_T[2]; ++t)
        for (int m = 0; m < F; ++m) {
            const double tw = 6.283185307179586;
            const double v = 3.0 * sin(tw * (t / 37.0 + m / 23.0)) + 2.0 * sin(tw * t / 9.3) * ((double)m / F) + 4.0 * (0.5 * F - m) / F +
                             (sin(tw * t / 61.0) > 0.0 ? 3.0 : 0.0) + 1.4 * uni();
            feats[2][(size_t)t * F + m] = (float)(0.7 * v);
        }
    for (int p = 1; p < NPROBE; ++p)  // AudioFeaturizer's time-mean subtraction (featurizer.py:79)
        for (int m = 0; m < F; ++m) {
            double s = 0.0;
            for (int t = 0; t < probe_T[p]; ++t) s += feats[p][(size_t)t * F + m];
            const float mean = (float)(s / probe_T[p]);
            for (int t = 0; t < probe_T[p]; ++t) feats[p][(size_t)t * F + m] -= mean;
        }
}

struct Scratch {  // device buffers of one creation-time function (an input a, an output y, a workspace), freed on every path out of it
    float *a = nullptr, *y = nullptr;
    void* ws = nullptr;
    ~Scratch() {
        hipFree(a);
        hipFree(y);
        hipFree(ws);
    }
};

// the probe utterances and what a forward of one of them needs on the device: features (sc.a), nemb embeddings (sc.y), a workspace for the heads named
struct Probes {
    std::vector<float> feats[NPROBE];
    Scratch sc;
    size_t wsb = 0;
    int create(const CamppModel& m, int nemb, bool f16, bool f32) {
        make_probes(m.cfg.input_size, feats);
        for (int p = 0; p < NPROBE; ++p) {
            if (f16) wsb = std::max(wsb, m.carve(nullptr, 1, CamppModel::probe_T[p], false).bytes);
            if (f32) wsb = std::max(wsb, m.carve(nullptr, 1, CamppModel::probe_T[p], true).bytes);
        }
        MV_HIP_OK(hipMalloc(reinterpret_cast<void**>(&sc.a), (size_t)CamppModel::probe_T[NPROBE - 1] * m.cfg.input_size * sizeof(float)));
        MV_HIP_OK(hipMalloc(reinterpret_cast<void**>(&sc.y), (size_t)nemb * m.cfg.embd_dim * sizeof(float)));
        MV_HIP_OK(hipMalloc(&sc.ws, wsb));
        return MV_OK;
    }
    int upload(int p) {
        MV_HIP_OK(hipMemcpy(sc.a, feats[p].data(), feats[p].size() * sizeof(float), hipMemcpyHostToDevice));
        return MV_OK;
    }
    int forward(const CamppModel& m, int p, float* emb, bool f32) { return m.forward_impl(sc.a, 1, CamppModel::probe_T[p], emb, sc.ws, wsb, nullptr, f32); }
};

float one_minus_cos(const float* a, const float* b, int n) {   // in fp64; 1 where either vector is zero
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int i = 0; i < n; ++i) {
        ab += (double)a[i] * b[i];
        aa += (double)a[i] * a[i];
        bb += (double)b[i] * b[i];
    }
    return (float)(1.0 - ((aa > 0.0 && bb > 0.0) ? ab / sqrt(aa * bb) : 0.0));
}

}  // namespace

// Three fixed probe utterances: they set the exact head's gain (largest stored value 16 x below the S16 saturation point) and, through both
// heads, the largest 1 - cos between the two embeddings decides which head forward() runs (campp_head.hip, header comment).
int CamppModel::choose_head() {
    if (cfg.head_precision == MV_CAMPP_HEAD_F16) {
        head_f32 = false;
        return MV_OK;
    }
    const int D = cfg.embd_dim;
    Probes pr;
    int rc;
    if ((rc = pr.create(*this, 2, true, true))) return rc;
    // ---- the exact head's gain: the probes' largest stored value, 16 x below the saturation point (the measurement repeats at the new gain: a map
    //      clamped upstream makes everything downstream of it read low) ----
    for (int round = 0; round < 8; ++round) {
        if ((rc = head.peak.clear())) return rc;
        for (int p = 0; p < NPROBE; ++p)
            if ((rc = pr.upload(p)) || (rc = pr.forward(*this, p, pr.sc.y, true))) return rc;
        MV_HIP_OK(hipDeviceSynchronize());
        float v = 0.0f;
        if (head.peak.raw(&v) != MV_OK) return MV_ERR_HIP;
        probe_peak = ldexpf(v, head.gain_k) / CS_XSCALE;
        if (!(v > 65504.0f / 16.0f) || head.gain_k >= 96) break;   // (an infinite or NaN peak: nothing a gain repairs)
        int e2 = 0;
        frexpf(v / (65504.0f / 16.0f), &e2);   // v / limit = f * 2^e2, f in [0.5, 1): 2^-e2 brings it to or below the limit
        const int step = std::isfinite(v) ? (e2 > 0 ? e2 : 1) : 16;
        if ((rc = head.set_gain(head.gain_k + step))) return rc;
    }
    if ((rc = head.peak.clear())) return rc;   // from here on the word reports what real inputs do
    if (cfg.head_precision == MV_CAMPP_HEAD_F32) {
        head_f32 = true;
        return MV_OK;
    }
    float worst = 0.0f;
    std::vector<float> e((size_t)2 * D);
    for (int p = 0; p < NPROBE; ++p) {
        if ((rc = pr.upload(p)) || (rc = pr.forward(*this, p, pr.sc.y, false)) || (rc = pr.forward(*this, p, pr.sc.y + D, true))) return rc;
        MV_HIP_OK(hipMemcpy(e.data(), pr.sc.y, e.size() * sizeof(float), hipMemcpyDeviceToHost));
        const float c = one_minus_cos(e.data(), e.data() + D, D);
        probe_calibration[p] = c;
        if (!(c <= worst)) worst = c;  // (a NaN from a non-finite fp16-head embedding sticks)
    }
    calibration = worst;
    head_f32 = !(calibration <= CAMPP_HEAD_THRESHOLD);  // also taken when the fp16 head produced a non-finite embedding
    return head.peak.clear();
}

// ---- x-vector sensitivity (round 6) -----------------------------------------------------------------------------------
// The head probes above compare the two FCM HEADS; a checkpoint whose embedding is sensitive to the 11-bit operands of the x-vector part
// (`campp_c64` seed 31: 3.3e-4 from the fp16 rounding of the x-vector weights alone) passes them unnoticed, and there is no
// exact form of that part to fall back to.  So create() MEASURES it: the x-vector part of the three probe utterances once more in exact fp32
// -- on the very rows the chosen head produced, the caller's fp32 weights in the reference layout as they are, every GEMM on the exact-fp32
// linear kernel (linear.hip, fp32 MFMA), everything else in host loops (a probe, not a path: ~330 small launches and copies, once) -- and
// 1 - cos against the shipped path's embedding of the same probe = what fp16 weights / stored tensors / pre-activation operands of the
// x-vector part cost on that input.  mv_model_info keys MV_INFO_CAMPP_XVEC_PROBE0 + p and MV_INFO_CAMPP_XVEC_SENSITIVITY (the largest) report
// it; mvector/models/campplus.py warns when it exceeds MV_CAMPP_XVEC_WARN.  Reference arithmetic: campplus.py:94-181,186-189,27-33.
// rows [T][32 * F8] in OUR channel order f * 32 + c (the chosen head's fp16 output as floats) -> emb [D], exact fp32
int CamppModel::xvector_exact(const Weights& w, const std::vector<float>& rows, int T, std::vector<float>& emb) const {
    const int cin0 = 32 * F8, G = cfg.growth_rate, D = cfg.embd_dim;
    const int T2 = (T - 1) / 2 + 1;
    Scratch sc;
    const size_t na = (size_t)T2 * std::max(5 * cin0, 1024 + 32 * 24), ny = (size_t)T2 * 1024;
    MV_HIP_OK(hipMalloc(reinterpret_cast<void**>(&sc.a), na * sizeof(float)));
    MV_HIP_OK(hipMalloc(reinterpret_cast<void**>(&sc.y), ny * sizeof(float)));
    auto gemm = [&](const std::vector<float>& A, int n, int K, const float* Wdev, const float* bias_dev, int O, std::vector<float>& Y) -> int {
        if ((size_t)n * K > na || (size_t)n * O > ny) return fail(MV_ERR_UNSUPPORTED, "campp x-vector probe: scratch too small");
        MV_HIP_OK(hipMemcpy(sc.a, A.data(), (size_t)n * K * sizeof(float), hipMemcpyHostToDevice));
        const int rc = linear_f32_launch(sc.a, K, Wdev, K, bias_dev, MV_ACT_NONE, sc.y, O, n, K, O, 0, nullptr);
        if (rc != MV_OK) return rc;
        Y.resize((size_t)n * O);
        MV_HIP_OK(hipMemcpy(Y.data(), sc.y, Y.size() * sizeof(float), hipMemcpyDeviceToHost));
        return MV_OK;
    };
    int rc;
    std::vector<float> s, t, A, Y;
    // tdnn: k = 5, stride 2, zero padding 2 on the reference's channel order c * F8 + f, then BN, ReLU (campplus.py:319-326)
    const float* Wd = nullptr;
    if ((rc = w.dev("xvector.tdnn.linear.weight", (int64_t)cfg.init_channels * cin0 * 5, &Wd))) return rc;
    A.assign((size_t)T2 * cin0 * 5, 0.0f);
    for (int t2 = 0; t2 < T2; ++t2)
        for (int j = 0; j < 5; ++j) {
            const int ti = 2 * t2 + j - 2;
            if (ti < 0 || ti >= T) continue;
            for (int c = 0; c < 32; ++c)
                for (int f = 0; f < F8; ++f) A[((size_t)t2 * cin0 + (c * F8 + f)) * 5 + j] = rows[(size_t)ti * cin0 + f * 32 + c];
        }
    if ((rc = gemm(A, T2, cin0 * 5, Wd, nullptr, cfg.init_channels, Y))) return rc;
    if ((rc = fold_bn(w, "xvector.tdnn.nonlinear.batchnorm", cfg.init_channels, s, t, 1e-5f))) return rc;
    std::vector<float> X, Xn;
    int ld = blocks[0].c_out;
    X.assign((size_t)T2 * ld, 0.0f);
    for (int i = 0; i < T2; ++i)
        for (int c = 0; c < cfg.init_channels; ++c) X[(size_t)i * ld + c] = std::max(0.0f, Y[(size_t)i * cfg.init_channels + c] * s[c] + t[c]);
    const int nseg = (T2 + 99) / 100;
    for (int bi = 0; bi < 3; ++bi) {
        const Block& Bk = blocks[bi];
        ld = Bk.c_out;
        for (size_t li = 0; li < Bk.layers.size(); ++li) {
            const int cin = Bk.layers[li].cin;
            const std::string p = "xvector.block" + std::to_string(bi + 1) + ".tdnnd" + std::to_string(li + 1);
            std::vector<float> s2, t2v, wa, ba, wb, bb, H, h((size_t)T2 * bn_ch);
            if ((rc = fold_bn(w, p + ".nonlinear1.batchnorm", cin, s, t, 1e-5f)) || (rc = fold_bn(w, p + ".nonlinear2.batchnorm", bn_ch, s2, t2v, 1e-5f)))
                return rc;
            A.resize((size_t)T2 * cin);
            for (int i = 0; i < T2; ++i)
                for (int c = 0; c < cin; ++c) A[(size_t)i * cin + c] = std::max(0.0f, X[(size_t)i * ld + c] * s[c] + t[c]);
            if ((rc = w.dev(p + ".linear1.weight", (int64_t)bn_ch * cin, &Wd)) || (rc = gemm(A, T2, cin, Wd, nullptr, bn_ch, H))) return rc;
            for (int i = 0; i < T2; ++i)
                for (int c = 0; c < bn_ch; ++c) h[(size_t)i * bn_ch + c] = std::max(0.0f, H[(size_t)i * bn_ch + c] * s2[c] + t2v[c]);
            // context = mean over time + mean over the frame's 100-frame segment (ceil mode: the last segment averages its own frames)
            if ((rc = w.host(p + ".cam_layer.linear1.weight", (int64_t)(bn_ch / 2) * bn_ch, wa)) || (rc = w.host(p + ".cam_layer.linear1.bias", bn_ch / 2, ba)) ||
                (rc = w.host(p + ".cam_layer.linear2.weight", (int64_t)G * (bn_ch / 2), wb)) || (rc = w.host(p + ".cam_layer.linear2.bias", G, bb)))
                return rc;
            std::vector<double> gmean(bn_ch, 0.0);
            for (int i = 0; i < T2; ++i)
                for (int c = 0; c < bn_ch; ++c) gmean[c] += h[(size_t)i * bn_ch + c];
            std::vector<float> gate((size_t)nseg * G);
            for (int sg = 0; sg < nseg; ++sg) {
                const int lo = sg * 100, hi = std::min(T2, lo + 100);
                std::vector<double> ctx(bn_ch, 0.0), g1(bn_ch / 2);
                for (int i = lo; i < hi; ++i)
                    for (int c = 0; c < bn_ch; ++c) ctx[c] += h[(size_t)i * bn_ch + c];
                for (int c = 0; c < bn_ch; ++c) ctx[c] = (double)((float)(ctx[c] / (hi - lo)) + (float)(gmean[c] / T2));
                for (int o = 0; o < bn_ch / 2; ++o) {
                    double acc = ba[o];
                    for (int c = 0; c < bn_ch; ++c) acc += (double)wa[(size_t)o * bn_ch + c] * ctx[c];
                    g1[o] = acc > 0.0 ? acc : 0.0;
                }
                for (int o = 0; o < G; ++o) {
                    double acc = bb[o];
                    for (int c = 0; c < bn_ch / 2; ++c) acc += (double)wb[(size_t)o * (bn_ch / 2) + c] * g1[c];
                    gate[(size_t)sg * G + o] = (float)(1.0 / (1.0 + exp(-acc)));
                }
            }
            // k = 3 dilated conv, zero padding: columns ci * 3 + j as the reference weight [G][bn_ch][3] has them
            A.assign((size_t)T2 * bn_ch * 3, 0.0f);
            for (int i = 0; i < T2; ++i)
                for (int j = 0; j < 3; ++j) {
                    const int ti = i + (j - 1) * Bk.dil;
                    if (ti < 0 || ti >= T2) continue;
                    for (int c = 0; c < bn_ch; ++c) A[((size_t)i * bn_ch + c) * 3 + j] = h[(size_t)ti * bn_ch + c];
                }
            if ((rc = w.dev(p + ".cam_layer.linear_local.weight", (int64_t)G * bn_ch * 3, &Wd)) || (rc = gemm(A, T2, bn_ch * 3, Wd, nullptr, G, Y))) return rc;
            for (int i = 0; i < T2; ++i)
                for (int o = 0; o < G; ++o) X[(size_t)i * ld + cin + o] = Y[(size_t)i * G + o] * gate[(size_t)(i / 100) * G + o];
        }
        const std::string tp = "xvector.transit" + std::to_string(bi + 1);
        if ((rc = fold_bn(w, tp + ".nonlinear.batchnorm", ld, s, t, 1e-5f))) return rc;
        A.resize((size_t)T2 * ld);
        for (int i = 0; i < T2; ++i)
            for (int c = 0; c < ld; ++c) A[(size_t)i * ld + c] = std::max(0.0f, X[(size_t)i * ld + c] * s[c] + t[c]);
        const float* bias_dev = nullptr;
        if (w.has(tp + ".linear.bias") && (rc = w.dev(tp + ".linear.bias", ld / 2, &bias_dev))) return rc;
        if ((rc = w.dev(tp + ".linear.weight", (int64_t)(ld / 2) * ld, &Wd)) || (rc = gemm(A, T2, ld, Wd, bias_dev, ld / 2, Y))) return rc;
        const int ldn = bi < 2 ? blocks[bi + 1].c_out : cfin;
        Xn.assign((size_t)T2 * ldn, 0.0f);
        for (int i = 0; i < T2; ++i)
            for (int c = 0; c < ld / 2; ++c) Xn[(size_t)i * ldn + c] = Y[(size_t)i * (ld / 2) + c];
        X.swap(Xn);
    }
    // out_nonlinear (BN, ReLU) -> mean | unbiased std over time -> dense + BN(affine = False) (folded at create: dense_w / dense_b, exact fp32)
    if ((rc = fold_bn(w, "xvector.out_nonlinear.batchnorm", cfin, s, t, 1e-5f))) return rc;
    std::vector<float> stats((size_t)2 * cfin);
    for (int c = 0; c < cfin; ++c) {
        double m = 0.0, q = 0.0;
        for (int i = 0; i < T2; ++i) m += std::max(0.0f, X[(size_t)i * cfin + c] * s[c] + t[c]);
        m /= T2;
        for (int i = 0; i < T2; ++i) {
            const double d = (double)std::max(0.0f, X[(size_t)i * cfin + c] * s[c] + t[c]) - m;
            q += d * d;
        }
        stats[c] = (float)m;
        stats[cfin + c] = (float)sqrt(q / (T2 - 1));
    }
    MV_HIP_OK(hipMemcpy(sc.a, stats.data(), stats.size() * sizeof(float), hipMemcpyHostToDevice));
    if ((rc = linear_f32_launch(sc.a, 2 * cfin, dense_w, 2 * cfin, dense_b, MV_ACT_NONE, sc.y, D, 1, 2 * cfin, D, 0, nullptr))) return rc;
    emb.resize(D);
    MV_HIP_OK(hipMemcpy(emb.data(), sc.y, (size_t)D * sizeof(float), hipMemcpyDeviceToHost));
    return MV_OK;
}

int CamppModel::probe_xvector(const Weights& w) {
    const int D = cfg.embd_dim, cin0 = 32 * F8;
    Probes pr;
    int rc;
    if ((rc = pr.create(*this, 1, !head_f32, head_f32))) return rc;
    float worst = 0.0f;
    for (int p = 0; p < NPROBE; ++p) {
        const int T = probe_T[p];
        if ((rc = pr.upload(p)) || (rc = pr.forward(*this, p, pr.sc.y, head_f32))) return rc;
        std::vector<float> e(D), ex;
        std::vector<half_t> rows16((size_t)T * cin0);
        MV_HIP_OK(hipMemcpy(e.data(), pr.sc.y, (size_t)D * sizeof(float), hipMemcpyDeviceToHost));
        MV_HIP_OK(hipMemcpy(rows16.data(), carve(pr.sc.ws, 1, T, head_f32).rows, rows16.size() * sizeof(half_t), hipMemcpyDeviceToHost));
        std::vector<float> rows(rows16.size());
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = (float)rows16[i];
        if ((rc = xvector_exact(w, rows, T, ex))) return rc;
        const float c = one_minus_cos(e.data(), ex.data(), D);
        xvec_probe[p] = c;
        if (!(c <= worst)) worst = c;
    }
    xvec_sensitivity = worst;
    return head.peak.clear();   // (the probes are not the caller's inputs)
}

}  // namespace mv
