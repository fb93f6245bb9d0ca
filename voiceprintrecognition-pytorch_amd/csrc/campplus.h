// CAM++: the handle and its FCM head, declared for the three files that define them -- campplus.hip (the x-vector part, workspace, forward),
// campp_head.hip (both forms of the head), campp_probe.hip (what runs only inside create(): probes, gain search, head choice, x-vector sensitivity).
#pragma once
#include "s16model.h"

namespace mv {

// The FCM head in its two forms (campp_head.hip, "Head precision"): fp16 maps through fcm.hip / fcmblock.hip, or exact through conv2ds.hip.
struct CamppHead {
    struct FcmConv {            // fp16 head
        half_t* w = nullptr;    // [ntaps][32][32], BN folded
        float* bias = nullptr;
        int ntaps = 9;
    };
    struct ResBlock {
        FcmConv conv1, conv2;   // conv2 carries the shortcut tap when the block has one
        S16Conv x1, x2, xsc;    // the exact head's records of the same convs, the shortcut conv (1x1) on its own
        bool has_shortcut = false;
        int stride = 1;
    };
    struct Maps {
        float *f0, *fa, *fb, *fc;  // exact head: the full-resolution map and three half-resolution ones
        half_t *m0, *m1, *m2;      // fp16 head: FCM maps (ping-pong)
    };
    int F = 0, F8 = 0;
    // head.conv1 (+ bn1) in its three forms
    float* c1_w = nullptr;   // [32][9] fp32 (BN folded)
    float* c1_b = nullptr;
    half_t* c1_a = nullptr;  // the same weights as MFMA fragments (fcm_c1_pack): first conv inside the first block's kernel
    float *c1_wx = nullptr, *c1_bx = nullptr;   // the exact head's: c1_w / c1_b times the gain
    ResBlock res[4];
    FcmConv out;
    S16Conv outx;
    // Range of the exact head.  S16 maps hold 64 * value in fp16 pairs and saturate at |value| = 1023.5 -- 64 x less than the fp16 head's maps, on
    // exactly the checkpoints (large BatchNorm gains) the exact head exists for.  The head is positively homogeneous (conv + folded BN + ReLU,
    // residual sums): run on gain * x with every bias times gain it produces gain * maps, exactly for a power of two.  create() measures the
    // largest stored value on the probe utterances (MvConv2dsDesc.peak) and picks gain = 2^-k so that it sits 16 x below the saturation point;
    // the first conv's weights / bias and the biases of the exact head carry the gain, the rows handed to the TDNN are multiplied by 2^k.
    int gain_k = 0;
    struct Gained { float* dev; std::vector<float> host; };   // host: unscaled (set_gain uploads it times the gain)
    std::vector<Gained> gained;    // c1_wx, c1_bx and every exact conv's bias
    S16Peak peak;   // largest |64 * gain * value| an exact-head launch wanted to store (sticky, diagnostic only)

    int create(MvModelBase* m, const Weights& w, int input_size);
    int set_gain(int k);   // the exact head's first conv and biases times gain = 2^-k
    // both: feats [B, T, F] fp32 -> rows fp16 [B, T, F8, 32]
    int forward_f16(const float* feats, int B, int T, const Maps& s, half_t* rows, hipStream_t st) const;
    int forward_exact(const float* feats, int B, int T, const Maps& s, half_t* rows, hipStream_t st) const;
};

struct CamppModel : MvModelBase {
    MvCamppCfg cfg;
    CamppHead head;
    // xvector
    ConvLayer tdnn;
    float *tdnn_scale = nullptr, *tdnn_shift = nullptr;
    struct DenseLayer {
        int cin;
        float *bn1_s, *bn1_t, *bn2_s, *bn2_t;
        ConvLayer lin1, local;
        float *wa, *ba, *wb, *bb;  // context FCs 128 -> 64 -> 32 (fp32)
    };
    struct Block {
        int c_in, c_out, dil;
        std::vector<DenseLayer> layers;
        float *tr_s, *tr_t;  // transit BN
        ConvLayer transit;
        MvCamLayerDesc* descs = nullptr;  // device array for cam_dense_block_kernel
        std::vector<MvCamLayerDesc> hdescs;  // the same on the host: what the per-layer forms are launched from
    };
    Block blocks[3];
    float *out_s = nullptr, *out_t = nullptr;
    float *dense_w = nullptr, *dense_b = nullptr;
    int F8 = 0, bn_ch = 0, cfin = 0;
    // what create() measured on the probe utterances (campp_probe.hip)
    static constexpr int NPROBE = 3;
    static constexpr int probe_T[NPROBE] = {96, 150, 200};
    static constexpr float CAMPP_HEAD_THRESHOLD = 5e-6f;
    float probe_peak = 0.0f;        // the largest head activation over the probe utterances (real units), what the gain was chosen from
    bool head_f32 = false;          // which head forward() runs (decided in create())
    float calibration = -1.0f;      // largest 1 - cos between the two heads over the probe utterances (-1: forced by MvCamppCfg.head_precision)
    float probe_calibration[NPROBE] = {-1.0f, -1.0f, -1.0f};
    float xvec_probe[NPROBE] = {-1.0f, -1.0f, -1.0f};
    float xvec_sensitivity = -1.0f;   // -1: not measured (MvCamppCfg.xvector_probe = MV_CAMPP_XVEC_PROBE_OFF)

    struct Ws {
        CamppHead::Maps maps;
        half_t* rows;          // [B, T, 32*F8]
        half_t* xb[3];         // dense-block buffers [B, T2, c_out]
        half_t* last;          // [B, T2, cfin]
        half_t* h;             // [B, T2, 128]
        half_t* act;           // [B, T2, widest block]: pre-activated transit input
        float *ctx, *g1, *gate, *stats;
        float* hpart;          // long utterances: time sums of h per (utterance, 160-frame chunk, segment inside the chunk)
        size_t bytes;
        int T2, nseg;
    };

    int create(const MvCamppCfg& c, const Weights& w);
    int info(int key, float* value) const override;
    Ws carve(void* base, int B, int T, bool f32) const;
    int workspace_bytes(int B, int T, size_t* bytes) const override;
    int forward(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st) const override {
        return forward_impl(feats, B, T, emb, ws, ws_bytes, st, head_f32);
    }
    int forward_impl(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st, bool f32) const;
    int five_launches(const Block& Bk, half_t* X, const Ws& s, int B, int li, hipStream_t st) const;
    // campp_probe.hip
    int choose_head();
    int probe_xvector(const Weights& w);
    int xvector_exact(const Weights& w, const std::vector<float>& rows, int T, std::vector<float>& emb) const;
};

}  // namespace mv
