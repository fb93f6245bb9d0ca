// Internal model scaffolding shared by every backbone: model.hip (EcapaTdnn, TDNN), campplus.hip (CAM++, with campp_head.hip and campp_probe.hip) and, through s16model.h, the S16 backbones.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "common.h"

namespace mv {

struct Weights {
    std::map<std::string, MvTensorRef> map;
    int init(const MvTensorRef* tensors, int n);
    bool has(const std::string& name) const;
    int dev(const std::string& name, int64_t numel, const float** out) const;       // device pointer, size-checked
    int host(const std::string& name, int64_t numel, std::vector<float>& out) const;  // host copy, size-checked
};

struct ConvLayer {
    half_t* w = nullptr;    // packed fp16 [Cout_pad][k][Cin_pad]
    float* bias = nullptr;  // [cout] or null
    int cout = 0, cin = 0, k = 1;
    int groups = 1;         // > 1: a native grouped 1x1 layer (conv1d_grouped_native): w packed per group, cin the layer's whole width
};

struct MvModelBase {
    int embd_dim = 0;
    int input_size = 0;
    std::vector<void*> owned;  // device allocations released by the destructor
    virtual ~MvModelBase();
    virtual int workspace_bytes(int B, int T, size_t* bytes) const = 0;
    virtual int forward(const float* feats, int B, int T, float* emb, void* ws, size_t ws_bytes, hipStream_t st) const = 0;
    // model-specific facts for tests and logs (mv_model_info): MV_INFO_* keys; unknown key -> error
    virtual int info(int key, float* value) const;

    void* dev_alloc(size_t bytes);
    float* upload(const std::vector<float>& v);
    int make_conv(const Weights& w, const std::string& weight_name, const std::string& bias_name, int cout, int cin, int k,
                  ConvLayer* out);
    int make_conv_from(const float* dev_w, const Weights* w, const std::string& bias_name, int cout, int cin, int k,
                       ConvLayer* out);
    int make_bn(const Weights& w, const std::string& prefix, int C, float** scale, float** shift);
};

int fold_bn(const Weights& w, const std::string& prefix, int C, std::vector<float>& scale, std::vector<float>& shift,
            float eps);
int fold_final_linear(MvModelBase* m, const Weights& w, const std::string& weight_name, const std::string& bias_name,
                      const std::string& bn_in, const std::string& bn_out, int O, int K, float** wf_out, float** bf_out);

// A layer's conv descriptor from what every layer has -- its weights, bias and geometry, x [B, T_in, ldx] and y [B, T_out, ldy] -- with the models'
// defaults: fp16 in / out, stride 1, dilation 1, no padding (reflect mode), no activations.  A call site names what differs (d.pre_act, d.scale, ...)
// and ends in conv1d_launch(d, stream, L.groups).
MvConv1dDesc conv_desc(const ConvLayer& L, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int T_in, int T_out);

// bump allocator over the caller-provided workspace (256-byte aligned slices)
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* p) : base(static_cast<char*>(p)) {}
    template <typename T>
    T* take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
    size_t total() const { return (off + 255) & ~size_t(255); }
};

// attentive statistics pooling (mvector/models/pooling.py:68-127)
struct AspLayer {
    int C = 0, A = 0;
    bool global_ctx = true;
    ConvLayer tdnn;   // x part of asp.tdnn (A x C)
    float* wms = nullptr;  // [A][2C] fp32: columns of asp.tdnn that multiply [mean; std]
    float* bn_scale = nullptr;
    float* bn_shift = nullptr;
    ConvLayer conv;   // asp.conv (C x A), weights times log2(e); the bias cancels in the softmax over time
    float logit_bound_log2 = -1.0f;  // max_c sum_k |W2[c,k]| * log2(e): bounds every attention logit
    int create(MvModelBase* m, const Weights& w, const std::string& prefix, int C, int A, bool global_ctx);
    size_t workspace_floats(int B, int T) const;
    // have_gstats: fws already holds the global mean | std of x ([B, 2C]) from the producer's fused statistics
    int forward(const half_t* x, int64_t ldx, int B, int T, half_t* h, float* fws, float* pooled, hipStream_t stream,
                bool have_gstats = false) const;
};

// W2 (C x A) of an attention head packed times log2(e), and the bound max_c sum_k |W2[c,k]| * log2(e) of every logit (-1: none)
int make_attention_projection(MvModelBase* m, const Weights& w, const std::string& name, int C, int A, ConvLayer* out, float* bound_log2);

// the other pooling heads of pooling.py (MV_POOL_SAP / _TAP / _TSP) over x [B, T, ldx] fp16 -> pooled fp32 [B, width()]
struct PoolHead {
    static constexpr int SAP_A = 128;   // SelfAttentivePooling's bottleneck: fixed at 128 in both models, not attention_channels
    int type = MV_POOL_TAP;
    int C = 0;
    ConvLayer sap1;                     // SAP linear1 (SAP_A x C, with bias): h = tanh(linear1(x))
    ConvLayer sap2;                     // SAP linear2 (C x SAP_A) times log2(e), bias dropped (it cancels in the softmax over time)
    float logit_bound_log2 = -1.0f;
    int create(MvModelBase* m, const Weights& w, const std::string& prefix, int type, int C);
    int width() const { return type == MV_POOL_TSP ? 2 * C : C; }
    int hidden_width() const { return type == MV_POOL_SAP ? SAP_A : 0; }   // fp16 [B, T, .] scratch the forward needs
    int forward(const half_t* x, int64_t ldx, int B, int T, half_t* h, float* pooled, hipStream_t stream) const;
};

// The pooling head of EcapaTdnn and TDNN, whichever pooling_type (MV_POOL_*) names: x [B, T, ldx] fp16 -> pooled fp32 [B, width()]
struct Pooling {
    int type = MV_POOL_ASP;
    AspLayer asp;     // MV_POOL_ASP
    PoolHead head;    // the other heads
    int create(MvModelBase* m, const Weights& w, const std::string& prefix, int type_, int C, int A, bool global_ctx) {   // A, global_ctx: the ASP's
        type = type_;
        return type == MV_POOL_ASP ? asp.create(m, w, prefix, C, A, global_ctx) : head.create(m, w, prefix, type, C);
    }
    int width() const { return type == MV_POOL_ASP ? 2 * asp.C : head.width(); }
    int hidden_width() const { return type == MV_POOL_ASP ? asp.A : head.hidden_width(); }   // fp16 [B, T, .] scratch the forward needs
    size_t workspace_floats(int B, int T) const { return type == MV_POOL_ASP ? asp.workspace_floats(B, T) : 0; }
    int forward(const half_t* x, int64_t ldx, int B, int T, half_t* h, float* fws, float* pooled, hipStream_t st) const {
        return type == MV_POOL_ASP ? asp.forward(x, ldx, B, T, h, fws, pooled, st) : head.forward(x, ldx, B, T, h, pooled, st);
    }
    // EcapaTdnn's norm behind the head: BatchNorm1d wrapped in a module of the reference's behind ASP, a plain one behind the others (ecapa_tdnn.py:229-250)
    const char* ecapa_bn_name() const { return type == MV_POOL_ASP ? "asp_bn.norm" : "asp_bn"; }
};

// the mv_*_create* entry points: the checks under the entry point's own name `fn`, the state_dict, the model.  pooling_type: the one argument of
// the models whose create() takes a pooling head (its range is checked here), none for the others
template <typename Model, typename Cfg, typename... PoolingType>
int create_model(const char* fn, const Cfg* cfg, const MvTensorRef* tensors, int32_t num_tensors, MvModel** out, PoolingType... pooling_type) {
    static_assert(sizeof...(PoolingType) <= 1, "at most the pooling_type");
    MV_REQUIRE(cfg != nullptr && out != nullptr, std::string(fn) + ": null argument");
    if constexpr (sizeof...(PoolingType) == 1)
        if (const int32_t p = (pooling_type, ...); p < MV_POOL_ASP || p > MV_POOL_TSP)
            return fail(MV_ERR_INVALID_ARGUMENT, std::string(fn) + ": pooling_type " + std::to_string(p) +
                                                     " is not MV_POOL_ASP (0), MV_POOL_SAP (1), MV_POOL_TAP (2) or MV_POOL_TSP (3)");
    int rc;
    Weights w;
    if ((rc = w.init(tensors, num_tensors)) != MV_OK) return rc;
    auto m = std::make_unique<Model>();
    if ((rc = m->create(*cfg, w, pooling_type...)) != MV_OK) return rc;
    *out = reinterpret_cast<MvModel*>(static_cast<MvModelBase*>(m.release()));
    return MV_OK;
}

}  // namespace mv
