// Host-side scaffolding shared by what runs conv2ds_kernel on S16 maps: eres2net.hip, resnet_se.hip, res2net.hip, CAM++'s exact head (campp_head.hip).
// The packed-conv record and its packer, the fp32 stem's weights, the launch descriptor builder, the peak word and the reshape -> pooling -> linear head.
// A model file keeps what is its own: block structs, make_block, cfg checks, the carve of its maps, run_block and forward.
#pragma once
#include "kernels.h"
#include "model.h"

namespace mv {

struct S16Conv {
    half_t* w = nullptr;   // split-packed (conv2ds_pack_host)
    float* bias = nullptr;
    float oscale = 0.0f;
    int cin16 = 0, cout16 = 0, ks = 1, stride = 1;
    int cin = 0, cout = 0;  // the layer's own channel counts (algorithmic FLOP accounting)
};

std::vector<int> s16_dense_map(int c);   // channel c at c
// channel c of a [scale * width] tensor lives at (c / width) * wpad + c % width
std::vector<int> s16_grouped_map(int width, int scale, int wpad);

// conv [cout][cin][ks][ks] (its bias optional) followed by BatchNorm `bn` (eps 1e-5; empty: none), folded and packed for conv2ds_kernel:
// out channel c -> row out_pos[c], in channel c -> column in_pos[c], zeros elsewhere.  `who` names the model in the messages.
// bias_host (optional): the uploaded bias [cout16] once more, for a handle that re-uploads it scaled (CAM++'s head gain).
int make_s16_conv_bn(MvModelBase* m, const Weights& w, const char* who, const std::string& conv, const std::string& bn, int cout, int cin, int ks,
                     int stride, const std::vector<int>& out_pos, int cout16, const std::vector<int>& in_pos, int cin16, S16Conv* L,
                     std::vector<float>* bias_host = nullptr);
// channels in their own order, zero rows / columns up to the next multiples of 16
inline int make_s16_conv_bn(MvModelBase* m, const Weights& w, const char* who, const std::string& conv, const std::string& bn, int cout, int cin,
                            int ks, int stride, S16Conv* L, std::vector<float>* bias_host = nullptr) {
    return make_s16_conv_bn(m, w, who, conv, bn, cout, cin, ks, stride, s16_dense_map(cout), (int)round_up(cout, 16), s16_dense_map(cin),
                            (int)round_up(cin, 16), L, bias_host);
}

// conv1 + bn1 of the fp32 VALU stem kernels: conv1.weight [C][taps] times the BN scale, the BN shift as bias
int fold_s16_stem(MvModelBase* m, const Weights& w, const char* who, int C, int taps, float** stem_w, float** stem_b);

// A layer's launch descriptor from what every launch has -- its weights, bias, scale and geometry, x [B, H, W, ldx] and y [B, Ho, Wo, ldy].  A call site
// names what differs (d.x2 / d.cin1, d.res, d.add / d.y2, d.epi, d.peak) and ALWAYS the bounds d.lo / d.hi, then ends in conv2ds_launch(d, stream).
MvConv2dsDesc s16_conv_desc(const S16Conv& L, const float* x, int64_t ldx, float* y, int64_t ldy, int B, int H, int W);

inline int s16_down(int n) { return (n - 1) / 2 + 1; }   // a 3x3 window with padding 1, or a 1x1 one, at stride 2
constexpr size_t S16_SLACK = 64;                         // floats behind every map: the conv loader reads whole 16-byte chunks

// The handle's peak word: largest |64 * value| a launch wanted to store (float bits; sticky, diagnostic only).  Absent on a handle built with
// MV_*_NO_PEAK (0x100) or-ed into the cfg's pooling_type: the launches then run the instantiations without it.
struct S16Peak {
    // *pool_type: pooling_type without the flag, refused unless one of MV_POOL_*
    int create(MvModelBase* m, int cfg_pooling_type, const char* who, int* pool_type);
    int alloc(MvModelBase* m, const char* who);   // the word, cleared: all create() does for a tracked handle (CAM++: no flag, its own info keys)
    int clear() const {   // the word (it must exist) back to 0
        MV_HIP_OK(hipMemset(d_peak, 0, sizeof(unsigned)));
        return MV_OK;
    }
    int raw(float* v) const {   // the word (it must exist) as it stands, as a float; no wait for the device
        unsigned bits = 0;
        MV_HIP_OK(hipMemcpy(&bits, d_peak, sizeof(bits), hipMemcpyDeviceToHost));
        *v = __builtin_bit_cast(float, bits);
        return MV_OK;
    }
    unsigned* word() const { return d_peak; }
    // true: `key` is MV_INFO_S16_PEAK / _SATURATED and *rc, *value are its answer (-1 without a word); waits for the device, not a hot-path call
    bool info(int key, float* value, int* rc) const;

private:
    int read(int key, float* value) const;
    unsigned* d_peak = nullptr;
};

// The tail ResNetSE and Res2Net share: the last map as fp16 rows [B, W, C * H] (x.reshape(B, -1, T')) -> Pooling (model.h) -> bn2 . linear . bn3 folded
struct S16Head {
    struct Ws {
        half_t *rows, *h;
        float *asp_f, *pooled, *lin_ws;
        size_t lin_ws_floats;
    };
    int create(MvModelBase* m, const Weights& w, int pool_type, int final_c, int final_h, int embd_dim);   // ends in a device synchronisation
    Ws carve(Carver& cv, int B, int W) const;
    int forward(const Ws& s, const float* map, int B, int H, int W, float* emb, hipStream_t st) const;

private:
    Pooling pool;
    float* fc_w = nullptr;
    float* fc_b = nullptr;
    int final_c = 0, final_h = 0, embd_dim = 0;
};

}  // namespace mv
