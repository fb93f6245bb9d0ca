// SphereFace2: a logistic loss over every column of the [B, N] cosine matrix with a learnable bias, as one streaming forward and one element-wise
// backward.  The contract -- the fp32 front, what is fp64 behind it, the summation order, what `saved` holds -- is in include/mvector_hip.h.
//
// Forward, two ordinary launches, no workgroup waits for another:
//   sf2_seg_kernel      grid (B * segments): the segment's sum of the column losses and of the column weights in fp64, and its best cosine (`pred`)
//   sf2_finish_kernel   one workgroup: a thread per row adds the segments in order and writes loss_rows / pred / saved; thread 0 adds the rows
// Backward, one launch: sf2_backward_kernel, element-wise, a thread per chunk of MV_MARGIN_CHUNK columns; one more workgroup at the end of the
//   grid adds the rows' weight sums of `saved` in order for the bias gradient.
//
// The segments, the chunks a thread owns and the two load paths (16-byte pieces on a row that starts on a 16-byte boundary, elements otherwise)
// are those of marginloss.hip: the same values reach the same threads whichever path ran.
#include "kernels.h"
#include "loss_elem.h"

namespace mv {

constexpr int SF_T = 256;                                  // threads of every workgroup here
constexpr int SF_CH = MV_MARGIN_CHUNK;                     // columns per chunk
constexpr int SF_SEG_CHUNKS = MV_MARGIN_SEG / SF_CH;       // chunks per segment
static_assert(MV_MARGIN_SEG % SF_CH == 0 && SF_SEG_CHUNKS % SF_T == 0, "a segment is a whole number of chunks per thread");
static_assert(SF_CH == 8, "a chunk is two (fp32) or one (16-bit) 16-byte pieces");

struct SfArgs {
    MvSphereFace2Cfg c;
    const void* logits;
    const int64_t* labels;
    const float* bias;
    int64_t stride;
    int B, N, nseg;
    uint32_t zero;   // always 0, and no compiler can know it: see sf_mul
};

// ---- the front: fp32, one operation at a time
// The fp32 product rounded on its own.  hipcc honours the contraction pragma below; a host compiler under -ffp-contract=fast (the test-suite's
// emulator build) fuses a product with the sum behind it whatever the pragma says.  So the product's bits pass through an integer OR with
// SfArgs::zero, a kernel argument that is always 0: the sum behind it then has no product to fuse with.  (A word derived from the configuration,
// as in marginloss.hip, does not do here: inside `if (margin_type == A)` the compiler knows margin_type.)
__device__ __forceinline__ float sf_mul(float a, float b, uint32_t zero) {
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, a * b) | zero);
}

struct SfFront {
    float z;   // zp at the target, zn elsewhere
    float h;   // (x + 1) / 2 of the argument x of g
};
// cj: the column's cosine; only the branch the column needs is formed (selects, no branch: the target is one lane's case)
__device__ __forceinline__ SfFront sf_front(const MvSphereFace2Cfg& c, float cj, bool is_target, float bias, uint32_t zero) {
#pragma clang fp contract(off)
    float x = cj;
    if (c.margin_type == MV_SF2_TYPE_A) {
        const float sq = sf_mul(cj, cj, zero);
        const float sine = sqrtf(1.0f - sq);
        const float a = sf_mul(cj, c.cos_m, zero);
        const float bb = sf_mul(sine, c.sin_m, zero);
        const float toward = cj > c.th ? a - bb : cj - c.mmm;
        const float away = a + bb;
        x = is_target ? toward : away;
    }
    SfFront f;
    f.h = (x + 1.0f) / 2.0f;
    float pw = f.h;
    for (int i = 1; i < c.t; ++i) pw = sf_mul(pw, f.h, zero);
    float g = 2.0f * pw - 1.0f;     // 2 * pw is exact: fused or not, one rounding
    if (c.margin_type == MV_SF2_TYPE_C) g = is_target ? g - c.margin : g + c.margin;
    f.z = sf_mul(c.scale, g, zero) + bias;
    return f;
}

// ---- behind the front: fp64.  x = -zp at the target, zn elsewhere; wgt = lambda at the target, 1 - lambda elsewhere.
// softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigma(x) share the one exp; a NaN x gives NaN in both
struct SfTerm {
    double l;   // wgt * softplus(x)
    double w;   // -lambda * sigma(-zp) at the target, (1 - lambda) * sigma(zn) elsewhere
};
__device__ __forceinline__ SfTerm sf_term(const MvSphereFace2Cfg& c, float z, bool is_target) {
    const double lam = (double)c.lanbuda;
    const double x = is_target ? -(double)z : (double)z;
    const double wgt = is_target ? lam : 1.0 - lam;
    const double e = exp(-fabs(x));
    const double sig = (x >= 0.0 ? 1.0 : e) / (1.0 + e);
    SfTerm t;
    t.l = wgt * ((x > 0.0 ? x : 0.0) + log1p(e));
    t.w = (is_target ? -wgt : wgt) * sig;
    return t;
}

// the chunk of SF_CH columns from j0 on (entries at or beyond N are not touched and hold 0)
template <class T>
__device__ __forceinline__ void sf_load_chunk(const T* row, int j0, int N, bool vec, float (&c)[SF_CH]) {
    if (vec && j0 + SF_CH <= N) {
        MlElem<T>::template ldv<SF_CH>(row + j0, c);
        return;
    }
#pragma unroll
    for (int g = 0; g < SF_CH; ++g) c[g] = j0 + g < N ? MlElem<T>::ld(row + j0 + g) : 0.0f;
}

// the rule of `pred` (mv_margin_ce_forward's): the largest cosine, the lowest column on ties, a NaN is never chosen
__device__ __forceinline__ bool sf_better(float c, int j, float cb, int jb) { return c > cb || (c == cb && j < jb); }

// the label of row b, -1 when it is outside [0, N)
__device__ __forceinline__ int sf_label(const SfArgs& a, int b) {
    const int64_t y = a.labels[b];
    return y >= 0 && y < (int64_t)a.N ? (int)y : -1;
}

// grid (B * nseg).  segl / segw [B, nseg] <- the segment's sum of l_j and of w_j; segc / segj <- its largest cosine and that column
template <class T>
__global__ __launch_bounds__(SF_T) void sf2_seg_kernel(SfArgs a, double* segl, double* segw, float* segc, int* segj) {
    __shared__ double redl[SF_T];
    __shared__ double redw[SF_T];
    __shared__ float redc[SF_T];
    __shared__ int redj[SF_T];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.nseg), seg = (int)(blockIdx.x - (unsigned)b * (unsigned)a.nseg);
    const T* row = static_cast<const T*>(a.logits) + (int64_t)b * a.stride;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int y = sf_label(a, b);
    const float bias = a.bias[0];
    float cb = -__builtin_inff();
    int jb = 0x7FFFFFFF;
    double sl = 0.0, sw = 0.0;
#pragma unroll 1
    for (int ch = tid; ch < SF_SEG_CHUNKS; ch += SF_T) {
        const int64_t j0l = (int64_t)seg * MV_MARGIN_SEG + (int64_t)ch * SF_CH;
        if (j0l >= a.N) break;
        const int j0 = (int)j0l;
        float c[SF_CH];
        sf_load_chunk<T>(row, j0, a.N, vec, c);
#pragma unroll
        for (int g = 0; g < SF_CH; ++g) {
            const int j = j0 + g;
            if (j < a.N) {
                const bool is_target = j == y;
                const SfTerm t = sf_term(a.c, sf_front(a.c, c[g], is_target, bias, a.zero).z, is_target);
                sl += t.l;
                sw += t.w;
                if (sf_better(c[g], j, cb, jb)) cb = c[g], jb = j;
            }
        }
    }
    redl[tid] = sl;
    redw[tid] = sw;
    redc[tid] = cb;
    redj[tid] = jb;
    __syncthreads();
#pragma unroll 1
    for (int h = SF_T / 2; h > 0; h >>= 1) {
        if (tid < h) {
            redl[tid] += redl[tid + h];
            redw[tid] += redw[tid + h];
            if (sf_better(redc[tid + h], redj[tid + h], redc[tid], redj[tid])) redc[tid] = redc[tid + h], redj[tid] = redj[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = (int64_t)b * a.nseg + seg;
        segl[o] = redl[0];
        segw[o] = redw[0];
        segc[o] = redc[0];
        segj[o] = redj[0];
    }
}

// one workgroup.  Thread t finishes the rows t, t + 256, ...; thread 0 then adds the rows' losses in ascending b.
__global__ __launch_bounds__(SF_T) void sf2_finish_kernel(SfArgs a, const double* segl, const double* segw, const float* segc, const int* segj,
                                                          float* loss, float* loss_rows, int32_t* pred, double* saved) {
    const int tid = threadIdx.x;
    for (int b = tid; b < a.B; b += SF_T) {
        float cb = -__builtin_inff();
        int jb = 0x7FFFFFFF;
        double L = 0.0, W = 0.0;
        for (int i = 0; i < a.nseg; ++i) {
            const int64_t o = (int64_t)b * a.nseg + i;
            L += segl[o];
            W += segw[o];
            if (sf_better(segc[o], segj[o], cb, jb)) cb = segc[o], jb = segj[o];
        }
        if (sf_label(a, b) < 0) L = W = (double)__builtin_nanf("");
        loss_rows[b] = (float)L;
        pred[b] = jb == 0x7FFFFFFF ? 0 : jb;
        saved[(int64_t)b * MV_SF2_SAVED] = L;
        saved[(int64_t)b * MV_SF2_SAVED + 1] = W;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int b = 0; b < a.B; ++b) total += saved[(int64_t)b * MV_SF2_SAVED];
        loss[0] = (float)(total / (double)a.B);
    }
}

// grid (B * tiles + 1), a tile = SF_T chunks.  A thread reads its chunk, then writes it: out may be the logits themselves.  The last workgroup
// writes the bias gradient.
template <class T>
__global__ __launch_bounds__(SF_T) void sf2_backward_kernel(SfArgs a, const double* saved, const float* grad_out, T* out, int64_t out_stride,
                                                            float* bias_grad, int tiles) {
    const double gB = (double)grad_out[0] / (double)a.B;
    if (blockIdx.x == (unsigned)a.B * (unsigned)tiles) {
        if (threadIdx.x == 0) {
            double W = 0.0;
            for (int b = 0; b < a.B; ++b) W += saved[(int64_t)b * MV_SF2_SAVED + 1];
            bias_grad[0] = (float)(gB * W);
        }
        return;
    }
    const int b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles);
    const int64_t j0l = ((int64_t)tile * SF_T + threadIdx.x) * SF_CH;
    if (j0l >= a.N) return;
    const int j0 = (int)j0l;
    const T* row = static_cast<const T*>(a.logits) + (int64_t)b * a.stride;
    T* orow = out + (int64_t)b * out_stride;
    const bool vec = ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(orow)) & 15) == 0;
    const int y = sf_label(a, b);
    const float bias = a.bias[0];
    const double st = (double)a.c.scale * (double)a.c.t;
    const double cos_m = (double)a.c.cos_m, sin_m = (double)a.c.sin_m;
    float c[SF_CH];
    sf_load_chunk<T>(row, j0, a.N, vec, c);
    float val[SF_CH];
#pragma unroll
    for (int g = 0; g < SF_CH; ++g) {
        const bool is_target = j0 + g == y;
        const SfFront f = sf_front(a.c, c[g], is_target, bias, a.zero);
        const SfTerm t = sf_term(a.c, f.z, is_target);
        double hp = 1.0;
        for (int i = 1; i < a.c.t; ++i) hp *= (double)f.h;
        double dx = 1.0;
        if (a.c.margin_type == MV_SF2_TYPE_A) {
            const double cd = (double)c[g];
            const double q = cd * sin_m / sqrt(1.0 - cd * cd);
            dx = is_target ? (c[g] > a.c.th ? cos_m + q : 1.0) : cos_m - q;
        }
        val[g] = y < 0 ? __builtin_nanf("") : (float)(gB * t.w * (st * hp * dx));
    }
    if (vec && j0 + SF_CH <= a.N) {
        MlElem<T>::template stv<SF_CH>(orow + j0, val);
        return;
    }
#pragma unroll
    for (int g = 0; g < SF_CH; ++g)
        if (j0 + g < a.N) MlElem<T>::st(orow + j0 + g, val[g]);
}

// ---- host side
static int64_t sf2_segments(int64_t N) { return N > 0 ? (N + MV_MARGIN_SEG - 1) / MV_MARGIN_SEG : 0; }

static size_t sf2_ws_bytes(int64_t B, int64_t N) { return (size_t)round_up(B * sf2_segments(N) * (8 + 8 + 4 + 4), 16); }

// what forward and backward check alike; B == 0 is decided by the caller in front of the pointer checks
static int sf2_check(const char* who, const MvSphereFace2Cfg* cfg, int32_t dtype, int64_t B, int64_t N, int64_t stride) {
    const std::string w(who);
    if (cfg == nullptr) return fail(MV_ERR_INVALID_ARGUMENT, w + ": null cfg");
    if (B < 0 || N < 0) return fail(MV_ERR_INVALID_ARGUMENT, w + ": negative B or N");
    if (cfg->margin_type != MV_SF2_TYPE_C && cfg->margin_type != MV_SF2_TYPE_A)
        return fail(MV_ERR_INVALID_ARGUMENT, w + ": unknown margin_type (MV_SF2_TYPE_C or MV_SF2_TYPE_A)");
    if (cfg->t < 1 || cfg->t > MV_SF2_MAX_T) return fail(MV_ERR_INVALID_ARGUMENT, w + ": t outside 1 .. 8");
    if (!(cfg->lanbuda >= 0.0f && cfg->lanbuda <= 1.0f)) return fail(MV_ERR_INVALID_ARGUMENT, w + ": lanbuda outside [0, 1]");
    if (dtype != MV_DT_F32 && dtype != MV_DT_F16 && dtype != MV_DT_BF16)
        return fail(MV_ERR_INVALID_ARGUMENT, w + ": unknown dtype (MV_DT_F32, MV_DT_F16 or MV_DT_BF16)");
    if (N > (int64_t)0x7FFFFFFF) return fail(MV_ERR_INVALID_ARGUMENT, w + ": N above 2^31 - 1");
    if (stride < N) return fail(MV_ERR_INVALID_ARGUMENT, w + ": stride below N");
    if (B > 0 && stride > 0 && B > INT64_MAX / 8 / stride) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B * stride beyond int64");
    if (B > 0x7FFFFFFF) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B above 2^31 - 1");
    if (B > 0 && N == 0) return fail(MV_ERR_INVALID_ARGUMENT, w + ": N = 0 (no classes) with B > 0");
    if (B > 0 && sf2_segments(N) > (int64_t)0x7FFFFFFF / B) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B * segments above 2^31 - 1");
    return MV_OK;
}

static SfArgs sf2_args(const MvSphereFace2Cfg* cfg, const void* logits, const int64_t* labels, const float* bias, int64_t B, int64_t N,
                       int64_t stride) {
    SfArgs a;
    a.c = *cfg;
    a.logits = logits;
    a.labels = labels;
    a.bias = bias;
    a.stride = stride;
    a.B = (int)B;
    a.N = (int)N;
    a.nseg = (int)sf2_segments(N);
    a.zero = 0;
    return a;
}

#define SF_DISPATCH(FN, ...)                                     \
    do {                                                         \
        if (dtype == MV_DT_F32) FN<float>(__VA_ARGS__);          \
        else if (dtype == MV_DT_F16) FN<half_t>(__VA_ARGS__);    \
        else FN<bf16_t>(__VA_ARGS__);                            \
    } while (0)

template <class T>
static void sf2_forward_launch(const SfArgs& a, double* segl, double* segw, float* segc, int* segj, float* loss, float* loss_rows, int32_t* pred,
                               double* saved, hipStream_t st) {
    MV_LAUNCH((sf2_seg_kernel<T>), ((unsigned)a.B * (unsigned)a.nseg, 1, 1), (SF_T, 1, 1), 0, st, a, segl, segw, segc, segj);
    MV_LAUNCH(sf2_finish_kernel, (1, 1, 1), (SF_T, 1, 1), 0, st, a, (const double*)segl, (const double*)segw, (const float*)segc, (const int*)segj,
              loss, loss_rows, pred, saved);
}

template <class T>
static void sf2_backward_launch(const SfArgs& a, const double* saved, const float* grad_out, void* out, int64_t out_stride, float* bias_grad,
                                hipStream_t st) {
    const int tiles = (int)ceil_div(ceil_div(a.N, SF_CH), SF_T);
    MV_LAUNCH((sf2_backward_kernel<T>), ((unsigned)a.B * (unsigned)tiles + 1u, 1, 1), (SF_T, 1, 1), 0, st, a, saved, grad_out, static_cast<T*>(out),
              out_stride, bias_grad, tiles);
}

}  // namespace mv

extern "C" size_t mv_sphereface2_workspace_bytes(int64_t B, int64_t N) {
    if (B <= 0 || N <= 0 || N > (int64_t)0x7FFFFFFF || B > 0x7FFFFFFF || mv::sf2_segments(N) > (int64_t)0x7FFFFFFF / B) return 0;
    return mv::sf2_ws_bytes(B, N);
}

extern "C" int mv_sphereface2_forward(const MvSphereFace2Cfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, const float* bias,
                                      int64_t B, int64_t N, int64_t stride, float* loss, float* loss_rows, int32_t* pred, double* saved,
                                      void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    const int rc = sf2_check("mv_sphereface2_forward", cfg, dtype, B, N, stride);
    if (rc != MV_OK) return rc;
    if (B == 0) return MV_OK;
    MV_REQUIRE(logits != nullptr && labels != nullptr, "mv_sphereface2_forward: null logits or labels");
    MV_REQUIRE(bias != nullptr, "mv_sphereface2_forward: null bias");
    MV_REQUIRE(loss != nullptr && loss_rows != nullptr && pred != nullptr && saved != nullptr, "mv_sphereface2_forward: null output");
    MV_REQUIRE(workspace != nullptr, "mv_sphereface2_forward: null workspace");
    if (workspace_bytes < sf2_ws_bytes(B, N))
        return fail(MV_ERR_WORKSPACE, "mv_sphereface2_forward: workspace smaller than mv_sphereface2_workspace_bytes(B, N)");
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(MV_ERR_WORKSPACE, "mv_sphereface2_forward: workspace not 16-byte aligned");
    const SfArgs a = sf2_args(cfg, logits, labels, bias, B, N, stride);
    const int64_t n = B * a.nseg;
    double* segl = static_cast<double*>(workspace);
    double* segw = segl + n;
    float* segc = reinterpret_cast<float*>(segw + n);
    int* segj = reinterpret_cast<int*>(segc + n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SF_DISPATCH(sf2_forward_launch, a, segl, segw, segc, segj, loss, loss_rows, pred, saved, st);
    return check_launch("sf2_seg_kernel / sf2_finish_kernel");
}

extern "C" int mv_sphereface2_backward(const MvSphereFace2Cfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, const float* bias,
                                       int64_t B, int64_t N, int64_t stride, const double* saved, const float* grad_out, void* out,
                                       int64_t out_stride, float* bias_grad, mv_stream_t stream) {
    using namespace mv;
    const int rc = sf2_check("mv_sphereface2_backward", cfg, dtype, B, N, stride);
    if (rc != MV_OK) return rc;
    MV_REQUIRE(out_stride >= N, "mv_sphereface2_backward: out_stride below N");
    MV_REQUIRE(B == 0 || out_stride == 0 || B <= INT64_MAX / 8 / out_stride, "mv_sphereface2_backward: B * out_stride beyond int64");
    if (B == 0) return MV_OK;
    MV_REQUIRE(ceil_div(ceil_div(N, SF_CH), SF_T) < (int64_t)0x7FFFFFFF / B, "mv_sphereface2_backward: B * column tiles + 1 above 2^31 - 1");
    MV_REQUIRE(logits != nullptr && labels != nullptr, "mv_sphereface2_backward: null logits or labels");
    MV_REQUIRE(bias != nullptr, "mv_sphereface2_backward: null bias");
    MV_REQUIRE(saved != nullptr && grad_out != nullptr && out != nullptr && bias_grad != nullptr,
               "mv_sphereface2_backward: null saved, grad_out, out or bias_grad");
    if (!(out == logits && out_stride == stride)) {   // in place is fine (a thread reads what it owns before it writes it); nothing else may overlap
        const int64_t es = dtype == MV_DT_F32 ? 4 : 2;
        const uintptr_t l0 = reinterpret_cast<uintptr_t>(logits), l1 = l0 + (uintptr_t)(((B - 1) * stride + N) * es);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(((B - 1) * out_stride + N) * es);
        MV_REQUIRE(o1 <= l0 || l1 <= o0, "mv_sphereface2_backward: out overlaps logits and is not the in-place form (out == logits, out_stride == stride)");
    }
    const SfArgs a = sf2_args(cfg, logits, labels, bias, B, N, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SF_DISPATCH(sf2_backward_launch, a, saved, grad_out, out, out_stride, bias_grad, st);
    return check_launch("sf2_backward_kernel");
}
