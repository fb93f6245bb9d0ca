// Triplet loss on angular margin with batch-hard mining over the [B, B] similarity matrix of the features, which is never stored.  The contract
// -- the order of every sum, the mining rules, the terms, the gradient -- is in include/mvector_hip.h.  The features are upcast on load and
// everything after that is fp64.
//
// Forward, three ordinary launches:
//   triplet_norm_kernel   grid (B): n_i and the row f^_i, written row-major [B, D] and transposed [D, B] into the workspace
//   triplet_mine_kernel   grid (ceil(B / MV_TRIPLET_ANCHORS)), up to 1024 threads: the anchors' rows in LDS; thread j walks column j of the
//                         transposed copy (lanes read consecutive addresses) and adds sim_ij for the workgroup's anchors in ascending d; the hardest
//                         positive and negative per anchor by a butterfly inside each wave, then over the waves
//   triplet_finish_kernel one wave: the three terms of every row, added in ascending i by one lane
// Backward, two launches: triplet_norm_kernel again (nothing is kept between the calls), and triplet_backward_kernel, grid (B): a gather -- row i
//   collects the anchors that chose it as bit masks over b and adds them in ascending b; no atomics.
#include "kernels.h"
#include "loss_elem.h"

namespace mv {

constexpr int TP_T = 256;                      // threads of every workgroup here
constexpr int TP_A = MV_TRIPLET_ANCHORS;       // anchors per workgroup of the mining kernel
constexpr int TP_DPT = MV_TRIPLET_MAX_D / TP_T;   // feature columns per thread of the backward
constexpr int TP_DEPTH = 16;                   // loads of the transposed copy a thread of the mining kernel keeps in flight
constexpr int TP_MINE_T = 1024;                // threads of the mining kernel at the most: a column of the transposed copy each
constexpr int TP_LDS_WAVES = (TP_MINE_T / 64) * 2 * TP_A * 12;   // the mining kernel's results per wave: a double and an int per anchor and kind
static_assert(TP_A == 4, "the anchors' rows are interleaved four doubles per column");
static_assert(MV_TRIPLET_MAX_B % 64 == 0 && MV_TRIPLET_MAX_D % TP_T == 0 && TP_A * MV_TRIPLET_MAX_D * 8 <= 65536, "the anchors' rows fit the LDS a launch may ask for");

// whether the candidate (vo, jo) replaces the current (vc, jc): the smaller (want_min) or larger value, the lower index on ties; a NaN replaces
// every number, and the lowest NaN stays (torch.min / torch.max)
__device__ __forceinline__ bool tp_takes(double vo, int jo, double vc, int jc, bool want_min) {
    const bool no = vo != vo, nc = vc != vc;
    if (no || nc) return no && (!nc || jo < jc);
    if (vo == vc) return jo < jc;
    return want_min ? vo < vc : vo > vc;
}

// red[0] <- red[0] + ... + red[255] by the halving tree; every thread returns it
__device__ __forceinline__ double tp_tree_sum(double* red, int tid) {
    __syncthreads();
#pragma unroll 1
    for (int h = TP_T / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double v = red[0];
    __syncthreads();
    return v;
}

// fp64 -> fp32 so that a following round-to-nearest to fp16 / bf16 is ONE rounding of the fp64 value (round to odd: the float keeps a sticky bit)
__device__ __forceinline__ float tp_round_odd(double v) {
    float f = (float)v;
    if ((double)f != v && f == f && f - f == 0.0f) {
        uint32_t u = __builtin_bit_cast(uint32_t, f);
        if (fabs((double)f) > fabs(v)) u -= 1;
        f = __builtin_bit_cast(float, u | 1u);
    }
    return f;
}
template <class T>
__device__ __forceinline__ void tp_store(T* p, double v) {
    if constexpr (sizeof(T) == 4) *p = (float)v;
    else MlElem<T>::st(p, tp_round_odd(v));
}

// grid (B).  nrm[i] = sqrt(sum_d f_id^2): thread t adds the columns t, t + 256, ... in ascending d, the 256 partial sums through the halving tree.
// fh [B, D] (and fhT [D, B] unless null) <- f / n, or f without `normalize`
template <class T>
__global__ __launch_bounds__(TP_T) void triplet_norm_kernel(const T* f, int64_t stride, int B, int D, int normalize, double* fh, double* fhT,
                                                            double* nrm) {
    __shared__ double red[TP_T];
    const int tid = threadIdx.x, i = blockIdx.x;
    const T* row = f + (int64_t)i * stride;
    double s = 0.0;
    for (int d = tid; d < D; d += TP_T) {
        const double x = (double)MlElem<T>::ld(row + d);
        s = fma(x, x, s);
    }
    red[tid] = s;
    const double n = sqrt(tp_tree_sum(red, tid));
    for (int d = tid; d < D; d += TP_T) {
        const double x = (double)MlElem<T>::ld(row + d);
        const double v = normalize ? x / n : x;
        fh[(int64_t)i * D + d] = v;
        if (fhT != nullptr) fhT[(int64_t)d * B + i] = v;
    }
    if (tid == 0) nrm[i] = n;
}

// grid (ceil(B / TP_A)), min(TP_MINE_T, B rounded up to whole waves) threads, dynamic LDS max(TP_A * D * 8, TP_LDS_WAVES) bytes.
// sim_ij = sum_d f^_id f^_jd by fma in ascending d, from 0.  The best of a wave by butterfly, the waves' in order: "smaller value, then lower
// index" is a total order, so the tree's shape does not show in the result.
__global__ __launch_bounds__(TP_MINE_T) void triplet_mine_kernel(const double* fh, const double* fhT, const int64_t* labels, int B, int D,
                                                                 double* mined, int32_t* index) {
    MV_DYN_SMEM(smem);
    double* fi = reinterpret_cast<double*>(smem);   // [D][TP_A]
    const int tid = threadIdx.x, nt = blockDim.x, i0 = blockIdx.x * TP_A;
    for (int idx = tid; idx < D * TP_A; idx += nt) {
        const int d = idx / TP_A, a = idx % TP_A;
        const int ia = i0 + a < B ? i0 + a : B - 1;       // a workgroup past the last anchor repeats it and writes nothing for it
        fi[idx] = fh[(int64_t)ia * D + d];
    }
    int64_t li[TP_A];
    double best[2 * TP_A];   // 2 a: the hardest positive of anchor a, 2 a + 1: its hardest negative
    int jb[2 * TP_A];
#pragma unroll
    for (int a = 0; a < TP_A; ++a) {
        li[a] = labels[i0 + a < B ? i0 + a : B - 1];
        best[2 * a] = __builtin_inf();
        best[2 * a + 1] = -__builtin_inf();
        jb[2 * a] = jb[2 * a + 1] = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int j = tid; j < B; j += nt) {
        double acc[TP_A] = {0.0, 0.0, 0.0, 0.0};
        const double* col = fhT + j;
        int d = 0;
        for (; d + TP_DEPTH <= D; d += TP_DEPTH) {      // TP_DEPTH loads leave before the first is used (written out: hipcc keeps one in flight)
            double x[TP_DEPTH];
#pragma unroll
            for (int u = 0; u < TP_DEPTH; ++u) x[u] = col[(int64_t)(d + u) * B];
#pragma unroll
            for (int u = 0; u < TP_DEPTH; ++u)
#pragma unroll
                for (int a = 0; a < TP_A; ++a) acc[a] = fma(x[u], fi[(d + u) * TP_A + a], acc[a]);
        }
        for (; d < D; ++d) {
            const double x = col[(int64_t)d * B];
#pragma unroll
            for (int a = 0; a < TP_A; ++a) acc[a] = fma(x, fi[d * TP_A + a], acc[a]);
        }
        const int64_t lj = labels[j];
#pragma unroll
        for (int a = 0; a < TP_A; ++a) {
            if (lj == li[a]) {
                if (tp_takes(acc[a], j, best[2 * a], jb[2 * a], true)) best[2 * a] = acc[a], jb[2 * a] = j;
            } else {
                if (tp_takes(acc[a], j, best[2 * a + 1], jb[2 * a + 1], false)) best[2 * a + 1] = acc[a], jb[2 * a + 1] = j;
            }
        }
    }
    __syncthreads();   // the anchors' rows are done with: their LDS now carries the waves' results
    double* wv = reinterpret_cast<double*>(smem);                               // [waves][2 * TP_A]
    int* wj = reinterpret_cast<int*>(smem + (TP_MINE_T / 64) * 2 * TP_A * 8);   // [waves][2 * TP_A]
    const int wave = tid >> 6, nw = nt >> 6;
#pragma unroll
    for (int k = 0; k < 2 * TP_A; ++k) {
        double v = best[k];
        int jj = jb[k];
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const double vo = __shfl_xor(v, m);
            const int jo = __shfl_xor(jj, m);
            if (tp_takes(vo, jo, v, jj, (k & 1) == 0)) v = vo, jj = jo;
        }
        if ((tid & 63) == 0) wv[wave * 2 * TP_A + k] = v, wj[wave * 2 * TP_A + k] = jj;
    }
    __syncthreads();
    if (tid < 2 * TP_A && i0 + tid / 2 < B) {
        double v = wv[tid];
        int jj = wj[tid];
        for (int w = 1; w < nw; ++w)
            if (tp_takes(wv[w * 2 * TP_A + tid], wj[w * 2 * TP_A + tid], v, jj, (tid & 1) == 0)) v = wv[w * 2 * TP_A + tid], jj = wj[w * 2 * TP_A + tid];
        mined[(int64_t)i0 * 2 + tid] = v;
        index[(int64_t)i0 * 2 + tid] = jj == 0x7FFFFFFF ? -1 : jj;
    }
}

// the three terms of row i (torch.clamp keeps a NaN, the two torch.where send it to their else-value)
struct TpTerms {
    double rank, over, shrt;
};
__device__ __forceinline__ TpTerms tp_terms(const MvTripletCfg& c, double ap, double an) {
    TpTerms t;
    const double x = c.margin - (ap - an);
    t.rank = x < 0.0 ? 0.0 : x;
    const double s = c.ap_value - ap, o = an - c.an_value;
    t.shrt = s > 0.0 ? s : 0.0;
    t.over = o > 0.0 ? o : 1.0;
    return t;
}
// alpha = d loss / d ap_i, beta = d loss / d an_i: the hinge passes where its argument is >= 0, the two where-terms where their condition holds
__device__ __forceinline__ void tp_coef(const MvTripletCfg& c, double ap, double an, double invB, double& alpha, double& beta) {
    const bool on = c.margin - (ap - an) >= 0.0;
    alpha = on ? -invB : 0.0;
    beta = on ? invB : 0.0;
    if (c.add_absolute) {
        if (c.ap_value - ap > 0.0) alpha -= c.absolute_loss_weight * invB;
        if (an - c.an_value > 0.0) beta += c.absolute_loss_weight * invB;
    }
}

// one wave; lane 0 adds the rows in ascending i (the contract's order: a tree would be another)
__global__ __launch_bounds__(64) void triplet_finish_kernel(MvTripletCfg c, const double* mined, int B, float* loss) {
    if (threadIdx.x != 0) return;
    double R = 0.0, O = 0.0, S = 0.0;
    for (int i = 0; i < B; ++i) {
        const TpTerms t = tp_terms(c, mined[(int64_t)i * 2], mined[(int64_t)i * 2 + 1]);
        R += t.rank;
        O += t.over;
        S += t.shrt;
    }
    double l = R / (double)B;
    if (c.add_absolute) l += c.absolute_loss_weight * (O / (double)B + S / (double)B);
    loss[0] = (float)l;
}

// grid (B).  Thread t owns the columns t, t + 256, ... of row i.
template <class T>
__global__ __launch_bounds__(TP_T) void triplet_backward_kernel(MvTripletCfg c, const double* fh, const double* nrm, const double* mined,
                                                                const int32_t* index, const float* grad_out, T* out, int64_t out_stride, int B,
                                                                int D) {
    __shared__ double red[TP_T];
    __shared__ uint64_t chose_p[MV_TRIPLET_MAX_B / 64];
    __shared__ uint64_t chose_q[MV_TRIPLET_MAX_B / 64];
    const int tid = threadIdx.x, i = blockIdx.x;
    const double invB = 1.0 / (double)B;
    double acc[TP_DPT];
    double alpha, beta;
    tp_coef(c, mined[(int64_t)i * 2], mined[(int64_t)i * 2 + 1], invB, alpha, beta);
    const int p = index[(int64_t)i * 2], q = index[(int64_t)i * 2 + 1];   // p is a row of i's label (i itself at the least); q is -1 or a row
    const bool rows_ok = p >= 0 && p < B && q >= -1 && q < B;             // anything else is not the forward's: the row is NaN, nothing is read
#pragma unroll
    for (int k = 0; k < TP_DPT; ++k) {
        const int d = tid + k * TP_T;
        acc[k] = 0.0;
        if (d < D) {
            acc[k] = rows_ok ? alpha * fh[(int64_t)p * D + d] : (double)__builtin_nanf("");
            if (rows_ok && q >= 0) acc[k] = fma(beta, fh[(int64_t)q * D + d], acc[k]);
        }
    }
    // who chose row i: thread w reads the mined rows 64 w .. 64 w + 63 into one mask per list; then every thread walks the set bits in ascending b
    for (int w = tid; w < (B + 63) / 64; w += TP_T) {
        uint64_t pm = 0, qm = 0;
        for (int k = 0; k < 64 && w * 64 + k < B; ++k) {
            const int b = w * 64 + k;
            if (index[(int64_t)b * 2] == i) pm |= (uint64_t)1 << k;
            if (index[(int64_t)b * 2 + 1] == i) qm |= (uint64_t)1 << k;
        }
        chose_p[w] = pm;
        chose_q[w] = qm;
    }
    __syncthreads();
#pragma unroll 1
    for (int w = 0; w < (B + 63) / 64; ++w) {
        const uint64_t pm = chose_p[w], qm = chose_q[w];
        uint64_t m = pm | qm;
        while (m != 0) {
            const int k = __builtin_ctzll(m), b = w * 64 + k;
            m &= m - 1;
            const bool by_p = (pm >> k) & 1, by_q = (qm >> k) & 1;
            tp_coef(c, mined[(int64_t)b * 2], mined[(int64_t)b * 2 + 1], invB, alpha, beta);
#pragma unroll
            for (int kk = 0; kk < TP_DPT; ++kk) {
                const int d = tid + kk * TP_T;
                if (d < D) {
                    const double v = fh[(int64_t)b * D + d];
                    if (by_p) acc[kk] = fma(alpha, v, acc[kk]);
                    if (by_q) acc[kk] = fma(beta, v, acc[kk]);
                }
            }
        }
    }
    if (c.normalize) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < TP_DPT; ++k) {
            const int d = tid + k * TP_T;
            if (d < D) s = fma(acc[k], fh[(int64_t)i * D + d], s);
        }
        red[tid] = s;
        const double dot = tp_tree_sum(red, tid), n = nrm[i];
#pragma unroll
        for (int k = 0; k < TP_DPT; ++k) {
            const int d = tid + k * TP_T;
            if (d < D) acc[k] = (acc[k] - dot * fh[(int64_t)i * D + d]) / n;
        }
    }
    const double g = (double)grad_out[0];
    T* orow = out + (int64_t)i * out_stride;
#pragma unroll
    for (int k = 0; k < TP_DPT; ++k) {
        const int d = tid + k * TP_T;
        if (d < D) tp_store<T>(orow + d, g * acc[k]);
    }
}

// ---- host side
static size_t triplet_ws_bytes(int64_t B, int64_t D) { return (size_t)round_up((2 * B * D + B) * 8, 16); }

static int triplet_check(const char* who, const MvTripletCfg* cfg, int32_t dtype, int64_t B, int64_t D, int64_t stride) {
    const std::string w(who);
    if (cfg == nullptr) return fail(MV_ERR_INVALID_ARGUMENT, w + ": null cfg");
    if (B < 0 || D < 0) return fail(MV_ERR_INVALID_ARGUMENT, w + ": negative B or D");
    if (dtype != MV_DT_F32 && dtype != MV_DT_F16 && dtype != MV_DT_BF16)
        return fail(MV_ERR_INVALID_ARGUMENT, w + ": unknown dtype (MV_DT_F32, MV_DT_F16 or MV_DT_BF16)");
    if (B > MV_TRIPLET_MAX_B) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B above MV_TRIPLET_MAX_B (4096)");
    if (D < 1 || D > MV_TRIPLET_MAX_D) return fail(MV_ERR_INVALID_ARGUMENT, w + ": D outside 1 .. MV_TRIPLET_MAX_D (2048)");
    if (stride < D) return fail(MV_ERR_INVALID_ARGUMENT, w + ": stride below D");
    if (B > 0 && B > INT64_MAX / 8 / stride) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B * stride beyond int64");
    return MV_OK;
}

static int triplet_ws_check(const char* who, void* workspace, size_t workspace_bytes, int64_t B, int64_t D) {
    const std::string w(who);
    if (workspace == nullptr) return fail(MV_ERR_INVALID_ARGUMENT, w + ": null workspace");
    if (workspace_bytes < triplet_ws_bytes(B, D)) return fail(MV_ERR_WORKSPACE, w + ": workspace smaller than mv_triplet_workspace_bytes(B, D)");
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(MV_ERR_WORKSPACE, w + ": workspace not 16-byte aligned");
    return MV_OK;
}

#define TP_DISPATCH(FN, ...)                                                             \
    do {                                                                                 \
        if (dtype == MV_DT_F32) FN<float>(__VA_ARGS__);                                  \
        else if (dtype == MV_DT_F16) FN<half_t>(__VA_ARGS__);                            \
        else FN<bf16_t>(__VA_ARGS__);                                                    \
    } while (0)

template <class T>
static void triplet_norm_launch(const void* f, int64_t stride, int B, int D, int normalize, double* fh, double* fhT, double* nrm, hipStream_t st) {
    MV_LAUNCH((triplet_norm_kernel<T>), ((unsigned)B, 1, 1), (TP_T, 1, 1), 0, st, static_cast<const T*>(f), stride, B, D, normalize, fh, fhT, nrm);
}

template <class T>
static void triplet_backward_launch(const MvTripletCfg& c, const double* fh, const double* nrm, const double* mined, const int32_t* index,
                                    const float* grad_out, void* out, int64_t out_stride, int B, int D, hipStream_t st) {
    MV_LAUNCH((triplet_backward_kernel<T>), ((unsigned)B, 1, 1), (TP_T, 1, 1), 0, st, c, fh, nrm, mined, index, grad_out, static_cast<T*>(out),
              out_stride, B, D);
}

}  // namespace mv

extern "C" size_t mv_triplet_workspace_bytes(int64_t B, int64_t D) {
    if (B <= 0 || B > MV_TRIPLET_MAX_B || D < 1 || D > MV_TRIPLET_MAX_D) return 0;
    return mv::triplet_ws_bytes(B, D);
}

extern "C" int mv_triplet_forward(const MvTripletCfg* cfg, const void* features, int32_t dtype, const int64_t* labels, int64_t B, int64_t D,
                                  int64_t stride, float* loss, double* mined, int32_t* index, void* workspace, size_t workspace_bytes,
                                  mv_stream_t stream) {
    using namespace mv;
    int rc = triplet_check("mv_triplet_forward", cfg, dtype, B, D, stride);
    if (rc != MV_OK) return rc;
    if (B == 0) return MV_OK;
    MV_REQUIRE(features != nullptr && labels != nullptr, "mv_triplet_forward: null features or labels");
    MV_REQUIRE(loss != nullptr && mined != nullptr && index != nullptr, "mv_triplet_forward: null output");
    rc = triplet_ws_check("mv_triplet_forward", workspace, workspace_bytes, B, D);
    if (rc != MV_OK) return rc;
    double* fh = static_cast<double*>(workspace);
    double* fhT = fh + B * D;
    double* nrm = fhT + B * D;
    hipStream_t st = static_cast<hipStream_t>(stream);
    TP_DISPATCH(triplet_norm_launch, features, stride, (int)B, (int)D, cfg->normalize, fh, fhT, nrm, st);
    const size_t lds = (size_t)(TP_A * D * 8 > TP_LDS_WAVES ? TP_A * D * 8 : TP_LDS_WAVES);
    const int mine_t = (int)(round_up(B, 64) < TP_MINE_T ? round_up(B, 64) : TP_MINE_T);
    MV_LAUNCH(triplet_mine_kernel, ((unsigned)ceil_div(B, TP_A), 1, 1), (mine_t, 1, 1), lds, st, (const double*)fh, (const double*)fhT, labels, (int)B,
              (int)D, mined, index);
    MV_LAUNCH(triplet_finish_kernel, (1, 1, 1), (64, 1, 1), 0, st, *cfg, (const double*)mined, (int)B, loss);
    return check_launch("triplet_norm_kernel / triplet_mine_kernel / triplet_finish_kernel");
}

extern "C" int mv_triplet_backward(const MvTripletCfg* cfg, const void* features, int32_t dtype, int64_t B, int64_t D, int64_t stride,
                                   const double* mined, const int32_t* index, const float* grad_out, void* out, int64_t out_stride, void* workspace,
                                   size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    int rc = triplet_check("mv_triplet_backward", cfg, dtype, B, D, stride);
    if (rc != MV_OK) return rc;
    MV_REQUIRE(out_stride >= D, "mv_triplet_backward: out_stride below D");
    MV_REQUIRE(B == 0 || B <= INT64_MAX / 8 / out_stride, "mv_triplet_backward: B * out_stride beyond int64");
    if (B == 0) return MV_OK;
    MV_REQUIRE(features != nullptr, "mv_triplet_backward: null features");
    MV_REQUIRE(mined != nullptr && index != nullptr && grad_out != nullptr && out != nullptr, "mv_triplet_backward: null mined, index, grad_out or out");
    rc = triplet_ws_check("mv_triplet_backward", workspace, workspace_bytes, B, D);
    if (rc != MV_OK) return rc;
    const int64_t es = dtype == MV_DT_F32 ? 4 : 2;
    const uintptr_t f0 = reinterpret_cast<uintptr_t>(features), f1 = f0 + (uintptr_t)(((B - 1) * stride + D) * es);
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(((B - 1) * out_stride + D) * es);
    MV_REQUIRE(o1 <= f0 || f1 <= o0, "mv_triplet_backward: out overlaps features");
    double* fh = static_cast<double*>(workspace);
    double* nrm = fh + 2 * B * D;
    hipStream_t st = static_cast<hipStream_t>(stream);
    TP_DISPATCH(triplet_norm_launch, features, stride, (int)B, (int)D, cfg->normalize, fh, (double*)nullptr, nrm, st);
    TP_DISPATCH(triplet_backward_launch, *cfg, (const double*)fh, (const double*)nrm, mined, index, grad_out, out, out_stride, (int)B, (int)D, st);
    return check_launch("triplet_norm_kernel / triplet_backward_kernel");
}
