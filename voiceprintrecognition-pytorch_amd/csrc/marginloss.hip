// Margin-softmax classification losses (CE, AM, ARM, AAM, sub-centre AAM): one fused forward and one fused backward over the [B, N * K] logit
// matrix.  The contract -- the definition of z, the summation order, what `saved` holds -- is in include/mvector_hip.h.
//
// Forward, three ordinary launches, no workgroup waits for another:
//   margin_seg_kernel<.., 0>   grid (B * segments): the segment's largest z (exact in any order) and its best centre cosine (for `pred`)
//   margin_seg_kernel<.., 1>   the same grid: sum exp(z - M) and sum z of the segment in fp64, M = the row maximum from the segment maxima; this is
//                              the second read of the logits, served largely from the Infinity Cache
//   margin_finish_kernel       one workgroup: a thread per row adds the segments in order and writes loss_rows / pred / saved; thread 0 adds the rows
// Backward: margin_backward_kernel, element-wise, a thread per chunk of MV_MARGIN_CHUNK centres; every row scalar comes from `saved`.
//
// A thread always owns the same chunks whatever the element type and whatever the row's alignment: the 16-byte path (K <= 3 and a row that starts on a
// 16-byte boundary) and the element path hand the same values to the same threads, so the bits do not depend on which of them ran.
#include "kernels.h"
#include "loss_elem.h"

namespace mv {

constexpr int ML_T = 256;                                  // threads of every workgroup here
constexpr int ML_CH = MV_MARGIN_CHUNK;                     // centres per chunk
constexpr int ML_SEG_CHUNKS = MV_MARGIN_SEG / ML_CH;       // chunks per segment
static_assert(MV_MARGIN_SEG % ML_CH == 0 && ML_SEG_CHUNKS % ML_T == 0, "a segment is a whole number of chunks per thread");
static_assert(ML_CH == 8, "a chunk of 8 K-groups is 2 K (fp32) or K (16-bit) 16-byte pieces");

struct MlArgs {
    MvMarginLossCfg c;
    const void* logits;
    const int64_t* labels;
    int64_t stride;
    int B, N, nseg;
};

// ---- z: fp32, one operation at a time
// The fp32 product rounded on its own.  hipcc honours the contraction pragma below; a host compiler under -ffp-contract=fast (the test-suite's
// emulator build) fuses a product with the sum behind it whatever the pragma says.  So the product's bits pass through an integer OR with a word
// that is 0 for every kind the entry points accept but that no compiler can know to be 0: the sum behind it then has no product to fuse with.
__device__ __forceinline__ float mul_rounded(float a, float b, const MvMarginLossCfg& c) {
    const uint32_t zero = (uint32_t)c.kind >> 8;
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, a * b) | zero);
}
__device__ __forceinline__ float ml_z_target(const MvMarginLossCfg& c, float cy) {
#pragma clang fp contract(off)
    if (c.kind == MV_LOSS_CE) return cy;
    if (c.kind == MV_LOSS_AM || c.kind == MV_LOSS_ARM) {
        const float d = cy - c.margin;
        return mul_rounded(c.scale, d, c);
    }
    const float sq = mul_rounded(cy, cy, c);
    const float sine = sqrtf(1.0f - sq);
    const float a = mul_rounded(cy, c.cos_m, c);
    const float bb = mul_rounded(sine, c.sin_m, c);
    const float phi = a - bb;
    float sel;
    if (c.easy_margin) sel = cy > 0.0f ? phi : cy;
    else sel = cy > c.th ? phi : cy - c.mmm;
    return mul_rounded(sel, c.scale, c);
}
// whether the target's z went through phi (the branch whose derivative is not s)
__device__ __forceinline__ bool ml_phi_branch(const MvMarginLossCfg& c, float cy) {
    if (c.kind != MV_LOSS_AAM && c.kind != MV_LOSS_SUBCENTER) return false;
    return c.easy_margin ? cy > 0.0f : cy > c.th;
}
// zeroed: the column is one ARM replaced by 0 (its derivative is 0)
__device__ __forceinline__ float ml_z(const MvMarginLossCfg& c, float cj, bool is_target, float zy, bool& zeroed) {
#pragma clang fp contract(off)
    float z = is_target ? zy : (c.kind == MV_LOSS_CE ? cj : mul_rounded(c.scale, cj, c));
    zeroed = false;
    if (c.kind == MV_LOSS_ARM) {
        const float d = z - zy;
        if (d < 0.0f) z = 0.0f, zeroed = true;
    }
    return z;
}

// the larger of a K-group, the lowest k on ties; a NaN in the group is the group's value (as torch.max)
#define ML_GROUP_STEP(v, k)                  \
    if (!((v) <= best) && best == best) {    \
        best = (v);                          \
        kb = (k);                            \
    }

struct MlTarget {
    int y;         // the label, -1 when it is outside [0, N)
    float zy;      // NaN when it is
};
template <class T>
__device__ __forceinline__ MlTarget ml_target(const MlArgs& a, const T* row, int b) {
    MlTarget t;
    const int64_t y = a.labels[b];
    if (y < 0 || y >= (int64_t)a.N) {
        t.y = -1;
        t.zy = __builtin_nanf("");
        return t;
    }
    const T* p = row + y * a.c.K;
    float best = MlElem<T>::ld(p);
    int kb = 0;
    for (int k = 1; k < a.c.K; ++k) {
        const float v = MlElem<T>::ld(p + k);
        ML_GROUP_STEP(v, k)
    }
    (void)kb;
    t.y = (int)y;
    t.zy = ml_z_target(a.c, best);
    return t;
}

// the chunk of ML_CH centres from j0 on: centre cosines c[] and the winning sub-centre ka[] (entries at or beyond N are not touched and hold 0)
template <class T, int KT>
__device__ __forceinline__ void ml_load_chunk(const T* row, int j0, int N, int K, bool vec, float (&c)[ML_CH], int (&ka)[ML_CH]) {
    if constexpr (KT != 0) {
        if (vec && j0 + ML_CH <= N) {
            float e[ML_CH * KT];
            MlElem<T>::template ldv<ML_CH * KT>(row + (int64_t)j0 * KT, e);
#pragma unroll
            for (int g = 0; g < ML_CH; ++g) {
                float best = e[g * KT];
                int kb = 0;
#pragma unroll
                for (int k = 1; k < KT; ++k) ML_GROUP_STEP(e[g * KT + k], k)
                c[g] = best;
                ka[g] = kb;
            }
            return;
        }
    }
    const int Kr = KT != 0 ? KT : K;
#pragma unroll
    for (int g = 0; g < ML_CH; ++g) {
        c[g] = 0.0f;
        ka[g] = 0;
        if (j0 + g < N) {
            const T* p = row + (int64_t)(j0 + g) * Kr;
            float best = MlElem<T>::ld(p);
            int kb = 0;
            for (int k = 1; k < Kr; ++k) {
                const float v = MlElem<T>::ld(p + k);
                ML_GROUP_STEP(v, k)
            }
            c[g] = best;
            ka[g] = kb;
        }
    }
}

__device__ __forceinline__ bool ml_better(float c, int j, float cb, int jb) { return c > cb || (c == cb && j < jb); }

// grid (B * nseg).  PASS 0: segz / segc / segj [B, nseg] <- the segment's largest z, its largest centre cosine and that centre.
// PASS 1: sege / segs [B, nseg] <- sum exp(z - M), sum z in fp64 (M: the largest of the row's segz).
template <class T, int KT, int PASS>
__global__ __launch_bounds__(ML_T) void margin_seg_kernel(MlArgs a, float* segz, float* segc, int* segj, double* sege, double* segs) {
    __shared__ double redd[ML_T];
    __shared__ double redd2[ML_T];
    __shared__ float redf[ML_T];
    __shared__ float redc[ML_T];
    __shared__ int redj[ML_T];
    const int tid = threadIdx.x;
    const int b = (int)(blockIdx.x / (unsigned)a.nseg), seg = (int)(blockIdx.x - (unsigned)b * (unsigned)a.nseg);
    const T* row = static_cast<const T*>(a.logits) + (int64_t)b * a.stride;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const MlTarget tgt = ml_target<T>(a, row, b);
    const float ninf = -__builtin_inff();
    float M = ninf;
    if constexpr (PASS == 1) {
        for (int i = tid; i < a.nseg; i += ML_T) {
            const float v = segz[(int64_t)b * a.nseg + i];
            if (v > M) M = v;
        }
        redf[tid] = M;
        __syncthreads();
#pragma unroll 1
        for (int h = ML_T / 2; h > 0; h >>= 1) {
            if (tid < h && redf[tid + h] > redf[tid]) redf[tid] = redf[tid + h];
            __syncthreads();
        }
        M = redf[0];
        __syncthreads();
    }
    float zmax = ninf, cb = ninf;
    int jb = 0x7FFFFFFF;
    double se = 0.0, sz = 0.0;
#pragma unroll 1
    for (int ch = tid; ch < ML_SEG_CHUNKS; ch += ML_T) {
        const int64_t j0l = (int64_t)seg * MV_MARGIN_SEG + (int64_t)ch * ML_CH;
        if (j0l >= a.N) break;
        const int j0 = (int)j0l;
        float c[ML_CH];
        int ka[ML_CH];
        ml_load_chunk<T, KT>(row, j0, a.N, a.c.K, vec, c, ka);
#pragma unroll
        for (int g = 0; g < ML_CH; ++g) {
            const int j = j0 + g;
            if (j < a.N) {
                bool zeroed;
                const float z = ml_z(a.c, c[g], j == tgt.y, tgt.zy, zeroed);
                if constexpr (PASS == 0) {
                    if (z > zmax) zmax = z;
                    if (ml_better(c[g], j, cb, jb)) cb = c[g], jb = j;
                } else {
                    se += exp((double)z - (double)M);
                    sz += (double)z;
                }
            }
        }
    }
    const int64_t o = (int64_t)b * a.nseg + seg;
    if constexpr (PASS == 0) {
        redf[tid] = zmax;
        redc[tid] = cb;
        redj[tid] = jb;
        __syncthreads();
#pragma unroll 1
        for (int h = ML_T / 2; h > 0; h >>= 1) {
            if (tid < h) {
                if (redf[tid + h] > redf[tid]) redf[tid] = redf[tid + h];
                if (ml_better(redc[tid + h], redj[tid + h], redc[tid], redj[tid])) redc[tid] = redc[tid + h], redj[tid] = redj[tid + h];
            }
            __syncthreads();
        }
        if (tid == 0) {
            segz[o] = redf[0];
            segc[o] = redc[0];
            segj[o] = redj[0];
        }
    } else {
        redd[tid] = se;
        redd2[tid] = sz;
        __syncthreads();
#pragma unroll 1
        for (int h = ML_T / 2; h > 0; h >>= 1) {
            if (tid < h) {
                redd[tid] += redd[tid + h];
                redd2[tid] += redd2[tid + h];
            }
            __syncthreads();
        }
        if (tid == 0) {
            sege[o] = redd[0];
            segs[o] = redd2[0];
        }
    }
}

// one workgroup.  Thread t finishes the rows t, t + 256, ...; thread 0 then adds the rows' losses in ascending b.
template <class T>
__global__ __launch_bounds__(ML_T) void margin_finish_kernel(MlArgs a, const float* segz, const float* segc, const int* segj, const double* sege,
                                                             const double* segs, float* loss, float* loss_rows, int32_t* pred, double* saved) {
    const int tid = threadIdx.x;
    for (int b = tid; b < a.B; b += ML_T) {
        const T* row = static_cast<const T*>(a.logits) + (int64_t)b * a.stride;
        const MlTarget tgt = ml_target<T>(a, row, b);
        float M = -__builtin_inff(), cb = -__builtin_inff();
        int jb = 0x7FFFFFFF;
        double S = 0.0, Z = 0.0;
        for (int i = 0; i < a.nseg; ++i) {
            const int64_t o = (int64_t)b * a.nseg + i;
            if (segz[o] > M) M = segz[o];
            if (ml_better(segc[o], segj[o], cb, jb)) cb = segc[o], jb = segj[o];
            S += sege[o];
            Z += segs[o];
        }
        const double logS = log(S);
        const double lse = (double)M + logS;
        double l = (1.0 - (double)a.c.eps) * (lse - (double)tgt.zy);
        if (a.c.eps > 0.0f) l += (double)a.c.eps * (lse - Z / (double)a.N);
        loss_rows[b] = (float)l;
        pred[b] = jb == 0x7FFFFFFF ? 0 : jb;
        double* sv = saved + (int64_t)b * MV_MARGIN_SAVED;
        sv[0] = (double)M;
        sv[1] = logS;
        sv[2] = (double)tgt.zy;
        sv[3] = l;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int b = 0; b < a.B; ++b) total += saved[(int64_t)b * MV_MARGIN_SAVED + 3];
        loss[0] = (float)(total / (double)a.B);
    }
}

// grid (B * tiles), a tile = ML_T chunks.  A thread reads the K-groups of its chunk, then writes them: out may be the logits themselves.
template <class T, int KT>
__global__ __launch_bounds__(ML_T) void margin_backward_kernel(MlArgs a, const double* saved, const float* grad_out, T* out, int64_t out_stride, int tiles) {
    const int b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)b * (unsigned)tiles);
    const int64_t j0l = ((int64_t)tile * ML_T + threadIdx.x) * ML_CH;
    if (j0l >= a.N) return;
    const int j0 = (int)j0l;
    const T* row = static_cast<const T*>(a.logits) + (int64_t)b * a.stride;
    T* orow = out + (int64_t)b * out_stride;
    const bool vec = ((reinterpret_cast<uintptr_t>(row) | reinterpret_cast<uintptr_t>(orow)) & 15) == 0;
    const int K = KT != 0 ? KT : a.c.K;
    const double* sv = saved + (int64_t)b * MV_MARGIN_SAVED;
    const double lse = sv[0] + sv[1];
    const float zy = (float)sv[2];
    const int64_t y64 = a.labels[b];
    const bool valid = y64 >= 0 && y64 < (int64_t)a.N;
    const int y = valid ? (int)y64 : -1;
    const double gB = (double)grad_out[0] / (double)a.B;
    const double q_off = (double)a.c.eps / (double)a.N, q_on = (1.0 - (double)a.c.eps) + q_off;
    const double s = a.c.kind == MV_LOSS_CE ? 1.0 : (double)a.c.scale;
    float c[ML_CH];
    int ka[ML_CH];
    ml_load_chunk<T, KT>(row, j0, a.N, K, vec, c, ka);
    float val[ML_CH];
#pragma unroll
    for (int g = 0; g < ML_CH; ++g) {
        const int j = j0 + g;
        const bool is_target = j == y;
        bool zeroed;
        const float z = ml_z(a.c, c[g], is_target, zy, zeroed);
        const double p = exp((double)z - lse);
        double dz = zeroed ? 0.0 : s;
        if (is_target && ml_phi_branch(a.c, c[g])) {
            const double cy = (double)c[g];
            dz = s * ((double)a.c.cos_m + cy * (double)a.c.sin_m / sqrt(1.0 - cy * cy));
        }
        val[g] = (float)(gB * (p - (is_target ? q_on : q_off)) * dz);
    }
    const float nanv = __builtin_nanf("");
    if constexpr (KT != 0) {
        if (vec && j0 + ML_CH <= a.N) {
            float o[ML_CH * KT];
#pragma unroll
            for (int g = 0; g < ML_CH; ++g)
#pragma unroll
                for (int k = 0; k < KT; ++k) o[g * KT + k] = !valid ? nanv : (k == ka[g] ? val[g] : 0.0f);
            MlElem<T>::template stv<ML_CH * KT>(orow + (int64_t)j0 * KT, o);
            return;
        }
    }
#pragma unroll
    for (int g = 0; g < ML_CH; ++g) {
        if (j0 + g < a.N) {
            T* p = orow + (int64_t)(j0 + g) * K;
            for (int k = 0; k < K; ++k) MlElem<T>::st(p + k, !valid ? nanv : (k == ka[g] ? val[g] : 0.0f));
        }
    }
}

// ---- host side
static int64_t margin_segments(int64_t N) { return N > 0 ? (N + MV_MARGIN_SEG - 1) / MV_MARGIN_SEG : 0; }

static size_t margin_ws_bytes(int64_t B, int64_t N) {
    const int64_t n = B * margin_segments(N);
    return (size_t)round_up(n * (8 + 8 + 4 + 4 + 4), 16);
}

// what forward and backward check alike; B == 0 is decided by the caller in front of the pointer checks
static int margin_check(const char* who, const MvMarginLossCfg* cfg, int32_t dtype, int64_t B, int64_t N, int64_t stride) {
    const std::string w(who);
    if (cfg == nullptr) return fail(MV_ERR_INVALID_ARGUMENT, w + ": null cfg");
    if (B < 0 || N < 0) return fail(MV_ERR_INVALID_ARGUMENT, w + ": negative B or N");
    if (cfg->kind < MV_LOSS_CE || cfg->kind > MV_LOSS_SUBCENTER)
        return fail(MV_ERR_INVALID_ARGUMENT, w + ": unknown kind (MV_LOSS_CE, MV_LOSS_AM, MV_LOSS_ARM, MV_LOSS_AAM or MV_LOSS_SUBCENTER)");
    if (dtype != MV_DT_F32 && dtype != MV_DT_F16 && dtype != MV_DT_BF16)
        return fail(MV_ERR_INVALID_ARGUMENT, w + ": unknown dtype (MV_DT_F32, MV_DT_F16 or MV_DT_BF16)");
    if (cfg->K < 1 || cfg->K > 8) return fail(MV_ERR_INVALID_ARGUMENT, w + ": K outside 1 .. 8");
    if (cfg->K != 1 && cfg->kind != MV_LOSS_SUBCENTER) return fail(MV_ERR_INVALID_ARGUMENT, w + ": K != 1 with a kind other than MV_LOSS_SUBCENTER");
    if (!(cfg->eps >= 0.0f && cfg->eps < 1.0f)) return fail(MV_ERR_INVALID_ARGUMENT, w + ": eps (label smoothing) outside [0, 1)");
    if (N > (int64_t)0x7FFFFFFF / cfg->K) return fail(MV_ERR_INVALID_ARGUMENT, w + ": N * K above 2^31 - 1");
    if (stride < N * cfg->K) return fail(MV_ERR_INVALID_ARGUMENT, w + ": stride below N * K");
    if (B > 0 && stride > 0 && B > INT64_MAX / 8 / stride) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B * stride beyond int64");
    if (B > 0x7FFFFFFF) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B above 2^31 - 1");
    if (B > 0 && N == 0) return fail(MV_ERR_INVALID_ARGUMENT, w + ": N = 0 (no classes) with B > 0");
    if (B > 0 && margin_segments(N) > (int64_t)0x7FFFFFFF / B) return fail(MV_ERR_INVALID_ARGUMENT, w + ": B * segments above 2^31 - 1");
    return MV_OK;
}

static MlArgs margin_args(const MvMarginLossCfg* cfg, const void* logits, const int64_t* labels, int64_t B, int64_t N, int64_t stride) {
    MlArgs a;
    a.c = *cfg;
    a.logits = logits;
    a.labels = labels;
    a.stride = stride;
    a.B = (int)B;
    a.N = (int)N;
    a.nseg = (int)margin_segments(N);
    return a;
}

// FN<T, KT>(...) for the element type and K of the call; K above 3 runs the element path with K at run time
#define ML_DISPATCH_K(FN, T, ...)                        \
    switch (cfg->K) {                                    \
        case 1: FN<T, 1>(__VA_ARGS__); break;            \
        case 2: FN<T, 2>(__VA_ARGS__); break;            \
        case 3: FN<T, 3>(__VA_ARGS__); break;            \
        default: FN<T, 0>(__VA_ARGS__); break;           \
    }
#define ML_DISPATCH(FN, ...)                                                     \
    do {                                                                         \
        if (dtype == MV_DT_F32) { ML_DISPATCH_K(FN, float, __VA_ARGS__) }        \
        else if (dtype == MV_DT_F16) { ML_DISPATCH_K(FN, half_t, __VA_ARGS__) }  \
        else { ML_DISPATCH_K(FN, bf16_t, __VA_ARGS__) }                          \
    } while (0)

struct MlWs {
    double *sege, *segs;
    float *segz, *segc;
    int* segj;
};

template <class T, int KT>
static void margin_forward_launch(const MlArgs& a, const MlWs& w, float* loss, float* loss_rows, int32_t* pred, double* saved, hipStream_t st) {
    const unsigned grid = (unsigned)a.B * (unsigned)a.nseg;
    MV_LAUNCH((margin_seg_kernel<T, KT, 0>), (grid, 1, 1), (ML_T, 1, 1), 0, st, a, w.segz, w.segc, w.segj, w.sege, w.segs);
    // (the second read alone, for tools/bench_margin_loss.py; nothing happens here unless mv_profile_enable(1))
    const int token = prof_begin(MV_PROF_MARGIN_SUMS, (double)a.B * a.N * a.c.K * sizeof(T), st);
    MV_LAUNCH((margin_seg_kernel<T, KT, 1>), (grid, 1, 1), (ML_T, 1, 1), 0, st, a, w.segz, w.segc, w.segj, w.sege, w.segs);
    prof_end(token, st);
    MV_LAUNCH((margin_finish_kernel<T>), (1, 1, 1), (ML_T, 1, 1), 0, st, a, (const float*)w.segz, (const float*)w.segc, (const int*)w.segj,
              (const double*)w.sege, (const double*)w.segs, loss, loss_rows, pred, saved);
}

template <class T, int KT>
static void margin_backward_launch(const MlArgs& a, const double* saved, const float* grad_out, void* out, int64_t out_stride, hipStream_t st) {
    const int tiles = (int)ceil_div(ceil_div(a.N, ML_CH), ML_T);
    MV_LAUNCH((margin_backward_kernel<T, KT>), ((unsigned)a.B * (unsigned)tiles, 1, 1), (ML_T, 1, 1), 0, st, a, saved, grad_out, static_cast<T*>(out),
              out_stride, tiles);
}

}  // namespace mv

#undef ML_GROUP_STEP

extern "C" size_t mv_margin_ce_workspace_bytes(int64_t B, int64_t N, int32_t K) {
    if (B <= 0 || N <= 0 || K < 1 || K > 8 || N > (int64_t)0x7FFFFFFF / K || B > 0x7FFFFFFF || mv::margin_segments(N) > (int64_t)0x7FFFFFFF / B) return 0;
    return mv::margin_ws_bytes(B, N);
}

extern "C" int mv_margin_ce_forward(const MvMarginLossCfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, int64_t B, int64_t N,
                                    int64_t stride, float* loss, float* loss_rows, int32_t* pred, double* saved, void* workspace,
                                    size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    const int rc = margin_check("mv_margin_ce_forward", cfg, dtype, B, N, stride);
    if (rc != MV_OK) return rc;
    if (B == 0) return MV_OK;
    MV_REQUIRE(logits != nullptr && labels != nullptr, "mv_margin_ce_forward: null logits or labels");
    MV_REQUIRE(loss != nullptr && loss_rows != nullptr && pred != nullptr && saved != nullptr, "mv_margin_ce_forward: null output");
    MV_REQUIRE(workspace != nullptr, "mv_margin_ce_forward: null workspace");
    if (workspace_bytes < margin_ws_bytes(B, N))
        return fail(MV_ERR_WORKSPACE, "mv_margin_ce_forward: workspace smaller than mv_margin_ce_workspace_bytes(B, N, K)");
    if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(MV_ERR_WORKSPACE, "mv_margin_ce_forward: workspace not 16-byte aligned");
    const MlArgs a = margin_args(cfg, logits, labels, B, N, stride);
    const int64_t n = B * a.nseg;
    MlWs w;
    w.sege = static_cast<double*>(workspace);
    w.segs = w.sege + n;
    w.segz = reinterpret_cast<float*>(w.segs + n);
    w.segc = w.segz + n;
    w.segj = reinterpret_cast<int*>(w.segc + n);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ML_DISPATCH(margin_forward_launch, a, w, loss, loss_rows, pred, saved, st);
    return check_launch("margin_seg_kernel / margin_finish_kernel");
}

extern "C" int mv_margin_ce_backward(const MvMarginLossCfg* cfg, const void* logits, int32_t dtype, const int64_t* labels, int64_t B, int64_t N,
                                     int64_t stride, const double* saved, const float* grad_out, void* out, int64_t out_stride, mv_stream_t stream) {
    using namespace mv;
    const int rc = margin_check("mv_margin_ce_backward", cfg, dtype, B, N, stride);
    if (rc != MV_OK) return rc;
    MV_REQUIRE(out_stride >= N * cfg->K, "mv_margin_ce_backward: out_stride below N * K");
    MV_REQUIRE(B == 0 || out_stride == 0 || B <= INT64_MAX / 8 / out_stride, "mv_margin_ce_backward: B * out_stride beyond int64");
    if (B == 0) return MV_OK;
    MV_REQUIRE(ceil_div(ceil_div(N, ML_CH), ML_T) <= (int64_t)0x7FFFFFFF / B, "mv_margin_ce_backward: B * column tiles above 2^31 - 1");
    MV_REQUIRE(logits != nullptr && labels != nullptr, "mv_margin_ce_backward: null logits or labels");
    MV_REQUIRE(saved != nullptr && grad_out != nullptr && out != nullptr, "mv_margin_ce_backward: null saved, grad_out or out");
    if (!(out == logits && out_stride == stride)) {   // in place is fine (a thread reads what it owns before it writes it); nothing else may overlap
        const int64_t es = dtype == MV_DT_F32 ? 4 : 2;
        const uintptr_t l0 = reinterpret_cast<uintptr_t>(logits), l1 = l0 + (uintptr_t)(((B - 1) * stride + N * cfg->K) * es);
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + (uintptr_t)(((B - 1) * out_stride + N * cfg->K) * es);
        MV_REQUIRE(o1 <= l0 || l1 <= o0, "mv_margin_ce_backward: out overlaps logits and is not the in-place form (out == logits, out_stride == stride)");
    }
    const MlArgs a = margin_args(cfg, logits, labels, B, N, stride);
    hipStream_t st = static_cast<hipStream_t>(stream);
    ML_DISPATCH(margin_backward_launch, a, saved, grad_out, out, out_stride, st);
    return check_launch("margin_backward_kernel");
}
