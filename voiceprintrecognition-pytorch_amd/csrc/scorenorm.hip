// Cohort score normalisation: per embedding the mean and standard deviation of its top-N cohort scores, and the Z / T / S(-adaptive)
// normalisation of a trials x enrolments score matrix with them.
//
// Replaces what a recipe does on the host today: an (enrol + test) x cohort matrix, a sort (or partition) of every row, mean / std of the
// best N, then the element-wise expression.  Here the n x m cohort scores never exist as a whole:
//   * the rows are walked in chunks of R; a chunk's [R, m] scores are written into the workspace by linear_f32_launch, the launcher
//     mv_cosine_f32 itself is (the same bits for a pair, whatever chunk it sits in), and R is small enough that the chunk is still in the
//     Infinity Cache when the next launch reads it;
//   * cohort_topn_stats_kernel, one workgroup per row, reduces the row to (mean, std): the row's sort keys go to LDS, four 8-bit radix-select
//     passes (integer LDS histogram atomics, as prune_cut_kernel of diarize.hip) find the key of the N'-th largest entry and how many entries
//     equal to it belong to the selection, a tie pass gives those to the lowest indices, and two fp64 passes over the kept entries give the
//     sums;
//   * score_norm_kernel is one element-wise launch.
// No workgroup waits for another, no atomics on floats, nothing is allocated and nothing synchronises.
//
// The summation order (the contract of include/mvector_hip.h): the workgroup of a row has T threads (T from m alone: CS_TIER_*); thread t owns
// the indices [t * seg, (t + 1) * seg), seg = ceil(m / T) made odd (consecutive threads then read consecutive LDS banks), and adds its kept
// entries in ascending index order; the T partial sums are folded by a halving tree (red[t] += red[t + s], s = T / 2 .. 1).
#include "kernels.h"
#include "order_key.h"

namespace mv {

// T by the measured time of the kernel alone over 8192 rows ("Score normalisation"): 256 threads win up to 4096 keys (0.13 ms against
// 0.15 / 0.22 ms with 512 / 1024), 512 threads from 6000 to 12000 (0.44 against 0.55 / 0.45 ms at 12000), 1024 threads from 16384 on (0.54 against
// 0.61 ms with 512; 1.27 against 1.78 / 2.90 ms at 32768)
constexpr int CS_TIER_SMALL = 4096;     // keys at most: 256 threads, <= 16 KiB of keys -- eight workgroups per compute unit
constexpr int CS_TIER_MID = 12288;      // 512 threads, <= 48 KiB -- two or three workgroups per compute unit
                                        // above: 1024 threads -- two workgroups up to 16384 keys (64 KiB), one up to 32768 (128 KiB)
constexpr int64_t CS_CHUNK_BYTES = 64ll << 20;   // a chunk's scores: a quarter of the 256 MiB Infinity Cache

// rows per chunk: `hint` when positive, else what CS_CHUNK_BYTES holds (a multiple of 16, the row tile of the cosine kernel); never more than n
static int64_t cohort_chunk_rows(int64_t n, int64_t m, int hint) {
    int64_t r = hint > 0 ? hint : (CS_CHUNK_BYTES / (m * 4)) & ~(int64_t)15;
    const int64_t rows = n > 0 ? n : 1;
    return r < rows ? r : rows;
}

// sum over the workgroup's T threads by the halving tree; the result is returned to every thread (red is free again on return)
template <int T>
__device__ __forceinline__ double tree_sum(double* red, double v, int tid) {
    red[tid] = v;
    __syncthreads();
#pragma unroll 1
    for (int s = T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double total = red[0];
    __syncthreads();
    return total;
}

// grid (rows).  scores [rows][m]: the chunk of cosine scores; mean / stdv [rows].  Dynamic LDS: the row's m keys.
template <int T>
__global__ __launch_bounds__(T) void cohort_topn_stats_kernel(const float* scores, int m, int top_n, float* mean, float* stdv) {
    static_assert(T >= 256 && T % 64 == 0, "the digit scan uses wave 0, the histogram is cleared by the first 256 threads");
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[T / 64];
    __shared__ unsigned sel[2];   // chosen high bits; rank left among the keys that share them (0 = the largest)
    __shared__ double red[T];
    MV_DYN_SMEM(smem);
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* src = scores + (int64_t)blockIdx.x * m;
    for (int j = tid; j < m; j += T) keys[j] = sort_key(src[j]);
    const int np = top_n < m ? top_n : m;   // N'
    if (tid == 0) sel[0] = 0u, sel[1] = (unsigned)(np - 1);
    // ---- the key of the N'-th largest entry: one byte per pass, digits walked from 255 down
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t high = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();   // (also: the keys, and sel of the pass before)
        const uint32_t prefix = sel[0];
        const unsigned rank = sel[1];
        for (int j = tid; j < m; j += T) {
            const uint32_t k = keys[j];
            if ((k & high) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);   // integer counts: order-free
        }
        __syncthreads();
        if (wave == 0) {   // lane l takes the digits 255 - 4 l .. 252 - 4 l; an inclusive scan over the lanes gives the entries above them
            const int d0 = 255 - 4 * lane;
            unsigned c[4], own = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[e] = hist[d0 - e];
                own += c[e];
            }
            unsigned incl = own;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned v = __shfl_up(incl, (unsigned)off);
                if (lane >= off) incl += v;
            }
            unsigned cum = incl - own;
#pragma unroll
            for (int e = 0; e < 4; ++e) {   // exactly one digit holds the rank (rank < entries that share the prefix)
                if (rank >= cum && rank < cum + c[e]) {
                    sel[0] = prefix | ((uint32_t)(d0 - e) << shift);
                    sel[1] = rank - cum;
                }
                cum += c[e];
            }
        }
        __syncthreads();
    }
    const uint32_t cut = sel[0];
    const unsigned need = sel[1] + 1u;   // entries equal to the cut that belong to the selection: the lowest indices
    // ---- ties: how many entries equal to the cut lie in front of this thread's segment
    const int seg = ((m + T - 1) / T) | 1;
    const int lo = tid * seg < m ? tid * seg : m, hi = lo + seg < m ? lo + seg : m;
    unsigned own = 0u;
    for (int j = lo; j < hi; ++j) own += keys[j] == cut ? 1u : 0u;
    unsigned incl = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned v = __shfl_up(incl, (unsigned)off);
        if (lane >= off) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned before = incl - own;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    // ---- mean, then the centred squares: fp64, the thread's kept entries in ascending index order, then the tree
    double s = 0.0;
    unsigned seen = before;
    for (int j = lo; j < hi; ++j) {
        const uint32_t k = keys[j];
        if (k > cut || (k == cut && seen++ < need)) s += (double)sort_key_value(k);
    }
    const double mu = tree_sum<T>(red, s, tid) / (double)np;
    double q = 0.0;
    seen = before;
    for (int j = lo; j < hi; ++j) {
        const uint32_t k = keys[j];
        if (k > cut || (k == cut && seen++ < need)) {
            const double d = (double)sort_key_value(k) - mu;
            q = __builtin_fma(d, d, q);
        }
    }
    const double var = tree_sum<T>(red, q, tid) / (double)np;
    if (tid == 0) {
        mean[blockIdx.x] = (float)mu;
        stdv[blockIdx.x] = (float)sqrt(var);
    }
}

static int cohort_stats_launch(const float* scores, int rows, int m, int top_n, float* mean, float* stdv, hipStream_t st) {
    const size_t lds = (size_t)round_up((int64_t)m * 4, 16);
    if (m <= CS_TIER_SMALL) {
        MV_LAUNCH(cohort_topn_stats_kernel<256>, ((unsigned)rows, 1, 1), (256, 1, 1), lds, st, scores, m, top_n, mean, stdv);
    } else if (m <= CS_TIER_MID) {
        MV_LAUNCH(cohort_topn_stats_kernel<512>, ((unsigned)rows, 1, 1), (512, 1, 1), lds, st, scores, m, top_n, mean, stdv);
    } else {
        if (MV_SET_MAX_SMEM(cohort_topn_stats_kernel<1024>, MV_COHORT_MAX_ROWS * 4) != hipSuccess)
            return fail(MV_ERR_HIP, "mv_cohort_stats_f32: cannot reserve dynamic LDS for cohort_topn_stats_kernel");
        MV_LAUNCH(cohort_topn_stats_kernel<1024>, ((unsigned)rows, 1, 1), (1024, 1, 1), lds, st, scores, m, top_n, mean, stdv);
    }
    return check_launch("cohort_topn_stats_kernel");
}

static int cohort_stats_check(int64_t n, int64_t m, int dim, int top_n) {
    MV_REQUIRE(n >= 0, "mv_cohort_stats_f32: negative n");
    MV_REQUIRE(m >= 1, "mv_cohort_stats_f32: m below 1");
    MV_REQUIRE(top_n >= 1, "mv_cohort_stats_f32: top_n below 1");
    MV_REQUIRE(dim >= 1, "mv_cohort_stats_f32: dim below 1");
    if (m > MV_COHORT_MAX_ROWS) return fail(MV_ERR_UNSUPPORTED, "mv_cohort_stats_f32: m above MV_COHORT_MAX_ROWS (32768: the keys of a row live in one workgroup's LDS)");
    return MV_OK;
}

// ------------------------------------------------------------------------------------------------ normalisation
// every operation one correctly rounded fp32 operation, in the order of the header
__device__ __forceinline__ float snorm_value(float s, uint32_t t, uint32_t e, const float* tm, const float* ts, const float* em, const float* es, int mode) {
#pragma clang fp contract(off)
    if (mode == MV_SNORM_Z) return (s - em[e]) / es[e];
    if (mode == MV_SNORM_T) return (s - tm[t]) / ts[t];
    const float a = (s - tm[t]) / ts[t];
    const float b = (s - em[e]) / es[e];
    return 0.5f * (a + b);
}

// the matrix as one array of `total` floats: [head, head + 4 nvec) in 16-byte pieces, one per thread; the total - 4 nvec elements in front
// of and behind them one per thread.  Every element is read by the thread that writes it, before it does: out == scores is fine.
__global__ __launch_bounds__(256) void score_norm_kernel(const float* scores, uint32_t total, uint32_t ne, const float* tm, const float* ts, const float* em,
                                                         const float* es, int mode, float* out, uint32_t head, uint32_t nvec) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid < nvec) {
        const uint32_t idx = head + 4u * gid;
        const float4v v = *reinterpret_cast<const float4v*>(scores + idx);
        uint32_t t = idx / ne, e = idx - t * ne;
        float4v r;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            r[c] = snorm_value(v[c], t, e, tm, ts, em, es, mode);
            if (++e == ne) e = 0u, ++t;
        }
        *reinterpret_cast<float4v*>(out + idx) = r;
    }
    if (gid < total - 4u * nvec) {
        const uint32_t idx = gid < head ? gid : gid + 4u * nvec;
        const uint32_t t = idx / ne, e = idx - t * ne;
        out[idx] = snorm_value(scores[idx], t, e, tm, ts, em, es, mode);
    }
}

}  // namespace mv

extern "C" size_t mv_cohort_stats_workspace_bytes(int32_t n, int32_t m, int32_t dim, int32_t rows_hint) {
    if (mv::cohort_stats_check(n, m, dim, 1) != MV_OK) return 0;
    return (size_t)mv::cohort_chunk_rows(n, m, rows_hint) * (size_t)m * 4;
}

extern "C" int mv_cohort_stats_f32(const float* x, int32_t n, const float* cohort, int32_t m, int32_t dim, int32_t top_n, float* mean, float* std,
                                   int32_t rows_hint, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    const int rc = cohort_stats_check(n, m, dim, top_n);
    if (rc != MV_OK) return rc;
    if (n == 0) return MV_OK;
    MV_REQUIRE(x != nullptr && cohort != nullptr && mean != nullptr && std != nullptr, "mv_cohort_stats_f32: null tensor");
    MV_REQUIRE(workspace != nullptr, "mv_cohort_stats_f32: null workspace");
    const int64_t R = cohort_chunk_rows(n, m, rows_hint);
    if (workspace_bytes < (size_t)R * (size_t)m * 4)
        return fail(MV_ERR_WORKSPACE, "mv_cohort_stats_f32: workspace smaller than mv_cohort_stats_workspace_bytes(n, m, dim, rows_hint)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 4 == 0, "mv_cohort_stats_f32: workspace not 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* chunk = static_cast<float*>(workspace);
    for (int64_t r0 = 0; r0 < n; r0 += R) {
        const int rows = (int)(n - r0 < R ? n - r0 : R);
        int rcl = linear_f32_launch(x + r0 * dim, dim, cohort, dim, nullptr, MV_ACT_NONE, chunk, m, rows, dim, m, 1, st);   // what mv_cosine_f32 runs
        if (rcl != MV_OK) return rcl;
        rcl = cohort_stats_launch(chunk, rows, m, top_n, mean + r0, std + r0, st);
        if (rcl != MV_OK) return rcl;
    }
    return MV_OK;
}

extern "C" int mv_score_norm_f32(const float* scores, int64_t n_trials, int64_t n_enroll, const float* trial_mean, const float* trial_std,
                                 const float* enroll_mean, const float* enroll_std, int32_t mode, float* out, mv_stream_t stream) {
    using namespace mv;
    MV_REQUIRE(n_trials >= 0 && n_enroll >= 0, "mv_score_norm_f32: negative n_trials or n_enroll");
    MV_REQUIRE(mode == MV_SNORM_S || mode == MV_SNORM_Z || mode == MV_SNORM_T, "mv_score_norm_f32: unknown mode (MV_SNORM_S, MV_SNORM_Z or MV_SNORM_T)");
    MV_REQUIRE(n_trials == 0 || n_enroll <= (int64_t)0x7FFFFFFF / n_trials, "mv_score_norm_f32: more than 2^31 - 1 elements");
    if (n_trials == 0 || n_enroll == 0) return MV_OK;
    MV_REQUIRE(scores != nullptr && out != nullptr, "mv_score_norm_f32: null tensor");
    MV_REQUIRE(mode == MV_SNORM_Z || (trial_mean != nullptr && trial_std != nullptr), "mv_score_norm_f32: null trial statistics");
    MV_REQUIRE(mode == MV_SNORM_T || (enroll_mean != nullptr && enroll_std != nullptr), "mv_score_norm_f32: null enrolment statistics");
    const uint32_t total = (uint32_t)(n_trials * n_enroll);
    // 16-byte pieces where both pointers reach a 16-byte boundary after the same number of floats
    const uintptr_t a = reinterpret_cast<uintptr_t>(scores), b = reinterpret_cast<uintptr_t>(out);
    uint32_t head = total, nvec = 0;
    if (a % 4 == 0 && a % 16 == b % 16) {
        const uint32_t h = (uint32_t)(((16 - a % 16) % 16) / 4);
        if (h <= total) head = h, nvec = (total - h) / 4;
    }
    const uint32_t rest = total - 4 * nvec;
    const uint32_t threads = nvec > rest ? nvec : rest;
    MV_LAUNCH(score_norm_kernel, ((unsigned)ceil_div(threads, 256), 1, 1), (256, 1, 1), 0, static_cast<hipStream_t>(stream), scores, total, (uint32_t)n_enroll,
              trial_mean, trial_std, enroll_mean, enroll_std, mode, out, head, nvec);
    return check_launch("score_norm_kernel");
}
