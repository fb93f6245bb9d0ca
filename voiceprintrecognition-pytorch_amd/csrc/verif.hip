// Verification metrics of an evaluation on the device: a stable key-value radix sort of the fp32 trial scores and one scan over the
// sorted sequence that yields what EER, minDCF and the threshold are made of.
//
// The reference (mvector/metric/metrics.py behind MVectorTrainer.evaluate) argsorts all N = trials x enrolments scores on the host, gathers an
// N-sized label array, runs two fp64 cumulative sums and sorts a second time to read one threshold.  Here:
//   mv_sort_scores_f32    LSD radix sort over four 8-bit digits of sort_key (order_key.h; NaNs last), each key travelling with its flat
//                         index.  One pass = five ordinary launches on the caller's stream:
//                           sort_count_kernel    per tile of VS_TILE keys the 256 digit counts (integer LDS atomics) -> table[digit][tile]
//                           scan_sums_kernel     sum of every chunk of VS_SCAN_CHUNK table entries
//                           scan_top_kernel      one workgroup: exclusive scan of the chunk sums, as many trips of 256 as it takes
//                           scan_apply_kernel    exclusive scan inside every chunk on top of its chunk's offset, in place
//                           sort_scatter_kernel  the tile is sorted by the digit inside LDS -- two stable 4-bit splits, each ranked by per-thread
//                                                digit counts and an LDS scan of the [16][256] count table -- and written out by striped lanes,
//                                                so that the lanes of a wave store runs of consecutive addresses per digit
//                         The table is digit-major, so its exclusive scan IS the global offset of (digit, tile); every pass is stable, the
//                         result has the order of numpy.argsort(kind='stable').
//   mv_verif_metrics_f32  the sort, then per sorted position the label recomputed from the index (trial_labels[idx / n_enroll] ==
//                         enroll_labels[idx % n_enroll]): targets per tile, scan_top_kernel over the tile counts, then T_i and the fp64
//                         rates per position (contraction off: each operation rounds once, as numpy's array operations do), per-tile
//                         partials and one finishing workgroup.
// DESIGN CONSTRAINT: no workgroup ever waits for another workgroup -- no look-back, no flags, no spinning on global memory.  The stream
// orders the launches and that is the only ordering used.  No floating-point atomics: results are bit-identical on every run and stream.
#include "common.h"
#include "order_key.h"

namespace mv {
namespace {

constexpr int VS_THREADS = 256;
constexpr int VS_ITEMS = 16;                          // keys per thread
constexpr int VS_TILE = VS_THREADS * VS_ITEMS;        // 4096 keys: 32 KiB of keys and indices + 16 KiB of counts in LDS
constexpr int VS_DIGITS = 256;                        // 8-bit digits, four passes
constexpr int VS_SCAN_ITEMS = 4;
constexpr int VS_SCAN_CHUNK = VS_THREADS * VS_SCAN_ITEMS;  // table entries per workgroup of the scan
constexpr int64_t VS_MAX_N = 2147483647;              // indices and counts are 32-bit
constexpr uint32_t VS_NONE = 0xFFFFFFFFu;

// exclusive prefix of one value per thread over the 256 threads of the block, *total = their sum.  wave_tot: 4 LDS words.
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned* wave_tot, unsigned* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, (unsigned)d);
        if (lane >= d) inc += o;
    }
    __syncthreads();  // the previous use of wave_tot has been read
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    unsigned base = 0u, tot = 0u;
    for (int k = 0; k < VS_THREADS / 64; ++k) {
        const unsigned t = wave_tot[k];
        base += k < w ? t : 0u;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------------ sort
// table[digit * tiles + tile] = keys of the tile with that digit; the first pass reads the scores themselves
__global__ __launch_bounds__(256) void sort_count_kernel(const uint32_t* keys, const float* scores, int64_t N, int shift, unsigned tiles,
                                                         uint32_t* table) {
    __shared__ unsigned hist[VS_DIGITS];
    const int tid = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const int64_t base = (int64_t)tile * VS_TILE;
    hist[tid] = 0u;
    __syncthreads();
    if (scores != nullptr) {
        for (int i = 0; i < VS_ITEMS; ++i) {
            const int64_t g = base + i * VS_THREADS + tid;
            if (g < N) atomicAdd(&hist[(sort_key(scores[g]) >> shift) & 255u], 1u);  // integer counts: order-free
        }
    } else {
        for (int i = 0; i < VS_ITEMS; ++i) {
            const int64_t g = base + i * VS_THREADS + tid;
            if (g < N) atomicAdd(&hist[(keys[g] >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    table[(int64_t)tid * tiles + tile] = hist[tid];
}

__global__ __launch_bounds__(256) void scan_sums_kernel(const uint32_t* a, int64_t n, uint32_t* sums) {
    __shared__ unsigned wave_tot[4];
    const int64_t first = (int64_t)blockIdx.x * VS_SCAN_CHUNK + threadIdx.x * VS_SCAN_ITEMS;
    unsigned s = 0u;
    for (int j = 0; j < VS_SCAN_ITEMS; ++j) s += first + j < n ? a[first + j] : 0u;
    unsigned total;
    block_excl_scan(s, wave_tot, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: a[0 .. n) -> its exclusive prefix sums in place, a[n] = the total; trips of 256 entries with a running carry
__global__ __launch_bounds__(256) void scan_top_kernel(uint32_t* a, int64_t n) {
    __shared__ unsigned wave_tot[4];
    unsigned carry = 0u;
    for (int64_t first = 0; first < n; first += VS_THREADS) {
        const int64_t i = first + threadIdx.x;
        const unsigned v = i < n ? a[i] : 0u;
        unsigned total;
        const unsigned ex = block_excl_scan(v, wave_tot, &total);
        if (i < n) a[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) a[n] = carry;
}

__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t* a, int64_t n, const uint32_t* sums) {
    __shared__ unsigned wave_tot[4];
    const int64_t first = (int64_t)blockIdx.x * VS_SCAN_CHUNK + threadIdx.x * VS_SCAN_ITEMS;
    unsigned v[VS_SCAN_ITEMS], s = 0u;
#pragma unroll
    for (int j = 0; j < VS_SCAN_ITEMS; ++j) {
        v[j] = first + j < n ? a[first + j] : 0u;
        s += v[j];
    }
    unsigned total;
    unsigned run = sums[blockIdx.x] + block_excl_scan(s, wave_tot, &total);
#pragma unroll
    for (int j = 0; j < VS_SCAN_ITEMS; ++j) {
        if (first + j < n) a[first + j] = run;
        run += v[j];
    }
}

// One tile: sorted by the pass's digit inside LDS (stable), then every key to table[digit][tile] + its rank among the tile's keys of that
// digit.  First pass: scores != NULL, the keys are made here and the values are the flat indices.  Last pass: scores_out != NULL takes the
// floats back instead of keys_out.
__global__ __launch_bounds__(256) void sort_scatter_kernel(const uint32_t* keys_in, const uint32_t* vals_in, const float* scores, int64_t N,
                                                           int shift, unsigned tiles, const uint32_t* table, uint32_t* keys_out,
                                                           uint32_t* vals_out, float* scores_out) {
    __shared__ uint32_t sk[VS_TILE];
    __shared__ uint32_t sv[VS_TILE];
    __shared__ unsigned cnt[16 * VS_THREADS];  // [nibble][thread]: flattened, its exclusive scan is the stable rank of the thread's first key of that nibble
    __shared__ unsigned wave_tot[4];
    __shared__ unsigned start[VS_DIGITS];
    __shared__ unsigned gbase[VS_DIGITS];
    const int tid = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const int64_t base = (int64_t)tile * VS_TILE;
    const int count = N - base < VS_TILE ? (int)(N - base) : VS_TILE;
    // coalesced in; the places past the end hold the largest key behind every real one, and a stable sort leaves them there
    if (scores != nullptr) {
        for (int i = 0; i < VS_ITEMS; ++i) {
            const int p = i * VS_THREADS + tid;
            sk[p] = p < count ? sort_key(scores[base + p]) : 0xFFFFFFFFu;
            sv[p] = (uint32_t)(base + p);
        }
    } else {
        for (int i = 0; i < VS_ITEMS; ++i) {
            const int p = i * VS_THREADS + tid;
            sk[p] = p < count ? keys_in[base + p] : 0xFFFFFFFFu;
            sv[p] = p < count ? vals_in[base + p] : 0u;
        }
    }
    gbase[tid] = table[(int64_t)tid * tiles + tile];
    __syncthreads();

    for (int half = 0; half < 2; ++half) {
        const int sh = shift + 4 * half;
        uint32_t k[VS_ITEMS], v[VS_ITEMS];
#pragma unroll
        for (int j = 0; j < VS_ITEMS; ++j) {  // thread tid owns places 16 tid .. 16 tid + 15
            k[j] = sk[tid * VS_ITEMS + j];
            v[j] = sv[tid * VS_ITEMS + j];
        }
#pragma unroll
        for (int d = 0; d < 16; ++d) cnt[d * VS_THREADS + tid] = 0u;
#pragma unroll
        for (int j = 0; j < VS_ITEMS; ++j) cnt[((k[j] >> sh) & 15u) * VS_THREADS + tid] += 1u;  // the thread's own column: no atomics
        __syncthreads();
        unsigned loc[16], s = 0u;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            loc[e] = cnt[16 * tid + e];
            s += loc[e];
        }
        unsigned total;
        unsigned run = block_excl_scan(s, wave_tot, &total);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            cnt[16 * tid + e] = run;
            run += loc[e];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < VS_ITEMS; ++j) {
            const unsigned slot = ((k[j] >> sh) & 15u) * VS_THREADS + tid;
            const unsigned pos = cnt[slot];
            cnt[slot] = pos + 1u;
            sk[pos] = k[j];
            sv[pos] = v[j];
        }
        __syncthreads();
    }

    for (int i = 0; i < VS_ITEMS; ++i) {  // where each digit's run starts in the sorted tile
        const int p = i * VS_THREADS + tid;
        const unsigned d = (sk[p] >> shift) & 255u;
        if (p == 0 || ((sk[p - 1] >> shift) & 255u) != d) start[d] = (unsigned)p;
    }
    __syncthreads();
    for (int i = 0; i < VS_ITEMS; ++i) {
        const int p = i * VS_THREADS + tid;
        if (p < count) {
            const uint32_t key = sk[p];
            const unsigned d = (key >> shift) & 255u;
            const int64_t dst = (int64_t)gbase[d] + ((unsigned)p - start[d]);
            if (dst < N) {  // always, with a table that is the scan of the counts
                if (scores_out != nullptr) {
                    scores_out[dst] = sort_key_value(key);
                } else {
                    keys_out[dst] = key;
                }
                vals_out[dst] = sv[p];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ metrics
__device__ __forceinline__ unsigned is_target(uint32_t idx, int64_t N, uint32_t n_enroll, const int32_t* trial_labels,
                                              const int32_t* enroll_labels) {
    if (idx >= N) return 0u;  // never, with an index that came out of the sort: no label is read outside its vector
    const uint32_t t = idx / n_enroll;
    return trial_labels[t] == enroll_labels[idx - t * n_enroll] ? 1u : 0u;
}

// x itself, through bits the optimiser cannot follow (`zero` is a value it cannot prove to be 0, which it always is): a product that
// went through here cannot be fused with the addition behind it
__device__ __forceinline__ double rounded(double x, uint64_t zero) { return __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, x) ^ zero); }

// The reference's expressions, one rounding per operation: a fused c is no longer numpy's number.  The pragma is what the device build
// honours; a host build with -ffp-contract=fast (the test-suite's emulator) fuses in its backend whatever the pragma says, hence rounded().
__device__ __forceinline__ void rates_at(uint32_t T, uint32_t I, double nt, double ni, double p_target, double q_target, double c_miss,
                                         double c_fa, uint64_t zero, double* gap, double* cost) {
#pragma clang fp contract(off)
    const double fnr = (double)T / nt;
    const double fpr = 1.0 - (double)I / ni;
    *gap = fnr - fpr;
    const double miss = rounded((c_miss * fnr) * p_target, zero), fa = rounded((c_fa * fpr) * q_target, zero);
    *cost = miss + fa;
}

struct VerifPart {
    double cost;    // min c_i
    uint32_t i1;    // first position with gap >= 0, VS_NONE: none
    uint32_t t1;    // T there
    uint32_t i2p1;  // last position with gap < 0, plus one; 0: none
    uint32_t t2;
};

// commutative and exact: smallest i1, largest i2, smallest cost
__device__ __forceinline__ void part_merge(VerifPart& a, const VerifPart& b) {
    if (b.i1 < a.i1) a.i1 = b.i1, a.t1 = b.t1;
    if (b.i2p1 > a.i2p1) a.i2p1 = b.i2p1, a.t2 = b.t2;
    a.cost = b.cost < a.cost ? b.cost : a.cost;
}

__device__ __forceinline__ VerifPart block_part_merge(VerifPart mine, VerifPart* red) {
    const int tid = threadIdx.x;
    red[tid] = mine;
    __syncthreads();
    for (int st = VS_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            VerifPart a = red[tid];
            part_merge(a, red[tid + st]);
            red[tid] = a;
        }
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void verif_count_kernel(const uint32_t* index, int64_t N, uint32_t n_enroll, const int32_t* trial_labels,
                                                          const int32_t* enroll_labels, uint32_t* tile_count) {
    __shared__ unsigned wave_tot[4];
    const int64_t base = (int64_t)blockIdx.x * VS_TILE;
    unsigned s = 0u;
    for (int i = 0; i < VS_ITEMS; ++i) {
        const int64_t g = base + i * VS_THREADS + threadIdx.x;
        if (g < N) s += is_target(index[g], N, n_enroll, trial_labels, enroll_labels);
    }
    unsigned total;
    block_excl_scan(s, wave_tot, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// tile_off: exclusive scan of the tile counts, tile_off[tiles] = NT
__global__ __launch_bounds__(256) void verif_scan_kernel(const uint32_t* index, int64_t N, uint32_t n_enroll, const int32_t* trial_labels,
                                                         const int32_t* enroll_labels, const uint32_t* tile_off, unsigned tiles, double p_target,
                                                         double q_target, double c_miss, double c_fa, uint32_t* tgt_cum, VerifPart* parts) {
    __shared__ unsigned char lab[VS_TILE];
    __shared__ uint32_t tcum[VS_TILE];
    __shared__ unsigned wave_tot[4];
    __shared__ VerifPart red[VS_THREADS];
    const int tid = threadIdx.x;
    const unsigned tile = blockIdx.x;
    const int64_t base = (int64_t)tile * VS_TILE;
    const int count = N - base < VS_TILE ? (int)(N - base) : VS_TILE;
    for (int i = 0; i < VS_ITEMS; ++i) {  // coalesced reads of the index, labels to LDS
        const int p = i * VS_THREADS + tid;
        lab[p] = p < count ? (unsigned char)is_target(index[base + p], N, n_enroll, trial_labels, enroll_labels) : 0;
    }
    __syncthreads();
    unsigned l[VS_ITEMS], s = 0u;
#pragma unroll
    for (int j = 0; j < VS_ITEMS; ++j) {  // thread tid owns places 16 tid .. 16 tid + 15
        l[j] = lab[tid * VS_ITEMS + j];
        s += l[j];
    }
    unsigned total;
    uint32_t T = tile_off[tile] + block_excl_scan(s, wave_tot, &total);
    const uint32_t n_target = tile_off[tiles];
    const double nt = (double)n_target, ni = (double)(uint32_t)(N - n_target);
    const uint64_t zero = (int64_t)n_target > N ? 1u : 0u;  // never: a count of N labels (see rounded())
    VerifPart mine = {INFINITY, VS_NONE, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < VS_ITEMS; ++j) {
        const int p = tid * VS_ITEMS + j;
        T += l[j];
        if (tgt_cum != nullptr) tcum[p] = T;
        if (p < count) {
            const uint32_t g = (uint32_t)(base + p);
            double gap, cost;
            rates_at(T, g + 1u - T, nt, ni, p_target, q_target, c_miss, c_fa, zero, &gap, &cost);
            if (gap >= 0.0) {
                if (mine.i1 == VS_NONE) mine.i1 = g, mine.t1 = T;
            } else if (gap < 0.0) {
                mine.i2p1 = g + 1u, mine.t2 = T;
            }
            mine.cost = cost < mine.cost ? cost : mine.cost;
        }
    }
    const VerifPart all = block_part_merge(mine, red);  // its barriers also cover tcum
    if (tid == 0) parts[tile] = all;
    if (tgt_cum != nullptr) {
        for (int i = 0; i < VS_ITEMS; ++i) {
            const int p = i * VS_THREADS + tid;
            if (p < count) tgt_cum[base + p] = tcum[p];
        }
    }
}

struct VerifDevResult {
    uint32_t n_target, i1, t1, i2p1, t2;
    float score_i1;
    double cost;
};

__global__ __launch_bounds__(256) void verif_finish_kernel(const VerifPart* parts, unsigned tiles, const uint32_t* tile_off, const float* sorted_scores,
                                                           VerifDevResult* out) {
    __shared__ VerifPart red[VS_THREADS];
    VerifPart mine = {INFINITY, VS_NONE, 0u, 0u, 0u};
    for (unsigned t = threadIdx.x; t < tiles; t += VS_THREADS) part_merge(mine, parts[t]);
    const VerifPart all = block_part_merge(mine, red);
    if (threadIdx.x == 0) {
        out->n_target = tile_off[tiles];
        out->i1 = all.i1, out->t1 = all.t1, out->i2p1 = all.i2p1, out->t2 = all.t2;
        out->score_i1 = all.i1 != VS_NONE ? sorted_scores[all.i1] : 0.0f;
        out->cost = all.cost;
    }
}

// ------------------------------------------------------------------------------------------------ host side
#define VS_TRY(expr)                   \
    do {                               \
        const int _rc = (expr);        \
        if (_rc != MV_OK) return _rc;  \
    } while (0)

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct SortPlan {
    unsigned tiles;
    int64_t entries, chunks;
    size_t off_keys, off_vals, off_table, off_sums, total;
};

SortPlan sort_plan(int64_t N) {
    SortPlan p;
    p.tiles = (unsigned)ceil_div(N, VS_TILE);
    p.entries = (int64_t)p.tiles * VS_DIGITS;
    p.chunks = ceil_div(p.entries, VS_SCAN_CHUNK);
    size_t off = 0;
    p.off_keys = off, off += align256((size_t)N * sizeof(uint32_t));
    p.off_vals = off, off += align256((size_t)N * sizeof(uint32_t));
    p.off_table = off, off += align256((size_t)p.entries * sizeof(uint32_t));
    p.off_sums = off, off += align256((size_t)(p.chunks + 1) * sizeof(uint32_t));
    p.total = off;
    return p;
}

// scores -> (A) -> (B = the output buffers, as keys) -> (A) -> the outputs, the scores as floats again
int sort_run(const float* scores, int64_t N, float* out_scores, uint32_t* out_index, char* ws, hipStream_t st) {
    const SortPlan p = sort_plan(N);
    uint32_t* keys_a = reinterpret_cast<uint32_t*>(ws + p.off_keys);
    uint32_t* vals_a = reinterpret_cast<uint32_t*>(ws + p.off_vals);
    uint32_t* keys_b = reinterpret_cast<uint32_t*>(out_scores);
    uint32_t* table = reinterpret_cast<uint32_t*>(ws + p.off_table);
    uint32_t* sums = reinterpret_cast<uint32_t*>(ws + p.off_sums);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 8 * pass;
        const bool to_a = pass % 2 == 0;
        const float* in_scores = pass == 0 ? scores : nullptr;
        const uint32_t* in_keys = pass == 0 ? nullptr : (to_a ? keys_b : keys_a);
        const uint32_t* in_vals = pass == 0 ? nullptr : (to_a ? out_index : vals_a);
        float* last_scores = pass == 3 ? out_scores : nullptr;
        uint32_t* to_keys = pass == 3 ? nullptr : (to_a ? keys_a : keys_b);
        uint32_t* to_vals = to_a ? vals_a : out_index;
        MV_LAUNCH(sort_count_kernel, (p.tiles, 1, 1), (VS_THREADS, 1, 1), 0, st, in_keys, in_scores, N, shift, p.tiles, table);
        VS_TRY(check_launch("sort_count_kernel"));
        MV_LAUNCH(scan_sums_kernel, ((unsigned)p.chunks, 1, 1), (VS_THREADS, 1, 1), 0, st, (const uint32_t*)table, p.entries, sums);
        VS_TRY(check_launch("scan_sums_kernel"));
        MV_LAUNCH(scan_top_kernel, (1, 1, 1), (VS_THREADS, 1, 1), 0, st, sums, p.chunks);
        VS_TRY(check_launch("scan_top_kernel"));
        MV_LAUNCH(scan_apply_kernel, ((unsigned)p.chunks, 1, 1), (VS_THREADS, 1, 1), 0, st, table, p.entries, (const uint32_t*)sums);
        VS_TRY(check_launch("scan_apply_kernel"));
        MV_LAUNCH(sort_scatter_kernel, (p.tiles, 1, 1), (VS_THREADS, 1, 1), 0, st, in_keys, in_vals, in_scores, N, shift, p.tiles,
                  (const uint32_t*)table, to_keys, to_vals, last_scores);
        VS_TRY(check_launch("sort_scatter_kernel"));
    }
    return MV_OK;
}

struct VerifPlan {
    int64_t N;
    unsigned tiles;
    size_t off_sort, off_scores, off_index, off_tiles, off_parts, off_result, total;
};

// false: a shape the entry points refuse
bool verif_plan(int64_t n_trials, int64_t n_enroll, VerifPlan* out) {
    if (n_trials < 1 || n_enroll < 1 || n_trials > VS_MAX_N || n_enroll > VS_MAX_N || n_trials * n_enroll > VS_MAX_N) return false;
    VerifPlan p;
    p.N = n_trials * n_enroll;
    p.tiles = (unsigned)ceil_div(p.N, VS_TILE);
    size_t off = 0;
    p.off_sort = off, off += sort_plan(p.N).total;
    p.off_scores = off, off += align256((size_t)p.N * sizeof(float));
    p.off_index = off, off += align256((size_t)p.N * sizeof(uint32_t));
    p.off_tiles = off, off += align256((size_t)(p.tiles + 1) * sizeof(uint32_t));
    p.off_parts = off, off += align256((size_t)p.tiles * sizeof(VerifPart));
    p.off_result = off, off += align256(sizeof(VerifDevResult));
    p.total = off;
    *out = p;
    return true;
}

}  // namespace
}  // namespace mv

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int32_t mv_sort_scores_tile(void) { return mv::VS_TILE; }

extern "C" size_t mv_sort_scores_workspace_bytes(int64_t N) { return N >= 1 && N <= mv::VS_MAX_N ? mv::sort_plan(N).total : 0; }

extern "C" int mv_sort_scores_f32(const float* scores, int64_t N, float* sorted_scores, uint32_t* sorted_index, void* workspace,
                                  size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(N >= 1 && N <= mv::VS_MAX_N, "mv_sort_scores_f32: N outside 1 .. 2^31 - 1");
    MV_REQUIRE(scores != nullptr && sorted_scores != nullptr && sorted_index != nullptr && scores != sorted_scores,
               "mv_sort_scores_f32: null or aliased buffer");
    MV_REQUIRE(workspace != nullptr, "mv_sort_scores_f32: null workspace");
    if (workspace_bytes < mv_sort_scores_workspace_bytes(N))
        return mv::fail(MV_ERR_WORKSPACE, "mv_sort_scores_f32: workspace smaller than mv_sort_scores_workspace_bytes(N)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mv_sort_scores_f32: workspace not 16-byte aligned");
    return mv::sort_run(scores, N, sorted_scores, sorted_index, static_cast<char*>(workspace), static_cast<hipStream_t>(stream));
}

extern "C" size_t mv_verif_metrics_workspace_bytes(int64_t n_trials, int64_t n_enroll) {
    mv::VerifPlan p;
    return mv::verif_plan(n_trials, n_enroll, &p) ? p.total : 0;
}

extern "C" int mv_verif_metrics_f32(const float* scores, int64_t n_trials, int64_t n_enroll, const int32_t* trial_labels,
                                    const int32_t* enroll_labels, const MvVerifCfg* cfg, MvVerifResult* result, float* sorted_scores,
                                    uint32_t* tgt_cum, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    VerifPlan p;
    MV_REQUIRE(n_trials >= 1 && n_enroll >= 1, "mv_verif_metrics_f32: no trials (N = 0)");
    MV_REQUIRE(verif_plan(n_trials, n_enroll, &p), "mv_verif_metrics_f32: N = n_trials * n_enroll outside 1 .. 2^31 - 1");
    MV_REQUIRE(scores != nullptr && trial_labels != nullptr && enroll_labels != nullptr && result != nullptr && scores != sorted_scores,
               "mv_verif_metrics_f32: null or aliased buffer");
    MV_REQUIRE(cfg != nullptr, "mv_verif_metrics_f32: null cfg");
    MV_REQUIRE(cfg->p_target > 0.0 && cfg->p_target < 1.0, "mv_verif_metrics_f32: p_target outside (0, 1)");
    MV_REQUIRE(cfg->c_miss >= 0.0 && cfg->c_fa >= 0.0, "mv_verif_metrics_f32: negative cost");
    MV_REQUIRE(workspace != nullptr, "mv_verif_metrics_f32: null workspace");
    if (workspace_bytes < p.total)
        return fail(MV_ERR_WORKSPACE, "mv_verif_metrics_f32: workspace smaller than mv_verif_metrics_workspace_bytes(n_trials, n_enroll)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mv_verif_metrics_f32: workspace not 16-byte aligned");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* ss = sorted_scores != nullptr ? sorted_scores : reinterpret_cast<float*>(ws + p.off_scores);
    uint32_t* index = reinterpret_cast<uint32_t*>(ws + p.off_index);
    uint32_t* tile_off = reinterpret_cast<uint32_t*>(ws + p.off_tiles);
    VerifPart* parts = reinterpret_cast<VerifPart*>(ws + p.off_parts);
    VerifDevResult* dev = reinterpret_cast<VerifDevResult*>(ws + p.off_result);

    VS_TRY(sort_run(scores, p.N, ss, index, ws + p.off_sort, st));
    MV_LAUNCH(verif_count_kernel, (p.tiles, 1, 1), (VS_THREADS, 1, 1), 0, st, (const uint32_t*)index, p.N, (uint32_t)n_enroll, trial_labels,
              enroll_labels, tile_off);
    VS_TRY(check_launch("verif_count_kernel"));
    MV_LAUNCH(scan_top_kernel, (1, 1, 1), (VS_THREADS, 1, 1), 0, st, tile_off, (int64_t)p.tiles);
    VS_TRY(check_launch("scan_top_kernel"));
    MV_LAUNCH(verif_scan_kernel, (p.tiles, 1, 1), (VS_THREADS, 1, 1), 0, st, (const uint32_t*)index, p.N, (uint32_t)n_enroll, trial_labels,
              enroll_labels, (const uint32_t*)tile_off, p.tiles, cfg->p_target, 1.0 - cfg->p_target, cfg->c_miss, cfg->c_fa, tgt_cum, parts);
    VS_TRY(check_launch("verif_scan_kernel"));
    MV_LAUNCH(verif_finish_kernel, (1, 1, 1), (VS_THREADS, 1, 1), 0, st, (const VerifPart*)parts, p.tiles, (const uint32_t*)tile_off,
              (const float*)ss, dev);
    VS_TRY(check_launch("verif_finish_kernel"));
    VerifDevResult host;
    MV_HIP_OK(hipMemcpyAsync(&host, dev, sizeof host, hipMemcpyDeviceToHost, st));
    MV_HIP_OK(hipStreamSynchronize(st));
    result->n_target = (int64_t)host.n_target;
    result->n_impostor = p.N - (int64_t)host.n_target;
    result->i1 = host.i1 == VS_NONE ? -1 : (int64_t)host.i1;
    result->i2 = (int64_t)host.i2p1 - 1;
    result->tgt_i1 = (int64_t)host.t1;
    result->tgt_i2 = (int64_t)host.t2;
    result->min_cost = host.cost;
    result->score_i1 = host.score_i1;
    result->reserved = 0;
    return MV_OK;
}
