// Energy voice activity detection: fp32 waveform rows -> per row the runs [a, b) of speech frames (the contract of include/mvector_hip.h,
// mv_vad_energy_f32; Kaldi's compute-vad restated: centred log energy per frame, a threshold from the row's mean log energy, a vote over a
// context window).
//
// Five ordinary launches on the caller's stream, B rows with their own lengths through the same grids (tile = VAD_F frames of one row):
//   vad_energy_kernel     a tile's samples go through LDS in stages of at most VAD_STAGE floats (a stage = as many whole frames as fit, with
//                         their frame_length - frame_shift overlap: a frame is never split across stages or workgroups; 16-byte loads where
//                         the row's address allows, scalar loads in front of and behind them).  32 lanes per frame: two fp64 passes over
//                         the LDS copy, lane sums folded by a butterfly.  logE of the tile's frames and the tile's sum of them.
//   vad_threshold_kernel  one workgroup per row: the tile sums in tile order -> thr, T.
//   vad_decide_kernel     logE > thr of the tile's frames and frames_context (+ 1: the predecessor's window) on either side as flags in LDS,
//                         an LDS prefix sum gives every window count; decisions, and how many positions t in 0 .. T differ from their
//                         predecessor (frame -1 and frame T are silence) per tile.
//   vad_scan_kernel       one workgroup: exclusive scan of the tile counts in place, the total behind them.
//   vad_scatter_kernel    boundary k of a row is the start (k even) or the end (k odd) of run k / 2.
// No workgroup waits for another (no look-back, no flags), no atomics: the stream orders the launches and that is the only ordering used.
// Nothing that was not written by a launch of the same call is read, so what the buffers held before does not matter.
#include "common.h"

namespace mv {
namespace {

constexpr int VAD_THREADS = 256;
// the energy kernel: 32 frames at a time, a stage of 49 default frames in two trips.  Measured on an MI355X ("The VAD"): 157 / 39 us at
// 60 / 10 minutes of audio against 191 / 84 us with 256 threads -- a workgroup's stages run one after the other, more lanes shorten each
constexpr int VAD_ENERGY_THREADS = 1024;
constexpr int VAD_F = MV_VAD_TILE_FRAMES;       // frames per tile, one decision per thread
constexpr int VAD_STAGE = 8192;                 // floats of one LDS stage: 32 KiB (two 1024-thread workgroups fill a compute unit's waves); >= the longest frame
constexpr int VAD_MAX_LENGTH = 4096;
constexpr int VAD_MAX_CONTEXT = 64;
constexpr int VAD_GROUP = 32;                   // lanes per frame
constexpr int VAD_SCAN_ITEMS = 8;               // tile counts per thread and trip of the scan
constexpr double VAD_EPS = 0x1p-23;
constexpr double VAD_LOG_EPS = -0x1.fe2804e87b348p+3;   // log(2^-23), correctly rounded: a floored frame is this value on every device
static_assert(VAD_F == VAD_THREADS && VAD_STAGE >= VAD_MAX_LENGTH && VAD_F + 2 * VAD_MAX_CONTEXT + 2 <= 2 * VAD_THREADS, "tile geometry");

__device__ __forceinline__ int64_t row_samples(const int64_t* num_samples, int b, int64_t L) {
    if (num_samples == nullptr) return L;
    const int64_t n = num_samples[b];
    return n < 0 ? 0 : (n > L ? L : n);   // a length outside 0 .. L reads nothing outside the row
}

__device__ __forceinline__ int frames_of(int64_t n, int length, int shift) { return n < length ? 0 : (int)(1 + (n - length) / shift); }

// sum over the 32 lanes of a frame's group, the same bits in every lane (a + b == b + a)
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int off = VAD_GROUP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, VAD_GROUP);
    return v;
}

// exclusive prefix of one value per thread over the 256 threads of the block, *total = their sum.  wave_tot: 4 LDS words.
__device__ __forceinline__ unsigned vad_excl_scan(unsigned v, unsigned* wave_tot, unsigned* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, (unsigned)d);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // the previous use of wave_tot has been read
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    unsigned base = 0u, tot = 0u;
    for (int k = 0; k < VAD_THREADS / 64; ++k) {
        const unsigned t = wave_tot[k];
        base += k < w ? t : 0u;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

// sum of red[0 .. 256) by the halving tree, left in red[0] (every thread of the block calls it, whatever the block's size)
__device__ __forceinline__ void tree_fold(double* red, int tid) {
#pragma unroll 1
    for (int s = VAD_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------ energies
// grid (B * tiles).  le [B, Tmax] fp64: logE, zeros at t >= T_b.  part [B, tiles]: the tile's sum of logE (tiles with a frame only).
__global__ __launch_bounds__(VAD_ENERGY_THREADS) void vad_energy_kernel(const float* wav, int64_t stride, const int64_t* num_samples, int64_t L, int length,
                                                                 int shift, double scale, int tiles, int Tmax, double* le, double* part) {
    __shared__ __attribute__((aligned(16))) float xs[VAD_STAGE + 4];
    __shared__ double le_s[VAD_F];
    const int tid = threadIdx.x, grp = tid / VAD_GROUP, j = tid % VAD_GROUP;
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int T = frames_of(row_samples(num_samples, b, L), length, shift);
    const int t0 = tile * VAD_F;
    double* le_row = le + (int64_t)b * Tmax;
    if (t0 >= T) {   // no frame of the row in this tile: the zeros behind T_b
        if (tid < VAD_F && t0 + tid < Tmax) le_row[t0 + tid] = 0.0;
        return;
    }
    const int nf = T - t0 < VAD_F ? T - t0 : VAD_F;
    const int per_stage = (VAD_STAGE - length) / shift + 1;
    const float* row = wav + (int64_t)b * stride;
    if (tid < VAD_F) le_s[tid] = 0.0;
    for (int f0 = 0; f0 < nf; f0 += per_stage) {
        const int cnt = nf - f0 < per_stage ? nf - f0 : per_stage;
        const int count = (cnt - 1) * shift + length;                     // <= VAD_STAGE, and the last sample lies inside the row's n_b
        const float* src = row + (int64_t)(t0 + f0) * shift;
        const int to_16 = (int)(((16 - reinterpret_cast<uintptr_t>(src) % 16) % 16) / 4);
        const int head = to_16 < count ? to_16 : count;
        const int nvec = (count - head) / 4;
        const int pad = (4 - head) % 4;                                    // sample k sits at xs[pad + k]: the 16-byte pieces are aligned in LDS too
        __syncthreads();                                                   // the stage before has been read (first trip: le_s is cleared)
        for (int i = tid; i < nvec; i += VAD_ENERGY_THREADS)
            *reinterpret_cast<float4v*>(xs + pad + head + 4 * i) = *reinterpret_cast<const float4v*>(src + head + 4 * i);
        for (int i = tid; i < count - 4 * nvec; i += VAD_ENERGY_THREADS) {
            const int k = i < head ? i : i + 4 * nvec;
            xs[pad + k] = src[k];
        }
        __syncthreads();
        const int trips = (cnt + VAD_ENERGY_THREADS / VAD_GROUP - 1) / (VAD_ENERGY_THREADS / VAD_GROUP);
        for (int it = 0; it < trips; ++it) {   // every lane takes every trip: the butterflies are wave-wide
            const int f = it * (VAD_ENERGY_THREADS / VAD_GROUP) + grp;
            const float* x = xs + pad + f * shift;
            const int n = f < cnt ? length : 0;
            double s = 0.0;
            for (int i = j; i < n; i += VAD_GROUP) s += (double)x[i] * scale;
            const double m = group_sum(s) / (double)length;
            double q = 0.0;
            for (int i = j; i < n; i += VAD_GROUP) {
                const double d = (double)x[i] * scale - m;
                q = __builtin_fma(d, d, q);
            }
            const double e = group_sum(q);
            if (f < cnt && j == 0) le_s[f0 + f] = e < VAD_EPS ? VAD_LOG_EPS : log(e);
        }
    }
    __syncthreads();
    if (tid < VAD_F && t0 + tid < Tmax) le_row[t0 + tid] = le_s[tid];   // (entries behind nf are the zeros le_s was cleared with)
    tree_fold(le_s, tid);
    if (tid == 0) part[(int64_t)b * tiles + tile] = le_s[0];
}

// grid (B).  thr [B] (workspace), thr_out [B] optional, num_frames [B]
__global__ __launch_bounds__(VAD_THREADS) void vad_threshold_kernel(const double* part, const int64_t* num_samples, int64_t L, int length, int shift,
                                                                    int tiles, double energy_threshold, double energy_mean_scale, double* thr,
                                                                    double* thr_out, int32_t* num_frames) {
    __shared__ double red[VAD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int T = frames_of(row_samples(num_samples, b, L), length, shift);
    const int used = (T + VAD_F - 1) / VAD_F;
    double s = 0.0;
    for (int k = tid; k < used; k += VAD_THREADS) s += part[(int64_t)b * tiles + k];
    red[tid] = s;
    tree_fold(red, tid);
    if (tid == 0) {
        const double v = energy_threshold + energy_mean_scale * (red[0] / (double)T);   // T = 0: 0 / 0
        thr[b] = v;
        if (thr_out != nullptr) thr_out[b] = v;
        num_frames[b] = T;
    }
}

// ------------------------------------------------------------------------------------------------ decisions
// grid (B * tiles).  dec [B, Tmax] uint8, zeros at t >= T_b.  counts [B * tiles]: positions t of the tile with decision(t) != decision(t - 1).
__global__ __launch_bounds__(VAD_THREADS) void vad_decide_kernel(const double* le, const double* thr, const int64_t* num_samples, int64_t L, int length,
                                                                 int shift, int ctx, double proportion, int tiles, int Tmax, uint8_t* dec,
                                                                 uint32_t* counts) {
    __shared__ unsigned pre[2 * VAD_THREADS];   // pre[i]: flags of the frames first .. first + i - 1
    __shared__ unsigned wave_tot[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int T = frames_of(row_samples(num_samples, b, L), length, shift);
    const int t0 = tile * VAD_F;
    const int first = t0 - ctx - 1;             // the predecessor of the tile's first frame votes over t0 - 1 - ctx .. t0 - 1 + ctx
    const int width = VAD_F + 2 * ctx + 1;
    const double* le_row = le + (int64_t)b * Tmax;
    const double th = thr[b];
    unsigned fl[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int i = 2 * tid + e, t = first + i;
        fl[e] = i < width && t >= 0 && t < T && le_row[t] > th ? 1u : 0u;
    }
    unsigned total;
    const unsigned ex = vad_excl_scan(fl[0] + fl[1], wave_tot, &total);
    pre[2 * tid] = ex;
    pre[2 * tid + 1] = ex + fl[0];
    __syncthreads();
    const int t = t0 + tid;
    unsigned d[2];                              // decision(t - 1), decision(t); silence outside 0 .. T - 1
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int u = t - 1 + e;
        d[e] = 0u;
        if (u >= 0 && u < T) {
            const int lo = u - ctx > 0 ? u - ctx : 0, hi = u + ctx < T - 1 ? u + ctx : T - 1;
            const unsigned num = pre[hi + 1 - first] - pre[lo - first];
            d[e] = (double)num >= (double)(hi - lo + 1) * proportion ? 1u : 0u;
        }
    }
    if (t < Tmax) dec[(int64_t)b * Tmax + t] = (uint8_t)d[1];
    const unsigned edge = t <= T && d[0] != d[1] ? 1u : 0u;
    vad_excl_scan(edge, wave_tot, &total);
    if (tid == 0) counts[blockIdx.x] = total;
}

// one workgroup: a[0 .. n) -> its exclusive prefix sums in place, a[n] = the total
__global__ __launch_bounds__(VAD_THREADS) void vad_scan_kernel(uint32_t* a, int64_t n) {
    __shared__ unsigned wave_tot[4];
    unsigned carry = 0u;
    for (int64_t first = 0; first < n; first += VAD_THREADS * VAD_SCAN_ITEMS) {
        const int64_t i0 = first + (int64_t)threadIdx.x * VAD_SCAN_ITEMS;
        unsigned v[VAD_SCAN_ITEMS], s = 0u;
#pragma unroll
        for (int e = 0; e < VAD_SCAN_ITEMS; ++e) {
            v[e] = i0 + e < n ? a[i0 + e] : 0u;
            s += v[e];
        }
        unsigned total;
        unsigned run = carry + vad_excl_scan(s, wave_tot, &total);
#pragma unroll
        for (int e = 0; e < VAD_SCAN_ITEMS; ++e) {
            if (i0 + e < n) a[i0 + e] = run;
            run += v[e];
        }
        carry += total;
    }
    if (threadIdx.x == 0) a[n] = carry;
}

// grid (B * tiles).  off: the scanned counts.  runs [B, max_runs, 2], num_runs [B]
__global__ __launch_bounds__(VAD_THREADS) void vad_scatter_kernel(const uint8_t* dec, const uint32_t* off, const int64_t* num_samples, int64_t L, int length,
                                                                  int shift, int tiles, int Tmax, int32_t* runs, int max_runs, int32_t* num_runs) {
    __shared__ unsigned wave_tot[4];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int T = frames_of(row_samples(num_samples, b, L), length, shift);
    const int t = tile * VAD_F + tid;
    const uint8_t* dec_row = dec + (int64_t)b * Tmax;
    const unsigned prev = t >= 1 && t - 1 < T ? dec_row[t - 1] : 0u;
    const unsigned cur = t < T ? dec_row[t] : 0u;
    const unsigned edge = t <= T && prev != cur ? 1u : 0u;
    unsigned total;
    const unsigned ex = vad_excl_scan(edge, wave_tot, &total);
    const unsigned row_first = off[(int64_t)b * tiles];
    if (edge != 0u) {
        const unsigned k = off[blockIdx.x] - row_first + ex;   // the row's k-th boundary: starts and ends alternate
        if ((int)(k >> 1) < max_runs) runs[((int64_t)b * max_runs + (k >> 1)) * 2 + (k & 1u)] = t;
    }
    if (tile == 0 && tid == 0) num_runs[b] = (int32_t)((off[(int64_t)(b + 1) * tiles] - row_first) >> 1);
}

// ------------------------------------------------------------------------------------------------ host side
size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct VadPlan {
    int Tmax, tiles;
    size_t off_le, off_dec, off_part, off_thr, off_counts, total;
};

// MV_OK, or the refusal both entry points share
int vad_plan(const MvVadCfg* cfg, int32_t B, int64_t L, VadPlan* out) {
    MV_REQUIRE(cfg != nullptr, "mv_vad_energy_f32: null cfg");
    MV_REQUIRE(cfg->frame_shift >= 1 && cfg->frame_shift <= cfg->frame_length && cfg->frame_length <= VAD_MAX_LENGTH,
               "mv_vad_energy_f32: frame sizes outside 1 <= frame_shift <= frame_length <= 4096");
    MV_REQUIRE(cfg->frames_context >= 0 && cfg->frames_context <= VAD_MAX_CONTEXT, "mv_vad_energy_f32: frames_context outside 0 .. 64");
    MV_REQUIRE(std::isfinite(cfg->energy_threshold) && std::isfinite(cfg->energy_mean_scale) && std::isfinite(cfg->proportion_threshold) &&
                   std::isfinite(cfg->scale),
               "mv_vad_energy_f32: non-finite energy_threshold, energy_mean_scale, proportion_threshold or scale");
    MV_REQUIRE(B >= 0 && L >= 0, "mv_vad_energy_f32: negative B or L");
    const int64_t Tmax = L < cfg->frame_length ? 0 : 1 + (L - cfg->frame_length) / cfg->frame_shift;
    MV_REQUIRE(B == 0 || Tmax + 1 <= (int64_t)0x7FFFFFFF / B, "mv_vad_energy_f32: B * (T(L) + 1) above 2^31 - 1");
    VadPlan p;
    p.Tmax = (int)Tmax;
    p.tiles = (int)(Tmax / VAD_F + 1);   // the positions 0 .. T(L): frame T closes a run that lasts to the end
    size_t off = 0;
    p.off_le = off, off += align256((size_t)B * (size_t)Tmax * sizeof(double));
    p.off_dec = off, off += align256((size_t)B * (size_t)Tmax);
    p.off_part = off, off += align256((size_t)B * (size_t)p.tiles * sizeof(double));
    p.off_thr = off, off += align256((size_t)B * sizeof(double));
    p.off_counts = off, off += align256(((size_t)B * (size_t)p.tiles + 1) * sizeof(uint32_t));
    p.total = off;
    *out = p;
    return MV_OK;
}

}  // namespace
}  // namespace mv

extern "C" size_t mv_vad_energy_workspace_bytes(const MvVadCfg* cfg, int32_t B, int64_t L) {
    mv::VadPlan p;
    return mv::vad_plan(cfg, B, L, &p) == MV_OK && B > 0 ? p.total : 0;
}

extern "C" int mv_vad_energy_f32(const MvVadCfg* cfg, const float* wav, int64_t wav_stride, const int64_t* num_samples, int32_t B, int64_t L,
                                 int32_t* num_frames, int32_t* num_runs, int32_t* runs, int32_t max_runs, double* log_energy, double* threshold,
                                 uint8_t* decisions, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    VadPlan p;
    const int rc = vad_plan(cfg, B, L, &p);
    if (rc != MV_OK) return rc;
    MV_REQUIRE(max_runs >= 0, "mv_vad_energy_f32: negative max_runs");
    if (B == 0) return MV_OK;
    MV_REQUIRE(wav != nullptr && num_frames != nullptr && num_runs != nullptr && (runs != nullptr || max_runs == 0), "mv_vad_energy_f32: null tensor");
    MV_REQUIRE(wav_stride >= L, "mv_vad_energy_f32: wav_stride below L");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(wav) % 4 == 0, "mv_vad_energy_f32: wav not 4-byte aligned");
    MV_REQUIRE(workspace != nullptr, "mv_vad_energy_f32: null workspace");
    if (workspace_bytes < p.total) return fail(MV_ERR_WORKSPACE, "mv_vad_energy_f32: workspace smaller than mv_vad_energy_workspace_bytes(cfg, B, L)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mv_vad_energy_f32: workspace not 16-byte aligned");
    char* ws = static_cast<char*>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* le = log_energy != nullptr ? log_energy : reinterpret_cast<double*>(ws + p.off_le);
    uint8_t* dec = decisions != nullptr ? decisions : reinterpret_cast<uint8_t*>(ws + p.off_dec);
    double* part = reinterpret_cast<double*>(ws + p.off_part);
    double* thr = reinterpret_cast<double*>(ws + p.off_thr);
    uint32_t* counts = reinterpret_cast<uint32_t*>(ws + p.off_counts);
    const unsigned grid = (unsigned)B * (unsigned)p.tiles;
    const int length = cfg->frame_length, shift = cfg->frame_shift;

    MV_LAUNCH(vad_energy_kernel, (grid, 1, 1), (VAD_ENERGY_THREADS, 1, 1), 0, st, wav, wav_stride, num_samples, L, length, shift, cfg->scale, p.tiles, p.Tmax, le, part);
    int rcl = check_launch("vad_energy_kernel");
    if (rcl != MV_OK) return rcl;
    MV_LAUNCH(vad_threshold_kernel, ((unsigned)B, 1, 1), (VAD_THREADS, 1, 1), 0, st, (const double*)part, num_samples, L, length, shift, p.tiles,
              cfg->energy_threshold, cfg->energy_mean_scale, thr, threshold, num_frames);
    if ((rcl = check_launch("vad_threshold_kernel")) != MV_OK) return rcl;
    MV_LAUNCH(vad_decide_kernel, (grid, 1, 1), (VAD_THREADS, 1, 1), 0, st, (const double*)le, (const double*)thr, num_samples, L, length, shift,
              cfg->frames_context, cfg->proportion_threshold, p.tiles, p.Tmax, dec, counts);
    if ((rcl = check_launch("vad_decide_kernel")) != MV_OK) return rcl;
    MV_LAUNCH(vad_scan_kernel, (1, 1, 1), (VAD_THREADS, 1, 1), 0, st, counts, (int64_t)grid);
    if ((rcl = check_launch("vad_scan_kernel")) != MV_OK) return rcl;
    MV_LAUNCH(vad_scatter_kernel, (grid, 1, 1), (VAD_THREADS, 1, 1), 0, st, (const uint8_t*)dec, (const uint32_t*)counts, num_samples, L, length, shift,
              p.tiles, p.Tmax, runs, max_runs, num_runs);
    return check_launch("vad_scatter_kernel");
}
