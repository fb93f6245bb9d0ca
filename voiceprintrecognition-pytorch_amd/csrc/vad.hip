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

// ================================================================================================ regions and gather
// Behind the VAD, still on the device (the contracts of include/mvector_hip.h, mv_vad_regions_i32 and mv_wave_gather_f32): the runs of speech
// frames become regions in samples -- EnergyVad.smooth restated in integers -- and the kept regions of every row are copied into a shorter row.
//   vad_join_kernel          one workgroup per row walks the row's runs in tiles of MV_VAD_REGION_TILE (one run per thread) and carries its scan
//                            values: a run is the head of a joined region when the gap in front of it stays, its tail when the gap behind it
//                            stays; flags -> exclusive scan -> the joined regions that are long enough, compacted into the workspace.
//   vad_pad_region_kernel    one workgroup per row: every kept region grows by speech_pad against its neighbours' middle; the row's sum of lengths.
//   wave_gather_scan_kernel  one workgroup per row: exclusive scan of the clamped region lengths into the workspace, the total behind them.
//   wave_gather_kernel       grid (output tiles of MV_WAVE_GATHER_TILE samples) x B: the region of the tile's first output by binary search over
//                            the scanned lengths, the next MV_VAD_REGION_TILE regions as a table in LDS (regions behind the table are searched
//                            in the workspace); four outputs per thread and trip -- one 16-byte load where they lie in one region and the source
//                            address allows, scalar loads otherwise; one 16-byte store where the row's address allows.  Words are copied as
//                            32-bit integers: no bit of a sample changes.
// As above: the stream orders the launches, no workgroup waits for another, no atomics, nothing is read that a launch of the same call did not write.
namespace mv {
namespace {

constexpr int VR_R = MV_VAD_REGION_TILE;          // runs / regions per tile, one per thread
constexpr int WG_TILE = MV_WAVE_GATHER_TILE;      // outputs per workgroup of the gather
constexpr int WG_TRIPS = WG_TILE / (4 * VAD_THREADS);
static_assert(VR_R == VAD_THREADS && WG_TILE % (4 * VAD_THREADS) == 0, "tile geometry");
typedef uint32_t word4v __attribute__((ext_vector_type(4)));

// vad_excl_scan for any integer type.  wave_tot: 4 LDS words of T.
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* wave_tot, T* total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    T inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, (unsigned)d);
        if (lane >= d) inc += o;
    }
    __syncthreads();   // the previous use of wave_tot has been read
    if (lane == 63) wave_tot[w] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int k = 0; k < VAD_THREADS / 64; ++k) {
        const T t = wave_tot[k];
        base += k < w ? t : (T)0;
        tot += t;
    }
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ int64_t run_start(const int32_t* run, int shift) { return (int64_t)run[0] * shift; }
// a run that reaches the last frame ends with the row
__device__ __forceinline__ int64_t run_end(const int32_t* run, int shift, int T, int64_t n) { return run[1] >= T ? n : (int64_t)run[1] * shift; }

// grid (B).  joined [B, max_runs, 2] (workspace): the joined regions of at least min_speech samples.  num_regions [B]: their count; a row with more
// runs than max_runs gets -1 here and in kept [B]
__global__ __launch_bounds__(VAD_THREADS) void vad_join_kernel(MvVadSmoothCfg c, const int32_t* num_frames, const int32_t* num_runs, const int32_t* runs,
                                                               int max_runs, const int64_t* num_samples, int64_t L, int32_t* joined,
                                                               int32_t* num_regions, int64_t* kept) {
    __shared__ int64_t head_start[VR_R];   // start of the tile's k-th head
    __shared__ unsigned wave_tot[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int nr = num_runs[b];
    if (nr > max_runs) {   // a truncated run list
        if (tid == 0) num_regions[b] = -1, kept[b] = -1;
        return;
    }
    const int T = num_frames[b], shift = c.frame_shift;
    const int64_t n = row_samples(num_samples, b, L);
    const int32_t* row = runs + (int64_t)b * max_runs * 2;
    int32_t* dst = joined + (int64_t)b * max_runs * 2;
    int64_t carry_start = 0;               // start of the last head of the tiles before
    unsigned count = 0u;
    for (int base = 0; base < nr; base += VR_R) {
        const int i = base + tid;
        int64_t s = 0, e = 0;
        unsigned head = 0u, tail = 0u;
        if (i < nr) {
            s = run_start(row + 2 * i, shift), e = run_end(row + 2 * i, shift, T, n);
            head = i == 0 || s - run_end(row + 2 * (i - 1), shift, T, n) >= c.min_silence ? 1u : 0u;
            tail = i == nr - 1 || run_start(row + 2 * (i + 1), shift) - e >= c.min_silence ? 1u : 0u;
        }
        unsigned heads, keeps;
        const unsigned hx = block_excl_scan<unsigned>(head, wave_tot, &heads);
        if (head != 0u) head_start[hx] = s;
        __syncthreads();
        const unsigned upto = hx + head;   // heads of the tile up to and including run i
        const int64_t first = upto > 0u ? head_start[upto - 1] : carry_start;
        if (heads > 0u) carry_start = head_start[heads - 1];
        const unsigned keep = tail != 0u && e - first >= c.min_speech ? 1u : 0u;
        const unsigned kx = block_excl_scan<unsigned>(keep, wave_tot, &keeps);   // (its barriers stand between these reads of head_start and the next tile's writes)
        if (keep != 0u) {
            dst[2 * (int64_t)(count + kx)] = (int32_t)first;
            dst[2 * (int64_t)(count + kx) + 1] = (int32_t)e;
        }
        count += keeps;
    }
    if (tid == 0) num_regions[b] = (int32_t)count;
}

// grid (B).  regions [B, max_runs, 2]: the first num_regions[b] pairs of a row; kept [B]: the sum of their lengths
__global__ __launch_bounds__(VAD_THREADS) void vad_pad_region_kernel(MvVadSmoothCfg c, const int32_t* joined, int max_runs, const int64_t* num_samples, int64_t L,
                                                                     const int32_t* num_regions, int32_t* regions, int64_t* kept) {
    __shared__ int64_t red[VAD_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int count = num_regions[b];
    if (count < 0) return;
    const int64_t n = row_samples(num_samples, b, L);
    const int32_t* src = joined + (int64_t)b * max_runs * 2;
    int32_t* dst = regions + (int64_t)b * max_runs * 2;
    int64_t sum = 0;
    for (int k = tid; k < count; k += VAD_THREADS) {
        const int64_t s = src[2 * k], e = src[2 * k + 1];
        int64_t lo = 0, hi = n;            // the middle of the gap to a neighbour (>> 1: numpy's // 2), else the row's ends
        if (k > 0) lo = src[2 * k - 1] + ((s - src[2 * k - 1]) >> 1);
        if (k + 1 < count) hi = e + ((src[2 * k + 2] - e) >> 1);
        const int64_t ns = s - c.speech_pad > lo ? s - c.speech_pad : lo, ne = e + c.speech_pad < hi ? e + c.speech_pad : hi;
        dst[2 * k] = (int32_t)ns, dst[2 * k + 1] = (int32_t)ne;
        sum += ne - ns;
    }
    red[tid] = sum;
#pragma unroll 1
    for (int s = VAD_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (tid < s) red[tid] += red[tid + s];
    }
    if (tid == 0) kept[b] = red[0];
}

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t n) { return v < 0 ? 0 : (v > n ? n : v); }

// grid (B).  offs [B, max_regions + 1] (workspace): where every region of the row starts in the output, the total at [count]; out_samples [B]
__global__ __launch_bounds__(VAD_THREADS) void wave_gather_scan_kernel(const int64_t* num_samples, int64_t L, const int32_t* num_regions, const int32_t* regions,
                                                                       int max_regions, int64_t* offs, int64_t* out_samples) {
    __shared__ int64_t wave_tot[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    int count = num_regions[b];
    if (count < 0) {   // a skipped row
        if (tid == 0) out_samples[b] = -1;
        return;
    }
    count = count < max_regions ? count : max_regions;
    const int64_t n = row_samples(num_samples, b, L);
    const int32_t* row = regions + (int64_t)b * max_regions * 2;
    int64_t* o = offs + (int64_t)b * (max_regions + 1);
    int64_t carry = 0;
    for (int base = 0; base < count; base += VR_R) {
        const int j = base + tid;
        int64_t len = 0;
        if (j < count) {
            const int64_t s = clamp_to(row[2 * j], n), e = clamp_to(row[2 * j + 1], n);
            len = e > s ? e - s : 0;
        }
        int64_t total;
        const int64_t ex = block_excl_scan<int64_t>(len, wave_tot, &total);
        if (j < count) o[j] = carry + ex;
        carry += total;
    }
    if (tid == 0) o[count] = carry, out_samples[b] = carry;
}

// grid (B * tiles).  out [B, L_out]: the words of the row's regions one behind the other, zeros behind them
__global__ __launch_bounds__(VAD_THREADS) void wave_gather_kernel(const uint32_t* wav, int64_t wav_stride, const int64_t* num_samples, int64_t L,
                                                                  const int32_t* num_regions, const int32_t* regions, int max_regions, const int64_t* offs,
                                                                  uint32_t* out, int64_t out_stride, int64_t L_out, int tiles) {
    __shared__ int64_t tab_off[VR_R + 1];   // output offsets of the regions j0 .. j0 + cnt, the last one closing the table
    __shared__ int64_t tab_src[VR_R];       // their (clamped) first samples
    const int tid = threadIdx.x;
    const int b = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int64_t o0 = (int64_t)tile * WG_TILE;
    int count = num_regions[b];
    count = count < max_regions ? count : max_regions;
    const int64_t n = row_samples(num_samples, b, L);
    const int32_t* row = regions + (int64_t)b * max_regions * 2;
    const int64_t* o = offs + (int64_t)b * (max_regions + 1);
    const int64_t total = count > 0 ? o[count] : 0;
    const uint32_t* src = wav + (int64_t)b * wav_stride;
    uint32_t* dst = out + (int64_t)b * out_stride;
    const bool dst16 = reinterpret_cast<uintptr_t>(dst) % 16 == 0;   // a thread's first output is a multiple of four
    int j0 = 0, cnt = 0;
    if (o0 < total) {   // the region of the tile's first output: the first j with o[j + 1] > o0
        int lo = 0, hi = count - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (o[mid + 1] > o0) hi = mid;
            else lo = mid + 1;
        }
        j0 = lo;
        cnt = count - j0 < VR_R ? count - j0 : VR_R;
        for (int g = tid; g <= cnt; g += VAD_THREADS) {
            tab_off[g] = o[j0 + g];
            if (g < cnt) tab_src[g] = clamp_to(row[2 * (j0 + g)], n);
        }
    }
    __syncthreads();
    // the region of output q < total -- the first j with o[j + 1] > q, which passes over empty regions: its outputs [begin, end), its first sample
    struct Located {
        int64_t begin, end, first;
    };
    const auto locate = [&](int64_t q) {
        if (q < tab_off[cnt]) {
            int lo = 0, hi = cnt - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (tab_off[mid + 1] > q) hi = mid;
                else lo = mid + 1;
            }
            return Located{tab_off[lo], tab_off[lo + 1], tab_src[lo]};
        }
        int lo = j0 + cnt, hi = count - 1;   // behind the table
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (o[mid + 1] > q) hi = mid;
            else lo = mid + 1;
        }
        return Located{o[lo], o[lo + 1], clamp_to(row[2 * lo], n)};
    };
#pragma unroll 1
    for (int it = 0; it < WG_TRIPS; ++it) {
        const int64_t p = o0 + (int64_t)it * 4 * VAD_THREADS + 4 * tid;
        if (p >= L_out) break;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (p < total) {
            const Located r = locate(p);
            if (p + 4 <= r.end) {           // four outputs of one region
                const uint32_t* from = src + r.first + (p - r.begin);
                if (reinterpret_cast<uintptr_t>(from) % 16 == 0) {
                    const word4v q = *reinterpret_cast<const word4v*>(from);
                    v[0] = q[0], v[1] = q[1], v[2] = q[2], v[3] = q[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = from[e];
                }
            } else {                        // a region ends among them (or the row does): every output is located by itself
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t q = p + e;
                    if (q < total) {
                        const Located s = q < r.end ? r : locate(q);
                        v[e] = src[s.first + (q - s.begin)];
                    }
                }
            }
        }
        if (dst16 && p + 4 <= L_out) {
            *reinterpret_cast<word4v*>(dst + p) = word4v{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < L_out) dst[p + e] = v[e];
        }
    }
}

// [a, a + an) and [b, b + bn) share a byte
bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
    return an > 0 && bn > 0 && ua < ub + bn && ub < ua + an;
}

}  // namespace
}  // namespace mv

extern "C" size_t mv_vad_regions_workspace_bytes(int32_t B, int32_t max_runs) {
    return B > 0 && max_runs > 0 ? mv::align256((size_t)B * (size_t)max_runs * 2 * sizeof(int32_t)) : 0;
}

extern "C" int mv_vad_regions_i32(const MvVadSmoothCfg* cfg, const int32_t* num_frames, const int32_t* num_runs, const int32_t* runs, int32_t max_runs,
                                  const int64_t* num_samples, int32_t B, int64_t L, int32_t* num_regions, int32_t* regions, int64_t* kept, void* workspace,
                                  size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    MV_REQUIRE(cfg != nullptr, "mv_vad_regions_i32: null cfg");
    MV_REQUIRE(cfg->frame_shift >= 1, "mv_vad_regions_i32: frame_shift below 1");
    MV_REQUIRE(cfg->min_silence >= 0 && cfg->min_speech >= 0 && cfg->speech_pad >= 0, "mv_vad_regions_i32: negative min_silence, min_speech or speech_pad");
    MV_REQUIRE(B >= 0 && L >= 0 && max_runs >= 0, "mv_vad_regions_i32: negative B, L or max_runs");
    MV_REQUIRE(L <= (int64_t)0x7FFFFFFF, "mv_vad_regions_i32: L above 2^31 - 1");
    if (B == 0) return MV_OK;
    MV_REQUIRE(num_frames != nullptr && num_runs != nullptr && num_regions != nullptr && kept != nullptr && ((runs != nullptr && regions != nullptr) || max_runs == 0),
               "mv_vad_regions_i32: null tensor");
    const size_t list_bytes = (size_t)B * (size_t)max_runs * 2 * sizeof(int32_t);
    MV_REQUIRE(!ranges_overlap(runs, list_bytes, regions, list_bytes), "mv_vad_regions_i32: regions aliases runs");
    const size_t need = mv_vad_regions_workspace_bytes(B, max_runs);
    MV_REQUIRE(workspace != nullptr || need == 0, "mv_vad_regions_i32: null workspace");
    if (workspace_bytes < need) return fail(MV_ERR_WORKSPACE, "mv_vad_regions_i32: workspace smaller than mv_vad_regions_workspace_bytes(B, max_runs)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mv_vad_regions_i32: workspace not 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* joined = static_cast<int32_t*>(workspace);
    MV_LAUNCH(vad_join_kernel, ((unsigned)B, 1, 1), (VAD_THREADS, 1, 1), 0, st, *cfg, num_frames, num_runs, runs, (int)max_runs, num_samples, L, joined, num_regions, kept);
    const int rcl = check_launch("vad_join_kernel");
    if (rcl != MV_OK) return rcl;
    MV_LAUNCH(vad_pad_region_kernel, ((unsigned)B, 1, 1), (VAD_THREADS, 1, 1), 0, st, *cfg, (const int32_t*)joined, (int)max_runs, num_samples, L,
              (const int32_t*)num_regions, regions, kept);
    return check_launch("vad_pad_region_kernel");
}

extern "C" size_t mv_wave_gather_workspace_bytes(int32_t B, int32_t max_regions) {
    return B > 0 && max_regions >= 0 ? mv::align256((size_t)B * ((size_t)max_regions + 1) * sizeof(int64_t)) : 0;
}

extern "C" int mv_wave_gather_f32(const float* wav, int64_t wav_stride, const int64_t* num_samples, const int32_t* num_regions, const int32_t* regions,
                                  int32_t max_regions, int32_t B, int64_t L, float* out, int64_t out_stride, int64_t L_out, int64_t* out_samples, void* workspace,
                                  size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    MV_REQUIRE(B >= 0 && L >= 0 && L_out >= 0 && max_regions >= 0, "mv_wave_gather_f32: negative B, L, L_out or max_regions");
    if (B == 0) return MV_OK;
    MV_REQUIRE(num_regions != nullptr && out_samples != nullptr && (regions != nullptr || max_regions == 0) && (wav != nullptr || L == 0) &&
                   (out != nullptr || L_out == 0),
               "mv_wave_gather_f32: null tensor");
    MV_REQUIRE(wav_stride >= L, "mv_wave_gather_f32: wav_stride below L");
    MV_REQUIRE(out_stride >= L_out, "mv_wave_gather_f32: out_stride below L_out");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(wav) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0, "mv_wave_gather_f32: wav or out not 4-byte aligned");
    MV_REQUIRE(!ranges_overlap(wav, ((size_t)(B - 1) * (size_t)wav_stride + (size_t)L) * sizeof(float), out,
                               ((size_t)(B - 1) * (size_t)out_stride + (size_t)L_out) * sizeof(float)),
               "mv_wave_gather_f32: out aliases wav");
    const int64_t tiles = (L_out + WG_TILE - 1) / WG_TILE;
    MV_REQUIRE(tiles <= (int64_t)0x7FFFFFFF / B, "mv_wave_gather_f32: B * ceil(L_out / MV_WAVE_GATHER_TILE) above 2^31 - 1");
    MV_REQUIRE(workspace != nullptr, "mv_wave_gather_f32: null workspace");
    if (workspace_bytes < mv_wave_gather_workspace_bytes(B, max_regions))
        return fail(MV_ERR_WORKSPACE, "mv_wave_gather_f32: workspace smaller than mv_wave_gather_workspace_bytes(B, max_regions)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mv_wave_gather_f32: workspace not 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t* offs = static_cast<int64_t*>(workspace);
    MV_LAUNCH(wave_gather_scan_kernel, ((unsigned)B, 1, 1), (VAD_THREADS, 1, 1), 0, st, num_samples, L, num_regions, regions, (int)max_regions, offs, out_samples);
    const int rcl = check_launch("wave_gather_scan_kernel");
    if (rcl != MV_OK || tiles == 0) return rcl;
    MV_LAUNCH(wave_gather_kernel, ((unsigned)(B * tiles), 1, 1), (VAD_THREADS, 1, 1), 0, st, reinterpret_cast<const uint32_t*>(wav), wav_stride, num_samples, L,
              num_regions, regions, (int)max_regions, (const int64_t*)offs, reinterpret_cast<uint32_t*>(out), out_stride, L_out, (int)tiles);
    return check_launch("wave_gather_kernel");
}
