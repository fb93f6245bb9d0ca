// Interleaved int16 PCM at any source rate -> mono float32 waveforms at the handle's target rate on the device: channel down-mix, polyphase FIR
// resampling (the filter of scipy.signal.resample_poly(x, up, down) with its defaults, which the package's stand-in AudioSegment.resample runs)
// and the dB normalisation of wave.hip.
//
// The reference does all of this per file on the host (mvector/predict.py:185-212: AudioSegment.from_file -> float conversion, channel mean,
// resample, normalize) and uploads float32; with this file a batch of 44.1 kHz stereo / 8 kHz / 48 kHz recordings travels as int16 as well.
//
//   x[i]  = (float)(sum_c pcm[i, c]) * (1 / 32768) / channels          (integer sum, power-of-two scale, ONE rounded fp32 division: the bits of
//                                                                        (pcm.astype(float32) / 32768).mean(axis=1))
//   g = gcd(dst, src), up = dst / g, down = src / g, half = 10 max(up, down), h = firwin(2 half + 1, 1 / max(up, down), kaiser 5.0) * up  (fp32)
//   y[m]  = sum_j x[j] h[t - j up],  t = m down + half,  0 <= m < n_out = ceil(n_in up / down)
//
// With j_hi = t / up and p = t % up the taps of one output are h[p + k up], k = 0 .. K - 1 (K = ceil((2 half + 1) / up); entries behind the last
// tap are zero), against x[j_hi - k] (zero outside the row).  THE order of the sum, on every build and for every shape: acc = 0, then
// acc = fmaf(x[j_hi - k], h[p + k up], acc) for k = 0, 1, .., K - 1 -- all K terms, the zero ones too.  A row's bits therefore depend on nothing
// but its own samples.
//
// Kernel shape: one workgroup of 256 threads per tile of `tile` (<= 1024) consecutive outputs of one row; lane l owns outputs m0 + l + 256 i.
//   - the source span of the tile is down-mixed once into LDS (every frame is needed by about K up / down outputs);
//   - the table lies in LDS in FILTER ORDER (index p + k up), not phase-major: consecutive outputs step the phase by down mod up, so with
//     up a multiple of 32 and down odd (44.1 / 22.05 / 11.025 kHz -> 16 kHz) the 32 lanes of a half-wave read 32 different banks with no
//     padding at all; up = 1 (48 -> 16 kHz, 16 -> 8 kHz) is one broadcast address; the x reads of neighbouring lanes are down / up apart;
//   - outputs are stored straight from registers, coalesced -- no staging of y, and a tile can be any length, so short rows keep the chip busy.
//   The other mapping (lanes on outputs up apart share a phase, wave-uniform coefficient) needs 64 up outputs per wave step -- 10240 outputs
//   and 113 KB of x for 44.1 kHz, more LDS than the CU has for 11.025 kHz -- plus an LDS round trip of y for a coalesced store.  See DESIGN.md.
//   PCM is read with 2-byte loads: frames of 3 channels are 6 bytes and rows may start anywhere, so nothing wider is aligned in general; the
//   loads of neighbouring lanes are adjacent and the pass over the PCM is a small part of the kernel (2 C bytes against K fmaf per frame).
//   Ratios whose table and minimal x span do not fit into LDS together (down > ~ 500 up) read the table from global memory instead: there
//   a wave touches at most `up` different coefficients per step.
//
// dB normalisation: each tile leaves the sum of its squares (fp32 per thread over its <= 4 outputs, fp64 across the threads in a fixed tree) in
// the caller's workspace; resample_scale_kernel adds a row's partial sums in a fixed order (fp64) and scales the row.  No atomics, no
// workgroup waits for another one: the stream orders the two launches.
#include "common.h"

#include <memory>
#include <vector>

namespace mv {

constexpr int RS_THREADS = 256, RS_PER = 4, RS_TILE_MAX = RS_THREADS * RS_PER;
constexpr int RS_SCALE_CHUNK = 4096;                 // samples per workgroup of the scale pass
constexpr int RS_RED_BYTES = RS_THREADS * 8;         // the tile kernel's fp64 reduction array opens its dynamic LDS (a kernel that asks for the
                                                     // 160 KiB attribute can hold no static LDS beside it)
constexpr int64_t RS_LDS_FLOATS = 156 * 1024 / 4;    // table + x span a tile may ask for behind it (the CU has 160 KiB)
constexpr int64_t RS_X_FLOATS = 12288;               // x span a tile gets by default: 48 KiB keeps three workgroups on a CU beside a 35 KB table

struct ResampleArgs {
    const int16_t* pcm;
    int64_t pcm_stride;
    const int64_t* num_frames;
    int64_t L_in;
    const float* table;    // K * up floats, filter order, zero behind tap 2 half
    float* wav;
    int64_t wav_stride, L_out;
    int64_t* num_out;
    int32_t* too_quiet;
    double* partial;       // [B][tiles_ws] sums of squares (normalize only)
    int32_t channels, up, down, half, K, tile, tiles, tiles_ws, normalize;
};

template <bool TABLE_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_tile_kernel(ResampleArgs a) {
    MV_DYN_SMEM(smem);
    double* red = reinterpret_cast<double*>(smem);
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    int64_t n = a.num_frames != nullptr ? a.num_frames[b] : a.L_in;
    n = n < 0 ? 0 : (n > a.L_in ? a.L_in : n);
    const int64_t n_out = (n * a.up + a.down - 1) / a.down;
    const int64_t m0 = (int64_t)tile * a.tile;
    const int64_t m_end = m0 + a.tile < a.L_out ? m0 + a.tile : a.L_out;   // the tile's share of the output row
    const int64_t m1 = m_end < n_out ? m_end : n_out;                      // ... and of the row's own samples
    float* dst = a.wav + (int64_t)b * a.wav_stride;
    if (tile == 0 && tid == 0) {
        if (a.num_out != nullptr) a.num_out[b] = n_out;
        if (!a.normalize && a.too_quiet != nullptr) a.too_quiet[b] = 0;
    }
    float sq = 0.0f;
    if (m0 < m1) {   // (the same for every thread of the workgroup)
        const int table_floats = a.K * a.up;
        float* hl = reinterpret_cast<float*>(smem + RS_RED_BYTES);
        float* xs = hl + (TABLE_LDS ? ((table_floats + 3) & ~3) : 0);
        if (TABLE_LDS)
            for (int i = tid; i < table_floats; i += RS_THREADS) hl[i] = a.table[i];
        // the frames the tile's outputs read: j_lo = j_hi(m0) - (K - 1) .. j_hi(m1 - 1)
        const int64_t j_lo = (m0 * a.down + a.half) / a.up - (a.K - 1);
        const int span = (int)(((m1 - 1) * a.down + a.half) / a.up - j_lo) + 1;
        const int16_t* src = a.pcm + (int64_t)b * a.pcm_stride;
        const int C = a.channels;
        const float inv = 1.0f / 32768.0f, fc = (float)C;
        for (int q = tid; q < span; q += RS_THREADS) {
            const int64_t j = j_lo + q;
            float v = 0.0f;
            if (j >= 0 && j < n) {
                const int16_t* f = src + j * C;
                int s = 0;
                for (int c = 0; c < C; ++c) s += f[c];
                v = (float)s * inv;
                if (C > 1) v = v / fc;
            }
            xs[q] = v;
        }
        __syncthreads();
        int xq[RS_PER], ph[RS_PER];
        float acc[RS_PER];
#pragma unroll
        for (int i = 0; i < RS_PER; ++i) {
            const int64_t m = m0 + tid + i * RS_THREADS;
            const int64_t t = (m < m1 ? m : m0) * a.down + a.half;   // (lanes behind the tile's end walk the first output's taps and drop the sum)
            const int64_t jh = t / a.up;
            ph[i] = (int)(t - jh * a.up);
            xq[i] = (int)(jh - j_lo);
            acc[i] = 0.0f;
        }
        const float* hs = TABLE_LDS ? hl : a.table;
        for (int k = 0; k < a.K; ++k) {
            const int hk = k * a.up;
#pragma unroll
            for (int i = 0; i < RS_PER; ++i) acc[i] = fmaf(xs[xq[i] - k], hs[ph[i] + hk], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < RS_PER; ++i) {
            const int64_t m = m0 + tid + i * RS_THREADS;
            if (m < m1) {
                dst[m] = acc[i];
                sq = fmaf(acc[i], acc[i], sq);
            }
        }
    }
    for (int64_t m = (m0 > m1 ? m0 : m1) + tid; m < m_end; m += RS_THREADS) dst[m] = 0.0f;   // behind the row's n_out samples
    if (a.normalize && tile < a.tiles_ws) {
        red[tid] = (double)sq;
        __syncthreads();
        for (int st = RS_THREADS / 2; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) a.partial[(int64_t)b * a.tiles_ws + tile] = red[0];
    }
}

// second pass of the dB normalisation: every workgroup of a row adds the row's partial sums in the same order, the first one reports the flag
__global__ __launch_bounds__(RS_THREADS) void resample_scale_kernel(const double* partial, int tiles_ws, const int64_t* num_frames, int64_t L_in,
                                                                    int up, int down, float target_db, float max_gain_db, float* wav,
                                                                    int64_t wav_stride, int32_t* too_quiet, int chunks) {
    __shared__ double red[RS_THREADS];
    __shared__ float gain_s;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    int64_t n = num_frames != nullptr ? num_frames[b] : L_in;
    n = n < 0 ? 0 : (n > L_in ? L_in : n);
    const int64_t n_out = (n * up + down - 1) / down;
    double part = 0.0;
    for (int i = tid; i < tiles_ws; i += RS_THREADS) part += partial[(int64_t)b * tiles_ws + i];
    red[tid] = part;
    __syncthreads();
    for (int st = RS_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) {
        const double mean_sq = n_out > 0 ? red[0] / (double)n_out : 0.0;
        // the gain rule of wave_prepare_kernel: digital silence gives +inf, which the reference rejects (max_gain_db)
        float gain_db = mean_sq > 0.0 ? target_db - 10.0f * log10f((float)mean_sq) : INFINITY;
        int flag = 0;
        if (gain_db > max_gain_db) {
            gain_db = 0.0f;  // the host raises after the batch; keep the row finite meanwhile
            flag = 1;
        }
        if (chunk == 0 && too_quiet != nullptr) too_quiet[b] = flag;
        gain_s = powf(10.0f, gain_db / 20.0f);
    }
    __syncthreads();
    const float gain = gain_s;
    float* dst = wav + (int64_t)b * wav_stride;
    const int64_t i0 = (int64_t)chunk * RS_SCALE_CHUNK;
    const int64_t i1 = i0 + RS_SCALE_CHUNK < n_out ? i0 + RS_SCALE_CHUNK : n_out;
    for (int64_t i = i0 + tid; i < i1; i += RS_THREADS) dst[i] *= gain;
}

// modified Bessel function of the first kind, order 0: sum_k ((x / 2)^k / k!)^2
static double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

// scipy.signal.firwin(2 half + 1, 1 / max_rate, window=('kaiser', 5.0)) * up in fp64, operation by operation, then rounded to fp32
static std::vector<float> design_taps(int up, int max_rate, int half) {
    const double pi = 3.14159265358979323846, beta = 5.0, cutoff = 1.0 / (double)max_rate, alpha = (double)half;
    const int numtaps = 2 * half + 1;
    std::vector<double> h(numtaps);
    const double i0_beta = bessel_i0(beta);
    double sum = 0.0;
    for (int i = 0; i < numtaps; ++i) {
        const double m = (double)i - alpha;
        const double y = pi * (i == half ? 1e-20 : cutoff * m);     // numpy.sinc's own guard at 0
        const double r = (m / alpha);
        const double w = bessel_i0(beta * sqrt(1.0 - r * r)) / i0_beta;
        h[i] = cutoff * (sin(y) / y) * w;
        sum += h[i];
    }
    std::vector<float> out(numtaps);
    for (int i = 0; i < numtaps; ++i) out[i] = (float)(h[i] / sum * (double)up);   // unity gain at DC, then * up
    return out;
}

static int64_t gcd64(int64_t a, int64_t b) {
    while (b != 0) {
        const int64_t r = a % b;
        a = b;
        b = r;
    }
    return a;
}

}  // namespace mv

struct MvResampler {
    int32_t up = 1, down = 1, half = 0, K = 1;          // of the rates (what mv_resampler_info reports)
    int32_t k_half = 0, k_K = 1;                        // what the kernel runs: up = down = 1 is the one-tap copy
    int32_t tile = 0, xcap = 0, table_lds = 0;
    std::vector<float> taps;                            // 2 half + 1, filter order
    float* d_table = nullptr;                           // k_K * up floats
};

static int64_t at_least_one(int64_t v) { return v > 0 ? v : 1; }   // (an empty row still gets the workgroup that writes its num_out and flag)
static int64_t resampler_span(const MvResampler* h, int64_t T) { return ((T - 1) * h->down) / h->up + h->k_K + 2; }   // frames T outputs read (upper bound)

extern "C" {

int mv_resampler_create(int32_t src_rate, int32_t dst_rate, MvResampler** out) {
    MV_REQUIRE(out != nullptr, "mv_resampler_create: null argument");
    MV_REQUIRE(src_rate > 0 && dst_rate > 0, "mv_resampler_create: sample rates must be positive");
    const int64_t g = mv::gcd64(dst_rate, src_rate);
    const int64_t up = dst_rate / g, down = src_rate / g, max_rate = up > down ? up : down;
    MV_REQUIRE(max_rate <= MV_RESAMPLER_MAX_RATE, "mv_resampler_create: max(up, down) above 1024 after reduction by the gcd of the rates");
    std::unique_ptr<MvResampler, decltype(&mv_resampler_destroy)> h(new MvResampler(), mv_resampler_destroy);   // (every early return destroys it)
    h->up = (int32_t)up;
    h->down = (int32_t)down;
    h->half = (int32_t)(10 * max_rate);
    h->K = (int32_t)mv::ceil_div(2 * h->half + 1, up);
    std::vector<float> table;
    if (max_rate == 1) {   // a pure down-mix copies x (resample_poly returns its input; firwin has no filter at cutoff 1)
        h->taps.assign(2 * h->half + 1, 0.0f);
        h->taps[h->half] = 1.0f;
        h->k_half = 0;
        h->k_K = 1;
        table.assign(1, 1.0f);
    } else {
        h->taps = mv::design_taps(h->up, (int)max_rate, h->half);
        h->k_half = h->half;
        h->k_K = h->K;
        table.assign((size_t)h->K * up, 0.0f);
        std::copy(h->taps.begin(), h->taps.end(), table.begin());
    }
    // LDS plan: the table beside the x span of a tile when both fit, else the table stays in global memory
    const int64_t table_floats = mv::round_up((int64_t)table.size(), 4);
    h->table_lds = table_floats + resampler_span(h.get(), 64) <= mv::RS_LDS_FLOATS ? 1 : 0;
    const int64_t x_max = mv::RS_LDS_FLOATS - (h->table_lds ? table_floats : 0);
    MV_REQUIRE(resampler_span(h.get(), 1) <= x_max, "mv_resampler_create: the taps of one output do not fit into LDS");
    int64_t x_lim = resampler_span(h.get(), 256) > mv::RS_X_FLOATS ? resampler_span(h.get(), 256) : mv::RS_X_FLOATS;
    if (x_lim > x_max) x_lim = x_max;
    int64_t tile = ((x_lim - h->k_K - 2) * up) / down + 1;
    if (tile > mv::RS_TILE_MAX) tile = mv::RS_TILE_MAX;
    h->tile = (int32_t)tile;
    h->xcap = (int32_t)resampler_span(h.get(), tile);
    MV_REQUIRE(h->tile >= 1 && h->xcap <= x_max, "mv_resampler_create: internal tile plan out of range");
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->d_table), table.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->d_table, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return mv::fail(MV_ERR_HIP, std::string("mv_resampler_create: ") + hipGetErrorString(e));
    *out = h.release();
    return MV_OK;
}

int mv_resampler_destroy(MvResampler* h) {
    if (h == nullptr) return MV_OK;
    hipFree(h->d_table);
    delete h;
    return MV_OK;
}

int mv_resampler_info(const MvResampler* h, MvResamplerInfo* info) {
    MV_REQUIRE(h != nullptr && info != nullptr, "mv_resampler_info: null argument");
    info->up = h->up;
    info->down = h->down;
    info->half = h->half;
    info->K = h->K;
    info->tile = h->tile;
    info->table_in_lds = h->table_lds;
    return MV_OK;
}

int mv_resampler_taps(const MvResampler* h, float* taps_host, int32_t n) {
    MV_REQUIRE(h != nullptr && taps_host != nullptr, "mv_resampler_taps: null argument");
    MV_REQUIRE(n == 2 * h->half + 1, "mv_resampler_taps: n must be 2 * half + 1");
    std::copy(h->taps.begin(), h->taps.end(), taps_host);
    return MV_OK;
}

int64_t mv_resampler_out_len(const MvResampler* h, int64_t n_in) {
    if (h == nullptr || n_in <= 0) return 0;
    return (n_in * h->up + h->down - 1) / h->down;
}

size_t mv_resampler_workspace_bytes(const MvResampler* h, int32_t B, int64_t L_in) {
    if (h == nullptr || B <= 0 || L_in < 0) return 0;
    const int64_t tiles = at_least_one(mv::ceil_div(mv_resampler_out_len(h, L_in), h->tile));
    return (size_t)mv::round_up(tiles * (int64_t)B * (int64_t)sizeof(double), 16);
}

int mv_resampler_forward_i16(const MvResampler* h, const int16_t* pcm, int64_t pcm_stride, int32_t channels, const int64_t* num_frames, int32_t B,
                             int64_t L_in, int32_t normalize, float target_db, float max_gain_db, float* wav, int64_t wav_stride, int64_t L_out,
                             int64_t* num_out, int32_t* too_quiet, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(h != nullptr, "mv_resampler_forward_i16: null handle");
    MV_REQUIRE(channels >= 1 && channels <= 8, "mv_resampler_forward_i16: channels outside 1 .. 8");
    MV_REQUIRE(B >= 0 && L_in >= 0 && L_in < ((int64_t)1 << 40) && L_out >= 0 && pcm_stride >= L_in * channels && wav_stride >= L_out,
               "mv_resampler_forward_i16: bad geometry");
    MV_REQUIRE(L_out >= mv_resampler_out_len(h, L_in), "mv_resampler_forward_i16: L_out smaller than mv_resampler_out_len(L_in)");
    if (B == 0) return MV_OK;
    MV_REQUIRE((pcm != nullptr || L_in == 0) && (wav != nullptr || L_out == 0), "mv_resampler_forward_i16: null buffer");
    MV_REQUIRE(workspace != nullptr, "mv_resampler_forward_i16: null workspace");
    MV_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mv_resampler_forward_i16: workspace must be 8-byte aligned");
    if (workspace_bytes < mv_resampler_workspace_bytes(h, B, L_in))
        return mv::fail(MV_ERR_WORKSPACE, "mv_resampler_forward_i16: workspace smaller than mv_resampler_workspace_bytes(B, L_in)");
    mv::ResampleArgs a;
    a.pcm = pcm; a.pcm_stride = pcm_stride; a.num_frames = num_frames; a.L_in = L_in; a.table = h->d_table;
    a.wav = wav; a.wav_stride = wav_stride; a.L_out = L_out; a.num_out = num_out; a.too_quiet = too_quiet;
    a.partial = static_cast<double*>(workspace);
    a.channels = channels; a.up = h->up; a.down = h->down; a.half = h->k_half; a.K = h->k_K; a.tile = h->tile;
    const int64_t n_out_max = mv_resampler_out_len(h, L_in);
    const int64_t tiles = at_least_one(mv::ceil_div(L_out, h->tile)), tiles_ws = at_least_one(mv::ceil_div(n_out_max, h->tile));
    const int64_t chunks = at_least_one(mv::ceil_div(n_out_max, mv::RS_SCALE_CHUNK));
    MV_REQUIRE(tiles * B < ((int64_t)1 << 31) && chunks * B < ((int64_t)1 << 31), "mv_resampler_forward_i16: too many tiles for one launch");
    a.tiles = (int32_t)tiles; a.tiles_ws = (int32_t)tiles_ws; a.normalize = normalize ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t smem = mv::RS_RED_BYTES + ((h->table_lds ? (size_t)mv::round_up((int64_t)h->k_K * h->up, 4) : 0) + (size_t)h->xcap) * sizeof(float);
    static mv::DeviceOnce attr_set;   // (per device: the attribute belongs to the current device's code object)
    int attr_set_slot;
    if (mv::device_once_pending(attr_set, &attr_set_slot)) {
        if (MV_SET_MAX_SMEM(mv::resample_tile_kernel<true>, 160 * 1024) != hipSuccess ||
            MV_SET_MAX_SMEM(mv::resample_tile_kernel<false>, 160 * 1024) != hipSuccess)
            return mv::fail(MV_ERR_HIP, "mv_resampler_forward_i16: cannot reserve dynamic LDS for resample_tile_kernel");
        mv::device_once_done(attr_set, attr_set_slot);
    }
    if (h->table_lds) MV_LAUNCH(mv::resample_tile_kernel<true>, ((unsigned)(tiles * B), 1, 1), (mv::RS_THREADS, 1, 1), smem, st, a);
    else MV_LAUNCH(mv::resample_tile_kernel<false>, ((unsigned)(tiles * B), 1, 1), (mv::RS_THREADS, 1, 1), smem, st, a);
    int rc = mv::check_launch("resample_tile_kernel");
    if (rc != MV_OK || !normalize) return rc;
    MV_LAUNCH(mv::resample_scale_kernel, ((unsigned)(chunks * B), 1, 1), (mv::RS_THREADS, 1, 1), 0, st, a.partial, a.tiles_ws, num_frames, L_in, h->up,
              h->down, target_db, max_gain_db, wav, wav_stride, too_quiet, (int)chunks);
    return mv::check_launch("resample_scale_kernel");
}

}  // extern "C"
