// Speaker search: the k best gallery rows per query by cosine similarity, without the queries x gallery score matrix.
//
// Replaces, for the recognition use case, the score matrix + host arg-max of mvector/predict.py:169-183 (sklearn cosine_similarity, then
// np.argmax per query): the scores are those of mv_cosine_f32 bit for bit (cosine_tile.h: the same per-element recipe on the f32 MFMA), the
// selection runs beside them and only [n, k] scores and indices leave the device.
//
// Structure (no workgroup waits for another, no atomics on floats, nothing n x m-sized is written):
//   * the gallery is cut into S contiguous slices of 16-row tiles, the queries into chunks whose running lists fit the workgroup's LDS; one
//     workgroup of four waves per (chunk, slice) walks its slice: per gallery tile the waves' K blocks of the 16 gallery rows are loaded once
//     (kept in registers up to dim 256, re-read through the caches above), then every 16-query tile of the chunk is scored against them;
//   * a score becomes the 64-bit word (sort_key << 32) | ~row, so that one unsigned compare orders by key descending, then row ascending;
//     it is first compared with the query's current k-th word -- almost every score ends there -- and the survivors of a tile are merged
//     into the query's sorted list in LDS by rank (the slot of an element is the number of elements above it), the 16 lanes of a query at once;
//   * each workgroup writes its [rows][k] lists to the workspace [S][n][k]; a second launch, one workgroup per query, merges the S sorted lists
//     head by head.
// Selection under a total order does not depend on the partition: the output is the same for every S, query batch and stream.
#include "cosine_tile.h"
#include "order_key.h"

namespace mv {

constexpr int ST_LIST_BYTES = 32768;   // LDS of a workgroup's running lists: rows_per_chunk * k * 8 bytes at most
constexpr int ST_MAX_CHUNK = 1024;     // query rows per chunk at most
constexpr int ST_HOLD = 4;             // K blocks of 16 per wave whose gallery fragment stays in registers: dim <= 256
constexpr int ST_MAX_SLICES = 4096;    // heads of the merge kernel in LDS
constexpr int ST_MAX_K = 64;
constexpr int ST_MAX_DIM = 2047;       // the range in which mv_cosine_f32 runs linear_f32_kernel<4>

// word 0 is "no candidate": a sort_key is never below 0x007FFFFF (-inf)
__device__ __forceinline__ uint64_t topk_word(float v, int64_t row) { return ((uint64_t)sort_key(v) << 32) | (uint32_t)~(uint32_t)row; }

struct TopkPlan {
    int chunk;     // query rows per workgroup (a multiple of 16)
    int nchunks;
    int slices;    // S
    size_t ws_bytes;
};

// S: `hint` when positive, else four workgroups per compute unit over the chunks; never more slices than gallery tiles
static TopkPlan topk_plan(int64_t n, int64_t m, int k, int hint) {
    TopkPlan p;
    int chunk = (ST_LIST_BYTES / (8 * k)) & ~15;
    chunk = chunk > ST_MAX_CHUNK ? ST_MAX_CHUNK : chunk;
    const int64_t n16 = round_up(n > 0 ? n : 1, 16);
    p.chunk = (int)(n16 < chunk ? n16 : chunk);
    p.nchunks = (int)ceil_div(n > 0 ? n : 1, p.chunk);
    const int64_t tiles = ceil_div(m, 16);
    int64_t s = hint > 0 ? hint : ceil_div(4 * (int64_t)device_cu_count(), p.nchunks);
    const int64_t grid_cap = (int64_t)0x7FFFFFFF / p.nchunks;
    s = s > ST_MAX_SLICES ? ST_MAX_SLICES : s;
    s = s > grid_cap ? grid_cap : s;
    s = s > tiles ? tiles : s;
    p.slices = (int)s;   // 0 for an empty gallery
    p.ws_bytes = (size_t)(p.slices > 0 ? p.slices : 1) * (size_t)(n > 0 ? n : 1) * k * 8;
    return p;
}

// grid (chunk, slice).  part [S][n][k]: the slice's list per query, best first, 0 behind the candidates it has.
template <bool HOLD>
__global__ __launch_bounds__(256) void cosine_topk_slice_kernel(const float* q, int n, const float* gal, int m, int dim, int k, int chunk, int slices,
                                                                uint64_t* part) {
    __shared__ float red[4][16][17];
    __shared__ float nrm[2][4][16];
    __shared__ uint64_t cand[16][16];
    __shared__ int flag[3];
    MV_DYN_SMEM(smem);
    uint64_t* lst = reinterpret_cast<uint64_t*>(smem);   // [nq][k]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = MV_UNIFORM(tid >> 6);
    const int i = lane & 15;
    const int g = lane >> 4;
    const int q0 = blockIdx.x * chunk;
    const int nq = n - q0 < chunk ? n - q0 : chunk;
    const int s = blockIdx.y;
    const int64_t tiles = ((int64_t)m + 15) / 16;
    const int t0 = (int)(s * tiles / slices), t1 = (int)((s + 1) * tiles / slices);
    for (int idx = tid; idx < nq * k; idx += 256) lst[idx] = 0;
    if (tid < 3) flag[tid] = 0;
    __syncthreads();
    const bool vec = (dim % 4 == 0) && ((reinterpret_cast<uintptr_t>(q) & 15) == 0) && ((reinterpret_cast<uintptr_t>(gal) & 15) == 0);
    int step = 0;
    for (int t = t0; t < t1; ++t) {
        const int64_t grow = (int64_t)t * 16 + i < m ? (int64_t)t * 16 + i : (int64_t)m - 1;   // clamp: duplicates are masked below
        const float* wrow = gal + grow * dim;
        float4v wh[ST_HOLD];
        if (HOLD) {
#pragma unroll
            for (int u = 0; u < ST_HOLD; ++u) {
                const int k0 = (wave + 4 * u) * 16;
                wh[u] = float4v{0.0f, 0.0f, 0.0f, 0.0f};
                if (k0 < dim) wh[u] = load4_guard(wrow, k0 + 4 * g, dim, vec);
            }
        }
        for (int qt = 0; qt < nq; qt += 16, ++step) {
            const int qr = q0 + qt + i < n ? q0 + qt + i : n - 1;
            const float* xrow = q + (int64_t)qr * dim;
            float4v acc = float4v{0.0f, 0.0f, 0.0f, 0.0f};
            float sqx = 0.0f, sqw = 0.0f;
            if (HOLD) {
                float4v xa[ST_HOLD];
#pragma unroll
                for (int u = 0; u < ST_HOLD; ++u) {
                    const int k0 = (wave + 4 * u) * 16;
                    xa[u] = float4v{0.0f, 0.0f, 0.0f, 0.0f};
                    if (k0 < dim) xa[u] = load4_guard(xrow, k0 + 4 * g, dim, vec);
                }
#pragma unroll
                for (int u = 0; u < ST_HOLD; ++u)
                    if ((wave + 4 * u) * 16 < dim) tile_block_step(xa[u], wh[u], acc, sqx, sqw, 1);
            } else {
                for (int k0 = wave * 16; k0 < dim; k0 += 64) {
                    float4v xa, wb;
                    tile_load_block(xrow, wrow, k0, g, dim, vec, xa, wb);
                    tile_block_step(xa, wb, acc, sqx, sqw, 1);
                }
            }
            sqx = tile_norm_fold(sqx);
            sqw = tile_norm_fold(sqw);
            if (g == 0) {
                nrm[0][wave][i] = sqx;
                nrm[1][wave][i] = sqw;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][4 * g + r][i] = acc[r];
            if (tid == 0) flag[(step + 1) % 3] = 0;   // the flag of the next step: last read two barriers ago
            __syncthreads();
            const int r = tid >> 4, c = tid & 15;   // element (query r, gallery row c) of the tile: the 16 lanes of a query are neighbours
            const bool live = qt + r < nq;
            uint64_t* L = lst + (live ? qt + r : 0) * k;
            uint64_t word = 0;
            if (live && (int64_t)t * 16 + c < m) {
                word = topk_word(tile_finish<4>(red, nrm, r, c, 1), (int64_t)t * 16 + c);
                if (word <= L[k - 1]) word = 0;   // not above the query's k-th: where almost every score ends
            }
            cand[r][c] = word;
            if (word != 0) flag[step % 3] = 1;
            __syncthreads();
            if (flag[step % 3] != 0) {   // (uniform: read behind the barrier, cleared no sooner than the barrier after the next)
                // the query's list and its survivors merged by rank, all 16 lanes of the query at once: an element's new slot is the number of
                // elements above it (words are unique; the zeros of a list that is not full keep their order behind everything else).
                // Lane c moves its own survivor and the old entries c, c + 16, ...; every slot below k receives exactly one element.
                int wpos = k, opos[ST_MAX_K / 16];
                uint64_t old[ST_MAX_K / 16];
                if (live) {
                    if (word != 0) {
                        wpos = 0;
                        for (int j = 0; j < k; ++j) wpos += L[j] > word ? 1 : 0;
                        for (int c2 = 0; c2 < 16; ++c2) wpos += cand[r][c2] > word ? 1 : 0;
                    }
#pragma unroll
                    for (int u = 0; u < ST_MAX_K / 16; ++u) {
                        const int j = c + 16 * u;
                        opos[u] = k;
                        if (j < k) {
                            old[u] = L[j];
                            opos[u] = j;
                            for (int c2 = 0; c2 < 16; ++c2) opos[u] += cand[r][c2] > old[u] ? 1 : 0;
                        }
                    }
                }
                __syncthreads();   // every old entry is read before any slot is rewritten
                if (live) {
                    if (wpos < k) L[wpos] = word;
#pragma unroll
                    for (int u = 0; u < ST_MAX_K / 16; ++u)
                        if (opos[u] < k && opos[u] != c + 16 * u) L[opos[u]] = old[u];
                }
                __syncthreads();   // the lists, before the next tile's compares read them
            }
        }
    }
    __syncthreads();
    uint64_t* out = part + ((int64_t)s * n + q0) * k;
    for (int idx = tid; idx < nq * k; idx += 256) out[idx] = lst[idx];
}

// one workgroup per query: the S sorted lists merged head by head.  Thread t owns the lists t, t + T, ... (T = blockDim.x: one wave up to 64
// slices, four above)
__global__ __launch_bounds__(256) void cosine_topk_merge_kernel(const uint64_t* part, int n, int k, int slices, float* scores, int32_t* index) {
    __shared__ uint64_t head[ST_MAX_SLICES];
    __shared__ unsigned char taken[ST_MAX_SLICES];
    __shared__ uint64_t wmax[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int threads = blockDim.x, waves = threads >> 6;
    const int64_t qi = blockIdx.x;
    for (int s = tid; s < slices; s += threads) {
        head[s] = part[((int64_t)s * n + qi) * k];
        taken[s] = 0;
    }
    for (int j = 0; j < k; ++j) {
        uint64_t best = 0;
        for (int s = tid; s < slices; s += threads) best = head[s] > best ? head[s] : best;
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            const uint64_t other = __shfl_xor(best, msk);
            best = other > best ? other : best;
        }
        uint64_t top = best;
        if (waves > 1) {
            if (lane == 0) wmax[j & 1][wave] = best;
            __syncthreads();   // (wmax[j & 1] is written again two rounds on, behind the next round's barrier)
            top = wmax[j & 1][0];
            for (int w = 1; w < waves; ++w) top = wmax[j & 1][w] > top ? wmax[j & 1][w] : top;
        }
        if (top != 0) {   // words are unique (they carry the row): one list has it at its head
            for (int s = tid; s < slices; s += threads) {
                if (head[s] == top) {
                    const int p = ++taken[s];
                    head[s] = p < k ? part[((int64_t)s * n + qi) * k + p] : 0;
                }
            }
        }
        if (tid == 0) {
            scores[qi * k + j] = top != 0 ? sort_key_value((uint32_t)(top >> 32)) : -INFINITY;
            index[qi * k + j] = top != 0 ? (int32_t)~(uint32_t)top : -1;
        }
    }
}

static int cosine_topk_check(int64_t n, int64_t m, int dim, int k) {
    MV_REQUIRE(n >= 0 && m >= 0, "mv_cosine_topk_f32: negative n or m");
    MV_REQUIRE(k >= 1 && k <= ST_MAX_K, "mv_cosine_topk_f32: k outside 1 .. 64");
    MV_REQUIRE(dim >= 1, "mv_cosine_topk_f32: dim below 1");
    if (dim > ST_MAX_DIM)
        return fail(MV_ERR_UNSUPPORTED, "mv_cosine_topk_f32: dim above 2047 (the range in which mv_cosine_f32 takes its four-wave form, whose bits the search returns)");
    return MV_OK;
}

}  // namespace mv

extern "C" size_t mv_cosine_topk_workspace_bytes(int32_t n, int32_t m, int32_t dim, int32_t k, int32_t slices_hint) {
    if (mv::cosine_topk_check(n, m, dim, k) != MV_OK) return 0;
    return mv::topk_plan(n, m, k, slices_hint).ws_bytes;
}

extern "C" int mv_cosine_topk_f32(const float* q, int32_t n, const float* g, int32_t m, int32_t dim, int32_t k, float* scores, int32_t* index,
                                  int32_t slices_hint, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    const int rc = cosine_topk_check(n, m, dim, k);
    if (rc != MV_OK) return rc;
    if (n == 0) return MV_OK;
    MV_REQUIRE(q != nullptr && (g != nullptr || m == 0) && scores != nullptr && index != nullptr, "mv_cosine_topk_f32: null tensor");
    MV_REQUIRE(workspace != nullptr, "mv_cosine_topk_f32: null workspace");
    const TopkPlan p = topk_plan(n, m, k, slices_hint);
    if (workspace_bytes < p.ws_bytes)
        return fail(MV_ERR_WORKSPACE, "mv_cosine_topk_f32: workspace smaller than mv_cosine_topk_workspace_bytes(n, m, dim, k, slices_hint)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "mv_cosine_topk_f32: workspace not 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint64_t* part = static_cast<uint64_t*>(workspace);
    if (p.slices > 0) {
        const size_t lds = (size_t)p.chunk * k * 8;
        if (dim <= 64 * ST_HOLD) {
            MV_LAUNCH(cosine_topk_slice_kernel<true>, ((unsigned)p.nchunks, (unsigned)p.slices, 1), (256, 1, 1), lds, st, q, n, g, m, dim, k, p.chunk, p.slices,
                      part);
        } else {
            MV_LAUNCH(cosine_topk_slice_kernel<false>, ((unsigned)p.nchunks, (unsigned)p.slices, 1), (256, 1, 1), lds, st, q, n, g, m, dim, k, p.chunk, p.slices,
                      part);
        }
        const int rcl = check_launch("cosine_topk_slice_kernel");
        if (rcl != MV_OK) return rcl;
    }
    MV_LAUNCH(cosine_topk_merge_kernel, ((unsigned)n, 1, 1), (p.slices <= 64 ? 64u : 256u, 1, 1), 0, st, part, n, k, p.slices, scores, index);
    return check_launch("cosine_topk_merge_kernel");
}
