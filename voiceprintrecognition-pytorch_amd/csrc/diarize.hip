// Speaker diarization behind the embeddings: chunk rows out of one resident waveform, the pruned / symmetrised affinity
// matrix with its degrees, and the lowest eigenpairs of the graph Laplacian L = diag(degree) - M.
//
// The reference (mvector/infer_utils/speaker_diarization.py) does all of this on the host in fp32: a Python loop of N
// argsorts (SpectralCluster.p_pruning), the Laplacian, scipy.linalg.eigh of the full N x N matrix (of which it reads
// lambdas[:16] and eig_vecs[:, :k]) and k_means.  Here:
//   mv_wave_chunks_f32         rows[i] = wav[start_i : start_i + len_i] | zeros, with the dB normalisation of wave.hip taken
//                              over the padded row (predict_batch normalises the already padded chunk)
//   mv_affinity_laplacian_f32  (a) per row the cut below which the n_prune smallest entries fall: radix select over
//                              order-preserving 32-bit keys in LDS; among equal values the LOWER column index is dropped
//                              first (numpy's default argsort leaves that open, so the rule is this library's),
//                              (b) M = 0.5f * (pruned + pruned^T) in fp32 with a zero diagonal, (c) degree_i = sum_j |M_ij| in fp64
//   mv_laplacian_eig_lowest    Chebyshev-filtered subspace iteration in fp64 on a block of min(32, N) vectors: filter the Ritz
//                              vectors with the scaled three-term recurrence that damps [largest Ritz value, 2 max degree],
//                              Cholesky-QR twice on column-scaled Y, Rayleigh-Ritz, residuals of the m wanted columns.
// Plain HIP C++ (fp64 FMAs, LDS, __syncthreads): whether the fp64 matrix instructions would pay is open.
// Every sum has one fixed order (per-workgroup partials, slices summed in slice order, integer atomics only for the
// radix histogram), so results are bit-identical from run to run and on any stream.
// The b x b problems (Cholesky, triangular inverse, cyclic Jacobi) are solved on the host between launches:
// mv_laplacian_eig_lowest synchronises its stream.
#include "common.h"
#include "order_key.h"

#include <vector>

namespace mv {
namespace {

constexpr int DZ_MAX_N = 16384;  // one row of keys is 64 KiB of LDS there, M is 1 GiB
constexpr int DZ_MAX_M = 16;     // the reference reads lambdas[:16]
constexpr int DZ_B = 32;         // widest block; the b x b matrices have this leading dimension
constexpr int PT_ROWS = 128, PT_K = 32;  // product tile: 128 rows x 32 columns of M against 32 rows of X, 4 x 4 outputs per thread
constexpr int PT_TARGET_WGS = 512;       // split K until about two workgroups per compute unit exist
constexpr int PT_MAX_SLICES = 16;
constexpr int GR_ROWS = 64;              // rows per workgroup of the b x b reductions

// ------------------------------------------------------------------------------------------------ chunks
__global__ __launch_bounds__(256) void wave_chunks_kernel(const float* wav, int64_t L, const int64_t* start, const int64_t* len, int64_t chunk_len,
                                                          int normalize, float target_db, float max_gain_db, float* rows, int64_t rows_stride,
                                                          int32_t* too_quiet) {
    __shared__ double red[256];
    __shared__ float gain_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t s = start[b], n = len[b];  // clamped here: the table lives on the device, the host cannot check it
    s = s < 0 ? 0 : (s > L ? L : s);
    n = n < 0 ? 0 : (n > chunk_len ? chunk_len : n);
    n = n > L - s ? L - s : n;
    const float* src = wav + s;
    float* dst = rows + (int64_t)b * rows_stride;
    float gain = 1.0f;
    if (normalize) {
        double part = 0.0;  // x * x is exact in fp64
        for (int64_t i = tid; i < n; i += 256) {
            const double x = (double)src[i];
            part = fma(x, x, part);
        }
        red[tid] = part;
        __syncthreads();
        for (int st = 128; st > 0; st >>= 1) {
            if (tid < st) red[tid] += red[tid + st];
            __syncthreads();
        }
        if (tid == 0) {
            const double mean_sq = red[0] / (double)chunk_len;  // over the padded row, zeros included
            float gain_db = mean_sq > 0.0 ? target_db - 10.0f * log10f((float)mean_sq) : INFINITY;
            int flag = 0;
            if (gain_db > max_gain_db) {
                gain_db = 0.0f;  // the host raises after the batch; the row stays unscaled meanwhile
                flag = 1;
            }
            if (too_quiet != nullptr) too_quiet[b] = flag;
            gain_s = powf(10.0f, gain_db / 20.0f);
        }
        __syncthreads();
        gain = gain_s;
    } else if (tid == 0 && too_quiet != nullptr) {
        too_quiet[b] = 0;
    }
    for (int64_t i = tid; i < chunk_len; i += 256) dst[i] = i < n ? src[i] * gain : 0.0f;
}

// ------------------------------------------------------------------------------------------------ affinity
// (keys: order_key of order_key.h, an unsigned image with the order of the floats)
// entry (row, col) survives the pruning of its row: above the cut, or equal to it from column tie_col on
__device__ __forceinline__ bool kept(uint32_t key, int col, uint32_t cut_key, uint32_t tie_col) {
    return key > cut_key || (key == cut_key && (uint32_t)col >= tie_col);
}

// one workgroup per row: cut[2 * row] = key of the n_prune-th smallest entry, cut[2 * row + 1] = first column from which an
// entry equal to the cut is kept
__global__ __launch_bounds__(256) void prune_cut_kernel(const float* S, int N, int n_prune, uint32_t* cut) {
    __shared__ uint32_t keys[DZ_MAX_N];
    __shared__ unsigned hist[256];
    __shared__ unsigned cnt[256];
    __shared__ unsigned sel[2];  // chosen high bits, rank left among the keys that share them
    const int row = blockIdx.x, tid = threadIdx.x;
    if (n_prune == 0) {  // nothing dropped: every key is above or at key 0 from column 0 on
        if (tid == 0) cut[2 * row] = 0u, cut[2 * row + 1] = 0u;
        return;
    }
    const float* src = S + (int64_t)row * N;
    for (int j = tid; j < N; j += 256) keys[j] = order_key(src[j]);
    if (tid == 0) sel[0] = 0u, sel[1] = (unsigned)(n_prune - 1);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t high = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
        hist[tid] = 0u;
        __syncthreads();
        const uint32_t prefix = sel[0];
        for (int j = tid; j < N; j += 256) {
            const uint32_t k = keys[j];
            if ((k & high) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);  // integer counts: order-free
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned r = sel[1];
            unsigned cum = 0u;
            for (unsigned d = 0; d < 256u; ++d) {
                const unsigned c = hist[d];
                if (r < cum + c) {
                    sel[0] = prefix | (d << shift);
                    sel[1] = r - cum;
                    break;
                }
                cum += c;
            }
        }
        __syncthreads();
    }
    const uint32_t cut_key = sel[0];
    const unsigned need = sel[1] + 1u;  // entries equal to the cut that fall, lowest columns first
    const int seg = (N + 255) / 256, lo = tid * seg, hi = lo + seg < N ? lo + seg : N;
    unsigned c = 0u;
    for (int j = lo; j < hi; ++j) c += keys[j] == cut_key ? 1u : 0u;
    cnt[tid] = c;
    __syncthreads();
    unsigned before = 0u;
    for (int t = 0; t < tid; ++t) before += cnt[t];
    if (before < need && need <= before + c) {  // the thread whose columns hold the last entry that falls
        for (int j = lo; j < hi; ++j) {
            if (keys[j] == cut_key && ++before == need) {
                cut[2 * row + 1] = (uint32_t)(j + 1);
                break;
            }
        }
    }
    if (tid == 0) cut[2 * row] = cut_key;
}

// M = 0.5f * (P + P^T), P = S with the pruned entries zeroed; zero diagonal.  32 x 32 tiles, the transposed one through LDS.
__global__ __launch_bounds__(256) void affinity_sym_kernel(const float* S, const uint32_t* cut, int N, float* M) {
    __shared__ float tt[32][33];
    const int tx = threadIdx.x % 32, ty = threadIdx.x / 32;
    const int bi = blockIdx.y * 32, bj = blockIdx.x * 32;
    for (int u = 0; u < 4; ++u) {
        const int r = bj + ty + 8 * u, c = bi + tx;
        float v = 0.0f;
        if (r < N && c < N) {
            const float x = S[(int64_t)r * N + c];
            v = kept(order_key(x), c, cut[2 * r], cut[2 * r + 1]) ? x : 0.0f;
        }
        tt[ty + 8 * u][tx] = v;
    }
    __syncthreads();
    for (int u = 0; u < 4; ++u) {
        const int r = bi + ty + 8 * u, c = bj + tx;
        if (r < N && c < N) {
            const float x = S[(int64_t)r * N + c];
            const float a = kept(order_key(x), c, cut[2 * r], cut[2 * r + 1]) ? x : 0.0f;
            M[(int64_t)r * N + c] = r == c ? 0.0f : 0.5f * (a + tt[tx][ty + 8 * u]);
        }
    }
}

__global__ __launch_bounds__(256) void degree_kernel(const float* M, int N, double* degree) {
    __shared__ double red[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* src = M + (int64_t)row * N;
    double part = 0.0;
    for (int j = tid; j < N; j += 256) part += fabs((double)src[j]);
    red[tid] = part;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    if (tid == 0) degree[row] = red[0];
}

// ------------------------------------------------------------------------------------------------ eigen solver: device side
// the fixed start block: splitmix64 of (seed, element index) -> uniform in [-1, 1)
__global__ __launch_bounds__(256) void eig_init_kernel(double* X, int64_t n_elems, uint64_t seed) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_elems) return;
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    X[i] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}

// part[slice][row][c] = sum over the slice's columns k of M[row][k] * X[k][c]; grid (row tiles, slices)
__global__ __launch_bounds__(256) void product_partial_kernel(const float* M, const double* X, int N, int b, int k_per_slice, double* part) {
    __shared__ float Ms[PT_ROWS][PT_K + 1];
    __shared__ __attribute__((aligned(16))) double Xs[PT_K][DZ_B];
    const int tid = threadIdx.x, lc = tid % 32, lr = tid / 32;
    const int row0 = blockIdx.x * PT_ROWS;
    const int k_lo = blockIdx.y * k_per_slice, k_hi = k_lo + k_per_slice < N ? k_lo + k_per_slice : N;
    const int r0 = 4 * (tid / 8), c0 = 4 * (tid % 8);
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int k0 = k_lo; k0 < k_hi; k0 += PT_K) {
        const int gk = k0 + lc;
#pragma unroll
        for (int u = 0; u < PT_ROWS / 8; ++u) {
            const int r = lr + 8 * u, gr = row0 + r;
            Ms[r][lc] = (gr < N && gk < k_hi) ? M[(int64_t)gr * N + gk] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < PT_K / 8; ++u) {
            const int k = lr + 8 * u, gkk = k0 + k;
            Xs[k][lc] = (gkk < k_hi && lc < b) ? X[(int64_t)gkk * b + lc] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (int k = 0; k < PT_K; ++k) {
            double x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = Xs[k][c0 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double a = (double)Ms[r0 + i][k];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fma(a, x[j], acc[i][j]);
            }
        }
        __syncthreads();
    }
    double* dst = part + (int64_t)blockIdx.y * N * b;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gr = row0 + r0 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (gr < N && c0 + j < b) dst[(int64_t)gr * b + c0 + j] = acc[i][j];
    }
}

// slices summed in slice order, then out = alpha * (L X - shift * X) - beta * Z with L X = degree * X - M X (Z may be NULL)
__global__ __launch_bounds__(256) void product_finish_kernel(const double* part, int nslices, const double* X, const double* degree, const double* Z,
                                                             double alpha, double shift, double beta, int N, int b, double* out) {
    const int64_t n_elems = (int64_t)N * b, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_elems) return;
    double mx = 0.0;
    for (int s = 0; s < nslices; ++s) mx += part[s * n_elems + i];
    const double x = X[i];
    double v = alpha * ((degree[i / b] * x - mx) - shift * x);
    if (Z != nullptr) v -= beta * Z[i];
    out[i] = v;
}

// part[chunk][i][j] = sum over the chunk's rows r of A[r][i] * B[r][j]  (32 x 32 with zeros beyond b)
__global__ __launch_bounds__(256) void gram_partial_kernel(const double* A, const double* B, int N, int b, double* part) {
    __shared__ __attribute__((aligned(16))) double As[GR_ROWS][DZ_B];
    __shared__ __attribute__((aligned(16))) double Bs[GR_ROWS][DZ_B];
    const int tid = threadIdx.x, lc = tid % 32, lr = tid / 32;
    const int row0 = blockIdx.x * GR_ROWS;
#pragma unroll
    for (int u = 0; u < GR_ROWS / 8; ++u) {
        const int r = lr + 8 * u, gr = row0 + r;
        const bool in = gr < N && lc < b;
        As[r][lc] = in ? A[(int64_t)gr * b + lc] : 0.0;
        Bs[r][lc] = in ? B[(int64_t)gr * b + lc] : 0.0;
    }
    __syncthreads();
    const int i = tid / 8, j0 = 4 * (tid % 8);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < GR_ROWS; ++r) {
        const double a = As[r][i];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fma(a, Bs[r][j0 + j], acc[j]);
    }
    double* dst = part + (int64_t)blockIdx.x * (DZ_B * DZ_B) + i * DZ_B + j0;
#pragma unroll
    for (int j = 0; j < 4; ++j) dst[j] = acc[j];
}

// part[chunk][c] = sum over the chunk's rows of (W[r][c] - theta[c] * V[r][c])^2
__global__ __launch_bounds__(256) void resid_partial_kernel(const double* W, const double* V, const double* theta, int N, int b, double* part) {
    __shared__ double red[8][DZ_B];
    const int tid = threadIdx.x, lc = tid % 32, lr = tid / 32;
    const int row0 = blockIdx.x * GR_ROWS;
    double acc = 0.0;
    if (lc < b) {
        const double th = theta[lc];
        for (int u = 0; u < GR_ROWS / 8; ++u) {
            const int gr = row0 + lr + 8 * u;
            if (gr < N) {
                const double d = W[(int64_t)gr * b + lc] - th * V[(int64_t)gr * b + lc];
                acc = fma(d, d, acc);
            }
        }
    }
    red[lr][lc] = acc;
    __syncthreads();
    if (lr == 0) {
        double s = 0.0;
        for (int u = 0; u < 8; ++u) s += red[u][lc];
        part[(int64_t)blockIdx.x * DZ_B + lc] = s;
    }
}

__global__ __launch_bounds__(256) void sum_slices_kernel(const double* part, int nslices, int n_elems, double* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_elems) return;
    double s = 0.0;
    for (int k = 0; k < nslices; ++k) s += part[(int64_t)k * n_elems + i];
    out[i] = s;
}

// Out[N][b] = A[N][b] * T[b][b]  (T with leading dimension 32)
__global__ __launch_bounds__(256) void rotate_kernel(const double* A, const double* T, int N, int b, double* Out) {
    __shared__ double Ts[DZ_B][DZ_B];
    const int tid = threadIdx.x;
    for (int e = tid; e < DZ_B * DZ_B; e += 256) Ts[e / DZ_B][e % DZ_B] = T[e];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + tid;
    if (i >= (int64_t)N * b) return;
    const int64_t row = i / b;
    const int c = (int)(i % b);
    const double* a = A + row * b;
    double acc = 0.0;
    for (int k = 0; k < b; ++k) acc = fma(a[k], Ts[k][c], acc);
    Out[i] = acc;
}

__global__ __launch_bounds__(256) void take_cols_kernel(const double* V, int N, int b, int m, double* out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * m) return;
    out[i] = V[(i / m) * b + i % m];
}

// ------------------------------------------------------------------------------------------------ eigen solver: host side
struct EigPlan {
    int b, row_tiles, k_per_slice, nslices, chunks;
    size_t off_block[5], off_part, off_gpart, off_small, off_upload, total;
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

EigPlan eig_plan(int N, int block) {
    EigPlan p;
    p.b = block;
    p.row_tiles = (int)ceil_div(N, PT_ROWS);
    int want = (int)ceil_div(PT_TARGET_WGS, p.row_tiles);
    want = want < 1 ? 1 : (want > PT_MAX_SLICES ? PT_MAX_SLICES : want);
    p.k_per_slice = (int)round_up(ceil_div(N, want), PT_K);
    p.nslices = (int)ceil_div(N, p.k_per_slice);
    p.chunks = (int)ceil_div(N, GR_ROWS);
    size_t off = 0;
    const size_t blk = align256((size_t)N * p.b * sizeof(double));
    for (int i = 0; i < 5; ++i) p.off_block[i] = off, off += blk;
    p.off_part = off, off += align256((size_t)p.nslices * N * p.b * sizeof(double));
    p.off_gpart = off, off += align256((size_t)p.chunks * DZ_B * DZ_B * sizeof(double));
    p.off_small = off, off += align256((size_t)DZ_B * DZ_B * sizeof(double));
    p.off_upload = off, off += align256((size_t)(DZ_B * DZ_B + DZ_B) * sizeof(double));
    p.total = off;
    return p;
}

// the limits of the solver, refused by name; *block = the block size with 0 resolved to min(32, N)
int eig_check(int N, const MvEigCfg* cfg, int* block) {
    MV_REQUIRE(cfg != nullptr, "mv_laplacian_eig_lowest: null cfg");
    MV_REQUIRE(N >= 2 && N <= DZ_MAX_N, "mv_laplacian_eig_lowest: N outside 2 .. 16384");
    const int most = N < DZ_B ? N : DZ_B;
    MV_REQUIRE(cfg->m >= 1 && cfg->m <= DZ_MAX_M && cfg->m <= N, "mv_laplacian_eig_lowest: m outside 1 .. min(16, N)");
    const int b = cfg->block == 0 ? most : cfg->block;
    MV_REQUIRE(b >= cfg->m && b <= most, "mv_laplacian_eig_lowest: block outside m .. min(32, N)");
    MV_REQUIRE(cfg->degree >= 1 && cfg->degree <= 256, "mv_laplacian_eig_lowest: filter degree outside 1 .. 256");
    MV_REQUIRE(cfg->max_iters >= 0, "mv_laplacian_eig_lowest: negative max_iters");
    MV_REQUIRE(cfg->tol > 0.0 && cfg->tol < 1.0, "mv_laplacian_eig_lowest: tol outside (0, 1)");
    *block = b;
    return MV_OK;
}

// G (b x b, ld 32, symmetric positive definite) -> T = D R^-1 with D = diag(1 / sqrt(G_jj)) and D G D = R^T R, so that Y T has
// orthonormal columns.  Returns false on a non-positive (or non-finite) pivot.
bool cholqr_factor(const double* G, int b, double* T) {
    double d[DZ_B], R[DZ_B][DZ_B], Ri[DZ_B][DZ_B];
    for (int j = 0; j < b; ++j) {
        if (!(G[j * DZ_B + j] > 0.0) || !std::isfinite(G[j * DZ_B + j])) return false;
        d[j] = 1.0 / sqrt(G[j * DZ_B + j]);
    }
    for (int j = 0; j < b; ++j) {  // upper Cholesky factor, column by column
        for (int i = 0; i <= j; ++i) {
            double s = 0.5 * (G[i * DZ_B + j] + G[j * DZ_B + i]) * d[i] * d[j];
            for (int k = 0; k < i; ++k) s -= R[k][i] * R[k][j];
            if (i < j) {
                R[i][j] = s / R[i][i];
            } else {
                if (!(s > 0.0) || !std::isfinite(s)) return false;
                R[j][j] = sqrt(s);
            }
        }
    }
    for (int j = 0; j < b; ++j) {  // R^-1 by back substitution
        for (int i = 0; i < b; ++i) Ri[i][j] = 0.0;
        Ri[j][j] = 1.0 / R[j][j];
        for (int i = j - 1; i >= 0; --i) {
            double s = 0.0;
            for (int k = i + 1; k <= j; ++k) s -= R[i][k] * Ri[k][j];
            Ri[i][j] = s / R[i][i];
        }
    }
    for (int e = 0; e < DZ_B * DZ_B; ++e) T[e] = 0.0;
    for (int i = 0; i < b; ++i)
        for (int j = i; j < b; ++j) T[i * DZ_B + j] = d[i] * Ri[i][j];
    return true;
}

// symmetric H (b x b, ld 32) -> eigenvalues ascending in theta, eigenvectors in the columns of Z (ld 32): cyclic Jacobi
void jacobi_eig(const double* Hin, int b, double* theta, double* Z) {
    double H[DZ_B][DZ_B], Q[DZ_B][DZ_B];
    double total = 0.0;
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < b; ++j) {
            H[i][j] = 0.5 * (Hin[i * DZ_B + j] + Hin[j * DZ_B + i]);
            Q[i][j] = i == j ? 1.0 : 0.0;
            total += H[i][j] * H[i][j];
        }
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < b; ++p)
            for (int q = p + 1; q < b; ++q) off += H[p][q] * H[p][q];
        if (!(off > 1e-36 * total)) break;
        for (int p = 0; p < b; ++p)
            for (int q = p + 1; q < b; ++q) {
                if (H[p][q] == 0.0) continue;
                const double th = (H[q][q] - H[p][p]) / (2.0 * H[p][q]);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < b; ++k) {
                    const double hp = H[k][p], hq = H[k][q];
                    H[k][p] = c * hp - s * hq, H[k][q] = s * hp + c * hq;
                }
                for (int k = 0; k < b; ++k) {
                    const double hp = H[p][k], hq = H[q][k];
                    H[p][k] = c * hp - s * hq, H[q][k] = s * hp + c * hq;
                }
                for (int k = 0; k < b; ++k) {
                    const double zp = Q[k][p], zq = Q[k][q];
                    Q[k][p] = c * zp - s * zq, Q[k][q] = s * zp + c * zq;
                }
            }
    }
    int order[DZ_B];
    for (int i = 0; i < b; ++i) order[i] = i;
    for (int i = 1; i < b; ++i) {  // stable insertion sort by eigenvalue
        const int o = order[i];
        int j = i;
        for (; j > 0 && H[order[j - 1]][order[j - 1]] > H[o][o]; --j) order[j] = order[j - 1];
        order[j] = o;
    }
    for (int e = 0; e < DZ_B * DZ_B; ++e) Z[e] = 0.0;
    for (int j = 0; j < b; ++j) {
        theta[j] = H[order[j]][order[j]];
        for (int k = 0; k < b; ++k) Z[k * DZ_B + j] = Q[k][order[j]];
    }
}

#define DZ_TRY(expr)                   \
    do {                               \
        const int _rc = (expr);        \
        if (_rc != MV_OK) return _rc;  \
    } while (0)

struct EigRun {
    const float* M;
    const double* degree;
    int N, b;
    EigPlan p;
    char* ws;
    hipStream_t stream;
    int products = 0;

    double* block(int i) const { return reinterpret_cast<double*>(ws + p.off_block[i]); }
    double* part() const { return reinterpret_cast<double*>(ws + p.off_part); }
    double* gpart() const { return reinterpret_cast<double*>(ws + p.off_gpart); }
    double* small() const { return reinterpret_cast<double*>(ws + p.off_small); }
    double* upload() const { return reinterpret_cast<double*>(ws + p.off_upload); }
    unsigned elem_blocks() const { return (unsigned)ceil_div((int64_t)N * b, 256); }

    // out = alpha * (L X - shift X) - beta Z
    int product(const double* X, const double* Z, double alpha, double shift, double beta, double* out) {
        MV_LAUNCH(product_partial_kernel, ((unsigned)p.row_tiles, (unsigned)p.nslices, 1), (256, 1, 1), 0, stream, M, X, N, b, p.k_per_slice, part());
        DZ_TRY(check_launch("product_partial_kernel"));
        MV_LAUNCH(product_finish_kernel, (elem_blocks(), 1, 1), (256, 1, 1), 0, stream, (const double*)part(), p.nslices, X, degree, Z, alpha, shift,
                  beta, N, b, out);
        ++products;
        return check_launch("product_finish_kernel");
    }

    // host <- A^T B (b x b, ld 32); synchronises
    int gram(const double* A, const double* B, double* host) {
        MV_LAUNCH(gram_partial_kernel, ((unsigned)p.chunks, 1, 1), (256, 1, 1), 0, stream, A, B, N, b, gpart());
        DZ_TRY(check_launch("gram_partial_kernel"));
        MV_LAUNCH(sum_slices_kernel, (DZ_B * DZ_B / 256, 1, 1), (256, 1, 1), 0, stream, (const double*)gpart(), p.chunks, DZ_B * DZ_B, small());
        DZ_TRY(check_launch("sum_slices_kernel"));
        MV_HIP_OK(hipMemcpyAsync(host, small(), DZ_B * DZ_B * sizeof(double), hipMemcpyDeviceToHost, stream));
        MV_HIP_OK(hipStreamSynchronize(stream));
        return MV_OK;
    }

    // Out = A T, T (b x b, ld 32) from the host
    int rotate(const double* A, const double* T_host, double* Out) {
        MV_HIP_OK(hipMemcpyAsync(upload(), T_host, DZ_B * DZ_B * sizeof(double), hipMemcpyHostToDevice, stream));
        MV_HIP_OK(hipStreamSynchronize(stream));  // T_host may be reused by the caller right away
        MV_LAUNCH(rotate_kernel, (elem_blocks(), 1, 1), (256, 1, 1), 0, stream, A, (const double*)upload(), N, b, Out);
        return check_launch("rotate_kernel");
    }

    // Y -> orthonormal columns in Q through `tmp` (Cholesky-QR twice); *ok = false on a non-positive pivot
    int orthonormalise(const double* Y, double* tmp, double* Q, bool* ok) {
        double G[DZ_B * DZ_B], T[DZ_B * DZ_B];
        *ok = false;
        DZ_TRY(gram(Y, Y, G));
        if (!cholqr_factor(G, b, T)) return MV_OK;
        DZ_TRY(rotate(Y, T, tmp));
        DZ_TRY(gram(tmp, tmp, G));
        if (!cholqr_factor(G, b, T)) return MV_OK;
        DZ_TRY(rotate(tmp, T, Q));
        *ok = true;
        return MV_OK;
    }

    // Rayleigh-Ritz on the orthonormal Q: W = L Q, H = Q^T W, V = Q Z, LV = W Z; theta ascending; residual of the m wanted columns
    int rayleigh_ritz(const double* Q, double* W, double* V, double* LV, int m, double* theta, double* resid) {
        double H[DZ_B * DZ_B], Z[DZ_B * DZ_B], r[DZ_B];
        DZ_TRY(product(Q, nullptr, 1.0, 0.0, 0.0, W));
        DZ_TRY(gram(Q, W, H));
        jacobi_eig(H, b, theta, Z);
        DZ_TRY(rotate(Q, Z, V));
        DZ_TRY(rotate(W, Z, LV));
        MV_HIP_OK(hipMemcpyAsync(upload() + DZ_B * DZ_B, theta, b * sizeof(double), hipMemcpyHostToDevice, stream));
        MV_HIP_OK(hipStreamSynchronize(stream));
        MV_LAUNCH(resid_partial_kernel, ((unsigned)p.chunks, 1, 1), (256, 1, 1), 0, stream, (const double*)LV, (const double*)V,
                  (const double*)(upload() + DZ_B * DZ_B), N, b, gpart());
        DZ_TRY(check_launch("resid_partial_kernel"));
        MV_LAUNCH(sum_slices_kernel, (1, 1, 1), (256, 1, 1), 0, stream, (const double*)gpart(), p.chunks, DZ_B, small());
        DZ_TRY(check_launch("sum_slices_kernel"));
        MV_HIP_OK(hipMemcpyAsync(r, small(), DZ_B * sizeof(double), hipMemcpyDeviceToHost, stream));
        MV_HIP_OK(hipStreamSynchronize(stream));
        double worst = 0.0;
        for (int j = 0; j < m; ++j) worst = r[j] > worst || r[j] != r[j] ? r[j] : worst;
        *resid = sqrt(worst);
        return MV_OK;
    }
};

}  // namespace
}  // namespace mv

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int mv_wave_chunks_f32(const float* wav, int64_t L, const int64_t* start, const int64_t* len, int32_t n, int64_t chunk_len,
                                  int32_t normalize, float target_db, float max_gain_db, float* rows, int64_t rows_stride, int32_t* too_quiet,
                                  mv_stream_t stream) {
    MV_REQUIRE(n >= 0 && L >= 0 && chunk_len >= 0 && rows_stride >= chunk_len, "mv_wave_chunks_f32: bad geometry");
    if (n == 0 || chunk_len == 0) return MV_OK;
    MV_REQUIRE((wav != nullptr || L == 0) && start != nullptr && len != nullptr && rows != nullptr, "mv_wave_chunks_f32: null buffer");
    MV_LAUNCH(mv::wave_chunks_kernel, ((unsigned)n, 1, 1), (256, 1, 1), 0, static_cast<hipStream_t>(stream), wav, L, start, len, chunk_len,
              normalize, target_db, max_gain_db, rows, rows_stride, too_quiet);
    return mv::check_launch("wave_chunks_kernel");
}

extern "C" size_t mv_affinity_laplacian_workspace_bytes(int32_t N) {
    return N >= 1 && N <= mv::DZ_MAX_N ? (size_t)N * 2 * sizeof(uint32_t) : 0;
}

extern "C" int mv_affinity_laplacian_f32(const float* S, int32_t N, int32_t n_prune, float* M, double* degree, void* workspace,
                                         size_t workspace_bytes, mv_stream_t stream) {
    MV_REQUIRE(N >= 1 && N <= mv::DZ_MAX_N, "mv_affinity_laplacian_f32: N outside 1 .. 16384");
    MV_REQUIRE(n_prune >= 0 && n_prune < N, "mv_affinity_laplacian_f32: n_prune outside 0 .. N - 1");
    MV_REQUIRE(S != nullptr && M != nullptr && degree != nullptr && S != M, "mv_affinity_laplacian_f32: null or aliased buffer");
    MV_REQUIRE(workspace != nullptr, "mv_affinity_laplacian_f32: null workspace");
    if (workspace_bytes < mv_affinity_laplacian_workspace_bytes(N))
        return mv::fail(MV_ERR_WORKSPACE, "mv_affinity_laplacian_f32: workspace smaller than mv_affinity_laplacian_workspace_bytes(N)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* cut = static_cast<uint32_t*>(workspace);
    MV_LAUNCH(mv::prune_cut_kernel, ((unsigned)N, 1, 1), (256, 1, 1), 0, st, S, N, n_prune, cut);
    DZ_TRY(mv::check_launch("prune_cut_kernel"));
    const unsigned tiles = (unsigned)mv::ceil_div(N, 32);
    MV_LAUNCH(mv::affinity_sym_kernel, (tiles, tiles, 1), (256, 1, 1), 0, st, S, (const uint32_t*)cut, N, M);
    DZ_TRY(mv::check_launch("affinity_sym_kernel"));
    MV_LAUNCH(mv::degree_kernel, ((unsigned)N, 1, 1), (256, 1, 1), 0, st, (const float*)M, N, degree);
    return mv::check_launch("degree_kernel");
}

extern "C" void mv_laplacian_eig_default_cfg(MvEigCfg* cfg) {
    if (cfg == nullptr) return;
    cfg->m = 16;
    cfg->block = 0;
    cfg->degree = 16;
    cfg->max_iters = 60;
    cfg->tol = 1e-6;
    cfg->seed = 0x6d76656967ull;
}

extern "C" size_t mv_laplacian_eig_lowest_workspace_bytes(int32_t N, const MvEigCfg* cfg) {
    int b = 0;
    if (mv::eig_check(N, cfg, &b) != MV_OK) return 0;
    return mv::eig_plan(N, b).total;
}

extern "C" int mv_laplacian_eig_lowest(const float* M, const double* degree, int32_t N, const MvEigCfg* cfg, double* lambdas, double* vecs,
                                       MvEigInfo* info, void* workspace, size_t workspace_bytes, mv_stream_t stream) {
    using namespace mv;
    int b = 0;
    DZ_TRY(eig_check(N, cfg, &b));
    MV_REQUIRE(M != nullptr && degree != nullptr && lambdas != nullptr && vecs != nullptr, "mv_laplacian_eig_lowest: null buffer");
    MV_REQUIRE(workspace != nullptr, "mv_laplacian_eig_lowest: null workspace");
    EigRun run;
    run.M = M, run.degree = degree, run.N = N, run.b = b;
    run.p = eig_plan(N, b);
    if (workspace_bytes < run.p.total)
        return fail(MV_ERR_WORKSPACE, "mv_laplacian_eig_lowest: workspace smaller than mv_laplacian_eig_lowest_workspace_bytes(N, cfg)");
    MV_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "mv_laplacian_eig_lowest: workspace not 16-byte aligned");
    run.ws = static_cast<char*>(workspace);
    run.stream = static_cast<hipStream_t>(stream);
    const int m = cfg->m;
    MvEigInfo out = {0, 0, 0, 0, 0.0, 0.0};

    // Gershgorin: every eigenvalue of L lies in [0, 2 max degree]
    std::vector<double> deg_host((size_t)N);
    MV_HIP_OK(hipMemcpyAsync(deg_host.data(), degree, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, run.stream));
    MV_HIP_OK(hipStreamSynchronize(run.stream));
    double ub = 0.0;
    for (int i = 0; i < N; ++i) {
        MV_REQUIRE(deg_host[i] >= 0.0 && std::isfinite(deg_host[i]), "mv_laplacian_eig_lowest: a degree is negative or not finite");
        ub = deg_host[i] > ub ? deg_host[i] : ub;
    }
    ub *= 2.0;
    out.ub = ub;

    double *V = run.block(0), *LV = run.block(1), *A = run.block(2), *B = run.block(3), *C = run.block(4);
    double theta[DZ_B];
    double resid = 0.0;
    bool ok = false;
    MV_LAUNCH(eig_init_kernel, (run.elem_blocks(), 1, 1), (256, 1, 1), 0, run.stream, A, (int64_t)N * b, (uint64_t)cfg->seed);
    DZ_TRY(check_launch("eig_init_kernel"));
    DZ_TRY(run.orthonormalise(A, B, C, &ok));
    if (!ok) return fail(MV_ERR_INVALID_ARGUMENT, "mv_laplacian_eig_lowest: the start block is rank deficient");
    DZ_TRY(run.rayleigh_ritz(C, A, V, LV, m, theta, &resid));  // V, LV = block 0, 1; A, B, C free again

    while (!(resid <= cfg->tol * ub) && out.iterations < cfg->max_iters) {
        ++out.iterations;
        double* Q = nullptr;
        for (int degree_now = cfg->degree;; degree_now = degree_now / 2) {
            // scaled Chebyshev filter that damps [a, ub] and grows fastest at a0 (Zhou & Saad 2007)
            const double a0 = theta[0], a = theta[b - 1] < ub ? theta[b - 1] : ub;
            const double e = 0.5 * (ub - a), c = 0.5 * (ub + a);
            if (!(e > 0.0) || !(a0 < c)) break;  // the block already spans everything below ub: nothing to filter
            double sigma = e / (a0 - c);
            const double tau = 2.0 / sigma;
            double *prev = V, *cur = A, *next = B, *spare = C;
            DZ_TRY(run.product(V, nullptr, sigma / e, c, 0.0, cur));
            for (int i = 2; i <= degree_now; ++i) {
                const double sigma2 = 1.0 / (tau - sigma);
                DZ_TRY(run.product(cur, prev, 2.0 * sigma2 / e, c, sigma * sigma2, next));
                sigma = sigma2;
                double* freed = prev == V ? spare : prev;  // V itself stays: a retry starts from it again
                prev = cur, cur = next, next = freed;
            }
            // two of A, B, C besides `cur` are free for the orthonormalisation
            double* t1 = cur == A ? B : A;
            double* t2 = (cur == C || t1 == C) ? (cur == B || t1 == B ? A : B) : C;
            DZ_TRY(run.orthonormalise(cur, t1, t2, &ok));
            if (ok) {
                Q = t2;
                break;
            }
            ++out.retries;  // non-positive pivot: the filter outran fp64, repeat this iteration with half the degree
            if (degree_now <= 1) break;
        }
        if (Q == nullptr) break;
        double* W = Q == A ? B : A;
        double* LV2 = (Q == C || W == C) ? (Q == B || W == B ? A : B) : C;
        DZ_TRY(run.rayleigh_ritz(Q, W, V, LV2, m, theta, &resid));
        // the rotated L V now lives in one of A, B, C; block 1 is not read again
    }

    out.products = run.products;
    out.residual = resid;
    out.converged = resid <= cfg->tol * ub ? 1 : 0;
    if (info != nullptr) *info = out;
    for (int j = 0; j < m; ++j) lambdas[j] = theta[j];
    MV_LAUNCH(take_cols_kernel, ((unsigned)ceil_div((int64_t)N * m, 256), 1, 1), (256, 1, 1), 0, run.stream, (const double*)V, N, b, m, vecs);
    DZ_TRY(check_launch("take_cols_kernel"));
    MV_HIP_OK(hipStreamSynchronize(run.stream));
    if (!out.converged) {
        char msg[160];
        snprintf(msg, sizeof msg, "mv_laplacian_eig_lowest: residual %.3e above tol * ub = %.3e after %d iterations", resid, cfg->tol * ub,
                 out.iterations);
        return fail(MV_ERR_NOT_CONVERGED, msg);
    }
    return MV_OK;
}
