// Mahalanobis OOD scores over a latent bank (Lee et al. 2018; the relative form of Ren et al. 2021): the
// moments of the bank - class counts and means, the overall mean, the within-class and the total scatter matrix - in fp64, and the
// scores of query rows against the fitted Gaussians, whitening fused with the distances in ONE launch.
//
// Moments.  maha_rows_kernel gives every row its class, or -1 where the label is outside [0, C) (MAHA_STATUS_LABEL) or an element
// is not finite (MAHA_STATUS_BANK): such a row is in no sum.  Every sum is fp64 in a fixed order: the rows of a slab are dealt to
// the 256 threads of a workgroup in strides (a thread adds its rows ascending), the 64 partials of a wave meet in a butterfly,
// the four waves are added in sequence, and a fold kernel adds the slabs ascending.  The split into slabs hangs on M alone.  ONE
// column-sum kernel gives the class means (rows taken by their class) and the overall mean (every row in class 0), ONE scatter
// kernel both matrices: it reads the mean of a row through its class.  A workgroup of the scatter kernel owns an 8 x 8 tile of
// the matrix, a thread the 64 products of its rows; the tiles below the diagonal are not computed, the fold mirrors them (the
// matrices are symmetric to the bit).  No floating-point atomics; the counts and the status word take integer ones.
//
// Scores.  A workgroup is ONE wave and owns 32 query rows.  x = q - mu0 and a tile of the stacked matrix (W over W0, 32 of its
// rows) pass through LDS in chunks of 64 columns; y = W x is a chain of v_mfma_f32_32x32x2_f32 steps over j ascending (zero padded
// to the step), bit for bit the fmaf chain, with the row of W in the accumulator register and the query row on the lane.  The 32
// values y_k of a tile go through LDS once, so that a lane holds all 32 of ITS query row, and are folded at once into the running
// sums d_c += (y_k - m_ck)^2 (W's tiles: 32 x C sums in LDS, a lane takes every second class) or d0 += (y_k - m0_k)^2 (W0's tiles,
// in a register), fmaf chains over k ascending.  m0 = W0 (mean0 - mu0) is the whitened rounding error of mu0, the counterpart of
// a class mean: without it the rounding of mu0 does not cancel in d0 as it does in every d_c.  Neither y (N, 2K) nor d (N, C) is
// written to memory.  The classes are the non-empty ones in ascending label order (cmap: their labels), so `<` keeps the lower
// label of a tie.
#include "common.h"
#include "jvae_hip.h"
#include <math.h>

#define MAHA_MAX_K 256
#define MAHA_MAX_C 128         // = MISCLASS_MAX_CLASSES
#define MAHA_STATUS_LABEL 1
#define MAHA_STATUS_BANK 2
#define MAHA_STATUS_QUERY 4
#define MAHA_BLOCK 256
#define MAHA_SLAB_ROWS 2048    // rows of a slab (eight per thread) until MAHA_MAX_SLABS is reached
#define MAHA_MAX_SLABS 32
#define MAHA_CT 16             // columns of a column-sum workgroup
#define MAHA_T 8               // edge of a scatter tile
#define MAHA_QT 32             // query rows of a workgroup
#define MAHA_JC 64             // columns of a staged chunk
#define MAHA_LD 33             // LDS stride of a staged column: 32 rows + 1, conflict-free both ways

static int maha_slabs(long M) {
    const long s = (M + MAHA_SLAB_ROWS - 1) / MAHA_SLAB_ROWS;
    return s < 1 ? 1 : (s > MAHA_MAX_SLABS ? MAHA_MAX_SLABS : (int)s);
}

struct MahaRange { long nb, ne; };
__device__ __forceinline__ MahaRange maha_range(long M, int slabs, int s) {
    const long per = (M + slabs - 1) / slabs, b = (long)s * per, e = b + per;
    MahaRange r;
    r.nb = b < M ? b : M;
    r.ne = e < M ? e : M;
    return r;
}

__global__ __launch_bounds__(MAHA_BLOCK) void maha_rows_kernel(const float* __restrict__ bank, const long long* __restrict__ labels,
                                                               int* __restrict__ rowcls, long M, int K, int C, int* status) {
    const long r = (long)blockIdx.x * MAHA_BLOCK + threadIdx.x;
    if (r >= M) return;
    const long long lab = labels[r];
    int flags = (lab < 0 || lab >= C) ? MAHA_STATUS_LABEL : 0;
    const float* p = bank + r * K;
    bool finite = true;
    for (int k = 0; k < K; ++k) finite &= fabsf(p[k]) < INFINITY;
    if (!finite) flags |= MAHA_STATUS_BANK;
    rowcls[r] = flags ? -1 : (int)lab;
    if (flags) atomicOr(status, flags);
}

// part[(s, c, k)] = the sum over the rows of slab s in class c (by_label = 0: over all its rows, c = 0) of column k; cnt[c] += rows
__global__ __launch_bounds__(MAHA_BLOCK) void maha_colsum_kernel(const float* __restrict__ bank, const int* __restrict__ rowcls,
                                                                 int by_label, double* __restrict__ part,
                                                                 unsigned long long* __restrict__ cnt, long M, int K, int slabs) {
    __shared__ double red[MAHA_BLOCK / 64][MAHA_CT];
    __shared__ int nred[MAHA_BLOCK / 64];
    const int k0 = blockIdx.x * MAHA_CT, c = blockIdx.y, s = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const MahaRange rg = maha_range(M, slabs, s);
    double acc[MAHA_CT];
#pragma unroll
    for (int j = 0; j < MAHA_CT; ++j) acc[j] = 0.;
    int n = 0;
    for (long r = rg.nb + threadIdx.x; r < rg.ne; r += MAHA_BLOCK) {
        const int cls = rowcls[r];
        if (cls < 0 || (by_label && cls != c)) continue;
        const float* p = bank + r * K + k0;
#pragma unroll
        for (int j = 0; j < MAHA_CT; ++j)
            if (k0 + j < K) acc[j] += (double)p[j];
        ++n;
    }
#pragma unroll
    for (int j = 0; j < MAHA_CT; ++j) acc[j] = wave_sum64(acc[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < MAHA_CT; ++j) red[wave][j] = acc[j];
        nred[wave] = n;
    }
    __syncthreads();
    if (threadIdx.x < MAHA_CT && k0 + threadIdx.x < K) {
        double t = red[0][threadIdx.x];
        for (int w = 1; w < MAHA_BLOCK / 64; ++w) t += red[w][threadIdx.x];
        part[((size_t)s * gridDim.y + c) * K + k0 + threadIdx.x] = t;
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < MAHA_BLOCK / 64; ++w) t += nred[w];
        if (t) atomicAdd(cnt + c, (unsigned long long)t);
    }
}

// mean[(c, k)] = the slabs' sums added ascending / cnt[c]; an empty class gets zeros
__global__ __launch_bounds__(MAHA_BLOCK) void maha_mean_fold_kernel(const double* __restrict__ part,
                                                                    const unsigned long long* __restrict__ cnt,
                                                                    double* __restrict__ mean, int C, int K, int slabs) {
    const int e = blockIdx.x * MAHA_BLOCK + threadIdx.x;
    if (e >= C * K) return;
    double acc = 0.;
    for (int s = 0; s < slabs; ++s) acc += part[(size_t)s * C * K + e];
    const unsigned long long n = cnt[e / K];
    mean[e] = n ? acc / (double)n : 0.;
}

// part[(s, i, j)] = the sum over the rows b of slab s of (b_i - mean[cls][i]) (b_j - mean[cls][j]), for the tiles on and above
// the diagonal; by_label = 0: cls = 0 for every row
__global__ __launch_bounds__(MAHA_BLOCK) void maha_scatter_kernel(const float* __restrict__ bank, const int* __restrict__ rowcls,
                                                                  int by_label, const double* __restrict__ means,
                                                                  double* __restrict__ part, long M, int K, int slabs) {
    if (blockIdx.x < blockIdx.y) return;               // mirrored by the fold
    __shared__ double red[MAHA_BLOCK / 64][MAHA_T * MAHA_T];
    const int i0 = blockIdx.y * MAHA_T, j0 = blockIdx.x * MAHA_T, s = blockIdx.z, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const MahaRange rg = maha_range(M, slabs, s);
    double acc[MAHA_T][MAHA_T];
#pragma unroll
    for (int a = 0; a < MAHA_T; ++a)
#pragma unroll
        for (int b = 0; b < MAHA_T; ++b) acc[a][b] = 0.;
    for (long r = rg.nb + threadIdx.x; r < rg.ne; r += MAHA_BLOCK) {
        const int cls = rowcls[r];
        if (cls < 0) continue;
        const float* p = bank + r * K;
        const double* mp = means + (size_t)(by_label ? cls : 0) * K;
        double xa[MAHA_T], xb[MAHA_T];
#pragma unroll
        for (int t = 0; t < MAHA_T; ++t) {
            xa[t] = i0 + t < K ? (double)p[i0 + t] - mp[i0 + t] : 0.;
            xb[t] = j0 + t < K ? (double)p[j0 + t] - mp[j0 + t] : 0.;
        }
#pragma unroll
        for (int a = 0; a < MAHA_T; ++a)
#pragma unroll
            for (int b = 0; b < MAHA_T; ++b) acc[a][b] = fma(xa[a], xb[b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < MAHA_T; ++a)
#pragma unroll
        for (int b = 0; b < MAHA_T; ++b) {
            const double t = wave_sum64(acc[a][b]);
            if (lane == 0) red[wave][a * MAHA_T + b] = t;
        }
    __syncthreads();
    if (threadIdx.x < MAHA_T * MAHA_T) {
        const int i = i0 + threadIdx.x / MAHA_T, j = j0 + threadIdx.x % MAHA_T;
        double t = red[0][threadIdx.x];
        for (int w = 1; w < MAHA_BLOCK / 64; ++w) t += red[w][threadIdx.x];
        if (i < K && j < K) part[((size_t)s * K + i) * K + j] = t;
    }
}

// out[(i, j)] = the slabs' sums added ascending / *n; an entry of a tile below the diagonal is read from its mirror image
__global__ __launch_bounds__(MAHA_BLOCK) void maha_scatter_fold_kernel(const double* __restrict__ part,
                                                                       const unsigned long long* __restrict__ n,
                                                                       double* __restrict__ out, int K, int slabs) {
    const int e = blockIdx.x * MAHA_BLOCK + threadIdx.x;
    if (e >= K * K) return;
    const int i = e / K, j = e % K;
    const size_t src = j / MAHA_T < i / MAHA_T ? (size_t)j * K + i : (size_t)i * K + j;
    double acc = 0.;
    for (int s = 0; s < slabs; ++s) acc += part[(size_t)s * K * K + src];
    out[e] = acc / (double)*n;
}

__global__ __launch_bounds__(64) void maha_scores_kernel(const float* __restrict__ q, const float* __restrict__ mu0,
                                                         const float* __restrict__ W, const float* __restrict__ m,
                                                         const float* __restrict__ m0, const int* __restrict__ cmap, float* __restrict__ d_out,
                                                         int* __restrict__ cls_out, float* __restrict__ rel_out,
                                                         float* __restrict__ pc, long N, int K, int Cn, int C, int* status) {
    __shared__ float s_x[MAHA_JC * MAHA_LD];           // x chunk: column jj of query row r at jj * LD + r
    __shared__ float s_w[MAHA_JC * MAHA_LD];           // chunk of a tile of the stacked matrix, the same way
    __shared__ float s_y[32 * MAHA_LD];                // y of a tile: output kk of query row r at kk * LD + r
    __shared__ __attribute__((aligned(16))) float s_m[MAHA_MAX_C * 32];      // the tile's columns of the class means
    __shared__ float s_d[MAHA_MAX_C * 32];             // running d_c of query row r at c * 32 + r
    __shared__ int s_inv[MAHA_MAX_C];                  // label -> its place among the non-empty classes, or -1
    __shared__ int s_bad[MAHA_QT];
    const int lane = threadIdx.x, h = lane >> 5, c = lane & 31;
    const long q0 = (long)blockIdx.x * MAHA_QT;
    const int nt = (K + 31) >> 5, nch = (K + MAHA_JC - 1) / MAHA_JC;

    for (int i = lane; i < Cn * 32; i += 64) s_d[i] = 0.f;
    for (int i = lane; i < C; i += 64) s_inv[i] = -1;
    if (lane < MAHA_QT) s_bad[lane] = 0;
    __syncthreads();
    for (int i = lane; i < Cn; i += 64) {
        const int label = cmap[i];
        if (label >= 0 && label < C) s_inv[label] = i;
    }
    float d0 = 0.f;

    for (int tile = 0; tile < 2 * nt; ++tile) {
        const int hf = tile >= nt, k0 = (tile - hf * nt) * 32;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        for (int ch = 0; ch < nch; ++ch) {
            const int j0 = ch * MAHA_JC, col = j0 + lane, jn = K - j0 < MAHA_JC ? K - j0 : MAHA_JC;
            const bool cin = col < K;
            __syncthreads();
            if (nch > 1 || tile == 0) {                // K <= 64: x stays resident
                const float mu = cin ? mu0[col] : 0.f;
                for (int rb = 0; rb < MAHA_QT; rb += 8) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const long row = q0 + rb + j;
                        v[j] = (row < N && cin) ? q[row * K + col] : mu;
                    }
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (!(fabsf(v[j]) < INFINITY)) s_bad[rb + j] = 1;
                        s_x[lane * MAHA_LD + rb + j] = v[j] - mu;
                    }
                }
            }
            for (int rb = 0; rb < 32; rb += 8) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = k0 + rb + j;
                    v[j] = (k < K && cin) ? W[((size_t)hf * K + k) * K + col] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) s_w[lane * MAHA_LD + rb + j] = v[j];
            }
            __syncthreads();
            const int ns = (jn + 1) >> 1;              // an odd K: the last step's second column is a staged zero
            for (int s = 0; s < ns; ++s) {
                const int o = (2 * s + h) * MAHA_LD + c;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(s_w[o], s_x[o], acc, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s_y[((r & 3) + 8 * (r >> 2) + 4 * h) * MAHA_LD + c] = acc[r];
        if (!hf) {
            for (int i = lane; i < Cn * 32; i += 64) {
                const int k = k0 + (i & 31);
                s_m[i] = k < K ? m[(size_t)(i >> 5) * K + k] : 0.f;
            }
        } else if (lane < 32) {
            s_m[lane] = k0 + lane < K ? m0[k0 + lane] : 0.f;
        }
        __syncthreads();
        float yv[32];
#pragma unroll
        for (int kk = 0; kk < 32; ++kk) yv[kk] = s_y[kk * MAHA_LD + c];
        // the rows of the tile past K are zeros in W and in m: fmaf(0, 0, s) = s
        if (!hf) {
            for (int cc = h; cc < Cn; cc += 2) {
                float s = s_d[cc * 32 + c];
                const float* mp = s_m + cc * 32;
#pragma unroll
                for (int kk = 0; kk < 32; kk += 4) {
                    const f32x4 m4 = *reinterpret_cast<const f32x4*>(mp + kk);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float t = yv[kk + j] - m4[j];
                        s = fmaf(t, t, s);
                    }
                }
                s_d[cc * 32 + c] = s;
            }
        } else {
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) {
                const float t = yv[kk] - s_m[kk];
                d0 = fmaf(t, t, d0);
            }
        }
    }
    __syncthreads();
    const long row = q0 + c;
    if (row >= N) return;
    const bool bad = s_bad[c] != 0;
    if (h == 0) {
        float best = INFINITY;
        int bi = -1;
        for (int cc = 0; cc < Cn; ++cc) {
            const float v = s_d[cc * 32 + c];
            if (v < best || bi < 0) {
                best = v;
                bi = cc;
            }
        }
        d_out[row] = bad ? NAN : best;
        rel_out[row] = bad ? NAN : best - d0;          // min_c (d_c - d0): rounding is monotone
        cls_out[row] = bad ? -1 : cmap[bi];
        if (bad) atomicOr(status, MAHA_STATUS_QUERY);
    }
    if (pc)
        for (int cf = h; cf < C; cf += 2) {
            const int cc = s_inv[cf];
            pc[row * C + cf] = bad ? NAN : (cc < 0 ? INFINITY : s_d[cc * 32 + c]);
        }
}

struct MahaWs { size_t rowcls, cnt0, colsum, scatter, total; };
static MahaWs maha_ws(long M, int K, int C) {
    const size_t S = (size_t)maha_slabs(M);
    MahaWs w;
    w.rowcls = 0;
    w.cnt0 = ((size_t)M * sizeof(int) + 7) & ~(size_t)7;
    w.colsum = w.cnt0 + 8;
    w.scatter = w.colsum + S * C * K * sizeof(double);
    w.total = w.scatter + S * K * K * sizeof(double);
    return w;
}

static int maha_check_moments(long M, int K, int C) {
    if (M < 1 || K < 1 || C < 1) return JVAE_EINVAL;
    if (K > MAHA_MAX_K || C > MAHA_MAX_C || M >= (1L << 31)) return JVAE_ENOTSUP;
    return 0;
}

extern "C" size_t jvae_maha_moments_workspace_bytes(long M, int K, int C) {
    if (maha_check_moments(M, K, C)) return 0;
    return maha_ws(M, K, C).total;
}

extern "C" int jvae_maha_moments_f32(const float* bank, const long long* labels, long M, int K, int C, long long* counts,
                                     double* means, double* mean0, double* Sw, double* St, int* status, void* ws,
                                     size_t ws_bytes, void* stream) {
    const int rc = maha_check_moments(M, K, C);
    if (rc) return rc;
    if (!bank || !labels || !counts || !means || !mean0 || !Sw || !St || !status || !ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    const MahaWs w = maha_ws(M, K, C);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int S = maha_slabs(M);
    int* rowcls = (int*)((char*)ws + w.rowcls);
    unsigned long long* cnt0 = (unsigned long long*)((char*)ws + w.cnt0);
    unsigned long long* cnt = (unsigned long long*)counts;
    double* colsum = (double*)((char*)ws + w.colsum);
    double* scatter = (double*)((char*)ws + w.scatter);
    hipError_t e = hipMemsetAsync(cnt, 0, (size_t)C * sizeof(long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(cnt0, 0, sizeof(long long), st);
    if (e != hipSuccess) return (int)e;
    const unsigned kc = (unsigned)cdiv(K, MAHA_CT), kt = (unsigned)cdiv(K, MAHA_T), kk = (unsigned)cdiv((long)K * K, MAHA_BLOCK);
    maha_rows_kernel<<<cdiv(M, MAHA_BLOCK), MAHA_BLOCK, 0, st>>>(bank, labels, rowcls, M, K, C, status);
    JVAE_LAUNCH_CHECK();
    maha_colsum_kernel<<<dim3(kc, (unsigned)C, (unsigned)S), MAHA_BLOCK, 0, st>>>(bank, rowcls, 1, colsum, cnt, M, K, S);
    JVAE_LAUNCH_CHECK();
    maha_mean_fold_kernel<<<cdiv((long)C * K, MAHA_BLOCK), MAHA_BLOCK, 0, st>>>(colsum, cnt, means, C, K, S);
    JVAE_LAUNCH_CHECK();
    maha_colsum_kernel<<<dim3(kc, 1, (unsigned)S), MAHA_BLOCK, 0, st>>>(bank, rowcls, 0, colsum, cnt0, M, K, S);
    JVAE_LAUNCH_CHECK();
    maha_mean_fold_kernel<<<cdiv(K, MAHA_BLOCK), MAHA_BLOCK, 0, st>>>(colsum, cnt0, mean0, 1, K, S);
    JVAE_LAUNCH_CHECK();
    maha_scatter_kernel<<<dim3(kt, kt, (unsigned)S), MAHA_BLOCK, 0, st>>>(bank, rowcls, 1, means, scatter, M, K, S);
    JVAE_LAUNCH_CHECK();
    maha_scatter_fold_kernel<<<kk, MAHA_BLOCK, 0, st>>>(scatter, cnt0, Sw, K, S);
    JVAE_LAUNCH_CHECK();
    maha_scatter_kernel<<<dim3(kt, kt, (unsigned)S), MAHA_BLOCK, 0, st>>>(bank, rowcls, 0, mean0, scatter, M, K, S);
    JVAE_LAUNCH_CHECK();
    maha_scatter_fold_kernel<<<kk, MAHA_BLOCK, 0, st>>>(scatter, cnt0, St, K, S);
    JVAE_LAUNCH_CHECK();
    return 0;
}

extern "C" int jvae_maha_scores_f32(const float* q, const float* mu0, const float* W, const float* m, const float* m0,
                                    const int* cmap, float* d, int* cls, float* rel, float* per_class, long N, int K, int Cn, int C,
                                    int* status, void* stream) {
    if (N < 0 || K < 1 || Cn < 1 || C < Cn) return JVAE_EINVAL;
    if (K > MAHA_MAX_K || C > MAHA_MAX_C || N >= (1L << 31)) return JVAE_ENOTSUP;
    if (N == 0) return 0;
    if (!q || !mu0 || !W || !m || !m0 || !cmap || !d || !cls || !rel || !status) return JVAE_EINVAL;
    maha_scores_kernel<<<cdiv(N, MAHA_QT), 64, 0, (hipStream_t)stream>>>(q, mu0, W, m, m0, cmap, d, cls, rel, per_class, N, K, Cn,
                                                                         C, status);
    JVAE_LAUNCH_CHECK();
    return 0;
}
