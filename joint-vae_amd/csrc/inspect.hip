// Latent-space inspection (reference module/sample.py::zsample, ft/inspection.py, utils/inspection.py): three kernels.
//
// 1. Per-group moments of the posterior.  mu, log_var (N, K), group (N,) ->
//      sums[g, 0..3, k] += sum over the samples of group g of mu, mu^2, v, v^2,  v = exp(log_var) taken in fp32 and widened;
//      counts[g] += the size of group g.
//    Rows are cut into slabs of IM_SLAB = 256 consecutive samples, columns into blocks of 64, groups into chunks of IM_GC = 4.  A
//    workgroup owns one (column block, group chunk, slab): a lane is a column, the four waves deal the slab's rows round-robin, and
//    every (wave, group, statistic, lane) has ONE fp64 cell in LDS that only its own lane ever touches.  A row outside the chunk adds
//    0 to the chunk's first cell instead of branching, so the loads of consecutive rows overlap.  The four waves are folded as
//    (w0 + w1) + (w2 + w3) into one partial per (slab, g, statistic, k); the second kernel adds the slabs in ascending order onto the
//    caller's accumulator.  No floating-point atomics: the order of every sum hangs on N alone, never on the number of CUs.  The
//    group sizes are exact counts, added with integer atomics by the workgroups of column block 0.
// 2. Nearest centroid.  mu (N, K), centroids (C, K) -> y_nearest (N,) = argmin_c |mu_n - m_c|^2 and d2 (N,), the winner's
//    squared distance.  A workgroup owns a sample, its four waves deal the centroids round-robin, the lanes of a wave walk k;
//    differences, squares and sums in fp64 (the fp32 operands are exact in it), the 64 lanes folded by a butterfly, one
//    rounding on the way out.  The comparison is made on the fp64 sums; ties go to the lowest index, a NaN distance wins over
//    every number (the lowest such index), as torch.argmin has it.
// 3. Histogram.  values (n,) fp32, edges (B + 1,) fp64 ascending, group (n,) or none -> counts[g, b] += the number of values of
//    group g with edges[b] <= x < edges[b + 1] (the last bin closed on the right); values outside [edges[0], edges[B]] and
//    non-finite ones are not counted, the number of the latter is added to *nonfinite.  The bin comes from a bisection of the
//    edges in fp64, so it is the comparison rule itself and not an arithmetic guess at it.  Where B <= 4096 and G B <= 4096 the
//    edges and a private set of 32-bit counters live in LDS and a workgroup adds its non-zero counters to the caller's with one
//    64-bit integer atomic each; beyond that the counters are the caller's own, updated by integer atomics.  Exact counts either way.
#include "common.h"
#include "jvae_internal.h"
#include <math.h>

// every product and sum below is rounded on its own unless written as fma
#pragma clang fp contract(off)

namespace {

constexpr int IM_BLOCK = 256;
constexpr int IM_WAVES = IM_BLOCK / 64;
constexpr int IM_SLAB = 256;                      // rows of a workgroup: fixed, so that the order of a sum hangs on N alone
constexpr int IM_GC = 4;                          // groups of a workgroup
constexpr int IM_STATS = 4;
constexpr int IM_MAX_K = 1 << 16;
constexpr int IM_MAX_G = 1 << 16;
constexpr long IM_MAX_N = 1L << 24;

__global__ __launch_bounds__(IM_BLOCK) void moments_kernel(const float* __restrict__ mu, const float* __restrict__ log_var,
                                                           const int* __restrict__ group, double* __restrict__ part,
                                                           unsigned long long* __restrict__ counts, int N, int K, int G) {
    __shared__ double acc[IM_WAVES][IM_GC][IM_STATS][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int g0 = blockIdx.y * IM_GC;
    const int n0 = blockIdx.z * IM_SLAB;
    const int n1 = min(n0 + IM_SLAB, N);
#pragma unroll
    for (int g = 0; g < IM_GC; ++g)
#pragma unroll
        for (int s = 0; s < IM_STATS; ++s) acc[w][g][s][lane] = 0.;
    if (blockIdx.x == 0) {                                         // the group sizes: one row per thread, exact
        const int n = n0 + (int)threadIdx.x;
        if (n < n1) {
            const int g = group ? group[n] : 0;
            if (g >= g0 && g < g0 + IM_GC && g < G) atomicAdd(&counts[g], 1ULL);
        }
    }
    const bool col = k < K;
#pragma unroll 4
    for (int n = n0 + w; n < n1; n += IM_WAVES) {
        const int g = group ? group[n] : 0;                        // the same for every lane of the wave
        const bool in = g >= g0 && g < g0 + IM_GC && g < G;
        const int slot = in ? g - g0 : 0;
        float m = 0.f, v = 0.f;
        if (col) {
            m = mu[(size_t)n * K + k];
            v = expf(log_var[(size_t)n * K + k]);
        }
        const double md = in ? (double)m : 0., vd = in ? (double)v : 0.;
        acc[w][slot][0][lane] += md;
        acc[w][slot][1][lane] += md * md;
        acc[w][slot][2][lane] += vd;
        acc[w][slot][3][lane] += vd * vd;
    }
    __syncthreads();
    // (w0 + w1) + (w2 + w3): thread t folds cell t of the chunk's IM_GC x IM_STATS x 64 = 1024 cells, then t + 256, ...
    for (int c = threadIdx.x; c < IM_GC * IM_STATS * 64; c += IM_BLOCK) {
        const int l = c & 63, s = (c >> 6) % IM_STATS, g = c / (64 * IM_STATS);
        const int kk = blockIdx.x * 64 + l;
        if (kk < K && g0 + g < G)
            part[(((size_t)blockIdx.z * G + (g0 + g)) * IM_STATS + s) * K + kk] =
                (acc[0][g][s][l] + acc[1][g][s][l]) + (acc[2][g][s][l] + acc[3][g][s][l]);
    }
}

__global__ __launch_bounds__(IM_BLOCK) void moments_fold_kernel(const double* __restrict__ part, double* __restrict__ sums, int slabs,
                                                                long cells) {
    const long i = (long)blockIdx.x * IM_BLOCK + threadIdx.x;
    if (i >= cells) return;
    double s = 0.;
    for (int b = 0; b < slabs; ++b) s += part[(size_t)b * cells + i];
    sums[i] += s;
}

// --------------------------------------------------------------------------------------------------- 2. nearest centroid
struct Best { double d; int i; };

// a before b: a NaN first (torch.argmin), then the smaller distance, then the lower index
__device__ __forceinline__ bool best_before(const Best& a, const Best& b) {
    const bool an = a.d != a.d, bn = b.d != b.d;
    if (an || bn) return an && (!bn || a.i < b.i);
    return a.d < b.d || (a.d == b.d && a.i < b.i);
}

__global__ __launch_bounds__(IM_BLOCK) void nearest_kernel(const float* __restrict__ mu, const float* __restrict__ cent,
                                                           long long* __restrict__ y, float* __restrict__ d2, int C, int K) {
    __shared__ Best red[IM_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* __restrict__ row = mu + (size_t)blockIdx.x * K;
    Best best{INFINITY, 0x7fffffff};                               // no centroid yet: every real one comes before it
    for (int c = w; c < C; c += IM_WAVES) {
        const float* __restrict__ m = cent + (size_t)c * K;
        double s = 0.;
        for (int k = lane; k < K; k += 64) {
            const double df = (double)row[k] - (double)m[k];
            s = fma(df, df, s);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const Best cand{s, c};
        if (best_before(cand, best)) best = cand;
    }
    if (lane == 0) red[w] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        Best b = red[0];
#pragma unroll
        for (int i = 1; i < IM_WAVES; ++i)
            if (best_before(red[i], b)) b = red[i];
        y[blockIdx.x] = b.i;
        d2[blockIdx.x] = (float)b.d;
    }
}

// ------------------------------------------------------------------------------------------------------------ 3. histogram
constexpr int IH_LDS_BINS = 4096;                  // edges of the LDS path (B + 1 doubles) and its counters (G B words)
constexpr int IH_PER_THREAD = 16;
constexpr int IH_MAX_GROUPS_BLOCKS = 1024;
constexpr long IH_MAX_CELLS = 1L << 26;

// bin of x: edges[b] <= x < edges[b + 1], the last bin closed on the right; -1 outside [edges[0], edges[B]], -2 non-finite.
// The bisection keeps 0 <= lo < hi <= B whatever the edges hold: the result is a valid index even for edges that do not ascend.
template <class E>
__device__ __forceinline__ int bin_of(float xf, const E* edges, int B) {
    if (!(fabsf(xf) <= 3.402823466e+38f)) return -2;                // NaN, +-inf
    const double x = (double)xf;
    if (!(x >= edges[0] && x <= edges[B])) return -1;
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (x >= edges[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

template <bool LDS>
__global__ __launch_bounds__(IM_BLOCK) void histogram_kernel(const float* __restrict__ values, const double* __restrict__ edges,
                                                             const int* __restrict__ group, unsigned long long* __restrict__ counts,
                                                             unsigned long long* __restrict__ nonfinite, long n, int B, int G) {
    __shared__ double e_lds[LDS ? IH_LDS_BINS + 1 : 1];
    __shared__ unsigned int c_lds[LDS ? IH_LDS_BINS : 1];
    const int cells = G * B;                                         // LDS path: <= IH_LDS_BINS
    if constexpr (LDS) {
        for (int i = threadIdx.x; i <= B; i += IM_BLOCK) e_lds[i] = edges[i];
        for (int i = threadIdx.x; i < cells; i += IM_BLOCK) c_lds[i] = 0u;
        __syncthreads();
    }
    unsigned int bad = 0;
    const long stride = (long)gridDim.x * IM_BLOCK;
    for (long i = (long)blockIdx.x * IM_BLOCK + threadIdx.x; i < n; i += stride) {
        const int g = group ? group[i] : 0;
        if (g < 0 || g >= G) continue;
        int b;
        if constexpr (LDS) b = bin_of(values[i], e_lds, B); else b = bin_of(values[i], edges, B);
        if (b == -2) ++bad;
        if (b < 0) continue;
        if constexpr (LDS) atomicAdd(&c_lds[g * B + b], 1u);
        else atomicAdd(&counts[(size_t)g * B + b], 1ULL);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad += __shfl_xor(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(nonfinite, (unsigned long long)bad);
    if constexpr (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += IM_BLOCK)
            if (c_lds[i]) atomicAdd(&counts[i], (unsigned long long)c_lds[i]);
    }
}

}  // namespace

extern "C" {

size_t jvae_latent_moments_workspace_bytes(int N, int K, int G) {
    if (N < 1 || K < 1 || G < 1 || K > IM_MAX_K || G > IM_MAX_G || N > IM_MAX_N) return 0;
    return sizeof(double) * (size_t)cdiv(N, IM_SLAB) * (size_t)G * IM_STATS * (size_t)K;
}

int jvae_latent_moments_f32(const float* mu, const float* log_var, const int* group, double* sums, long long* counts, int N, int K,
                            int G, void* ws, size_t ws_bytes, void* stream) {
    if (!sums || !counts || N < 0 || K < 1 || G < 1 || ((uintptr_t)sums & 7) || ((uintptr_t)counts & 7)) return JVAE_EINVAL;
    if (K > IM_MAX_K || G > IM_MAX_G || N > IM_MAX_N) return JVAE_ENOTSUP;
    if (N == 0) return 0;
    if (!mu || !log_var) return JVAE_EINVAL;
    const int slabs = cdiv(N, IM_SLAB), kb = cdiv(K, 64), gc = cdiv(G, IM_GC);
    if (slabs > 65535 || gc > 65535) return JVAE_ENOTSUP;
    if (!ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (ws_bytes < jvae_latent_moments_workspace_bytes(N, K, G)) return JVAE_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    moments_kernel<<<dim3((unsigned)kb, (unsigned)gc, (unsigned)slabs), IM_BLOCK, 0, s>>>(mu, log_var, group, part,
                                                                                        (unsigned long long*)counts, N, K, G);
    JVAE_LAUNCH_CHECK();
    const long cells = (long)G * IM_STATS * K;
    moments_fold_kernel<<<cdiv(cells, IM_BLOCK), IM_BLOCK, 0, s>>>(part, sums, slabs, cells);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_nearest_centroid_f32(const float* mu, const float* centroids, long long* y_nearest, float* d2, long N, int K, int C,
                              void* stream) {
    if (!y_nearest || !d2 || N < 0 || K < 1 || C < 1) return JVAE_EINVAL;
    if (K > IM_MAX_K || C > IM_MAX_G || N > (1L << 30)) return JVAE_ENOTSUP;
    if (N == 0) return 0;
    if (!mu || !centroids) return JVAE_EINVAL;
    nearest_kernel<<<(unsigned)N, IM_BLOCK, 0, (hipStream_t)stream>>>(mu, centroids, y_nearest, d2, C, K);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_histogram_f32(const float* values, const double* edges, const int* group, long long* counts, long long* nonfinite, long n,
                       int B, int G, void* stream) {
    if (!edges || !counts || !nonfinite || n < 0 || B < 1 || G < 1 || ((uintptr_t)edges & 7) || ((uintptr_t)counts & 7) ||
        ((uintptr_t)nonfinite & 7))
        return JVAE_EINVAL;
    if ((long)G * B > IH_MAX_CELLS || n > (1L << 40)) return JVAE_ENOTSUP;
    if (n == 0) return 0;
    if (!values) return JVAE_EINVAL;
    const long want = (n + (long)IM_BLOCK * IH_PER_THREAD - 1) / ((long)IM_BLOCK * IH_PER_THREAD);
    const unsigned grid = (unsigned)(want < IH_MAX_GROUPS_BLOCKS ? want : IH_MAX_GROUPS_BLOCKS);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* c = (unsigned long long*)counts;
    unsigned long long* bad = (unsigned long long*)nonfinite;
    if (B <= IH_LDS_BINS && (long)G * B <= IH_LDS_BINS)
        histogram_kernel<true><<<grid, IM_BLOCK, 0, s>>>(values, edges, group, c, bad, n, B, G);
    else
        histogram_kernel<false><<<grid, IM_BLOCK, 0, s>>>(values, edges, group, c, bad, n, B, G);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
