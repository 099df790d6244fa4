// Model ensembles (reference module/aggregation.py, module/cascad.py, results/aggregation.py:321-374): three kernels.
//
// 1. Class posteriors of latent draws.  z (R, K) rows, a conditional Gaussian prior (means (C, K), whitening factor T as
//    GaussianPrior._var_parameter holds it: (C,), (C, K) or (C, K, K) lower triangle, log_det (C,) = log|Sigma_c|):
//      u[c, r]    = |T_c (z_r - m_c)|^2                          (GaussianPrior.mahala: wd_k = d_k t | d_k t_k | sum_{j <= k} T_kj d_j)
//      logp[c, r] = (-(K / 2) log 2 pi - u / 2) - log_det[c] / 2
//      P[t, c, r] = softmax_c(logp[., r] / temps[t])             (max-shifted; a NaN temperature passes logp through)
//    A workgroup owns TR = 32 / 16 / 8 rows (K <= 256 / 512 / 1024; halved while rows and log-densities exceed 48 KiB of LDS):
//    it stages them ONCE in LDS (row stride K + 1: the lanes of
//    a wave walk different rows without bank conflicts) - the only read of z - and deals the TR x C (row, class) pairs to its
//    256 threads, row fastest, so that a wave reads one class's operands as broadcasts (L2) and writes runs of TR consecutive
//    floats.  A pair is one sequential walk over K (full: over the triangle) in fp64 - the fp32 operands are exact in it, so logp
//    carries one rounding, its own on the way out, and P none of logp's.  The TR x C log-densities meet in LDS (fp64); the (row, temperature) pairs are dealt the same way for the soft-max.  Nothing of size
//    C x R x K exists, no thread keeps an array over C or K.
// 2. Pairwise latent mutual information.  P0 (nT, C, L0, N), P1 (nT, C, L1, N):
//      Im[t, n] = 1 / (L0 L1) sum_{a, b} log sum_c P0[t, c, a, n] P1[t, c, b, n]
//    A lane owns a sample (64 consecutive floats per load), a wave a 4 x 4 tile of draw pairs in registers: per class 8 loads
//    feed 16 fmaf.  blockIdx.y is a run of 4 draws of P0, the four waves of the workgroup take the tiles of P1 round-robin;
//    logs are added in fp64 - tile, then wave, then (w0 + w1) + (w2 + w3) through LDS - and one fp64 partial per (t, run, n)
//    goes to the workspace; the second kernel adds the runs in ascending order and divides once.  The order is fixed by
//    (L0, L1) alone.  A pair whose class sum is exactly 0 gives log 0 = -inf, and so does its sample's mean.
// 3. Score aggregation.  E <= 8 sources x_e (C, N) with factors f_e, one thread per sample as in wim.hip:
//      MEAN       a = m + log((sum_e exp(f x_e - m)) / E), m = max_e f x_e        log_mean_exp, on iws with f = 1
//      JOINT      a = f sum_e x_e  (ascending e)                                   joint_posterior, on zdist with f = -1/2
//      MEAN_SOFT  post[t] = (sum_e softmax_c(f x_e / T_t)) / E; NaN temperature: (sum_e f x_e) / E     `mean~`, on kl with f = -1
//      VOTE       the sources are (N,) int64 predictions, a = count_c / E
//    post[t] = softmax_c(a / T_t), a itself for a NaN temperature (VOTE: a for every t); amax / argmax of one slot (-1: a),
//    equal maxima to the lowest class, a NaN kept (nan_max).  The soft-max slots are written as x = a / T first and rewritten
//    in place by the thread that wrote them.  A vote outside [0, C) is never used as an index: the sample's row is NaN and the
//    status word is set to 1.
// No atomics anywhere: one writer per output element, every sum in an order the shape fixes - the same bits run to run.
#include "common.h"
#include "jvae_internal.h"
#include <math.h>

// every product and sum below is rounded on its own unless written as fmaf
#pragma clang fp contract(off)

namespace {

constexpr int AG_BLOCK = 256;
constexpr int AG_MAX_C = 128;          // ops.MISCLASS_MAX_CLASSES
constexpr int AG_MAX_K = 1024;         // PS_MAX_K
constexpr int AG_MAX_E = 8;
constexpr int AG_MAX_T = 16;
constexpr long AG_MAX_N = 1L << 30;
constexpr size_t AG_MAX_LDS = 48 << 10;  // dynamic LDS of a class-posterior workgroup: the rows and their log-densities

enum { VAR_SCALAR = 0, VAR_DIAG = 1, VAR_FULL = 2 };
enum { AG_MEAN = 0, AG_JOINT = 1, AG_MEAN_SOFT = 2, AG_VOTE = 3 };

struct Temps { float v[AG_MAX_T]; int n; };       // by value in the kernel arguments

// torch.max keeps a NaN; the FIRST NaN / maximum wins (torch.argmax)
__device__ __forceinline__ bool ag_better(float x, float best) { return best == best && (x > best || x != x); }

// ------------------------------------------------------------------------------------------------- 1. class posteriors
// fp64 throughout: the fp32 operands are exact in it, so logp carries one rounding (its own, on the way out) and P none of logp's
__device__ __forceinline__ double cp_quad(const float* zr, const float* __restrict__ m, const float* __restrict__ T, int c, int K,
                                          int var_dim) {
    double u = 0.;
    if (var_dim == VAR_SCALAR) {
        const double t = T[c];
        for (int k = 0; k < K; ++k) { const double wd = ((double)zr[k] - (double)m[k]) * t; u = fma(wd, wd, u); }
    } else if (var_dim == VAR_DIAG) {
        const float* __restrict__ tc = T + (size_t)c * K;
        for (int k = 0; k < K; ++k) { const double wd = ((double)zr[k] - (double)m[k]) * (double)tc[k]; u = fma(wd, wd, u); }
    } else {
        const float* __restrict__ tc = T + (size_t)c * K * K;
        for (int k = 0; k < K; ++k) {
            const float* __restrict__ row = tc + (size_t)k * K;
            double wd = 0.;
            for (int j = 0; j <= k; ++j) wd = fma((double)row[j], (double)zr[j] - (double)m[j], wd);
            u = fma(wd, wd, u);
        }
    }
    return u;
}

__global__ __launch_bounds__(AG_BLOCK) void class_posterior_kernel(const float* __restrict__ z, const float* __restrict__ means,
                                                                   const float* __restrict__ T, const float* __restrict__ log_det,
                                                                   Temps temps, float* __restrict__ logp, float* __restrict__ P,
                                                                   long R, int K, int C, int var_dim, int tr_log2, double cst) {
    extern __shared__ double lds[];
    const int TR = 1 << tr_log2, stride = K + 1;
    double* lp = lds;                                              // C x TR (first: 8-byte aligned)
    float* zs = reinterpret_cast<float*>(lds + (size_t)C * TR);    // TR x (K + 1)
    const long r0 = (long)blockIdx.x * TR;
    for (int i = threadIdx.x; i < TR * K; i += AG_BLOCK) {
        const int row = i / K, k = i - row * K;
        zs[row * stride + k] = r0 + row < R ? z[(size_t)(r0 + row) * K + k] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TR * C; i += AG_BLOCK) {
        const int row = i & (TR - 1), c = i >> tr_log2;
        const double u = cp_quad(zs + row * stride, means + (size_t)c * K, T, c, K, var_dim);
        const double v = (cst - u * 0.5) - (double)log_det[c] * 0.5;
        lp[c * TR + row] = v;
        if (logp && r0 + row < R) logp[(size_t)c * R + r0 + row] = (float)v;
    }
    if (!P) return;
    __syncthreads();
    for (int i = threadIdx.x; i < TR * temps.n; i += AG_BLOCK) {
        const int row = i & (TR - 1), t = i >> tr_log2;
        if (r0 + row >= R) continue;
        float* __restrict__ out = P + (size_t)t * C * R + r0 + row;
        const float tf = temps.v[t];
        if (tf != tf) {
            for (int c = 0; c < C; ++c) out[(size_t)c * R] = (float)lp[c * TR + row];
            continue;
        }
        const double tv = tf;
        double top = -INFINITY, sum = 0.;
        for (int c = 0; c < C; ++c) { const double x = lp[c * TR + row] / tv; if (top == top && (x > top || x != x)) top = x; }
        for (int c = 0; c < C; ++c) sum += exp(lp[c * TR + row] / tv - top);
        for (int c = 0; c < C; ++c) out[(size_t)c * R] = (float)(exp(lp[c * TR + row] / tv - top) / sum);
    }
}

// ------------------------------------------------------------------------------------------- 2. latent mutual information
constexpr int MI_TILE = 4;             // draws of each side in a wave's register tile

__global__ __launch_bounds__(AG_BLOCK) void latent_mi_kernel(const float* __restrict__ P0, const float* __restrict__ P1,
                                                             double* __restrict__ part, int C, int L0, int L1, long N) {
    __shared__ double red[AG_BLOCK / 64][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long n = (long)blockIdx.x * 64 + lane;
    const size_t nn = (size_t)(n < N ? n : N - 1);             // a lane past the end reads the last sample and writes nothing
    const int a0 = blockIdx.y * MI_TILE, t = blockIdx.z;
    const float* __restrict__ p0 = P0 + (size_t)t * C * L0 * N + nn;
    const float* __restrict__ p1 = P1 + (size_t)t * C * L1 * N + nn;
    size_t ia[MI_TILE];
#pragma unroll
    for (int i = 0; i < MI_TILE; ++i) ia[i] = (size_t)min(a0 + i, L0 - 1) * N;
    double acc = 0.;
    for (int b0 = w * MI_TILE; b0 < L1; b0 += (AG_BLOCK / 64) * MI_TILE) {
        size_t ib[MI_TILE];
#pragma unroll
        for (int j = 0; j < MI_TILE; ++j) ib[j] = (size_t)min(b0 + j, L1 - 1) * N;
        float s[MI_TILE][MI_TILE];
#pragma unroll
        for (int i = 0; i < MI_TILE; ++i)
#pragma unroll
            for (int j = 0; j < MI_TILE; ++j) s[i][j] = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* __restrict__ q0 = p0 + (size_t)c * L0 * N;
            const float* __restrict__ q1 = p1 + (size_t)c * L1 * N;
            float x[MI_TILE], y[MI_TILE];
#pragma unroll
            for (int i = 0; i < MI_TILE; ++i) { x[i] = q0[ia[i]]; y[i] = q1[ib[i]]; }
#pragma unroll
            for (int i = 0; i < MI_TILE; ++i)
#pragma unroll
                for (int j = 0; j < MI_TILE; ++j) s[i][j] = fmaf(x[i], y[j], s[i][j]);
        }
        double tile = 0.;
#pragma unroll
        for (int i = 0; i < MI_TILE; ++i)
#pragma unroll
            for (int j = 0; j < MI_TILE; ++j)
                if (a0 + i < L0 && b0 + j < L1) tile += (double)logf(s[i][j]);
        acc += tile;
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && n < N)
        part[((size_t)t * gridDim.y + blockIdx.y) * N + n] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

__global__ __launch_bounds__(AG_BLOCK) void latent_mi_fold_kernel(const double* __restrict__ part, float* __restrict__ Im, int runs,
                                                                  long N, double count) {
    const long n = (long)blockIdx.x * AG_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int t = blockIdx.y;
    double s = 0.;
    for (int r = 0; r < runs; ++r) s += part[((size_t)t * runs + r) * N + n];
    Im[(size_t)t * N + n] = (float)(s / count);
}

// --------------------------------------------------------------------------------------------------- 3. score aggregation
struct AggArgs {                       // by value in the kernel arguments, as WimArgs
    const void* src[AG_MAX_E];
    float f[AG_MAX_E];
    int E, mode, slot;
};

// a[c] of sample n for MEAN / JOINT / VOTE (VOTE: the sample's votes have been checked)
__device__ __forceinline__ float agg_elem(const AggArgs& g, int c, long n, long N) {
    const size_t at = (size_t)c * N + n;
    if (g.mode == AG_JOINT) {
        float s = static_cast<const float*>(g.src[0])[at];
        for (int e = 1; e < g.E; ++e) s += static_cast<const float*>(g.src[e])[at];
        return g.f[0] * s;
    }
    if (g.mode == AG_VOTE) {
        int count = 0;
        for (int e = 0; e < g.E; ++e) count += static_cast<const long long*>(g.src[e])[n] == (long long)c;
        return (float)count / (float)g.E;
    }
    float m = -INFINITY;
    for (int e = 0; e < g.E; ++e) {
        const float x = g.f[e] * static_cast<const float*>(g.src[e])[at];
        if (x > m || x != x) m = x;
    }
    float s = 0.f;
    for (int e = 0; e < g.E; ++e) s += expf(g.f[e] * static_cast<const float*>(g.src[e])[at] - m);
    return logf(s / (float)g.E) + m;
}

__global__ __launch_bounds__(AG_BLOCK) void aggregate_scores_kernel(AggArgs g, Temps temps, float* __restrict__ post,
                                                                    float* __restrict__ a_out, float* __restrict__ amax,
                                                                    long long* __restrict__ argmax, int* __restrict__ status,
                                                                    int C, long N) {
    const long n = (long)blockIdx.x * AG_BLOCK + threadIdx.x;
    if (n >= N) return;
    const size_t plane = (size_t)C * N;
    bool bad = false;
    if (g.mode == AG_VOTE) {
        for (int e = 0; e < g.E; ++e) {
            const long long y = static_cast<const long long*>(g.src[e])[n];
            bad |= y < 0 || y >= (long long)C;
        }
        if (bad) *status = 1;          // every writer stores the same word
    }
    float best = -INFINITY;
    long long arg = 0;
    const bool want = amax || argmax;
    bool kept = false;                 // a_out holds this sample's aggregated row
    // a[c] of this sample: NaN after a bad vote, read back once written out, else recomputed - with neither `post` nor `a` to
    // keep it in, a soft-max slot asked for its maximum alone computes the row three times (maximum, sum, values)
    auto row = [&](int c) { return bad ? NAN : (kept ? a_out[(size_t)c * N + n] : agg_elem(g, c, n, N)); };
    if (g.mode != AG_MEAN_SOFT && (a_out || (want && g.slot < 0))) {
        for (int c = 0; c < C; ++c) {
            const float v = row(c);
            if (a_out) a_out[(size_t)c * N + n] = v;
            if (g.slot < 0 && (c == 0 || ag_better(v, best))) { best = v; arg = c; }
        }
        kept = a_out != nullptr;
    }
    for (int t = 0; t < temps.n; ++t) {
        if (!post && !(want && g.slot == t)) continue;
        const float tv = temps.v[t];
        const bool pass = tv != tv || g.mode == AG_VOTE;       // the slot is the aggregated row itself
        float* __restrict__ out = post ? post + (size_t)t * plane + n : nullptr;
        // x[c] = a[c] / T of a soft-max slot: kept in the slot itself once written there
        auto scaled = [&](int c, bool written) { return written && out ? out[(size_t)c * N] : row(c) / tv; };
        float top_e[AG_MAX_E], sum_e[AG_MAX_E];
        float top = -INFINITY;
        Kahan sum;
        if (!pass && g.mode == AG_MEAN_SOFT) {
#pragma unroll
            for (int e = 0; e < AG_MAX_E; ++e) {
                top_e[e] = -INFINITY;
                sum_e[e] = 1.f;
                if (e >= g.E) continue;
                const float* __restrict__ src = static_cast<const float*>(g.src[e]) + n;
                for (int c = 0; c < C; ++c) { const float x = g.f[e] * src[(size_t)c * N] / tv; if (ag_better(x, top_e[e])) top_e[e] = x; }
                Kahan s;
                for (int c = 0; c < C; ++c) s.add(expf(g.f[e] * src[(size_t)c * N] / tv - top_e[e]));
                sum_e[e] = s.s;
            }
        } else if (!pass) {
            for (int c = 0; c < C; ++c) {
                const float x = scaled(c, false);
                if (out) out[(size_t)c * N] = x;
                if (ag_better(x, top)) top = x;
            }
            for (int c = 0; c < C; ++c) sum.add(expf(scaled(c, true) - top));
        }
        for (int c = 0; c < C; ++c) {
            float v;
            if (g.mode == AG_MEAN_SOFT) {
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < AG_MAX_E; ++e) {
                    if (e >= g.E) continue;
                    const float x = g.f[e] * static_cast<const float*>(g.src[e])[(size_t)c * N + n];
                    s += pass ? x : expf(x / tv - top_e[e]) / sum_e[e];
                }
                v = s / (float)g.E;
            } else {
                v = pass ? row(c) : expf(scaled(c, true) - top) / sum.s;
            }
            if (out) out[(size_t)c * N] = v;
            if (g.slot == t && (c == 0 || ag_better(v, best))) { best = v; arg = c; }
        }
    }
    if (amax) amax[n] = best;
    if (argmax) argmax[n] = arg;
}

bool temps_from_host(const float* temps, int nT, Temps& out) {
    if (nT < 0 || nT > AG_MAX_T || (nT && !temps)) return false;
    out.n = nT;
    for (int t = 0; t < AG_MAX_T; ++t) out.v[t] = t < nT ? temps[t] : NAN;
    return true;
}

}  // namespace

extern "C" {

int jvae_class_posterior_f32(const float* z, const float* means, const float* T, const float* log_det, const float* temps, int nT,
                             float* logp, float* P, long R, int K, int C, int var_dim, void* stream) {
    Temps tp;
    if (!z || !means || !T || !log_det || (!logp && !P) || !temps_from_host(temps, nT, tp) || (P && nT < 1)) return JVAE_EINVAL;
    if (R < 0 || K < 1 || K > AG_MAX_K || C < 1 || C > AG_MAX_C || var_dim < VAR_SCALAR || var_dim > VAR_FULL) return JVAE_EINVAL;
    if (R > AG_MAX_N) return JVAE_EINVAL;
    if (R == 0) return 0;
    int tr_log2 = K <= 256 ? 5 : (K <= 512 ? 4 : 3);
    auto lds_of = [&](int l2) { return (sizeof(float) * ((size_t)K + 1) + sizeof(double) * (size_t)C) << l2; };
    while (lds_of(tr_log2) > AG_MAX_LDS) --tr_log2;            // e.g. C = 128: 32 rows up to K = 127, 16 up to 511
    const int TR = 1 << tr_log2;
    const size_t lds = lds_of(tr_log2);
    const double cst = -log(2. * M_PI) * K / 2.;
    class_posterior_kernel<<<cdiv(R, TR), AG_BLOCK, lds, (hipStream_t)stream>>>(z, means, T, log_det, tp, logp, P, R, K, C, var_dim,
                                                                              tr_log2, cst);
    JVAE_LAUNCH_CHECK();
    return 0;
}

size_t jvae_latent_mi_workspace_bytes(int nT, int L0, long N) {
    if (nT < 1 || L0 < 1 || N < 1) return 0;
    return sizeof(double) * (size_t)nT * cdiv(L0, MI_TILE) * (size_t)N;
}

int jvae_latent_mi_f32(const float* P0, const float* P1, float* Im, int nT, int C, int L0, int L1, long N, void* ws, size_t ws_bytes,
                       void* stream) {
    if (!P0 || !P1 || !Im || nT < 1 || nT > AG_MAX_T || C < 1 || C > AG_MAX_C || L0 < 1 || L1 < 1 || L0 > 65535 * MI_TILE || N < 0
        || N > AG_MAX_N)
        return JVAE_EINVAL;
    if ((double)nT * C * (double)(L0 > L1 ? L0 : L1) * (double)N > 1e15) return JVAE_EINVAL;
    if (N == 0) return 0;
    if (!ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (ws_bytes < jvae_latent_mi_workspace_bytes(nT, L0, N)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int runs = cdiv(L0, MI_TILE);
    latent_mi_kernel<<<dim3((unsigned)cdiv(N, 64), (unsigned)runs, (unsigned)nT), AG_BLOCK, 0, st>>>(P0, P1, (double*)ws, C, L0, L1, N);
    JVAE_LAUNCH_CHECK();
    latent_mi_fold_kernel<<<dim3((unsigned)cdiv(N, AG_BLOCK), (unsigned)nT), AG_BLOCK, 0, st>>>((const double*)ws, Im, runs, N,
                                                                                              (double)L0 * (double)L1);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_aggregate_scores_f32(const void* const* srcs, const float* factors, int E, int mode, const float* temps, int nT, float* post,
                              float* a, float* amax, long long* argmax, int slot, int C, long N, int* status, void* stream) {
    Temps tp;
    if (!srcs || !factors || E < 1 || E > AG_MAX_E || mode < AG_MEAN || mode > AG_VOTE || !temps_from_host(temps, nT, tp)) return JVAE_EINVAL;
    if (C < 1 || C > AG_MAX_C || N < 0 || N > AG_MAX_N || (!post && !a && !amax && !argmax)) return JVAE_EINVAL;
    if ((post && nT < 1) || slot < -1 || slot >= nT || (mode == AG_MEAN_SOFT && (a || ((amax || argmax) && slot < 0)))) return JVAE_EINVAL;
    if (mode == AG_VOTE && !status) return JVAE_EINVAL;
    AggArgs g;
    g.E = E;
    g.mode = mode;
    g.slot = slot;
    for (int e = 0; e < AG_MAX_E; ++e) {
        g.src[e] = e < E ? srcs[e] : nullptr;
        g.f[e] = e < E ? factors[e] : 0.f;
        if (e < E && !g.src[e]) return JVAE_EINVAL;
    }
    if (N == 0) return 0;
    aggregate_scores_kernel<<<cdiv(N, AG_BLOCK), AG_BLOCK, 0, (hipStream_t)stream>>>(g, tp, post, a, amax, argmax, status, C, N);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
