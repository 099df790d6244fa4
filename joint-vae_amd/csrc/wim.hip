// WIM score rows (reference ft/wim.py:132-201, WIMJob.batch_dist_measures): the OOD / misclassification scores a model
// fine-tuned with an alternate prior reads from an evaluation under BOTH priors.  With x = f * v the scaled all-class loss of a
// source (v (C, N): kl, zdist, iws or total; f = -1, -1/2, +1 or -1 for elbo = -total), y the sample's estimated label and
// a (N,) the same loss under the alternate, single prior:
//   kind 0  Y        x[y]                            `k~`
//   kind 1  SOFT_Y   softmax_c(x)[y]                 `softk~`
//   kind 2  LSE_AT   logsumexp_c(x) - f * a          `k@`
//   kind 3  Y_AT     x[y] - f * a                    `k~@`
// ONE launch writes every requested row of up to four sources: blockIdx.y is the source, a thread owns one sample, so the 64
// lanes of a wave read 64 consecutive floats of a class row (one 256-byte segment).  A thread walks the class axis once for the
// maximum and once for sum exp(x - max) (the second walk hits L2) and derives all of its source's rows from the two results: a
// source is read twice whatever the number of rows; a source asked for gathers only is not walked at all.  No atomics: every
// output element has one writer.  f * v is exact for the factors above, so kinds 0 and 3 are the torch expressions bit for bit;
// kinds 1 and 2 are the max-shifted fp32 forms torch uses, the sum compensated (up to 128 sequential terms).
// A label outside [0, C) is never used as an index: its sample gets NaN in kinds 0, 1, 3 and the status word is set to 1.
#include "common.h"
#include "jvae_internal.h"

namespace {

constexpr int WIM_BLOCK = 256;         // samples per workgroup: four waves, one lane per sample
constexpr int WIM_MAX_C = 128;         // classes (ops.MISCLASS_MAX_CLASSES)
constexpr int WIM_MAX_S = 4;           // sources per launch
constexpr int WIM_MAX_R = 16;          // rows per launch: four kinds of four sources
constexpr long WIM_MAX_N = 1L << 30;

enum { WIM_Y = 0, WIM_SOFT_Y = 1, WIM_LSE_AT = 2, WIM_Y_AT = 3 };

struct WimArgs {                       // by value in the kernel arguments: nothing is staged in device memory
    const float* src[WIM_MAX_S];
    const float* alt[WIM_MAX_S];
    float f[WIM_MAX_S];
    int spec_src[WIM_MAX_R], spec_kind[WIM_MAX_R], spec_row[WIM_MAX_R];
    int R;
};

__global__ __launch_bounds__(WIM_BLOCK) void wim_scores_kernel(WimArgs a, const long long* __restrict__ y_est,
                                                               float* __restrict__ out, int* __restrict__ status, int C, long N,
                                                               long out_stride) {
    const long n = (long)blockIdx.x * WIM_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int s = blockIdx.y;
    bool gather = false, walk = false;
    for (int r = 0; r < a.R; ++r) {
        if (a.spec_src[r] != s) continue;
        gather |= a.spec_kind[r] != WIM_LSE_AT;
        walk |= a.spec_kind[r] == WIM_SOFT_Y || a.spec_kind[r] == WIM_LSE_AT;
    }
    if (!gather && !walk) return;
    const float* __restrict__ src = a.src[s];
    const float f = a.f[s];
    float xy = NAN;
    if (gather) {
        const long long y = y_est[n];
        if (y >= 0 && y < (long long)C) xy = f * src[(size_t)y * N + n];
        else *status = 1;              // every writer stores the same word
    }
    float top = -INFINITY, sum = 0.f;
    if (walk) {
#pragma unroll 4
        for (int c = 0; c < C; ++c) top = nan_max(top, f * src[(size_t)c * N + n]);
        float comp = 0.f;              // Kahan
#pragma unroll 4
        for (int c = 0; c < C; ++c) {
            const float e = expf(f * src[(size_t)c * N + n] - top) - comp, t = sum + e;
            comp = (t - sum) - e;
            sum = t;
        }
    }
    const float fa = a.alt[s] ? f * a.alt[s][n] : 0.f;
    for (int r = 0; r < a.R; ++r) {
        if (a.spec_src[r] != s) continue;
        float res;
        switch (a.spec_kind[r]) {
            case WIM_Y: res = xy; break;
            case WIM_SOFT_Y: res = expf(xy - top) / sum; break;
            case WIM_LSE_AT: res = (logf(sum) + top) - fa; break;
            default: res = xy - fa; break;
        }
        out[(size_t)a.spec_row[r] * out_stride + n] = res;
    }
}

// Running tally of the fine-tuning loop's printed losses: ONE workgroup adds this batch's per-group sums of every row and the
// per-group counts to the caller's device accumulators.  For each (row, group) pair a thread sums, in fp64 and in index order,
// the samples tid, tid + 256, ... of that group; the 256 partial sums are folded by a tree over LDS.  A fixed order throughout:
// the same bits run to run; one writer per accumulator, no atomics.
constexpr int TALLY_BLOCK = 256;

__device__ __forceinline__ double tally_fold(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();                       // the previous fold's result has been read by thread 0
    red[tid] = v;
    __syncthreads();
    for (int s = TALLY_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(TALLY_BLOCK) void group_tally_kernel(const float* __restrict__ values, const int* __restrict__ group,
                                                                  double* __restrict__ sums, long long* __restrict__ counts,
                                                                  int R, int N, int G) {
    __shared__ double red[TALLY_BLOCK];
    const int tid = threadIdx.x;
    for (int g = 0; g < G; ++g) {
        double cnt = 0.;                   // exact in fp64 far beyond any batch size
        for (int n = tid; n < N; n += TALLY_BLOCK) cnt += group[n] == g ? 1. : 0.;
        const double c = tally_fold(cnt, red);
        if (tid == 0) counts[g] += (long long)c;
        for (int r = 0; r < R; ++r) {
            double acc = 0.;
            for (int n = tid; n < N; n += TALLY_BLOCK)
                if (group[n] == g) acc += (double)values[(size_t)r * N + n];
            const double t = tally_fold(acc, red);
            if (tid == 0) sums[(size_t)r * G + g] += t;
        }
    }
}

}  // namespace

extern "C" {

int jvae_group_tally_f32(const float* values, const int* group, double* sums, long long* counts, int R, int N, int G,
                         void* stream) {
    if (!sums || !counts || R < 1 || G < 1 || N < 0 || (long)R * G > 4096) return JVAE_EINVAL;
    if (N == 0) return 0;
    if (!values || !group) return JVAE_EINVAL;
    group_tally_kernel<<<1, TALLY_BLOCK, 0, (hipStream_t)stream>>>(values, group, sums, counts, R, N, G);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_wim_scores_f32(const float* const* srcs, const float* const* alts, const float* factors, int S, const long long* y_est,
                        const int* specs, int R, float* out, long out_stride, int C, long N, int* status, void* stream) {
    if (!srcs || !alts || !factors || !out || !status || S < 1 || S > WIM_MAX_S || R < 0 || R > WIM_MAX_R || (R && !specs)) return JVAE_EINVAL;
    if (N < 0 || N > WIM_MAX_N || out_stride < N) return JVAE_EINVAL;
    if (C < 1 || C > WIM_MAX_C) return JVAE_ENOTSUP;
    WimArgs a;
    for (int s = 0; s < WIM_MAX_S; ++s) {
        a.src[s] = s < S ? srcs[s] : nullptr;
        a.alt[s] = s < S ? alts[s] : nullptr;
        a.f[s] = s < S ? factors[s] : 0.f;
        if (s < S && !a.src[s]) return JVAE_EINVAL;
    }
    a.R = R;
    for (int r = 0; r < WIM_MAX_R; ++r) {
        a.spec_src[r] = a.spec_kind[r] = a.spec_row[r] = -1;
        if (r >= R) continue;
        const int s = specs[3 * r], kind = specs[3 * r + 1], row = specs[3 * r + 2];
        if (s < 0 || s >= S || kind < WIM_Y || kind > WIM_Y_AT || row < 0) return JVAE_EINVAL;
        if ((kind == WIM_LSE_AT || kind == WIM_Y_AT) && !a.alt[s]) return JVAE_EINVAL;
        if (kind != WIM_LSE_AT && !y_est) return JVAE_EINVAL;
        for (int q = 0; q < r; ++q)
            if (a.spec_row[q] == row) return JVAE_EINVAL;      // one writer per output element
        a.spec_src[r] = s;
        a.spec_kind[r] = kind;
        a.spec_row[r] = row;
    }
    if (R == 0 || N == 0) return 0;
    wim_scores_kernel<<<dim3((unsigned)cdiv(N, WIM_BLOCK), (unsigned)S), WIM_BLOCK, 0, (hipStream_t)stream>>>(a, y_est, out, status, C,
                                                                                                             N, out_stride);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
