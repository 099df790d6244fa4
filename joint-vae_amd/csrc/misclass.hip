// Misclassification detection (reference cvae.py:1913-2079): what sits around the device ROC of csrc/roc.hip.
//
//   scores     one launch turns a (C, N) fp32 source (the all-class kl / zdist / iws losses, or the logits as the recorder
//              stores them) into all of its requested score rows (batch_dist_measures, cvae.py:1024-1063):
//                kind 0  max_c softmax_c(-v / T)      softkl[-T], softzdist-T, softiws-T
//                kind 1  max_c softmax_c(+v / T)      softiws (T = 1), baseline[-T]
//                kind 2  max_c (-v)                   kl, zdist, max
//                kind 3  max_c v                      logits
//                kind 4  sum_c p log p, p = softmax v hyz
//              and the rest of the class-axis table (cvae.py:985-1068), which the OOD pass asks for; l = -v, d = l - max_c l,
//              e = exp d, T = an additive constant:
//                kind 5  log sum_c e + max_c l + T    sum (T = 0)          kind 6  the same on l = +v: iws (T = log C)
//                kind 7  log mean_c e + max_c l       mean                 kind 8  std_c l, unbiased       std
//                kind 9  (std_c e / mean_c e)^2       nstd                 kind 10 max_c l - median_c l    mag
//                kind 11 sum_c(d e) / (C mean_c e) - log mean_c e  IYx     kind 12 / 13  -v / v of a (1, N) source: mse, wmse, elbo
//              A workgroup stages a (C, 64) tile of the source in LDS once; one lane per sample then loops over the classes
//              for every row, so the source is read from HBM once whatever the number of temperatures.  fp32 throughout, the
//              max-subtracted softmax torch uses: exp(x - max) / sum, whose largest term is 1 / sum.
//   split      compacts the (M, N) score rows into ins (M, n_correct) and outs (M, N - n_correct) by a byte mask: ONE
//              exclusive scan of the mask (wave ballots + a scan of the 1024-sample block counts) gives every sample its slot,
//              shared by all rows; the order inside a row is kept (the ROC sorts anyway).  n_correct stays on the device: the
//              scatter reads it there, both row sets go into one M * N buffer, ins first.
//   confusion  tp[m][k] = #{correct, s >= thr[m][k]}, fp[m][k] = #{missed, s >= thr[m][k]} (cvae.py:2009-2015) on exactly
//              widened scores, as roc.hip compares them; integer counts, so the result does not depend on any order.
#include "common.h"
#include "jvae_internal.h"

namespace {

constexpr int MISC_TILE = 64;          // samples per workgroup of the score kernel: one wave, one lane per sample
constexpr int MISC_MAX_C = 128;        // classes: the (C, 64) fp32 tile is at most 32 KiB of LDS
constexpr int MISC_MAX_K = 16;         // kept thresholds per row: the counters of the confusion kernel live in registers
constexpr int MISC_SCAN = 1024;        // samples per block of the mask scan
constexpr int MISC_CONF_PER = 8;       // samples per thread of the confusion kernel
constexpr long MISC_MAX_N = 1L << 24;  // as jvae_roc_curve_f32: counts stay in int32

// kinds 5 .. 13 of one sample: col[c * MISC_TILE] = v_c, l = -v (lse+: l = v), d = l - lmax, e = exp d.  The order of operations
// is the reference's (cvae.py:985-1068); `add` is the constant of the lse rows.  An unknown kind gives NaN.
__device__ float misc_axis_row(const float* col, int C, int kind, float add) {
    if (kind == 12) return -col[0];
    if (kind == 13) return col[0];
    const float sign = kind == 6 ? 1.f : -1.f;
    const float n = (float)C;
    float lmax = -INFINITY;
    for (int c = 0; c < C; ++c) lmax = nan_max(lmax, sign * col[c * MISC_TILE]);
    if (kind == 10) {                  // lmax - the lower middle element, found by its rank; a NaN is in lmax already
        const int k = (C - 1) / 2;
        float med = lmax;
        for (int i = 0; i < C; ++i) {
            const float x = -col[i * MISC_TILE];
            int lt = 0, eq = 0;
            for (int j = 0; j < C; ++j) {
                const float y = -col[j * MISC_TILE];
                lt += y < x;
                eq += y == x;
            }
            if (lt <= k && k < lt + eq) med = x;
        }
        return lmax - med;
    }
    if (kind == 8) {                   // torch.std (ddof = 1) of l - lmax, which is that of l: two passes, 0 / 0 = NaN for C = 1
        Kahan m, q;                  // l - lmax as hi + lo, exactly (TwoSum): at an ELBO's spread its rounding would be the error
        float lo_sum = 0.f;
        for (int c = 0; c < C; ++c) {
            const float l = -col[c * MISC_TILE], hi = l - lmax, b = hi - l;
            m.add(hi);
            lo_sum += (l - (hi - b)) + (-lmax - b);
        }
        const float mean = (m.s + lo_sum) / n;
        for (int c = 0; c < C; ++c) {
            const float l = -col[c * MISC_TILE], hi = l - lmax, b = hi - l;
            const float t = (hi - mean) + ((l - (hi - b)) + (-lmax - b));
            q.add(t * t);
        }
        return sqrtf(q.s / (float)(C - 1));
    }
    if (kind < 5 || kind > 11) return NAN;
    Kahan e;
    for (int c = 0; c < C; ++c) e.add(expf(sign * col[c * MISC_TILE] - lmax));
    if (kind == 5 || kind == 6) return logf(e.s) + lmax + add;
    const float mean = e.s / n;
    if (kind == 7) return logf(mean) + lmax;
    if (kind == 9) {
        Kahan q;
        for (int c = 0; c < C; ++c) {
            const float t = expf(-col[c * MISC_TILE] - lmax) - mean;
            q.add(t * t);
        }
        const float r = expf(logf(sqrtf(q.s / (float)(C - 1))) - logf(mean));
        return r * r;
    }
    const float m = logf(mean);        // kind 11
    Kahan w;
    for (int c = 0; c < C; ++c) {
        const float d = -col[c * MISC_TILE] - lmax;
        w.add(d * expf(d));
    }
    return w.s / (n * expf(m)) - m;
}

__global__ __launch_bounds__(MISC_TILE) void misclass_scores_kernel(const float* __restrict__ src, const int* __restrict__ kinds,
                                                                    const float* __restrict__ temps,
                                                                    const int* __restrict__ rows, float* __restrict__ out,
                                                                    int R, int C, long N, long out_stride) {
    __shared__ float s[MISC_MAX_C * MISC_TILE];
    const int lane = threadIdx.x;
    const long n = (long)blockIdx.x * MISC_TILE + lane;
    if (n >= N) return;                // no barrier below: a lane only reads the column it staged itself
    for (int c = 0; c < C; ++c) s[c * MISC_TILE + lane] = src[(size_t)c * N + n];
    for (int r = 0; r < R; ++r) {
        const int kind = kinds[r];
        const float T = temps[r];
        float res;
        if (kind >= 5) {
            res = misc_axis_row(s + lane, C, kind, T);
        } else if (kind == 2 || kind == 3) {
            float best = -INFINITY;
            for (int c = 0; c < C; ++c) {
                const float v = s[c * MISC_TILE + lane];
                best = nan_max(best, kind == 2 ? -v : v);
            }
            res = best;
        } else {
            const bool neg = kind == 0;
            float best = -INFINITY;
            for (int c = 0; c < C; ++c) {
                const float v = s[c * MISC_TILE + lane];
                best = nan_max(best, (neg ? -v : v) / T);
            }
            float sum = 0.f;
            for (int c = 0; c < C; ++c) {
                const float v = s[c * MISC_TILE + lane];
                sum += expf((neg ? -v : v) / T - best);
            }
            if (kind == 4) {
                float h = 0.f;
                for (int c = 0; c < C; ++c) {
                    const float p = expf(s[c * MISC_TILE + lane] / T - best) / sum;
                    h += p * logf(p);  // p == 0 gives NaN, as torch's p * p.log() does: the ROC flags the row
                }
                res = h;
            } else {
                res = 1.f / sum;       // exp(best - best) / sum: the largest softmax term
            }
        }
        out[(size_t)rows[r] * out_stride + n] = res;
    }
}

// number of set mask bytes among the samples before this thread's in its block (+ the block's total in *total)
__device__ __forceinline__ int misc_block_prefix(bool set, int* wave_sums, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(set);
    const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_sums[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < MISC_SCAN / 64; ++w) {
        const int v = wave_sums[w];
        before += w < wave ? v : 0;
        all += v;
    }
    *total = all;
    return before + in_wave;
}

__global__ __launch_bounds__(MISC_SCAN) void misclass_count_kernel(const unsigned char* __restrict__ mask, int* __restrict__ bsum,
                                                                   long N) {
    __shared__ int wave_sums[MISC_SCAN / 64];
    const long i = (long)blockIdx.x * MISC_SCAN + threadIdx.x;
    int total;
    misc_block_prefix(i < N && mask[i] != 0, wave_sums, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// exclusive scan of the block counts by one workgroup (chunks of 1024 with a running carry) + the grand total
__global__ __launch_bounds__(MISC_SCAN) void misclass_offsets_kernel(const int* __restrict__ bsum, int* __restrict__ boff,
                                                                     int* __restrict__ n_correct, int nb) {
    __shared__ int s[MISC_SCAN];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < nb; base += MISC_SCAN) {
        const int v = base + t < nb ? bsum[base + t] : 0;
        s[t] = v;
        __syncthreads();
        for (int o = 1; o < MISC_SCAN; o <<= 1) {
            const int add = t >= o ? s[t - o] : 0;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        if (base + t < nb) boff[base + t] = carry + s[t] - v;
        carry += s[MISC_SCAN - 1];
        __syncthreads();
    }
    if (t == 0) *n_correct = carry;
}

__global__ __launch_bounds__(MISC_SCAN) void misclass_pos_kernel(const unsigned char* __restrict__ mask, const int* __restrict__ boff,
                                                                 int* __restrict__ pos, long N) {
    __shared__ int wave_sums[MISC_SCAN / 64];
    const long i = (long)blockIdx.x * MISC_SCAN + threadIdx.x;
    int total;
    const int before = misc_block_prefix(i < N && mask[i] != 0, wave_sums, &total);
    if (i < N) pos[i] = boff[blockIdx.x] + before;
}

__global__ __launch_bounds__(256) void misclass_scatter_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ mask,
                                                               const int* __restrict__ pos, const int* __restrict__ n_correct,
                                                               float* __restrict__ out, int M, long N) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int m = blockIdx.y;
    const long nc = *n_correct, p = pos[i];
    const float v = scores[(size_t)m * N + i];
    if (mask[i]) out[(size_t)m * nc + p] = v;                                   // p < nc
    else out[(size_t)M * nc + (size_t)m * (N - nc) + (i - p)] = v;               // i - p < N - nc
}

__global__ __launch_bounds__(256) void misclass_confusion_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ mask,
                                                                 const double* __restrict__ thr, int* __restrict__ tp,
                                                                 int* __restrict__ fp, long N, int K) {
    __shared__ int acc[2 * MISC_MAX_K];
    const int m = blockIdx.y, t = threadIdx.x;
    if (t < 2 * MISC_MAX_K) acc[t] = 0;
    double th[MISC_MAX_K];
#pragma unroll
    for (int k = 0; k < MISC_MAX_K; ++k) th[k] = k < K ? thr[(size_t)m * K + k] : (double)INFINITY;
    int ctp[MISC_MAX_K], cfp[MISC_MAX_K];
#pragma unroll
    for (int k = 0; k < MISC_MAX_K; ++k) ctp[k] = cfp[k] = 0;
    const long base = (long)blockIdx.x * (256 * MISC_CONF_PER) + t;
    for (int j = 0; j < MISC_CONF_PER; ++j) {
        const long i = base + (long)j * 256;
        if (i >= N) break;
        const double v = (double)scores[(size_t)m * N + i];
        const bool ok = mask[i] != 0;
#pragma unroll
        for (int k = 0; k < MISC_MAX_K; ++k) {
            const int ge = k < K && v >= th[k];    // a NaN score or threshold counts nowhere, as numpy's >= does
            ctp[k] += ge && ok;
            cfp[k] += ge && !ok;
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MISC_MAX_K; ++k) {
        int a = ctp[k], b = cfp[k];
        for (int o = 32; o > 0; o >>= 1) {
            a += __shfl_xor(a, o, 64);
            b += __shfl_xor(b, o, 64);
        }
        if ((t & 63) == 0 && k < K) {
            if (a) atomicAdd(&acc[k], a);
            if (b) atomicAdd(&acc[MISC_MAX_K + k], b);
        }
    }
    __syncthreads();
    if (t < K && acc[t]) atomicAdd(&tp[(size_t)m * K + t], acc[t]);
    if (t >= MISC_MAX_K && t - MISC_MAX_K < K && acc[t]) atomicAdd(&fp[(size_t)m * K + t - MISC_MAX_K], acc[t]);
}

struct MiscWs { size_t pos, bsum, boff, total; };
inline size_t misc_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline MiscWs misc_ws(long N) {
    const size_t nb = (size_t)cdiv(N, MISC_SCAN);
    MiscWs w;
    size_t o = 0;
    w.pos = o;  o += misc_align(sizeof(int) * (size_t)N);
    w.bsum = o; o += misc_align(sizeof(int) * nb);
    w.boff = o; o += misc_align(sizeof(int) * nb);
    w.total = o;
    return w;
}

}  // namespace

extern "C" {

int jvae_misclass_scores_f32(const float* src, const int* kinds, const float* temps, const int* rows, float* out,
                             int R, int C, long N, long out_stride, void* stream) {
    if (!src || !kinds || !temps || !rows || !out || R < 0 || N < 0 || out_stride < N) return JVAE_EINVAL;
    if (C < 1 || C > MISC_MAX_C || N > MISC_MAX_N) return JVAE_EINVAL;
    if (R == 0 || N == 0) return 0;
    misclass_scores_kernel<<<cdiv(N, MISC_TILE), MISC_TILE, 0, (hipStream_t)stream>>>(src, kinds, temps, rows, out, R, C, N,
                                                                                      out_stride);
    JVAE_LAUNCH_CHECK();
    return 0;
}

size_t jvae_misclass_split_workspace_bytes(long N) {
    if (N < 1 || N > MISC_MAX_N) return 0;
    return misc_ws(N).total;
}

int jvae_misclass_split_f32(const float* scores, const unsigned char* mask, float* out, int* n_correct, int M, long N,
                            void* ws, size_t ws_bytes, void* stream) {
    if (!scores || !mask || !out || !n_correct || !ws) return JVAE_EINVAL;
    if (M < 1 || M > 65535 || N < 1 || N > MISC_MAX_N) return JVAE_EINVAL;
    const MiscWs w = misc_ws(N);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 3) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    int* pos = (int*)(base + w.pos);
    int* bsum = (int*)(base + w.bsum);
    int* boff = (int*)(base + w.boff);
    const int nb = cdiv(N, MISC_SCAN);
    misclass_count_kernel<<<nb, MISC_SCAN, 0, st>>>(mask, bsum, N);
    JVAE_LAUNCH_CHECK();
    misclass_offsets_kernel<<<1, MISC_SCAN, 0, st>>>(bsum, boff, n_correct, nb);
    JVAE_LAUNCH_CHECK();
    misclass_pos_kernel<<<nb, MISC_SCAN, 0, st>>>(mask, boff, pos, N);
    JVAE_LAUNCH_CHECK();
    misclass_scatter_kernel<<<dim3((unsigned)cdiv(N, 256), (unsigned)M), 256, 0, st>>>(scores, mask, pos, n_correct, out, M, N);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_misclass_confusion_f32(const float* scores, const unsigned char* mask, const double* thr, int* tp, int* fp,
                                int M, long N, int K, void* stream) {
    if (!scores || !mask || !thr || !tp || !fp) return JVAE_EINVAL;
    if (M < 1 || M > 65535 || N < 1 || N > MISC_MAX_N || K < 1 || K > MISC_MAX_K) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(tp, 0, sizeof(int) * (size_t)M * K, st);
    if (e == hipSuccess) e = hipMemsetAsync(fp, 0, sizeof(int) * (size_t)M * K, st);
    if (e != hipSuccess) return (int)e;
    misclass_confusion_kernel<<<dim3((unsigned)cdiv(N, 256 * MISC_CONF_PER), (unsigned)M), 256, 0, st>>>(scores, mask, thr, tp, fp,
                                                                                                        N, K);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
