// Device-side ROC of OOD scores: AUC and the FPR / thresholds at a list of kept TPRs, for M score rows in one call.
//
// Reference: utils/roc_curves.py:38-210 (roc_curve: a Python `while` over every in-distribution score taken as a threshold,
// with inner pointer loops), called per method and per OOD set by ClassificationVariationalNetwork.ood_detection_rates
// (cvae.py:1843-1868).  The modes are the one-sided test (two_sided False / True, roc_curves.py:85-88), 'around-mean'
// (roc_curves.py:68-72) and the strided quantiles of the tuple mode (roc_curves.py:74-83): low = [-inf, s[::f_low], inf],
// up = [-inf, s[::f_up], inf] over the sorted in-scores s THEMSELVES.  The reference takes them from an interpolating cubic
// spline evaluated at its own knots, i.e. s again up to FITPACK's rounding, and then compares each score with its own noisy
// image: that noise is not reproduced, the loop on the noise-free thresholds is, bit for bit.
//
// The pointer loops are monotone in the iteration index `it`, so every iteration stands alone:
//   low[it], up[-1 - it]      thresholds (fp64, the reference's own expressions over exactly widened fp32 scores)
//   c_low = min(n - 1, #{s < low}),  c_up = min(n - 1, #{s > up})     two binary searches in a sorted row (the n - 1 caps are
//                                                                     the pointer loops stopping one short of the end)
//   tpr = 1 - (c_low + c_up)_in / n_in,  fpr = 1 - (c_low + c_up)_out / n_out
// and the walk visits the prefix of `it` with low < up, it < nt - 1.  The kept-TPR cursor of roc_curves.py:181-189 moves over
// a non-increasing tpr: K binary searches.  The AUC (sklearn's trapezoid over the visited points plus (0, 0)) is summed in
// 64-bit integers over the counts - integer addition is exact in any order - and divided once.
//
// Sort: bitonic network on the order-preserving integer image of the scores (uint32 for the fp32 rows, the raw bits of the
// non-negative fp64 |s - c| for the around-mean deltas); strides below the 2048-key tile run in LDS, longer ones in HBM.
// Rows are padded to a power of two (>= one tile) with the largest key, which sorts behind every real score.
#include "common.h"
#include "jvae_internal.h"
#include "roc_sort.h"                  // ROC_TILE, roc_pad, roc_key / roc_unkey, the bitonic passes, roc_sort_rows, roc_mean_kernel, ROC_MAX_N

namespace {

struct RocWs {                         // carve-up of the caller's workspace (all offsets multiples of 256 bytes)
    size_t kin, kout, d, negin, negout, acc, c, V, total;
};
inline size_t roc_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline RocWs roc_ws(int M, long n_in, long n_out) {
    const size_t Pin = (size_t)roc_pad(n_in), Pout = (size_t)roc_pad(n_out), nt = (size_t)n_in + 2;
    RocWs w;
    size_t o = 0;
    w.kin = o;    o += roc_align(sizeof(uint32_t) * Pin * M);
    w.kout = o;   o += roc_align(sizeof(uint32_t) * Pout * M);
    w.d = o;      o += roc_align(sizeof(uint64_t) * Pin * M);
    w.negin = o;  o += roc_align(sizeof(int) * nt * M);
    w.negout = o; o += roc_align(sizeof(int) * nt * M);
    w.acc = o;    o += roc_align(sizeof(unsigned long long) * M);
    w.c = o;      o += roc_align(sizeof(double) * M);
    w.V = o;      o += roc_align(sizeof(int) * M);
    w.total = o;
    return w;
}

// keys of both row sets (z = 0: ins, 1: outs) + the status word (bit 0: NaN score, bit 1: non-finite in-score of an
// around-mean row, bit 2: malformed mode word).  atomicOr on an integer flag: the result does not depend on the order.
__global__ __launch_bounds__(256) void roc_keys_kernel(const float* __restrict__ ins, const float* __restrict__ outs,
                                                       const int* __restrict__ modes, uint32_t* __restrict__ kin,
                                                       uint32_t* __restrict__ kout, int* __restrict__ status,
                                                       long n_in, long n_out, long Pin, long Pout) {
    const int m = blockIdx.y, z = blockIdx.z;
    const long n = z ? n_out : n_in, P = z ? Pout : Pin;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint32_t key = 0xFFFFFFFFu;
    int bad = 0;
    if (i < n) {
        const float v = (z ? outs : ins)[(size_t)m * n + i];
        key = roc_key(v);
        if (v != v) bad |= 1;
        if (z == 0 && modes[m] == 1 && !isfinite(v)) bad |= 2;
    }
    int f_low, f_up;
    if (z == 0 && i == 0 && roc_decode(modes[m], f_low, f_up) < 0) bad |= 4;
    (z ? kout : kin)[(size_t)m * P + i] = key;
    if (bad) atomicOr(&status[m], bad);
}

// abs(ins - center) in fp64 (roc_curves.py:70) as sortable bits: non-negative doubles order as their bit patterns
__global__ __launch_bounds__(256) void roc_delta_kernel(const float* __restrict__ ins, const int* __restrict__ modes,
                                                        const double* __restrict__ c, uint64_t* __restrict__ d, long n, long P) {
    const int m = blockIdx.y;
    if (modes[m] != 1) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    uint64_t key = ~(uint64_t)0;
    if (i < n) key = (uint64_t)__double_as_longlong(fabs((double)ins[(size_t)m * n + i] - c[m]));
    d[(size_t)m * P + i] = key;
}

struct RocRow {
    const uint32_t* kin; const uint32_t* kout; const uint64_t* d;
    double c; int mode; long n_in, n_out, nt;
    long f_low, f_up, n_low, n_up;     // quantile rows: strides and lengths of the two threshold vectors
};
__device__ __forceinline__ RocRow roc_row(int m, const uint32_t* kin, const uint32_t* kout, const uint64_t* d, const double* c,
                                          const int* modes, long n_in, long n_out, long Pin, long Pout) {
    RocRow r;
    r.kin = kin + (size_t)m * Pin; r.kout = kout + (size_t)m * Pout; r.d = d + (size_t)m * Pin;
    int f_low, f_up;
    const int kind = roc_decode(modes[m], f_low, f_up);
    r.mode = kind < 0 ? 0 : kind;      // a malformed word is flagged in the status; its row runs as a one-sided one
    r.c = r.mode == 1 ? c[m] : 0.0;
    r.n_in = n_in; r.n_out = n_out;
    r.f_low = f_low; r.f_up = f_up;
    r.n_low = r.n_up = 0;
    if (r.mode == 2) {                 // len([-inf, s[::f], inf])
        r.n_low = (n_in + f_low - 1) / f_low + 2;
        r.n_up = (n_in + f_up - 1) / f_up + 2;
        r.nt = r.n_low < r.n_up ? r.n_low : r.n_up;
    } else {
        r.nt = n_in + 1 + r.mode;
    }
    return r;
}

// all_thresholds['low'][it], all_thresholds['up'][-1 - it] (roc_curves.py:68-72,81-88), 0 <= it < nt
__device__ __forceinline__ void roc_thresholds(const RocRow& r, long it, double& low, double& up) {
    if (r.mode == 2) {                 // it <= nt - 1 <= n_low - 1 and q >= n_up - nt >= 0: every index is inside the row
        const long q = r.n_up - 1 - it;
        low = it == 0 ? -(double)INFINITY
                      : (it == r.n_low - 1 ? (double)INFINITY : (double)roc_unkey(r.kin[(it - 1) * r.f_low]));
        up = q == 0 ? -(double)INFINITY : (q == r.n_up - 1 ? (double)INFINITY : (double)roc_unkey(r.kin[(q - 1) * r.f_up]));
    } else if (r.mode) {                      // delta = [0, sort(|ins - c|)..., inf] read from its far end
        const long q = r.n_in + 1 - it;
        const double D = q == 0 ? 0.0 : (q == r.n_in + 1 ? (double)INFINITY : __longlong_as_double((long long)r.d[q - 1]));
        low = -D + r.c;
        up = D + r.c;
    } else {
        low = it == 0 ? -(double)INFINITY : (double)roc_unkey(r.kin[it - 1]);
        up = (double)INFINITY;
    }
}

// min(n - 1, #{s < low}) + min(n - 1, #{s > up}) in a sorted row: where the pointer loops of roc_curves.py:141-144 stop
__device__ __forceinline__ int roc_neg(const uint32_t* __restrict__ keys, long n, double low, double up) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((double)roc_unkey(keys[mid]) < low) lo = mid + 1; else hi = mid;
    }
    const long c_low = lo < n - 1 ? lo : n - 1;
    lo = 0; hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if ((double)roc_unkey(keys[mid]) > up) hi = mid; else lo = mid + 1;
    }
    const long c_up = n - lo < n - 1 ? n - lo : n - 1;
    return (int)(c_low + c_up);
}

// one thread per iteration of the reference's while loop (roc_curves.py:138-150); V = number of iterations it makes
__global__ __launch_bounds__(256) void roc_counts_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ kout,
                                                         const uint64_t* __restrict__ d, const double* __restrict__ c,
                                                         const int* __restrict__ modes, int* __restrict__ negin,
                                                         int* __restrict__ negout, int* __restrict__ V,
                                                         long n_in, long n_out, long Pin, long Pout) {
    const int m = blockIdx.y;
    const RocRow r = roc_row(m, kin, kout, d, c, modes, n_in, n_out, Pin, Pout);
    const long it = (long)blockIdx.x * 256 + threadIdx.x;
    if (it >= r.nt - 1) return;
    double low, up;
    roc_thresholds(r, it, low, up);
    if (!(low < up)) return;
    negin[(size_t)m * (n_in + 2) + it] = roc_neg(r.kin, n_in, low, up);
    negout[(size_t)m * (n_in + 2) + it] = roc_neg(r.kout, n_out, low, up);
    bool next = false;
    if (it + 1 < r.nt - 1) {
        roc_thresholds(r, it + 1, low, up);
        next = low < up;
    }
    if (!next) V[m] = (int)(it + 1);   // low is non-decreasing and up non-increasing: exactly one thread of the row gets here
}

// 2 n_in n_out AUC = sum_it (F[it] - F[it+1]) (T[it] + T[it+1]) over the visited points and the closing (0, 0)
// (roc_curves.py:202-205), F / T = counts of outs / ins kept.  Exact in 64-bit integers, so the order of the adds is free.
__global__ __launch_bounds__(256) void roc_auc_kernel(const int* __restrict__ negin, const int* __restrict__ negout,
                                                      const int* __restrict__ V, unsigned long long* __restrict__ acc,
                                                      long n_in, long n_out) {
    const int m = blockIdx.y, t = threadIdx.x;
    const long it = (long)blockIdx.x * 256 + t, v = V[m];
    const int* ni = negin + (size_t)m * (n_in + 2);
    const int* no = negout + (size_t)m * (n_in + 2);
    long long term = 0;
    if (it < v) {
        const long long F0 = n_out - no[it], T0 = n_in - ni[it];
        const long long F1 = it + 1 < v ? n_out - no[it + 1] : 0, T1 = it + 1 < v ? n_in - ni[it + 1] : 0;
        term = (F0 - F1) * (T0 + T1);
    }
    __shared__ unsigned long long red[256];
    red[t] = (unsigned long long)term;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0 && red[0]) atomicAdd(&acc[m], red[0]);
}

// The kept-TPR cursor (roc_curves.py:181-189), one thread per row.  The cursor sits on slot j from iteration `start`; it
// leaves at the first iteration e with tpr < kept[j] (which records nothing) and slot j keeps what iteration e - 1 wrote:
// its rates and the thresholds of iteration e.  tpr is non-increasing in `it` in all three modes (low never falls, up never
// rises): one binary search per slot.
__global__ __launch_bounds__(64) void roc_kept_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ kout,
                                                      const uint64_t* __restrict__ d, const double* __restrict__ c,
                                                      const int* __restrict__ modes, const int* __restrict__ negin,
                                                      const int* __restrict__ negout, const int* __restrict__ V,
                                                      const unsigned long long* __restrict__ acc,
                                                      const double* __restrict__ kept, double* __restrict__ auc,
                                                      double* __restrict__ kept_fpr, double* __restrict__ kept_tpr,
                                                      double* __restrict__ thr_low, double* __restrict__ thr_up,
                                                      int M, int K, long n_in, long n_out, long Pin, long Pout) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= M) return;
    const RocRow r = roc_row(m, kin, kout, d, c, modes, n_in, n_out, Pin, Pout);
    const int* ni = negin + (size_t)m * (n_in + 2);
    const int* no = negout + (size_t)m * (n_in + 2);
    const long v = V[m];
    for (int j = 0; j < K; ++j) {      // roc_curves.py:98-100
        kept_fpr[(size_t)m * K + j] = 1.0;
        kept_tpr[(size_t)m * K + j] = 0.0;
        thr_low[(size_t)m * K + j] = -(double)INFINITY;
        thr_up[(size_t)m * K + j] = (double)INFINITY;
    }
    long start = 0;
    for (int j = K - 1; j >= 0 && start < v; --j) {
        const double kt = kept[j];
        long lo = start, hi = v;
        while (lo < hi) {
            const long mid = (lo + hi) >> 1;
            const double tpr = 1.0 - (double)ni[mid] / (double)n_in;
            if (tpr < kt) hi = mid; else lo = mid + 1;
        }
        if (lo > start) {
            const long e = lo - 1;
            double low, up;
            roc_thresholds(r, e + 1, low, up);
            kept_fpr[(size_t)m * K + j] = 1.0 - (double)no[e] / (double)n_out;
            kept_tpr[(size_t)m * K + j] = 1.0 - (double)ni[e] / (double)n_in;
            thr_low[(size_t)m * K + j] = low;
            thr_up[(size_t)m * K + j] = up;
        }
        start = lo + 1;
    }
    auc[m] = (double)(long long)acc[m] / (2.0 * (double)n_in * (double)n_out);
}

}  // namespace

extern "C" {

size_t jvae_roc_workspace_bytes(int M, long n_in, long n_out) {
    if (M < 1 || n_in < 1 || n_out < 1 || n_in > ROC_MAX_N || n_out > ROC_MAX_N) return 0;
    return roc_ws(M, n_in, n_out).total;
}

int jvae_roc_curve_f32(const float* ins, const float* outs, const double* kept_tpr, const int* two_sided,
                       double* auc, double* kept_fpr, double* kept_tpr_out, double* thr_low, double* thr_up, int* status,
                       int M, long n_in, long n_out, int K, void* ws, size_t ws_bytes, void* stream) {
    if (!ins || !outs || !two_sided || !auc || !status || !ws || (K > 0 && (!kept_tpr || !kept_fpr || !kept_tpr_out || !thr_low || !thr_up)))
        return JVAE_EINVAL;
    if (M < 1 || M > 65535 || K < 0 || n_in < 1 || n_out < 1 || n_in > ROC_MAX_N || n_out > ROC_MAX_N) return JVAE_EINVAL;
    const RocWs w = roc_ws(M, n_in, n_out);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 7) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    uint32_t* kin = (uint32_t*)(base + w.kin);
    uint32_t* kout = (uint32_t*)(base + w.kout);
    uint64_t* d = (uint64_t*)(base + w.d);
    int* negin = (int*)(base + w.negin);
    int* negout = (int*)(base + w.negout);
    unsigned long long* acc = (unsigned long long*)(base + w.acc);
    double* c = (double*)(base + w.c);
    int* V = (int*)(base + w.V);
    const long Pin = roc_pad(n_in), Pout = roc_pad(n_out), Pmax = Pin > Pout ? Pin : Pout;

    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)M, st);
    if (e == hipSuccess) e = hipMemsetAsync(base + w.acc, 0, w.total - w.acc, st);      // acc, c, V
    if (e != hipSuccess) return (int)e;

    roc_keys_kernel<<<dim3((unsigned)cdiv(Pmax, 256), (unsigned)M, 2), 256, 0, st>>>(ins, outs, two_sided, kin, kout, status,
                                                                                     n_in, n_out, Pin, Pout);
    JVAE_LAUNCH_CHECK();
    int rc = roc_sort_rows<uint32_t>(kin, Pin, M, nullptr, st);
    if (rc == 0) rc = roc_sort_rows<uint32_t>(kout, Pout, M, nullptr, st);
    if (rc) return rc;
    // around-mean rows only (the kernels return at once on the others)
    roc_mean_kernel<<<M, 1024, 0, st>>>(ins, two_sided, c, n_in);
    JVAE_LAUNCH_CHECK();
    roc_delta_kernel<<<dim3((unsigned)cdiv(Pin, 256), (unsigned)M), 256, 0, st>>>(ins, two_sided, c, d, n_in, Pin);
    JVAE_LAUNCH_CHECK();
    rc = roc_sort_rows<uint64_t>(d, Pin, M, two_sided, st);
    if (rc) return rc;

    const dim3 its((unsigned)cdiv(n_in + 1, 256), (unsigned)M);
    roc_counts_kernel<<<its, 256, 0, st>>>(kin, kout, d, c, two_sided, negin, negout, V, n_in, n_out, Pin, Pout);
    JVAE_LAUNCH_CHECK();
    roc_auc_kernel<<<its, 256, 0, st>>>(negin, negout, V, acc, n_in, n_out);
    JVAE_LAUNCH_CHECK();
    roc_kept_kernel<<<cdiv(M, 64), 64, 0, st>>>(kin, kout, d, c, two_sided, negin, negout, V, acc, kept_tpr, auc, kept_fpr,
                                                kept_tpr_out, thr_low, thr_up, M, K, n_in, n_out, Pin, Pout);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
