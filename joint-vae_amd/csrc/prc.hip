// Device-side precision-recall figures of OOD scores: AUPR-in / AUPR-out (scikit-learn's average_precision_score), the
// trapezoid AUCPR of both sides (auc(recall, precision) of precision_recall_curve) and the smallest detection error, for M
// score rows in one call.  The companions of the ROC (roc.hip) in the tables of the OOD literature (ODIN: FPR@95, detection
// error, AUROC, AUPR-in, AUPR-out); the reference's tests/test_misclassification_and_ood.py asks for the AUCPR.
//
// With the scores widened exactly to fp64, every figure has terms only at the DISTINCT scores v of the positive row.  For
// the in-side, with tp = #{ins >= v}, fp = #{outs >= v}, tp' = #{ins > v}, fp' = #{outs > v}:
//   dR = (tp - tp') / n_in,  P = tp / (tp + fp),  P' = tp' / (tp' + fp')  (1 when tp' + fp' = 0)
//   aupr_in  = sum dR * P                 aucpr_in = sum dR * (P + P') / 2
//   dete     = min(0.5, min_v 0.5 * (n_in - tp) / n_in + 0.5 * fp / n_out)
// and the out-side figures are the same sweep over the distinct out-scores with the rows swapped and <= / < (out = positive,
// score negated).  Both rows are sorted once; a thread that sits on the first element of a tie group of its row finds the
// group's end and the two counts in the other row by binary search - every search runs over [0, n), never into the padding.
//
// Keys are 64-bit in every mode, ascending: mode 0 the order-preserving image of the fp32 score with -0 canonicalised to +0
// (IEEE-equal scores are ONE tie group, as for numpy), mode 1 ('around-mean', score = -|s - c|) the bit pattern of the fp64
// distance |s - c|, c from roc_mean_kernel - ascending distance is descending score, so the roles of >= and <= swap instead
// of the keys being inverted (the image of distance 0 would be the padding key).  Mode 2 (quantile rows) has no scalar score:
// five NaNs.  Sums: fp64, an LDS tree per workgroup, then the partials in index order by one thread - no float atomics.
#include "common.h"
#include "jvae_internal.h"
#include "roc_sort.h"                  // roc_pad, roc_key_canonical, roc_decode, roc_mean_kernel, roc_sort_rows, ROC_MAX_N

namespace {

constexpr int PRC_THREADS = 256;       // threads (= sorted elements) per workgroup of the sweep

struct PrcWs {                         // carve-up of the caller's workspace (all offsets multiples of 256 bytes)
    size_t kin, kout, c, part, total;
};
inline size_t prc_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline long prc_blocks(long n_in, long n_out) { return cdiv(n_in > n_out ? n_in : n_out, PRC_THREADS); }
inline PrcWs prc_ws(int M, long n_in, long n_out) {
    const size_t Pin = (size_t)roc_pad(n_in), Pout = (size_t)roc_pad(n_out);
    PrcWs w;
    size_t o = 0;
    w.kin = o;  o += prc_align(sizeof(uint64_t) * Pin * M);
    w.kout = o; o += prc_align(sizeof(uint64_t) * Pout * M);
    w.c = o;    o += prc_align(sizeof(double) * M);
    w.part = o; o += prc_align(sizeof(double) * 3 * 2 * (size_t)prc_blocks(n_in, n_out) * M);
    w.total = o;
    return w;
}

// keys of both row sets (z = 0: ins, 1: outs) + the status word of the ROC (bit 0: NaN score, bit 1: non-finite in-score of
// an around-mean row, bit 2: malformed mode word, whose row runs as a one-sided one).  A quantile row sets nothing.
__global__ __launch_bounds__(256) void prc_keys_kernel(const float* __restrict__ ins, const float* __restrict__ outs,
                                                       const int* __restrict__ modes, const double* __restrict__ c,
                                                       uint64_t* __restrict__ kin, uint64_t* __restrict__ kout,
                                                       int* __restrict__ status, long n_in, long n_out, long Pin, long Pout) {
    const int m = blockIdx.y, z = blockIdx.z;
    const long n = z ? n_out : n_in, P = z ? Pout : Pin;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    int f_low, f_up;
    const int kind = roc_decode(modes[m], f_low, f_up);
    uint64_t key = ~(uint64_t)0;
    int bad = 0;
    if (i < n) {
        const float v = (z ? outs : ins)[(size_t)m * n + i];
        if (kind == 1) {
            key = (uint64_t)__double_as_longlong(fabs((double)v - c[m]));
            if (z == 0 && !isfinite(v)) bad |= 2;
        } else {
            key = (uint64_t)roc_key_canonical(v);                      // -0 and +0: one key
        }
        if (v != v) bad |= 1;
    }
    if (z == 0 && i == 0 && kind < 0) bad |= 4;
    (z ? kout : kin)[(size_t)m * P + i] = key;
    if (bad && kind != 2) atomicOr(&status[m], bad);
}

// first index of the ascending keys[lo, hi) with keys[i] >= k (STRICT: > k); hi when there is none
template <bool STRICT>
__device__ __forceinline__ long prc_bound(const uint64_t* __restrict__ keys, long lo, long hi, uint64_t k) {
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        const uint64_t v = keys[mid];
        if (STRICT ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The sweep of one side (z = 0: in = positive, 1: out = positive with the score negated): one thread per element of the sorted
// positive row a; the first thread of each tie group forms the group's terms.  part[m][z][block] = {sum dR * P,
// sum dR * (P + P') / 2, min detection error (z = 0; 0.5 where there is none)}.
__global__ __launch_bounds__(PRC_THREADS) void prc_sweep_kernel(const uint64_t* __restrict__ kin, const uint64_t* __restrict__ kout,
                                                                const int* __restrict__ modes, double* __restrict__ part,
                                                                long n_in, long n_out, long Pin, long Pout, long nblk) {
    const int m = blockIdx.y, z = blockIdx.z, t = threadIdx.x;
    const long na = z ? n_out : n_in, nb = z ? n_in : n_out;
    if ((long)blockIdx.x * PRC_THREADS >= na) return;                  // the whole workgroup: nothing of this side is here
    const uint64_t* a = (z ? kout + (size_t)m * Pout : kin + (size_t)m * Pin);
    const uint64_t* b = (z ? kin + (size_t)m * Pin : kout + (size_t)m * Pout);
    // kept = score >= v on the in-side, <= v on the out-side; the keys of an around-mean row run against the score
    const bool upper = (z == 0) != (modes[m] == 1);
    const long i = (long)blockIdx.x * PRC_THREADS + t;
    double ap = 0.0, trap = 0.0, err = 0.5;
    if (i < na) {
        const uint64_t k = a[i];
        if (i == 0 || a[i - 1] != k) {
            const long a_lt = i, a_le = prc_bound<true>(a, i + 1, na, k);
            const long b_lt = prc_bound<false>(b, 0, nb, k), b_le = prc_bound<true>(b, b_lt, nb, k);
            const long tp = upper ? na - a_lt : a_le, tq = upper ? na - a_le : a_lt;      // tq, fq: tp', fp'
            const long fp = upper ? nb - b_lt : b_le, fq = upper ? nb - b_le : b_lt;
            const double dR = (double)(tp - tq) / (double)na;
            const double P = (double)tp / (double)(tp + fp);
            const double Q = tq + fq ? (double)tq / (double)(tq + fq) : 1.0;
            ap = dR * P;
            trap = dR * (P + Q) / 2.0;
            if (z == 0) err = 0.5 * ((double)(na - tp) / (double)na) + 0.5 * ((double)fp / (double)nb);
        }
    }
    __shared__ double s_ap[PRC_THREADS], s_trap[PRC_THREADS], s_err[PRC_THREADS];
    s_ap[t] = ap; s_trap[t] = trap; s_err[t] = err;
    __syncthreads();
    for (int o = PRC_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) {
            s_ap[t] += s_ap[t + o];
            s_trap[t] += s_trap[t + o];
            s_err[t] = fmin(s_err[t], s_err[t + o]);
        }
        __syncthreads();
    }
    if (t == 0) {
        double* p = part + (((size_t)m * 2 + z) * nblk + blockIdx.x) * 3;
        p[0] = s_ap[0]; p[1] = s_trap[0]; p[2] = s_err[0];
    }
}

// figures[m] = {aupr_in, aupr_out, aucpr_in, aucpr_out, dete}: thread f of row m folds one figure's partials in index order
__global__ __launch_bounds__(64) void prc_fold_kernel(const double* __restrict__ part, const int* __restrict__ modes,
                                                      double* __restrict__ figures, long n_in, long n_out, long nblk) {
    const int m = blockIdx.x, f = threadIdx.x;
    if (f >= 5) return;
    int f_low, f_up;
    if (roc_decode(modes[m], f_low, f_up) == 2) {
        figures[(size_t)m * 5 + f] = __longlong_as_double(0x7FF8000000000000LL);
        return;
    }
    const int z = f & 1 & (f < 4), slot = f >> 1;
    const long nb = ((z ? n_out : n_in) + PRC_THREADS - 1) / PRC_THREADS;
    const double* p = part + ((size_t)m * 2 + z) * nblk * 3 + slot;
    double acc = slot == 2 ? 0.5 : 0.0;
    for (long b = 0; b < nb; ++b) acc = slot == 2 ? fmin(acc, p[b * 3]) : acc + p[b * 3];
    figures[(size_t)m * 5 + f] = acc;
}

}  // namespace

extern "C" {

size_t jvae_pr_workspace_bytes(int M, long n_in, long n_out) {
    if (M < 1 || M > 65535 || n_in < 1 || n_out < 1 || n_in > ROC_MAX_N || n_out > ROC_MAX_N) return 0;
    return prc_ws(M, n_in, n_out).total;
}

int jvae_pr_metrics_f32(const float* ins, const float* outs, const int* modes, double* figures, int* status,
                        int M, long n_in, long n_out, void* ws, size_t ws_bytes, void* stream) {
    if (!ins || !outs || !modes || !figures || !status || !ws) return JVAE_EINVAL;
    if (M < 1 || M > 65535 || n_in < 1 || n_out < 1 || n_in > ROC_MAX_N || n_out > ROC_MAX_N) return JVAE_EINVAL;
    const PrcWs w = prc_ws(M, n_in, n_out);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 7) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    uint64_t* kin = (uint64_t*)(base + w.kin);
    uint64_t* kout = (uint64_t*)(base + w.kout);
    double* c = (double*)(base + w.c);
    double* part = (double*)(base + w.part);
    const long Pin = roc_pad(n_in), Pout = roc_pad(n_out), Pmax = Pin > Pout ? Pin : Pout, nblk = prc_blocks(n_in, n_out);

    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)M, st);
    if (e != hipSuccess) return (int)e;
    roc_mean_kernel<<<M, 1024, 0, st>>>(ins, modes, c, n_in);          // around-mean rows only
    JVAE_LAUNCH_CHECK();
    prc_keys_kernel<<<dim3((unsigned)cdiv(Pmax, 256), (unsigned)M, 2), 256, 0, st>>>(ins, outs, modes, c, kin, kout, status,
                                                                                     n_in, n_out, Pin, Pout);
    JVAE_LAUNCH_CHECK();
    int rc = roc_sort_rows<uint64_t>(kin, Pin, M, nullptr, st);
    if (rc == 0) rc = roc_sort_rows<uint64_t>(kout, Pout, M, nullptr, st);
    if (rc) return rc;
    prc_sweep_kernel<<<dim3((unsigned)nblk, (unsigned)M, 2), PRC_THREADS, 0, st>>>(kin, kout, modes, part, n_in, n_out, Pin, Pout,
                                                                                   nblk);
    JVAE_LAUNCH_CHECK();
    prc_fold_kernel<<<M, 64, 0, st>>>(part, modes, figures, n_in, n_out, nblk);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
