// SCOD: selective classification in the presence of out-of-distribution data (reference tests/scod.py).  One rejection score
// (the HIGHer the more likely to REJECT) is applied to the union of the in-distribution test set and the OOD sets; sweeping it
// gives the selective risk and the false-positive rate as functions of the coverage.
//
// Score rows (scoring_r / scoring_g / scoring, scod.py:60-144): M variants (r kind, g kind, weight) of one recorded set in ONE
// launch, row m = r + weight * g with
//   r   0          (any name no branch of scoring_r matches, 'zdist' - the wim default - among them)
//       0.5 * v[y]                    'dist' (v = zdist), 'predist' (v = pre-zdist)
//       0.5 * zdist[y] - lse          'logmsp', lse = logsumexp_c(-0.5 zdist): a torch row the kernel reads
//       1 - v                         a recorded 'odin-*' row
//   g   0          (any model type but 'wim')
//       s * (k[y] - k@)               s = 1/2 for 'elbo' (k = zdist), -1 for 'iws', 1 for any other key
// y the estimated label of the sample.  Every product, difference and sum is rounded on its own (the torch expressions round
// each tensor operation): this file is built with floating-point contraction off, and says so again below.  A label outside
// [0, C) is never used as an index: its sample gets NaN and the status word is set to 1.
//
// Curves (scrisk, scod.py:17-57, and the figures of scod.py:231-235): per row, 64-bit keys - the sortable score bits in the high
// word (roc_key_canonical: -0 and +0 are one score), (position << 2) | {0 correct, 1 wrong, 2 ood} in the low word - go through
// the padded bitonic network of roc_sort.h: the order is the stable one, IEEE-equal scores by position, and the payload
// travels with the key.  One packed inclusive scan in sort order then gives the
// wrong and the in-distribution counts (both below 2^24: a 32-bit half each); the OOD count of position i is i + 1 minus the
// in count.  tpr = in / n_in, fpr = ood / n_ood, selective_risk = wrong / in (0 / 0 -> 0): correctly rounded fp32 divisions of
// integers below 2^24, which fp32 holds exactly.  The scan is tile totals, one exclusive scan of the totals per row, tile scan.
// Figures: min of fpr and of selective_risk over tpr >= 0.95 (fp32 comparison, as torch makes it), and the trapezoids of
// (fpr, tpr), (tpr, sr) and (tpr, 0.5 sr + 0.5 fpr) in fp64 over the fp32 curve values: every term (x1 - x0) (y1 + y0) / 2 has
// the bits of numpy's, the terms are summed by a fixed tree per tile and a fixed walk over the tiles.  No float atomics;
// the same bits run to run.  The number of launches depends on the padded row length alone, not on M.
#include "common.h"
#include "jvae_internal.h"
#include "roc_sort.h"

#pragma clang fp contract(off)

namespace {

constexpr int SCOD_BLOCK = 256;
constexpr int SCOD_MAX_ROWS = 32;      // variants per score launch (the arguments travel by value)
constexpr long SCOD_MAX_N = 1L << 30;  // samples per score launch

enum { SCOD_SKIP = -1 };               // r kind: the row is g alone (unweighted); g kind: the row is r alone
enum { SCOD_R_ZERO = 0, SCOD_R_HALF_Y = 1, SCOD_R_LOGMSP = 2, SCOD_R_ODIN = 3 };
enum { SCOD_G_ZERO = 0, SCOD_G_HALF = 1, SCOD_G_NEG = 2, SCOD_G_PLAIN = 3 };

struct ScodArgs {
    const float* r_src[SCOD_MAX_ROWS];  // (C, N) for HALF_Y / LOGMSP, (N,) for ODIN
    const float* r_aux[SCOD_MAX_ROWS];  // (N,) the log-sum-exp row of LOGMSP
    const float* g_src[SCOD_MAX_ROWS];  // (C, N)
    const float* g_alt[SCOD_MAX_ROWS];  // (N,)
    float weight[SCOD_MAX_ROWS];
    signed char r_kind[SCOD_MAX_ROWS], g_kind[SCOD_MAX_ROWS];
};

__global__ __launch_bounds__(SCOD_BLOCK) void scod_scores_kernel(ScodArgs a, const long long* __restrict__ y_est,
                                                                 float* __restrict__ out, int* __restrict__ status, int C, long N,
                                                                 long out_stride) {
    const long n = (long)blockIdx.x * SCOD_BLOCK + threadIdx.x;
    if (n >= N) return;
    const int m = blockIdx.y, rk = a.r_kind[m], gk = a.g_kind[m];
    const bool gather = rk == SCOD_R_HALF_Y || rk == SCOD_R_LOGMSP || gk > SCOD_G_ZERO;
    long long y = 0;
    bool ok = true;
    if (gather) {
        y = y_est[n];
        ok = y >= 0 && y < (long long)C;
        if (!ok) *status = 1;          // every writer stores the same word
    }
    float r = 0.f;
    if (rk == SCOD_R_HALF_Y || rk == SCOD_R_LOGMSP) {
        r = ok ? 0.5f * a.r_src[m][(size_t)y * N + n] : NAN;
        if (rk == SCOD_R_LOGMSP) r = r - a.r_aux[m][n];
    } else if (rk == SCOD_R_ODIN) {
        r = 1.f - a.r_src[m][n];
    }
    float g = 0.f;
    if (gk > SCOD_G_ZERO) {
        const float d = ok ? a.g_src[m][(size_t)y * N + n] - a.g_alt[m][n] : NAN;
        g = gk == SCOD_G_HALF ? 0.5f * d : (gk == SCOD_G_NEG ? -d : d);
    }
    float res;
    if (gk == SCOD_SKIP) res = r;
    else if (rk == SCOD_SKIP) res = g;
    else {
        const float wg = a.weight[m] * g;          // rounded, then added: never one fused operation
        res = r + wg;
    }
    out[(size_t)m * out_stride + n] = res;
}

// ---------------------------------------------------------------------------------------------------------------- curves
typedef unsigned long long u64;

struct ScodWs {                        // carve-up of the caller's workspace (all offsets multiples of 256 bytes)
    size_t keys, off, area, mins, total;
};
inline size_t scod_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline ScodWs scod_ws(int M, long n) {
    const size_t P = (size_t)roc_pad(n), T = P / ROC_TILE;
    ScodWs w;
    size_t o = 0;
    w.keys = o; o += scod_align(sizeof(u64) * P * M);
    w.off = o;  o += scod_align(sizeof(u64) * T * M);          // tile totals, then their exclusive scan, wrong << 32 | in
    w.area = o; o += scod_align(sizeof(double) * 3 * T * M);   // per tile: the three trapezoid sums
    w.mins = o; o += scod_align(sizeof(float) * 2 * T * M);    // per tile: min fpr, min selective risk over tpr >= 0.95
    w.total = o;
    return w;
}

// low word of a key -> wrong << 32 | in (the padding's low word reads 3: neither)
__device__ __forceinline__ u64 scod_flags(u64 key) {
    const unsigned code = (unsigned)key & 3u;
    return (code < 2u ? 1ull : 0ull) | (code == 1u ? 1ull << 32 : 0ull);
}

__global__ __launch_bounds__(256) void scod_keys_kernel(const float* __restrict__ scores, const long long* __restrict__ y_true,
                                                        const long long* __restrict__ y_est, u64* __restrict__ keys,
                                                        int* __restrict__ status, long n, long P) {
    const int m = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    u64 key = ~0ull;
    if (i < n) {
        const float v = scores[(size_t)m * n + i];
        const long long yt = y_true[i];
        const unsigned code = yt < 0 ? 2u : (yt != y_est[i] ? 1u : 0u);
        key = ((u64)roc_key_canonical(v) << 32) | (u64)(((unsigned)i << 2) | code);    // -0 and +0: equal, so by position
        if (v != v) atomicOr(&status[m], 1);       // an integer flag: the result does not depend on the order
    }
    keys[(size_t)m * P + i] = key;
}

// fixed-order reduction over a workgroup of 1024: xor butterfly inside each wave, then the 16 wave results in sequence
template <typename T, typename Op>
__device__ __forceinline__ T scod_block_reduce(T v, T* red, Op op) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    T r = red[0];
    for (int i = 1; i < nw; ++i) r = op(r, red[i]);
    return r;
}

// inclusive scan over a workgroup of 1024 (s: 2048 words of LDS); the packed halves never carry into each other (< 2^24)
__device__ __forceinline__ u64 scod_block_scan(u64 v, u64* s) {
    const int t = threadIdx.x;
    int cur = 0;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        u64 x = s[cur * 1024 + t];
        if (t >= o) x += s[cur * 1024 + t - o];
        cur ^= 1;
        s[cur * 1024 + t] = x;
        __syncthreads();
    }
    return s[cur * 1024 + t];
}

__global__ __launch_bounds__(ROC_TILE_THREADS) void scod_tile_totals_kernel(const u64* __restrict__ keys, u64* __restrict__ off,
                                                                            long P) {
    __shared__ u64 red[16];
    const int t = threadIdx.x;
    const long T = P / ROC_TILE;
    const u64* row = keys + (size_t)blockIdx.y * P + (size_t)blockIdx.x * ROC_TILE;
    const u64 v = scod_flags(row[t]) + scod_flags(row[t + ROC_TILE_THREADS]);
    const u64 sum = scod_block_reduce(v, red, [](u64 a, u64 b) { return a + b; });
    if (t == 0) off[(size_t)blockIdx.y * T + blockIdx.x] = sum;
}

// per row: tile totals -> their exclusive scan, in place; the grand total must show n_in in-distribution samples
__global__ __launch_bounds__(1024) void scod_offsets_kernel(u64* __restrict__ off, int* __restrict__ status, long T, long n_in) {
    __shared__ u64 s[2048];
    const int t = threadIdx.x;
    u64* row = off + (size_t)blockIdx.x * T;
    const long per = (T + 1023) / 1024, lo = (long)t * per, hi = lo + per < T ? lo + per : T;
    u64 sum = 0;
    for (long i = lo; i < hi; ++i) sum += row[i];
    const u64 incl = scod_block_scan(sum, s);
    u64 run = incl - sum;
    for (long i = lo; i < hi; ++i) {
        const u64 v = row[i];
        row[i] = run;
        run += v;
    }
    if (t == 1023 && (long)(unsigned)incl != n_in) atomicOr(&status[blockIdx.x], 2);
}

struct ScodPoint { float tpr, sr, fpr, half; };
__device__ __forceinline__ ScodPoint scod_point(u64 cum, long count, float n_in, float n_ood) {
    const unsigned in_c = (unsigned)cum, wrong_c = (unsigned)(cum >> 32), ood_c = (unsigned)count - in_c;
    ScodPoint p;
    p.tpr = (float)in_c / n_in;
    p.fpr = (float)ood_c / n_ood;
    p.sr = in_c ? (float)wrong_c / (float)in_c : 0.f;
    const float a = 0.5f * p.sr, b = 0.5f * p.fpr;
    p.half = a + b;                    // 0.5 * sr + 0.5 * fpr, formed in fp32
    return p;
}

struct ScodAcc { double roc = 0., st = 0., scodt = 0.; float fpr95 = INFINITY, sr95 = INFINITY; };
__device__ __forceinline__ void scod_visit(ScodAcc& a, const ScodPoint& p, const ScodPoint& q, bool has_prev) {
    if (has_prev) {                    // numpy's trapezoid term of (p -> q): d * (y1 + y0) / 2
        const double dx_roc = (double)q.fpr - (double)p.fpr, dx = (double)q.tpr - (double)p.tpr;
        const double t_roc = dx_roc * ((double)q.tpr + (double)p.tpr), t_st = dx * ((double)q.sr + (double)p.sr);
        const double t_scodt = dx * ((double)q.half + (double)p.half);
        a.roc += t_roc * 0.5;
        a.st += t_st * 0.5;
        a.scodt += t_scodt * 0.5;
    }
    if (q.tpr >= 0.95f) {
        a.fpr95 = fminf(a.fpr95, q.fpr);
        a.sr95 = fminf(a.sr95, q.sr);
    }
}

// Tile scan, curve values, per-tile partial figures.  A thread owns the sorted positions base + 2t, base + 2t + 1.
__global__ __launch_bounds__(ROC_TILE_THREADS) void scod_curves_kernel(const u64* __restrict__ keys, const u64* __restrict__ off,
                                                                       float* __restrict__ curves, double* __restrict__ area,
                                                                       float* __restrict__ mins, int M, long n, long P, long n_in) {
    __shared__ u64 s[2048];
    __shared__ double redd[16];
    __shared__ float redf[16];
    const int t = threadIdx.x, m = blockIdx.y;
    const long T = P / ROC_TILE, base = (long)blockIdx.x * ROC_TILE, i0 = base + 2 * t;
    const u64* row = keys + (size_t)m * P + base;
    const u64 f0 = scod_flags(row[2 * t]), f1 = scod_flags(row[2 * t + 1]);
    const u64 incl = scod_block_scan(f0 + f1, s);
    const u64 before = off[(size_t)m * T + blockIdx.x] + incl - (f0 + f1);
    const float fin = (float)n_in, food = (float)(n - n_in);
    ScodAcc acc;
    if (i0 < n) {
        const ScodPoint prev = scod_point(before, i0, fin, food);          // position i0 - 1 (unused for i0 == 0)
        const ScodPoint p0 = scod_point(before + f0, i0 + 1, fin, food);
        scod_visit(acc, prev, p0, i0 > 0);
        if (curves) {
            curves[((size_t)0 * M + m) * n + i0] = p0.tpr;
            curves[((size_t)1 * M + m) * n + i0] = p0.sr;
            curves[((size_t)2 * M + m) * n + i0] = p0.fpr;
        }
        if (i0 + 1 < n) {
            const ScodPoint p1 = scod_point(before + f0 + f1, i0 + 2, fin, food);
            scod_visit(acc, p0, p1, true);
            if (curves) {
                curves[((size_t)0 * M + m) * n + i0 + 1] = p1.tpr;
                curves[((size_t)1 * M + m) * n + i0 + 1] = p1.sr;
                curves[((size_t)2 * M + m) * n + i0 + 1] = p1.fpr;
            }
        }
    }
    const auto add = [](double a, double b) { return a + b; };
    const auto low = [](float a, float b) { return fminf(a, b); };
    const double roc = scod_block_reduce(acc.roc, redd, add);
    const double st = scod_block_reduce(acc.st, redd, add);
    const double scodt = scod_block_reduce(acc.scodt, redd, add);
    const float fpr95 = scod_block_reduce(acc.fpr95, redf, low);
    const float sr95 = scod_block_reduce(acc.sr95, redf, low);
    if (t == 0) {
        const size_t tile = (size_t)m * T + blockIdx.x;
        area[3 * tile] = roc;
        area[3 * tile + 1] = st;
        area[3 * tile + 2] = scodt;
        mins[2 * tile] = fpr95;
        mins[2 * tile + 1] = sr95;
    }
}

// per row: the tiles' partial figures in a fixed order -> figures[m] = fpr95, sr95, auroc, aust, auscodt
__global__ __launch_bounds__(1024) void scod_figures_kernel(const double* __restrict__ area, const float* __restrict__ mins,
                                                            double* __restrict__ figures, long T) {
    __shared__ double redd[16];
    __shared__ float redf[16];
    const int t = threadIdx.x, m = blockIdx.x;
    double a[3] = {0., 0., 0.};
    float lo[2] = {INFINITY, INFINITY};
    for (long i = t; i < T; i += 1024) {
        const size_t tile = (size_t)m * T + i;
        for (int k = 0; k < 3; ++k) a[k] += area[3 * tile + k];
        for (int k = 0; k < 2; ++k) lo[k] = fminf(lo[k], mins[2 * tile + k]);
    }
    const auto add = [](double x, double y) { return x + y; };
    const auto low = [](float x, float y) { return fminf(x, y); };
    for (int k = 0; k < 3; ++k) a[k] = scod_block_reduce(a[k], redd, add);
    for (int k = 0; k < 2; ++k) lo[k] = scod_block_reduce(lo[k], redf, low);
    if (t == 0) {
        figures[5 * (size_t)m] = (double)lo[0];
        figures[5 * (size_t)m + 1] = (double)lo[1];
        for (int k = 0; k < 3; ++k) figures[5 * (size_t)m + 2 + k] = a[k];
    }
}

}  // namespace

extern "C" {

int jvae_scod_scores_f32(const float* const* r_src, const float* const* r_aux, const float* const* g_src,
                         const float* const* g_alt, const int* kinds, const float* weights, const long long* y_est,
                         float* out, long out_stride, int M, int C, long N, int* status, void* stream) {
    if (!r_src || !r_aux || !g_src || !g_alt || !kinds || !weights || !out || !status) return JVAE_EINVAL;
    if (M < 0 || M > SCOD_MAX_ROWS || N < 0 || N > SCOD_MAX_N || out_stride < N || C < 1) return JVAE_EINVAL;
    ScodArgs a;
    for (int m = 0; m < SCOD_MAX_ROWS; ++m) {
        a.r_src[m] = a.r_aux[m] = a.g_src[m] = a.g_alt[m] = nullptr;
        a.weight[m] = 0.f;
        a.r_kind[m] = a.g_kind[m] = 0;
        if (m >= M) continue;
        const int rk = kinds[2 * m], gk = kinds[2 * m + 1];
        if (rk < SCOD_SKIP || rk > SCOD_R_ODIN || gk < SCOD_SKIP || gk > SCOD_G_PLAIN || (rk == SCOD_SKIP && gk == SCOD_SKIP))
            return JVAE_EINVAL;
        if ((rk > SCOD_R_ZERO && !r_src[m]) || (rk == SCOD_R_LOGMSP && !r_aux[m]) || (gk > SCOD_G_ZERO && (!g_src[m] || !g_alt[m])))
            return JVAE_EINVAL;
        if ((rk == SCOD_R_HALF_Y || rk == SCOD_R_LOGMSP || gk > SCOD_G_ZERO) && !y_est) return JVAE_EINVAL;
        a.r_src[m] = r_src[m]; a.r_aux[m] = r_aux[m]; a.g_src[m] = g_src[m]; a.g_alt[m] = g_alt[m];
        a.weight[m] = weights[m];
        a.r_kind[m] = (signed char)rk;
        a.g_kind[m] = (signed char)gk;
    }
    if (M == 0 || N == 0) return 0;
    scod_scores_kernel<<<dim3((unsigned)cdiv(N, SCOD_BLOCK), (unsigned)M), SCOD_BLOCK, 0, (hipStream_t)stream>>>(
        a, y_est, out, status, C, N, out_stride);
    JVAE_LAUNCH_CHECK();
    return 0;
}

size_t jvae_scod_workspace_bytes(int M, long n) {
    if (M < 1 || M > 65535 || n < 2 || n > ROC_MAX_N) return 0;
    return scod_ws(M, n).total;
}

int jvae_scod_curve_f32(const float* scores, const long long* y_true, const long long* y_est, float* curves, double* figures,
                        int* status, int M, long n, long n_in, void* ws, size_t ws_bytes, void* stream) {
    if (!scores || !y_true || !y_est || !status || !ws || (!curves && !figures)) return JVAE_EINVAL;
    if (M < 1 || M > 65535 || n < 2 || n > ROC_MAX_N || n_in < 1 || n_in >= n) return JVAE_EINVAL;
    const ScodWs w = scod_ws(M, n);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 15) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    u64* keys = (u64*)(base + w.keys);
    u64* off = (u64*)(base + w.off);
    double* area = (double*)(base + w.area);
    float* mins = (float*)(base + w.mins);
    const long P = roc_pad(n), T = P / ROC_TILE;

    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)M, st);
    if (e != hipSuccess) return (int)e;
    scod_keys_kernel<<<dim3((unsigned)cdiv(P, 256), (unsigned)M), 256, 0, st>>>(scores, y_true, y_est, keys, status, n, P);
    JVAE_LAUNCH_CHECK();
    const int rc = roc_sort_rows<u64>(keys, P, M, nullptr, st);
    if (rc) return rc;
    const dim3 tiles((unsigned)T, (unsigned)M);
    scod_tile_totals_kernel<<<tiles, ROC_TILE_THREADS, 0, st>>>(keys, off, P);
    JVAE_LAUNCH_CHECK();
    scod_offsets_kernel<<<M, 1024, 0, st>>>(off, status, T, n_in);
    JVAE_LAUNCH_CHECK();
    scod_curves_kernel<<<tiles, ROC_TILE_THREADS, 0, st>>>(keys, off, curves, area, mins, M, n, P, n_in);
    JVAE_LAUNCH_CHECK();
    if (figures) {
        scod_figures_kernel<<<M, 1024, 0, st>>>(area, mins, figures, T);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
