// Semi-supervised training: the class-marginal KL of the unlabelled rows of a training batch (the bound of
// Hershey & Olsen 2007 for the KL between a Gaussian and a Gaussian mixture; no counterpart in the reference).
//
// A row with a label y >= 0 keeps the kl / zdist / var_kl the latent kernel gave it, bit for bit, and its row of r is one-hot on
// its label (all zero for a label >= C, which is never an index).  A row with y < 0 has no class: with q = N(mu, diag e^lv),
// p_c = N(m_c, (T_c^T T_c)^-1) and weights pi_c
//
//   d_c  = sum_k t_ck^2 (mu_k - m_ck)^2                                  the direct form, never the expanded Gram form
//   v_c  = sum_k e^lv_k t_ck^2 - sum_k lv_k - sum_k log t_ck^2 - K        (GaussianPrior.kl's distance and var_kl)
//   KL_c = 1/2 (d_c + w v_c),   Q_c = KL_c - log pi_c
//   U    = -log sum_c exp(-Q_c) = a - log s,   a = min_c Q_c,  s = sum_c exp(-(Q_c - a))
//   r_c  = exp(-(Q_c - a)) / s,     kl = U,  zdist = sum_c r_c d_c,  var_kl = sum_c r_c v_c
//
// Everything between the fp32 operands and the ONE rounding of an output is fp64: t^2 = t t and mu - m are exact there, so a
// class a thousand units away loses nothing to the class next door.
//
// Forward, ONE launch (ss_fwd_kernel): a workgroup owns SS_ROWS rows, a wave SS_RW of them, a lane one class of the staged tile.
// The means and t^2 of SS_CT classes x SS_KC coordinates are staged k-major in LDS (a whole (C, K) table is never assumed to
// fit); a wave stages mu and e^lv of its rows beside them; every lane walks the chunk for its class.  At the end of a class tile the
// wave folds (a, s, s_d, s_v) as aggpost_core.h folds its pairs: the tile's smallest Q shifts the tile's sum, the smaller of the
// two shifts rescales the other side, one factor is exactly 1.  Q is parked in the call's workspace (fp64, (N, C)) by the lane
// that reads it back for r once (a, s) are final.  A workgroup without an unlabelled row stages nothing.
//
// Backward, two launches, g = d loss / d kl:
//   ss_bwd_rows_kernel  a wave per row, lanes over k, c ascending: g_mu = g sum_c r_c t_c^2 (mu - m_c),
//                       g_lv = g w/2 (e^lv sum_c r_c t_c^2 - 1); a labelled row: zeros, and g goes back to the incoming kl
//   ss_bwd_cols_kernel  a thread per (c, k), 16 contiguous chunks of rows in row order, the chunks folded in chunk order (the
//                       partition of class_fold.h): g_means = -t^2 sum_n g r (mu - m), g_T = sum_n g r (t ((mu - m)^2 + w e^lv) - w / t)
// fp64 fma chains from fp32 operands (r is the fp32 the forward returned), fixed orders, no atomics: the same bits every run.
#include <math.h>
#include "common.h"
#include "jvae_hip.h"

#define SS_MAX_K 1024
#define SS_MAX_C 1024
#define SS_MAX_N (1 << 20)
#define SS_CT 64                   // classes of a staged tile: one per lane
#define SS_KC 32                   // coordinates of a staged chunk
#define SS_RW 2                    // rows of a wave
#define SS_WAVES 4
#define SS_ROWS (SS_WAVES * SS_RW)
#define SS_CHUNKS 16               // column pass: row chunks of an output

namespace {

enum { VAR_SCALAR = 0, VAR_DIAG = 1 };

struct SsP {
    const float* mu;        // (N, K)
    const float* lv;        // (N, K), clipped
    const long long* y;     // (N,), < 0: unlabelled
    const float* means;     // (C, K)
    const float* T;         // (C,) | (C, K)
    const double* log_pi;   // (C,) or null: uniform
    int var_dim, N, K, C;
    float w;
};

bool ss_in_range(long N, long K, long C) { return N >= 0 && N <= SS_MAX_N && K >= 1 && K <= SS_MAX_K && C >= 1 && C <= SS_MAX_C; }

__device__ __forceinline__ double wave_min64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void ss_fwd_kernel(SsP p, const float* __restrict__ kl_in, const float* __restrict__ zd_in,
                                                     const float* __restrict__ vkl_in, float* __restrict__ kl,
                                                     float* __restrict__ zd, float* __restrict__ vkl, float* __restrict__ r,
                                                     double* __restrict__ qws) {
    __shared__ float mt[SS_KC][SS_CT + 1];             // + 1: the transposing store walks c at a stride of 65 words
    __shared__ double tt[SS_KC][SS_CT + 1];
    __shared__ double rm[SS_WAVES][SS_RW][SS_KC], re[SS_WAVES][SS_RW][SS_KC];
    __shared__ double ld[SS_WAVES][SS_CT];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = p.N, K = p.K, C = p.C;
    const long n0 = (long)blockIdx.x * SS_ROWS;
    long row[SS_RW];
    bool unl[SS_RW];
    bool any = false;                                  // block-uniform: does the workgroup own an unlabelled row?
    for (int j = 0; j < SS_ROWS; ++j) any |= n0 + j < N && p.y[n0 + j] < 0;
#pragma unroll
    for (int j = 0; j < SS_RW; ++j) {
        row[j] = n0 + wv * SS_RW + j;
        unl[j] = row[j] < N && p.y[row[j]] < 0;        // wave-uniform
        if (row[j] < N && !unl[j]) {                   // a labelled row passes through with its bits
            const long n = row[j];
            const long long cls = p.y[n];
            if (lane == 0) { kl[n] = kl_in[n]; zd[n] = zd_in[n]; vkl[n] = vkl_in[n]; }
            for (int c = lane; c < C; c += 64) r[n * C + c] = (long long)c == cls ? 1.f : 0.f;
        }
    }
    if (!any) return;

    const double w = (double)p.w;
    double a[SS_RW], s[SS_RW], sd[SS_RW], sv[SS_RW], slv[SS_RW];
#pragma unroll
    for (int j = 0; j < SS_RW; ++j) { a[j] = INFINITY; s[j] = 0.; sd[j] = 0.; sv[j] = 0.; slv[j] = 0.; }

    for (int c0 = 0; c0 < C; c0 += SS_CT) {
        double d[SS_RW], tr[SS_RW], slog = 0.;
#pragma unroll
        for (int j = 0; j < SS_RW; ++j) { d[j] = 0.; tr[j] = 0.; }
        for (int kc = 0; kc < K; kc += SS_KC) {
            const int kn = K - kc < SS_KC ? K - kc : SS_KC;
            __syncthreads();                           // the tiles are free
            for (int i = tid; i < SS_CT * SS_KC; i += 256) {
                const int c = i / SS_KC, kk = i - c * SS_KC;
                const bool in = c0 + c < C && kk < kn;
                float m = 0.f, t = 1.f;                // a class past the end: a finite stand-in, masked below
                if (in) {
                    m = p.means[(size_t)(c0 + c) * K + kc + kk];
                    t = p.var_dim == VAR_DIAG ? p.T[(size_t)(c0 + c) * K + kc + kk] : p.T[c0 + c];
                }
                mt[kk][c] = m;
                tt[kk][c] = (double)t * (double)t;     // exact
            }
            if (lane < SS_KC) {
#pragma unroll
                for (int j = 0; j < SS_RW; ++j) {
                    const bool in = unl[j] && lane < kn;
                    const double m = in ? (double)p.mu[(size_t)row[j] * K + kc + lane] : 0.;
                    const double l = in ? (double)p.lv[(size_t)row[j] * K + kc + lane] : 0.;
                    rm[wv][j][lane] = m;
                    re[wv][j][lane] = exp(l);
                    if (c0 == 0) slv[j] += l;
                }
            }
            __syncthreads();
            for (int kk = 0; kk < kn; ++kk) {
                const double m = (double)mt[kk][lane], t2 = tt[kk][lane];
                if ((kk & (SS_WAVES - 1)) == wv) slog += log(t2);          // the waves share the logarithms of a class
#pragma unroll
                for (int j = 0; j < SS_RW; ++j) {
                    const double x = rm[wv][j][kk] - m;
                    d[j] = fma(t2, x * x, d[j]);
                    tr[j] = fma(re[wv][j][kk], t2, tr[j]);
                }
            }
        }
        ld[wv][lane] = slog;
        __syncthreads();
        slog = ((ld[0][lane] + ld[1][lane]) + ld[2][lane]) + ld[3][lane];
        const int c = c0 + lane;
        const bool in = c < C;
        const double lpi = p.log_pi ? (in ? p.log_pi[c] : 0.) : -log((double)C);
#pragma unroll
        for (int j = 0; j < SS_RW; ++j) {
            if (c0 == 0) slv[j] = wave_sum64(slv[j]);
            if (!unl[j]) continue;                     // wave-uniform
            const double v = in ? ((tr[j] - slv[j]) - slog) - (double)K : 0.;
            const double dc = in ? d[j] : 0.;
            const double Q = in ? 0.5 * (dc + w * v) - lpi : (double)INFINITY;
            if (in) qws[(size_t)row[j] * C + c] = Q;
            // the tile's shifted sums, then the fold: the side with the smaller shift passes through with a factor of exactly 1
            const double at = wave_min64(Q), as = at < (double)INFINITY ? at : 0.;
            const double e = in ? exp(-(Q - as)) : 0.;
            const double st = wave_sum64(e), sdt = wave_sum64(e * dc), svt = wave_sum64(e * v);
            const double an = fmin(a[j], at), ans = an < (double)INFINITY ? an : 0.;
            const double fl = a[j] < (double)INFINITY ? exp(-(a[j] - ans)) : 0., fr = at < (double)INFINITY ? exp(-(at - ans)) : 0.;
            s[j] = s[j] * fl + st * fr;
            sd[j] = sd[j] * fl + sdt * fr;
            sv[j] = sv[j] * fl + svt * fr;
            a[j] = an;
        }
    }
#pragma unroll
    for (int j = 0; j < SS_RW; ++j) {
        if (!unl[j]) continue;
        const long n = row[j];
        const double as = a[j] < (double)INFINITY ? a[j] : 0., inv = 1. / s[j];
        if (lane == 0) {
            kl[n] = (float)(a[j] - log(s[j]));
            zd[n] = (float)(sd[j] * inv);
            vkl[n] = (float)(sv[j] * inv);
        }
        for (int c = lane; c < C; c += 64)             // the lane that parked Q_c reads it back
            r[n * C + c] = (float)(exp(-(qws[(size_t)n * C + c] - as)) * inv);
    }
}

__global__ __launch_bounds__(256) void ss_bwd_rows_kernel(SsP p, const float* __restrict__ g, const float* __restrict__ r,
                                                          float* __restrict__ g_kl_in, float* __restrict__ g_mu,
                                                          float* __restrict__ g_lv) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long n = (long)blockIdx.x * 4 + wv;
    const int K = p.K, C = p.C;
    if (n >= p.N) return;
    const bool lab = p.y[n] >= 0;                      // wave-uniform
    const float gf = g ? g[n] : 0.f;
    if (lane == 0) g_kl_in[n] = lab ? gf : 0.f;
    const double gn = (double)gf, hw = 0.5 * (double)p.w;
    const float* rr = r + (size_t)n * C;
    for (int k = lane; k < K; k += 64) {
        const size_t at = (size_t)n * K + k;
        if (lab) { g_mu[at] = 0.f; g_lv[at] = 0.f; continue; }
        const double m = (double)p.mu[at], e = exp((double)p.lv[at]);
        double sa = 0., sb = 0.;
        for (int c = 0; c < C; ++c) {
            const float rc = rr[c];
            if (rc == 0.f) continue;                   // wave-uniform
            const double t = (double)(p.var_dim == VAR_DIAG ? p.T[(size_t)c * K + k] : p.T[c]);
            const double rt2 = (double)rc * (t * t);
            sa = fma(rt2, m - (double)p.means[(size_t)c * K + k], sa);
            sb += rt2;
        }
        g_mu[at] = (float)(gn * sa);
        g_lv[at] = (float)(gn * (hw * (e * sb - 1.)));
    }
}

__global__ __launch_bounds__(64 * SS_CHUNKS) void ss_bwd_cols_kernel(SsP p, const float* __restrict__ g,
                                                                     const float* __restrict__ r, float* __restrict__ g_means,
                                                                     float* __restrict__ g_T) {
    __shared__ double pm[SS_CHUNKS][64], pt[SS_CHUNKS][64];
    const int ix = threadIdx.x & 63, chunk = threadIdx.x >> 6;
    const int N = p.N, K = p.K, C = p.C;
    const long i = (long)blockIdx.x * 64 + ix;
    const int per = (N + SS_CHUNKS - 1) / SS_CHUNKS;
    const long nb = (long)chunk * per, ne = nb + per < N ? nb + per : N;
    const bool in = i < (long)C * K;
    const int c = in ? (int)(i / K) : 0, k = in ? (int)(i - (long)c * K) : 0;
    const double m = (double)p.means[(size_t)c * K + k];
    const double t = (double)(p.var_dim == VAR_DIAG ? p.T[(size_t)c * K + k] : p.T[c]);
    const double w = (double)p.w, wt = w / t;
    const bool want_T = g_T != nullptr;
    double sm = 0., sT = 0.;
    if (in && g) {
        for (long n = nb; n < ne; ++n) {
            if (p.y[n] >= 0) continue;
            const double coef = (double)g[n] * (double)r[(size_t)n * C + c];
            if (coef == 0.) continue;
            const double x = (double)p.mu[(size_t)n * K + k] - m;
            sm = fma(coef, x, sm);
            if (want_T) sT = fma(coef, t * fma(w, exp((double)p.lv[(size_t)n * K + k]), x * x) - wt, sT);
        }
    }
    pm[chunk][ix] = sm;
    pt[chunk][ix] = sT;
    __syncthreads();
    if (chunk == 0 && in) {
        double am = 0., aT = 0.;
#pragma unroll
        for (int q = 0; q < SS_CHUNKS; ++q) { am += pm[q][ix]; aT += pt[q][ix]; }
        if (g_means) g_means[i] = (float)(0. - (t * t) * am);
        if (g_T) g_T[i] = (float)aT;
    }
}

bool ss_misaligned(const void* q, uintptr_t mask) { return ((uintptr_t)q & mask) != 0; }

// -1: a malformed call; 0: fine
int ss_vet(SsP* p, const float* mu, const float* lv, const long long* y, const float* means, const float* T, const double* log_pi,
           int var_dim, float w, int N, int K, int C) {
    if (!ss_in_range(N, K, C)) return JVAE_EINVAL;
    if (var_dim != VAR_SCALAR && var_dim != VAR_DIAG) return JVAE_EINVAL;   // the full factor has no entry here
    if (!(fabsf(w) < INFINITY)) return JVAE_EINVAL;
    if (!means || !T) return JVAE_EINVAL;
    if (N > 0 && (!mu || !lv || !y)) return JVAE_EINVAL;                    // an empty batch has no per-sample arrays
    if (ss_misaligned(mu, 3) || ss_misaligned(lv, 3) || ss_misaligned(means, 3) || ss_misaligned(T, 3) || ss_misaligned(y, 7) ||
        ss_misaligned(log_pi, 7))
        return JVAE_EINVAL;
    p->mu = mu; p->lv = lv; p->y = y; p->means = means; p->T = T; p->log_pi = log_pi;
    p->var_dim = var_dim; p->N = N; p->K = K; p->C = C; p->w = w;
    return 0;
}

}  // namespace

extern "C" {

size_t jvae_semi_keep_bytes(int N, int C) { return ss_in_range(N, 1, C) ? sizeof(float) * (size_t)N * C : 0; }

size_t jvae_semi_fwd_workspace_bytes(int N, int C) { return ss_in_range(N, 1, C) ? sizeof(double) * (size_t)N * C : 0; }

int jvae_semi_class_marginal_fwd_f32(const float* mu, const float* lv, const long long* y, const float* means, const float* T,
                                     const double* log_pi, int var_dim, float w, int N, int K, int C, const float* kl_in,
                                     const float* zdist_in, const float* var_kl_in, float* kl, float* zdist, float* var_kl, float* r,
                                     size_t r_bytes, void* ws, size_t ws_bytes, void* stream) {
    SsP p;
    const int rc = ss_vet(&p, mu, lv, y, means, T, log_pi, var_dim, w, N, K, C);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!kl_in || !zdist_in || !var_kl_in || !kl || !zdist || !var_kl || !r || !ws) return JVAE_EINVAL;
    if (ss_misaligned(kl_in, 3) || ss_misaligned(zdist_in, 3) || ss_misaligned(var_kl_in, 3) || ss_misaligned(kl, 3) ||
        ss_misaligned(zdist, 3) || ss_misaligned(var_kl, 3) || ss_misaligned(r, 3) || ss_misaligned(ws, 7))
        return JVAE_EINVAL;
    if (r_bytes < jvae_semi_keep_bytes(N, C) || ws_bytes < jvae_semi_fwd_workspace_bytes(N, C)) return JVAE_EWORKSPACE;
    ss_fwd_kernel<<<cdiv(N, SS_ROWS), 256, 0, (hipStream_t)stream>>>(p, kl_in, zdist_in, var_kl_in, kl, zdist, var_kl, r, (double*)ws);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_semi_class_marginal_bwd_f32(const float* g_kl, const float* mu, const float* lv, const long long* y, const float* means,
                                     const float* T, int var_dim, float w, int N, int K, int C, const float* r, size_t r_bytes,
                                     float* g_kl_in, float* g_mu, float* g_lv, float* g_means, float* g_T, void* stream) {
    SsP p;
    const int rc = ss_vet(&p, mu, lv, y, means, T, nullptr, var_dim, w, N, K, C);
    if (rc) return rc;
    if (N > 0 && (!r || !g_kl_in || !g_mu || !g_lv)) return JVAE_EINVAL;
    if (ss_misaligned(g_kl, 3) || ss_misaligned(r, 3) || ss_misaligned(g_kl_in, 3) || ss_misaligned(g_mu, 3) ||
        ss_misaligned(g_lv, 3) || ss_misaligned(g_means, 3) || ss_misaligned(g_T, 3))
        return JVAE_EINVAL;
    if (g_T && var_dim != VAR_DIAG) return JVAE_EINVAL;       // the scalar factor is not learned (GaussianPrior)
    if (N > 0 && r_bytes < jvae_semi_keep_bytes(N, C)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (N > 0) {
        ss_bwd_rows_kernel<<<cdiv(N, 4), 256, 0, st>>>(p, g_kl, r, g_kl_in, g_mu, g_lv);
        JVAE_LAUNCH_CHECK();
    }
    if (g_means || g_T) {                                     // N = 0: the class sums are empty sums, zeros are written
        ss_bwd_cols_kernel<<<cdiv((long)C * K, 64), 64 * SS_CHUNKS, 0, st>>>(p, g_kl, r, g_means, g_T);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
