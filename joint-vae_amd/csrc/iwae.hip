// Importance-weighted bound (Burda et al. 2016) of the training step: the loss tail that turns the step's (L+1, N, K) draws, the
// per-draw reconstruction rows wmse_s (L, N) and the class-conditional Gaussian prior into
//
//   log w_l = log p(x | z_l) + beta (log p(z_l | y) - log q(z_l | x))                      l = 1..L (row 0 of z takes no part)
//   bound_n = logsumexp_l(log w_l) - log L,   wt_l = softmax_l(log w_l),   ess_n = 1 / sum_l wt_l^2
//
// and its backward.  No counterpart in the reference (its `iws`, jvae_iws_f32, is an evaluation score without gradient).
//
//   log p(x | z_l) = -D/2 (wmse_s[l,n] + 2 log sigma + log 2pi)                              iws_rows_kernel's convention
//   log p(z_l | y) = -K/2 log 2pi - 1/2 |T_y (z_l - m_y)|^2 + sum_k log|t_yk|                GaussianPrior.log_density
//                    (scalar variance: K log|t_y|)
//   log q(z_l | x) = -1/2 sum_k (eps_lk^2 + lv_k) - K/2 log 2pi
//
// The two K/2 log 2pi cancel in the difference and are never formed.  Operands and results are fp32.  log w is of the order of
// D (10^3 to 10^5) while only its differences between the draws of a sample matter, and one fp32 rounding of it (2^-24 x 10^4)
// would already move a weight by a part in a thousand: log w is formed in fp64 (fixed-order sums: a lane's K / 64 addends in
// sequence, then the butterfly) and never stored - what is stored is the fp32 value of log w - max, small where it matters.
// That keeps the TAIL from adding such a rounding; it does not mend the operands: wmse_s arrives as an fp32 row, magnified by
// D/2, and a weight is as good as that row.
//
// Forward, ONE launch, one workgroup per sample.  Pass 1: the four waves take the draws in turn (lanes over K) and keep the
// largest log w; the workgroup's maximum M goes through LDS.  Pass 2: the same waves form the same log w again (the same code on
// the same operands: the same bits) and park fp32(log w - M) <= 0 in the sample's column of `wt`: exactly 0 for the leader.
// After the barrier thread t folds the draws t, t + 256, ... - the sums of e_l = expf(parked) and of e_l^2 - and the
// workgroup's fixed butterfly-and-tree sum joins the 256 partial sums.  The largest term is exactly 1, so every output is
// finite for finite inputs whatever the size of log w; a draw that leads by more than the fp32 exponent range leaves e = 0 for
// the others: wt exactly one-hot, ess = S^2 / Q = 1 exactly.  bound = fp32(M + log S - log L), rounded once.  With `state` the
// (max, S, Q, count) of earlier slabs of draws is merged in: one of the two scale factors is exp(0) = 1.
//
// Backward, per sample by one wave (direct partial derivatives; g = d loss / d bound_n), each product chain in fp64 and rounded
// once:
//   g_wmse_s[l,n] = -g wt_l D/2       g_z[l] = -g wt_l beta t^2 (z_l - m_y)  (row 0: zero)       g_lv = g beta/2
//   per-sample contributions to its class:   mean  +g beta sum_l wt_l t^2 (z_l - m_y),   T (diag)  g beta sum_l wt_l (1/t - t d^2)
// kept in fp64 and folded per class in sample order over a fixed partition of 16 contiguous sample chunks (the scheme of
// means_grad_kernel in latent.hip): no atomics, the same bits from run to run.  sigma: -g D [/ sigma], summed in a fixed order
// in fp64 (value, log) or per sample (coded).
//
// A label outside [0, C) is never an index: NaN in every output of that sample, nothing added to any class.
#include <math.h>
#include "common.h"
#include "jvae_internal.h"
#include "class_fold.h"

namespace {

enum { SIG_VALUE = 0, SIG_LOG = 1, SIG_CODED = 2, SIG_RMSE = 3 };
enum { PRIOR_GAUSS = 0 };
enum { VAR_SCALAR = 0, VAR_DIAG = 1 };

struct IwP {
    const float* wmse_s;    // (L, N)
    const float* z;         // (L+1, N, K), row 0 = the mean latent
    const float* lv;        // (N, K) clipped log-variance
    const float* eps;       // (L, N, K)
    const long long* y;     // (N,)
    const float* means;     // (C, K)
    const float* T;         // (C,) | (C, K) whitening factor
    const float* sigma;     // 1 value | 1 log value | N log values
    int sigma_kind, var_dim;
    int L, N, K, C;
    float D, beta;
};

// log w of draw l of sample n in fp64, by one wave, valid in every lane.  a0 = -D/2 (2 log sigma + log 2pi), slog = sum_k log|t_k|.
__device__ __forceinline__ double iw_log_w(const IwP& p, const int n, const int l, const int lane, const float* __restrict__ m,
                                           const float* __restrict__ Tc, const double a0, const double slog) {
    const int K = p.K;
    const float* zr = p.z + ((long)(l + 1) * p.N + n) * K;
    const float* er = p.eps + ((long)l * p.N + n) * K;
    double dist = 0., q = 0.;
    for (int k = lane; k < K; k += 64) {
        const double t = (double)(p.var_dim == VAR_DIAG ? Tc[k] : Tc[0]);
        const double wd = t * ((double)zr[k] - (double)m[k]);
        dist = fma(wd, wd, dist);
        const double e = (double)er[k];
        q += fma(e, e, (double)p.lv[(long)n * K + k]);
    }
    dist = wave_sum64(dist);
    q = wave_sum64(q);
    return a0 - 0.5 * (double)p.D * (double)p.wmse_s[(long)l * p.N + n] + (double)p.beta * (0.5 * (q - dist) + slog);
}

__global__ __launch_bounds__(256) void iw_fwd_kernel(IwP p, float* __restrict__ bound, float* wt, float* __restrict__ ess,
                                                     double* state) {
    __shared__ float red[17];
    __shared__ double mx[4];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = p.L, N = p.N, K = p.K;
    const long long cls = p.y[n];
    if (cls < 0 || cls >= (long long)p.C) {                  // block-uniform
        for (int l = tid; l < L; l += 256) wt[(long)l * N + n] = NAN;
        if (tid == 0) {
            bound[n] = NAN; ess[n] = NAN;
            if (state) for (int j = 0; j < 4; ++j) state[(long)j * N + n] = (double)NAN;
        }
        return;
    }
    const float* m = p.means + (long)cls * K;
    const float* Tc = p.T + (p.var_dim == VAR_DIAG ? (long)cls * K : (long)cls);
    // -1/2 log|Sigma_y| = sum_k log|t_yk|
    double slog;
    if (p.var_dim == VAR_DIAG) {
        double s = 0.;
        for (int k = lane; k < K; k += 64) s += log(fabs((double)Tc[k]));
        slog = wave_sum64(s);
    } else {
        slog = (double)K * log(fabs((double)Tc[0]));
    }
    const double sg = (double)p.sigma[p.sigma_kind == SIG_CODED ? n : 0];
    const double log_sigma = p.sigma_kind == SIG_VALUE ? log(sg) : sg;
    const double a0 = -0.5 * (double)p.D * (2. * log_sigma + 1.8378770664093454836);
    // pass 1: the largest log w of the sample
    double mw = -INFINITY;
    for (int l = wv; l < L; l += 4) mw = fmax(mw, iw_log_w(p, n, l, lane, m, Tc, a0, slog));
    if (lane == 0) mx[wv] = mw;
    __syncthreads();
    const double M = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
    // pass 2: the same log w again, parked as fp32(log w - M) in the sample's column of wt
    for (int l = wv; l < L; l += 4) {
        const double lw = iw_log_w(p, n, l, lane, m, Tc, a0, slog);
        if (lane == 0) wt[(long)l * N + n] = (float)(lw - M);
    }
    __syncthreads();                                          // the column is read back by the whole workgroup
    float s = 0.f, q2 = 0.f;
    for (int l = tid; l < L; l += 256) {
        const float e = expf(wt[(long)l * N + n]);
        s += e;
        q2 = fmaf(e, e, q2);
    }
    const float S = block_sum(s, red);
    const float Q = block_sum(q2, red);
    for (int l = tid; l < L; l += 256) wt[(long)l * N + n] = expf(wt[(long)l * N + n]) / S;
    if (tid == 0) {
        double Mt = M, St = (double)S, Qt = (double)Q, cnt = (double)L;
        if (state) {
            // exact merge of (max, shifted sums) pairs: the side that holds the larger maximum is scaled by exp(0) = 1; a fresh
            // state is all zeros: count 0, nothing to merge
            const double m0 = state[n], S0 = state[(long)N + n], Q0 = state[2L * N + n], c0 = state[3L * N + n];
            Mt = c0 > 0. ? fmax(m0, M) : M;
            const double f0 = c0 > 0. ? exp(m0 - Mt) : 0., f1 = exp(M - Mt);
            St = S0 * f0 + St * f1;
            Qt = Q0 * (f0 * f0) + Qt * (f1 * f1);
            cnt = c0 + cnt;
            state[n] = Mt; state[(long)N + n] = St; state[2L * N + n] = Qt; state[3L * N + n] = cnt;
        }
        bound[n] = (float)(Mt + log(St) - log(cnt));
        ess[n] = (float)(St * St / Qt);
    }
}

// one wave per sample: gradients of the sample's own tensors and its fp64 contributions to its class
__global__ __launch_bounds__(256) void iw_bwd_kernel(IwP p, const float* __restrict__ g, const float* __restrict__ wt,
                                                     float* __restrict__ g_wmse_s, float* __restrict__ g_z,
                                                     float* __restrict__ g_lv, double* __restrict__ gd_scratch,
                                                     double* __restrict__ gt_scratch, double* __restrict__ gsig_part,
                                                     float* __restrict__ gsig_coded) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int L = p.L, N = p.N, K = p.K;
    if (n >= N) return;
    const long long cls = p.y[n];
    const double gn = g ? (double)g[n] : 0.;
    float* z0 = g_z + (long)n * K;
    if (cls < 0 || cls >= (long long)p.C) {
        for (int l = lane; l < L; l += 64) g_wmse_s[(long)l * N + n] = NAN;
        for (int k = lane; k < K; k += 64) {
            z0[k] = 0.f;
            for (int l = 1; l <= L; ++l) g_z[((long)l * N + n) * K + k] = NAN;
            g_lv[(long)n * K + k] = NAN;
            if (gd_scratch) gd_scratch[(long)n * K + k] = 0.;
            if (gt_scratch) gt_scratch[(long)n * K + k] = 0.;
        }
        if (lane == 0 && gsig_part) gsig_part[n] = 0.;
        if (lane == 0 && gsig_coded) gsig_coded[n] = NAN;
        return;
    }
    const float* m = p.means + (long)cls * K;
    const float* Tc = p.T + (p.var_dim == VAR_DIAG ? (long)cls * K : (long)cls);
    const double hD = 0.5 * (double)p.D;
    for (int l = lane; l < L; l += 64) g_wmse_s[(long)l * N + n] = (float)(-gn * (double)wt[(long)l * N + n] * hD);
    const double gb = gn * (double)p.beta;
    for (int k = lane; k < K; k += 64) {
        const double t = (double)(p.var_dim == VAR_DIAG ? Tc[k] : Tc[0]);
        const double t2 = t * t, rt = 1. / t, mk = (double)m[k];
        double sm = 0., sT = 0.;
        z0[k] = 0.f;
        for (int l = 1; l <= L; ++l) {
            const long o = ((long)l * N + n) * K + k;
            const double w = (double)wt[(long)(l - 1) * N + n];
            const double d = (double)p.z[o] - mk;
            const double td = t2 * d;
            g_z[o] = (float)(-gb * (w * td));
            sm = fma(w, td, sm);
            sT = fma(w, rt - t * (d * d), sT);
        }
        g_lv[(long)n * K + k] = (float)(0.5 * gb);
        if (gd_scratch) gd_scratch[(long)n * K + k] = gb * sm;
        if (gt_scratch) gt_scratch[(long)n * K + k] = gb * sT;
    }
    const double gs = -gn * (double)p.D;
    if (lane == 0 && gsig_part) gsig_part[n] = p.sigma_kind == SIG_VALUE ? gs / (double)p.sigma[0] : gs;
    if (lane == 0 && gsig_coded) gsig_coded[n] = (float)gs;
}

// out[0] = fp32 of the fp64 sum of v[0..n): each thread its stride in order, then the butterfly, then the waves in sequence
__global__ __launch_bounds__(256) void iw_vec_sum_kernel(const double* __restrict__ v, float* __restrict__ out, int n) {
    __shared__ double red[16];
    double s = 0.;
    for (int i = threadIdx.x; i < n; i += 256) s += v[i];
    s = block_sum64(s, red);
    if (threadIdx.x == 0) out[0] = (float)s;
}

// -1: a malformed call; -2: a configuration this file does not compute (never computed wrongly); 0: fine
int iw_vet(IwP* p, const float* wmse_s, const float* z, const float* lv, const float* eps, const long long* y,
           const float* means, const float* T, const float* sigma, int sigma_kind, int prior, int var_dim, float beta,
           int L, int N, int K, int C, int D) {
    if (L < 1 || K < 1 || N < 0 || C < 1 || D < 1) return JVAE_EINVAL;
    if (!means || !T || (!sigma && !(sigma_kind == SIG_CODED && N == 0))) return JVAE_EINVAL;
    if (N > 0 && (!wmse_s || !z || !lv || !eps || !y)) return JVAE_EINVAL;      // an empty batch has no per-sample arrays
    if (sigma_kind < 0 || sigma_kind > 3 || prior < 0 || prior > 2 || var_dim < 0 || var_dim > 2) return JVAE_EINVAL;
    if (!(beta == beta)) return JVAE_EINVAL;
    if (prior != PRIOR_GAUSS || var_dim > VAR_DIAG || sigma_kind == SIG_RMSE) return JVAE_ENOTSUP;
    if ((long)C * K > 0x7fffffffL) return JVAE_ENOTSUP;     // the class fold indexes (class, k) cells with an int
    p->wmse_s = wmse_s; p->z = z; p->lv = lv; p->eps = eps; p->y = y; p->means = means; p->T = T; p->sigma = sigma;
    p->sigma_kind = sigma_kind; p->var_dim = var_dim; p->L = L; p->N = N; p->K = K; p->C = C; p->D = (float)D; p->beta = beta;
    return 0;
}

}  // namespace

extern "C" {

int jvae_iw_bound_fwd_f32(const float* wmse_s, const float* z, const float* lv, const float* eps, const long long* y,
                          const float* means, const float* T, const float* sigma, int sigma_is_log, int prior, int var_dim,
                          float beta, int L, int N, int K, int C, int D, float* bound, float* wt, float* ess, double* state,
                          void* stream) {
    IwP p;
    const int rc = iw_vet(&p, wmse_s, z, lv, eps, y, means, T, sigma, sigma_is_log, prior, var_dim, beta, L, N, K, C, D);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!bound || !wt || !ess) return JVAE_EINVAL;
    hipLaunchKernelGGL(iw_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, p, bound, wt, ess, state);
    JVAE_LAUNCH_CHECK();
    return 0;
}

size_t jvae_iw_bound_bwd_workspace_bytes(int N, int K) {
    if (N < 0 || K < 1) return 0;
    return sizeof(double) * ((size_t)2 * N * K + (size_t)N);
}

int jvae_iw_bound_bwd_f32(const float* g_bound, const float* wt, const float* z, const long long* y, const float* means,
                          const float* T, const float* sigma, int sigma_is_log, int prior, int var_dim, float beta,
                          int L, int N, int K, int C, int D, float* g_wmse_s, float* g_z, float* g_lv, float* g_means,
                          float* g_T, float* g_sigma, void* ws, size_t ws_bytes, void* stream) {
    IwP p;
    // wmse_s, lv and eps take no part in the direct derivatives: `wt` stands in for them in the vetting
    const int rc = iw_vet(&p, wt, z, wt, wt, y, means, T, sigma, sigma_is_log, prior, var_dim, beta, L, N, K, C, D);
    if (rc) return rc;
    if (N > 0 && (!g_wmse_s || !g_z || !g_lv)) return JVAE_EINVAL;
    if (g_T && var_dim != VAR_DIAG) return JVAE_EINVAL;      // the scalar factor is not learned (GaussianPrior)
    p.wmse_s = p.lv = p.eps = nullptr;
    const size_t NK = (size_t)N * K;
    const bool fold = g_means || g_T || g_sigma;
    if (fold && (!ws || ws_bytes < jvae_iw_bound_bwd_workspace_bytes(N, K) || ((uintptr_t)ws & 7))) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double* gd = g_means ? (double*)ws : nullptr;
    double* gt = g_T ? (double*)ws + NK : nullptr;
    const bool coded = sigma_is_log == SIG_CODED;
    // coded: the per-sample value IS the result; value / log: N fp64 parts, summed below
    double* gs = (g_sigma && !coded) ? (double*)ws + 2 * NK : nullptr;
    if (N > 0) {
        hipLaunchKernelGGL(iw_bwd_kernel, dim3(cdiv(N, 4)), dim3(256), 0, st, p, g_bound, wt, g_wmse_s, g_z, g_lv, gd, gt, gs,
                           (g_sigma && coded) ? g_sigma : (float*)nullptr);
        JVAE_LAUNCH_CHECK();
    }
    if (g_means || g_T) {                                     // N = 0: the class sums are empty sums, zeros are written
        hipLaunchKernelGGL(iw_class_fold_kernel, dim3(cdiv((long)C * K, 64), 2), dim3(1024), 0, st, (const double*)gd, g_means,
                           (const double*)gt, g_T, y, N, C, K);
        JVAE_LAUNCH_CHECK();
    }
    if (g_sigma && !coded) {
        hipLaunchKernelGGL(iw_vec_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)gs, g_sigma, N);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
