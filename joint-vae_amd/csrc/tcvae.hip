// The beta-TCVAE split of the training step (Chen et al. 2018, "Isolating sources of disentanglement in VAEs"; DESIGN.md section
// 7w): the loss tail that turns the step's draws z (L+1, N, K), the posteriors (mu, lv) of the SAME batch and the class-conditional
// Gaussian prior into
//
//   mi = A - J,  tc = J - P,  dwkl = P - Bp,  reg = alpha mi + beta_tc tc + gamma dwkl          (means over the L draws)
//   A  = log q(z_li | x_i)        = -1/2 sum_k (eps^2 + lv_ik) - K/2 log 2pi                       as iwae.hip's log q
//   J  = log q(z_li)              = logsumexp_{j in S_i} sum_k l_ijk - c_i
//   P  = sum_k log q(z_lik)       = sum_k [logsumexp_{j in S_i} l_ijk - c_i]
//   Bp = log p(z_li | y_i)                                                                         as iwae.hip's log p(z | y)
//   l_ijk = -1/2 (lv_jk + (z_lik - mu_jk)^2 e^(-lv_jk) + log 2pi),   c_i = log |S_i| + log n_i
//
// and its backward.  S_i: the rows of the batch with the label of sample i (one class: the whole batch).  No counterpart in the
// reference.  The two logsumexp ARE the aggregate posterior of aggpost.hip with the batch as the bank and the labels as the groups:
// the forward launches that file's kernels (aggpost_core.h: prepare, joint, marginal - the same arithmetic, the same bits for the
// same pair), the joint launch keeping every Q_ij = c_j + sum_k d^2 w for the backward, and ends in tc_finish_kernel.
//
// Forward.  tc_prepare_kernel (the stored operands of aggpost.hip's prepare launch, one thread per element, and labels -> groups:
// a label outside [0, C) gives a row group -3 and a query group -1, which meet nobody), agp_joint_kernel<true, true, TC_PART> (pieces
// of one 64-row tile, so that a batch of 512 fills 64 workgroups), agp_dims_kernel<true>, then tc_finish_kernel, one workgroup per
// sample, its four waves taking the draws in turn: the pieces' (a, s) are merged in piece order against the smallest a (one factor
// is exactly 1), the merged pairs are kept as (a, 1 / s) - pairJ (L N), pairK (L N, K) - and each logarithm is ended in fp64: J, the K marginals
// (a lane's K / 64 in sequence, then the butterfly), A and Bp as iwae.hip forms them; the three differences are formed in fp64,
// summed over the wave's draws in sequence, the four waves in sequence, divided by L and rounded once.
//
// Backward (direct partial derivatives; g = d loss / d reg_i; coefJ = g (beta_tc - alpha) / L, coefP = g (gamma - beta_tc) / L):
//   weight(l,i,j,k) = coefJ r_ij + coefP r_ijk,  r_ij = 2^(kk (Q_ij - a_q)) / s_q,  r_ijk = 2^(kk (Q_ijk - a_qk)) / s_qk  (fp32,
//   the same expression in both passes; Q_ijk = fmaf(d d, w, lv) is formed again, Q_ij is read back); every sum over it is an fp64
//   fma chain rounded once.
//   Both passes look at 64 labels at a time (one per lane, a ballot) and walk the members of the set in ascending order.
//   tc_bwd_rows_kernel  one workgroup per sample, a wave per draw, lanes over k, j ascending:
//                       g_z = -sum_j weight d w + g gamma / L t^2 (z - m); per-sample fp64 contributions to the class (means, T)
//   tc_bwd_cols_kernel  a wave owns TC_RJ rows j and 64 coordinates, i ascending then l ascending:
//                       g_mu = sum weight d w,   g_lv = sum weight (d^2 w - 1) / 2 - g_j alpha / 2
//   iw_class_fold_kernel (class_fold.h) folds the class contributions.
// With alpha = beta_tc = gamma both coefficients are exactly 0 and the walks are skipped.  No floating-point atomics: the same
// inputs give the same bits.
//
// A label outside [0, C) is never an index: NaN in every output of that sample, it is in nobody's set and adds to no class.
#include <math.h>
#include "common.h"
#include "jvae_hip.h"
#include "aggpost_core.h"
#include "class_fold.h"

#define TC_MAX_K 1024
#define TC_MAX_N 8192
#define TC_MAX_Q (1L << 26)        // L N^2: 256 MB of kept Q
#define TC_RJ 2                    // column pass: rows of a wave
#define TC_PART AGP_TILE           // joint launch: rows of a piece (one tile: a batch of 512 rows fills 64 workgroups)
#define TC_HALF_LOG2PI 0.91893853320467274178

namespace {

enum { VAR_SCALAR = 0, VAR_DIAG = 1 };

struct TcP {
    const float* z;         // (L+1, N, K), row 0 = the mean latent
    const float* mu;        // (N, K)
    const float* lv;        // (N, K)
    const float* eps;       // (L, N, K)
    const long long* y;     // (N,)
    const float* means;     // (C, K)
    const float* T;         // (C,) | (C, K)
    const double* log_n;    // (C,) log of the training samples behind a class, or null: n_i = |S_i|
    int var_dim, L, N, K, C;
    float alpha, beta_tc, gamma;
};

// the kept tensors and the scratch of one call, carved out of two allocations
struct TcKeep {
    float* qall;            // (L N, Np)
    float2* pairJ;          // (L N)
    float2* pairK;          // (L N, K)
    float* wrow;            // (N, K)
};
struct TcWs {
    float *muT, *wT, *lvT, *c;
    int *group, *zgroup, *cnt;
    float2 *pair, *dpair;
};

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
int tc_pieces(long N) { return (int)((N + TC_PART - 1) / TC_PART); }      // of the joint launch; the marginal launch: agp_pieces

bool tc_in_range(int L, int N, int K) {
    return L >= 1 && N >= 1 && N <= TC_MAX_N && K >= 1 && K <= TC_MAX_K && (long)L * N * N <= TC_MAX_Q;
}

size_t tc_keep_layout(TcKeep* k, char* base, int L, int N, int K) {
    const size_t M = (size_t)L * N, Np = (size_t)agp_padded(N);
    size_t o = 0;
    if (k) k->qall = (float*)(base + o);
    o += up16(M * Np * sizeof(float));
    if (k) k->pairJ = (float2*)(base + o);
    o += up16(M * sizeof(float2));
    if (k) k->pairK = (float2*)(base + o);
    o += up16(M * K * sizeof(float2));
    if (k) k->wrow = (float*)(base + o);
    o += up16((size_t)N * K * sizeof(float));
    return o;
}

size_t tc_ws_layout(TcWs* w, char* base, int L, int N, int K) {
    const size_t M = (size_t)L * N, Np = (size_t)agp_padded(N), pm = (size_t)tc_pieces(N) * M, dm = (size_t)agp_pieces(N) * M;
    size_t o = 0;
    float** f[4] = {w ? &w->muT : nullptr, w ? &w->wT : nullptr, w ? &w->lvT : nullptr, nullptr};
    for (int i = 0; i < 3; ++i) {
        if (w) *f[i] = (float*)(base + o);
        o += up16(Np * K * sizeof(float));
    }
    if (w) w->c = (float*)(base + o);
    o += up16(Np * sizeof(float));
    if (w) w->group = (int*)(base + o);
    o += up16(Np * sizeof(int));
    if (w) w->zgroup = (int*)(base + o);
    o += up16(M * sizeof(int));
    if (w) w->cnt = (int*)(base + o);
    o += up16(pm * sizeof(int));
    if (w) w->pair = (float2*)(base + o);
    o += up16(pm * sizeof(float2));
    if (w) w->dpair = (float2*)(base + o);
    o += up16(dm * K * sizeof(float2));
    return o;
}

__device__ __forceinline__ bool tc_label_ok(long long cls, int C) { return cls >= 0 && cls < (long long)C; }

// One thread per element of the padded batch: the stored operands of aggpost.hip's prepare launch with the same values (agp_w; c =
// fp32 of the fp64 sum of the row's lv, k ascending, by the row's first thread; k-major, padding rows zero), w once more in the
// layout of mu for the kernels whose lanes walk k, and the groups: group[j] (Np) the label, -3 for a label out of range, -2 for a
// padding row; zgroup[q] (L N) the label of the query's sample, -1 out of range.
__global__ __launch_bounds__(256) void tc_prepare_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                         const long long* __restrict__ y, float* __restrict__ muT,
                                                         float* __restrict__ wT, float* __restrict__ lvT, float* __restrict__ c,
                                                         float* __restrict__ wrow, int* __restrict__ group, int* __restrict__ zgroup,
                                                         int L, int N, int Np, int K, int C) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < (long)L * N) {
        const long long cls = y[t % N];
        zgroup[t] = tc_label_ok(cls, C) ? (int)cls : -1;
    }
    if (t >= (long)Np * K) return;
    const long n = t / K;
    const int k = (int)(t - n * K);
    const bool in = n < N;
    const float m = in ? mu[t] : 0.f, l = in ? lv[t] : 0.f;
    const float w = in ? agp_w(l) : 0.f;
    muT[(size_t)k * Np + n] = m;
    wT[(size_t)k * Np + n] = w;
    lvT[(size_t)k * Np + n] = l;
    if (in) wrow[t] = w;
    if (k == 0) {
        double sum = 0.;
        if (in)
            for (int kk = 0; kk < K; ++kk) sum += (double)lv[(size_t)n * K + kk];
        c[n] = (float)sum;
        group[n] = in ? (tc_label_ok(y[n], C) ? (int)y[n] : -3) : -2;
    }
}

// the pieces' (a, s) of one sum merged in piece order: A the smallest a, S = sum_p s_p 2^(kk (a_p - A)); stride: floats2 between pieces
__device__ __forceinline__ float2 tc_merge(const float2* __restrict__ p, size_t stride, int pieces) {
    float A = INFINITY;
    for (int i = 0; i < pieces; ++i) A = fminf(A, p[i * stride].x);
    const float As = A < INFINITY ? A : 0.f;
    float S = 0.f;
    for (int i = 0; i < pieces; ++i) {
        const float2 v = p[i * stride];
        const float term = v.y * agp_exp2(AGP_KK * (v.x - As));
        S = i ? S + term : term;
    }
    return make_float2(A, S);
}

__global__ __launch_bounds__(256) void tc_finish_kernel(TcP p, const float2* __restrict__ pair, const float2* __restrict__ dpair,
                                                        const int* __restrict__ cnt, int pieces, int dpieces, float2* __restrict__ pairJ,
                                                        float2* __restrict__ pairK, float* __restrict__ reg,
                                                        float* __restrict__ mi, float* __restrict__ tc, float* __restrict__ dwkl) {
    __shared__ double part[4][3];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = p.L, N = p.N, K = p.K;
    const size_t M = (size_t)L * N;
    const long long cls = p.y[i];
    const bool ok = tc_label_ok(cls, p.C);                    // block-uniform
    double s_mi = 0., s_tc = 0., s_dw = 0.;
    const float* m = p.means + (ok ? (long)cls * K : 0);
    const float* Tc = p.T + (ok ? (p.var_dim == VAR_DIAG ? (long)cls * K : (long)cls) : 0);
    double slog = 0.;
    if (ok) {
        if (p.var_dim == VAR_DIAG) {
            double s = 0.;
            for (int k = lane; k < K; k += 64) s += log(fabs((double)Tc[k]));
            slog = wave_sum64(s);
        } else {
            slog = (double)K * log(fabs((double)Tc[0]));
        }
    }
    for (int l = wv; l < L; l += 4) {
        const size_t q = (size_t)l * N + i;
        const float2 pj = tc_merge(pair + q, M, pieces);
        long rows = 0;
        for (int pc = 0; pc < pieces; ++pc) rows += cnt[(size_t)pc * M + q];
        if (lane == 0) pairJ[q] = make_float2(pj.x, 1.f / pj.y);
        const double logB = log((double)rows);
        const double ci = logB + (p.log_n && ok ? p.log_n[cls] : logB);
        const float* zr = p.z + ((size_t)(l + 1) * N + i) * K;
        const float* er = p.eps + q * K;
        double ps = 0., qs = 0., dist = 0.;
        for (int k = lane; k < K; k += 64) {
            const float2 pk = tc_merge(dpair + (size_t)k * M + q, (size_t)K * M, dpieces);
            pairK[q * K + k] = make_float2(pk.x, 1.f / pk.y);
            ps += -0.5 * (double)pk.x + log((double)pk.y) - TC_HALF_LOG2PI - ci;
            const double e = (double)er[k];
            qs += fma(e, e, (double)p.lv[(size_t)i * K + k]);
            if (ok) {
                const double t = (double)(p.var_dim == VAR_DIAG ? Tc[k] : Tc[0]);
                const double wd = t * ((double)zr[k] - (double)m[k]);
                dist = fma(wd, wd, dist);
            }
        }
        ps = wave_sum64(ps);
        qs = wave_sum64(qs);
        dist = wave_sum64(dist);
        const double kl2pi = (double)K * TC_HALF_LOG2PI;
        const double A = -0.5 * qs - kl2pi;
        const double J = -0.5 * (double)pj.x + log((double)pj.y) - kl2pi - ci;
        const double Bp = -kl2pi - 0.5 * dist + slog;
        s_mi += A - J;
        s_tc += J - ps;
        s_dw += ps - Bp;
    }
    if (lane == 0) {
        part[wv][0] = s_mi; part[wv][1] = s_tc; part[wv][2] = s_dw;
    }
    __syncthreads();
    if (tid == 0) {
        double v[3];
        for (int c = 0; c < 3; ++c) v[c] = (((part[0][c] + part[1][c]) + part[2][c]) + part[3][c]) / (double)L;
        const double r = (double)p.alpha * v[0] + (double)p.beta_tc * v[1] + (double)p.gamma * v[2];
        reg[i] = ok ? (float)r : NAN;
        mi[i] = ok ? (float)v[0] : NAN;
        tc[i] = ok ? (float)v[1] : NAN;
        dwkl[i] = ok ? (float)v[2] : NAN;
    }
}

// weight of the pair (query, row j) at coordinate k; Qj = the kept joint Q, (aJ, iJ) = (a_q, 1 / s_q), (aK, iK) the coordinate's.
// dw receives d w, dd the rounded square.
__device__ __forceinline__ float tc_weight(float coefJ, float coefP, float Qj, float aJ, float iJ, float zk, float mu, float w,
                                           float lv, float aK, float iK, float& dw, float& dd) {
    const float d = zk - mu;
    dd = d * d;
    dw = d * w;
    const float Qk = fmaf(dd, w, lv);
    const float rJ = agp_exp2(AGP_KK * (Qj - aJ)) * iJ;
    const float rK = agp_exp2(AGP_KK * (Qk - aK)) * iK;
    return coefJ * rJ + coefP * rK;
}

// one workgroup per sample: g_z of its draws (a wave per draw) and its fp64 contributions to its class
__global__ __launch_bounds__(256) void tc_bwd_rows_kernel(TcP p, const float* __restrict__ g, TcKeep kp, int Np, float cJ, float cP,
                                                          float* __restrict__ g_z, double* __restrict__ gd_scratch,
                                                          double* __restrict__ gt_scratch) {
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int L = p.L, N = p.N, K = p.K;
    const long long cls = p.y[i];
    const bool ok = tc_label_ok(cls, p.C);                    // block-uniform
    const float gi = g ? g[i] : 0.f;
    for (int k = tid; k < K; k += 256) g_z[(size_t)i * K + k] = 0.f;             // the mean latent takes no part
    if (!ok) {
        for (int l = wv; l < L; l += 4)
            for (int k = lane; k < K; k += 64) g_z[((size_t)(l + 1) * N + i) * K + k] = NAN;
        for (int k = tid; k < K; k += 256) {
            if (gd_scratch) gd_scratch[(size_t)i * K + k] = 0.;
            if (gt_scratch) gt_scratch[(size_t)i * K + k] = 0.;
        }
        return;
    }
    const float* m = p.means + (long)cls * K;
    const float* Tc = p.T + (p.var_dim == VAR_DIAG ? (long)cls * K : (long)cls);
    const float coefJ = gi * cJ, coefP = gi * cP;
    const bool walk = coefJ != 0.f || coefP != 0.f;
    const double gg = (double)gi * (double)p.gamma / (double)L;
    for (int l = wv; l < L; l += 4) {
        const size_t q = (size_t)l * N + i;
        const float2 pj = kp.pairJ[q];                        // (a, 1 / s)
        const float* Qrow = kp.qall + q * Np;
        const float* zr = p.z + ((size_t)(l + 1) * N + i) * K;
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int k = k0 + lane;
            const bool in = k < K;
            const float zk = in ? zr[k] : 0.f;
            const float2 pk = in ? kp.pairK[q * K + k] : make_float2(0.f, 1.f);
            double acc = 0.;
            if (walk) {
                // 64 rows at a time: the lanes look at their labels, the members of the set are then walked in ascending order
                for (int jb = 0; jb < N; jb += 64) {
                    const int jl = jb + lane;
                    unsigned long long members = __ballot(jl < N && p.y[jl < N ? jl : 0] == cls);
                    const float Ql = Qrow[jl];                 // jl < Np
                    while (members) {                          // wave-uniform
                        const int b = __ffsll((long long)members) - 1;
                        members &= members - 1;
                        const float Qj = __shfl(Ql, b, 64);
                        const size_t at = (size_t)(jb + b) * K + k;
                        const float mu = in ? p.mu[at] : 0.f, w = in ? kp.wrow[at] : 0.f, lv = in ? p.lv[at] : 0.f;
                        float dw, dd;
                        const float wgt = tc_weight(coefJ, coefP, Qj, pj.x, pj.y, zk, mu, w, lv, pk.x, pk.y, dw, dd);
                        acc = fma((double)wgt, (double)dw, acc);
                    }
                }
            }
            if (in) {
                const double t = (double)(p.var_dim == VAR_DIAG ? Tc[k] : Tc[0]);
                const double td = (t * t) * ((double)zk - (double)m[k]);
                g_z[((size_t)(l + 1) * N + i) * K + k] = (float)(gg * td - acc);
            }
        }
    }
    // the class contributions: the draws in sequence, -gamma g / L times the gradients of log p(z | y)
    for (int k = tid; k < K; k += 256) {
        const double t = (double)(p.var_dim == VAR_DIAG ? Tc[k] : Tc[0]);
        const double t2 = t * t, rt = 1. / t, mk = (double)m[k];
        double sm = 0., sT = 0.;
        for (int l = 1; l <= L; ++l) {
            const double d = (double)p.z[((size_t)l * N + i) * K + k] - mk;
            sm += t2 * d;
            sT += rt - t * (d * d);
        }
        if (gd_scratch) gd_scratch[(size_t)i * K + k] = -gg * sm;
        if (gt_scratch) gt_scratch[(size_t)i * K + k] = -gg * sT;
    }
}

// a wave owns TC_RJ rows j and 64 coordinates; the queries in the order i ascending, then l ascending
__global__ __launch_bounds__(256) void tc_bwd_cols_kernel(TcP p, const float* __restrict__ g, TcKeep kp, int Np, float cJ, float cP,
                                                          float* __restrict__ g_mu, float* __restrict__ g_lv) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int L = p.L, N = p.N, K = p.K;
    const int j0 = (blockIdx.x * 4 + wv) * TC_RJ;              // even: the TC_RJ values of Q are one aligned load
    const int k = blockIdx.y * 64 + lane;
    if (j0 >= N) return;                                      // wave-uniform
    const bool in = k < K;
    long long yj[TC_RJ];
    bool okj[TC_RJ];
    float mu[TC_RJ], w[TC_RJ], lv[TC_RJ];
    double amu[TC_RJ], alv[TC_RJ];
#pragma unroll
    for (int r = 0; r < TC_RJ; ++r) {
        const int j = j0 + r;
        const bool row = j < N;
        yj[r] = row ? p.y[j] : -1;
        okj[r] = row && tc_label_ok(yj[r], p.C);
        const size_t at = (size_t)(row ? j : 0) * K + (in ? k : 0);
        mu[r] = p.mu[at]; w[r] = kp.wrow[at]; lv[r] = p.lv[at];
        amu[r] = 0.; alv[r] = 0.;
    }
    // 64 samples at a time: the lanes look at their labels and gradients, the members of the rows' sets are then walked in
    // ascending order
    for (int ib = 0; ib < N; ib += 64) {
        const int il = ib + lane;
        const long long yl = il < N ? p.y[il] : -1;
        const float gl = (g && il < N) ? g[il] : 0.f;
        unsigned long long set[TC_RJ], members = 0;
#pragma unroll
        for (int r = 0; r < TC_RJ; ++r) {
            set[r] = __ballot(okj[r] && yl == yj[r]);
            members |= set[r];
        }
        while (members) {                                     // wave-uniform
            const int b = __ffsll((long long)members) - 1;
            members &= members - 1;
            const int i = ib + b;
            const float gi = __shfl(gl, b, 64);
            const float coefJ = gi * cJ, coefP = gi * cP;
            if (coefJ == 0.f && coefP == 0.f) continue;
            for (int l = 0; l < L; ++l) {
                const size_t q = (size_t)l * N + i;
                const float2 pj = kp.pairJ[q];                // (a, 1 / s)
                const float zk = in ? p.z[((size_t)(l + 1) * N + i) * K + k] : 0.f;
                const float2 pk = in ? kp.pairK[q * K + k] : make_float2(0.f, 1.f);
                const float2 Q2 = *reinterpret_cast<const float2*>(kp.qall + q * Np + j0);  // j0 + 1 < Np
                const float Qs[TC_RJ] = {Q2.x, Q2.y};
#pragma unroll
                for (int r = 0; r < TC_RJ; ++r) {
                    if (!((set[r] >> b) & 1)) continue;
                    float dw, dd;
                    const float wgt = tc_weight(coefJ, coefP, Qs[r], pj.x, pj.y, zk, mu[r], w[r], lv[r], pk.x, pk.y, dw, dd);
                    amu[r] = fma((double)wgt, (double)dw, amu[r]);
                    alv[r] = fma((double)wgt, 0.5 * (double)fmaf(dd, w[r], -1.f), alv[r]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < TC_RJ; ++r) {
        const int j = j0 + r;
        if (j >= N || !in) continue;
        const float gj = g ? g[j] : 0.f;
        g_mu[(size_t)j * K + k] = okj[r] ? (float)amu[r] : NAN;
        g_lv[(size_t)j * K + k] = okj[r] ? (float)(alv[r] - 0.5 * (double)gj * (double)p.alpha) : NAN;
    }
}

static_assert(TC_RJ == 2, "the column pass reads its rows' Q as one float2");

// -1: a malformed call; -2: a configuration this file does not compute; 0: fine
int tc_vet(TcP* p, const float* z, const float* mu, const float* lv, const float* eps, const long long* y, const float* means,
           const float* T, const double* log_n, int var_dim, float alpha, float beta_tc, float gamma, int L, int N, int K, int C) {
    if (L < 1 || K < 1 || N < 0 || C < 1) return JVAE_EINVAL;
    if (var_dim < 0 || var_dim > 2) return JVAE_EINVAL;
    if (!(alpha == alpha) || !(beta_tc == beta_tc) || !(gamma == gamma)) return JVAE_EINVAL;
    if (!means || !T) return JVAE_EINVAL;
    if (N > 0 && (!z || !mu || !lv || !eps || !y)) return JVAE_EINVAL;      // an empty batch has no per-sample arrays
    if (var_dim > VAR_DIAG || K > TC_MAX_K || N > TC_MAX_N || (long)L * N * N > TC_MAX_Q) return JVAE_ENOTSUP;
    if ((long)C * K > 0x7fffffffL) return JVAE_ENOTSUP;
    p->z = z; p->mu = mu; p->lv = lv; p->eps = eps; p->y = y; p->means = means; p->T = T; p->log_n = log_n;
    p->var_dim = var_dim; p->L = L; p->N = N; p->K = K; p->C = C; p->alpha = alpha; p->beta_tc = beta_tc; p->gamma = gamma;
    return 0;
}

}  // namespace

extern "C" {

int jvae_tc_joint_partition(void) { return TC_PART; }

size_t jvae_tc_keep_bytes(int L, int N, int K) { return tc_in_range(L, N, K) ? tc_keep_layout(nullptr, nullptr, L, N, K) : 0; }

size_t jvae_tc_fwd_workspace_bytes(int L, int N, int K) { return tc_in_range(L, N, K) ? tc_ws_layout(nullptr, nullptr, L, N, K) : 0; }

size_t jvae_tc_bwd_workspace_bytes(int N, int K) {
    if (N < 0 || K < 1) return 0;
    return sizeof(double) * (size_t)2 * N * K;
}

int jvae_tc_objective_fwd_f32(const float* z, const float* mu, const float* lv, const float* eps, const long long* y,
                              const float* means, const float* T, const double* log_n, int var_dim, float alpha, float beta_tc,
                              float gamma, int L, int N, int K, int C, float* reg, float* mi, float* tc, float* dwkl, void* keep,
                              size_t keep_bytes, void* ws, size_t ws_bytes, void* stream) {
    TcP p;
    const int rc = tc_vet(&p, z, mu, lv, eps, y, means, T, log_n, var_dim, alpha, beta_tc, gamma, L, N, K, C);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!reg || !mi || !tc || !dwkl) return JVAE_EINVAL;
    if (!keep || !ws || ((uintptr_t)keep & 15) || ((uintptr_t)ws & 15)) return JVAE_EINVAL;
    if (keep_bytes < jvae_tc_keep_bytes(L, N, K) || ws_bytes < jvae_tc_fwd_workspace_bytes(L, N, K)) return JVAE_EWORKSPACE;
    TcKeep kp;
    TcWs w;
    tc_keep_layout(&kp, (char*)keep, L, N, K);
    tc_ws_layout(&w, (char*)ws, L, N, K);
    hipStream_t st = (hipStream_t)stream;
    const long M = (long)L * N, Np = agp_padded(N);
    const int pieces = tc_pieces(N), dpieces = agp_pieces(N);
    const float* zq = z + (size_t)N * K;                      // the queries: rows 1..L of z
    const long elems = Np * K > M ? Np * K : M;
    tc_prepare_kernel<<<cdiv(elems, 256), 256, 0, st>>>(mu, lv, y, w.muT, w.wT, w.lvT, w.c, kp.wrow, w.group, w.zgroup, L,
                                                        N, (int)Np, K, C);
    JVAE_LAUNCH_CHECK();
    const dim3 grid((unsigned)cdiv(M, AGP_QT), (unsigned)pieces);
    agp_joint_kernel<true, true, TC_PART><<<grid, AGP_BLOCK, 0, st>>>(zq, w.zgroup, w.muT, w.wT, w.c, w.group, w.pair, w.cnt, M, N, Np,
                                                                      K, nullptr, kp.qall);
    JVAE_LAUNCH_CHECK();
    const dim3 dgrid(grid.x, (unsigned)dpieces, (unsigned)cdiv(K, AGP_KD));
    agp_dims_kernel<true><<<dgrid, AGP_BLOCK, 0, st>>>(zq, w.zgroup, w.muT, w.wT, w.lvT, w.group, w.dpair, M, N, Np, K);
    JVAE_LAUNCH_CHECK();
    tc_finish_kernel<<<N, 256, 0, st>>>(p, w.pair, w.dpair, w.cnt, pieces, dpieces, kp.pairJ, kp.pairK, reg, mi, tc, dwkl);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_tc_objective_bwd_f32(const float* g_reg, const float* z, const float* mu, const float* lv, const long long* y,
                              const float* means, const float* T, int var_dim, float alpha, float beta_tc, float gamma, int L,
                              int N, int K, int C, const void* keep, size_t keep_bytes, float* g_z, float* g_mu, float* g_lv,
                              float* g_means, float* g_T, void* ws, size_t ws_bytes, void* stream) {
    TcP p;
    // eps and log_n take no part in the direct derivatives: z stands in for eps in the vetting
    const int rc = tc_vet(&p, z, mu, lv, z, y, means, T, nullptr, var_dim, alpha, beta_tc, gamma, L, N, K, C);
    if (rc) return rc;
    p.eps = nullptr;
    if (N > 0 && (!g_z || !g_mu || !g_lv || !keep || ((uintptr_t)keep & 15))) return JVAE_EINVAL;
    if (g_T && var_dim != VAR_DIAG) return JVAE_EINVAL;       // the scalar factor is not learned (GaussianPrior)
    if (N > 0 && keep_bytes < jvae_tc_keep_bytes(L, N, K)) return JVAE_EWORKSPACE;
    const bool fold = g_means || g_T;
    if (fold && (!ws || ws_bytes < jvae_tc_bwd_workspace_bytes(N, K) || ((uintptr_t)ws & 7))) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const size_t NK = (size_t)N * K;
    double* gd = g_means ? (double*)ws : nullptr;
    double* gt = g_T ? (double*)ws + NK : nullptr;
    if (N > 0) {
        TcKeep kp;
        tc_keep_layout(&kp, (char*)keep, L, N, K);
        const int Np = (int)agp_padded(N);
        const float cJ = (float)(((double)beta_tc - (double)alpha) / (double)L);
        const float cP = (float)(((double)gamma - (double)beta_tc) / (double)L);
        tc_bwd_rows_kernel<<<N, 256, 0, st>>>(p, g_reg, kp, Np, cJ, cP, g_z, gd, gt);
        JVAE_LAUNCH_CHECK();
        const dim3 grid((unsigned)cdiv(N, 4 * TC_RJ), (unsigned)cdiv(K, 64));
        tc_bwd_cols_kernel<<<grid, 256, 0, st>>>(p, g_reg, kp, Np, cJ, cP, g_mu, g_lv);
        JVAE_LAUNCH_CHECK();
    }
    if (fold) {                                               // N = 0: the class sums are empty sums, zeros are written
        iw_class_fold_kernel<<<dim3(cdiv((long)C * K, 64), 2), dim3(1024), 0, st>>>((const double*)gd, g_means, (const double*)gt,
                                                                                 g_T, y, N, C, K);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
