// The MMD-regularised bound of the training step (InfoVAE, Zhao, Song and Ermon 2019; WAE-MMD, Tolstikhin et al. 2018; DESIGN.md
// section 7y): the loss tail that turns the step's draws z (L+1, N, K), a second noise tensor e' (L, N, K) and the class-conditional
// Gaussian prior into the per-row terms of the unbiased U-statistic of MMD^2 between q(z, y) and pi_hat(y) p(z | y)
//
//   p_li = m_{y_i} + e'_li / t_{y_i}                                       (ops.prior_sample's 'scalar' / 'diag' expression, bit for bit)
//   m_i  = mean_l [ 1/(N-1) sum_{j in S_i, j != i} k(z_li, z_lj) + 1/(N-1) sum_{j in S_i, j != i} k(p_li, p_lj)
//                 - 2/N sum_{j in S_i} k(z_li, p_lj) ]
//   k(a, b) = sum_s C_s / (C_s + |a - b|^2)  ('imq')   |   sum_s exp(-|a - b|^2 / (2 h_s))  ('rbf'),   at most 8 terms
//
// and its backward.  S_i: the rows of the batch with the label of sample i (joint = 0 or one class: the whole batch).  Row 0 of z,
// the mean latent, takes no part.  No counterpart in the reference.
//
// Squared distances are taken in the DIRECT form sum_k (a_k - b_k)^2, an fp32 chain fmaf(d, d, acc) over k.  The matrix-core
// expansion |a|^2 + |b|^2 - 2ab is not used: it cancels on exactly the near pairs that carry the kernel's weight (for |a - b| <<
// |a| its absolute error is u |a|^2, not u |a - b|^2), and the bound the tests hold this file to counts the K roundings of the
// direct chain.  At N = 512, K = 64 the three blocks are about 5 x 10^7 fused multiply-adds per draw: the work is operand
// staging, not arithmetic, so the column tiles of z and p are staged in LDS once per workgroup and reused - by the zz and zp
// blocks for the row's z, by the pp and pz blocks for the row's p.
//
// Forward.  mmd_prepare_kernel forms p (a bad label: zeros, never read into a sum) and the groups: the label, 0 for every row
// when joint = 0, -1 for a label outside [0, C) - a group that meets nobody, itself included.  mmd_pair_kernel<false>: a workgroup
// owns MMD_TI rows of one draw and one piece of the columns; a lane is a row, a wave takes MMD_CW of the MMD_TJ columns of a
// step; the squared distances of the step are accumulated over chunks of MMD_KC coordinates, the kernel values are formed in
// fp32 and added to the thread's three fp64 sums in ascending column order; the four waves' sums are added in wave order and
// stored per piece.  mmd_finish_kernel adds the pieces in piece order and the draws in draw order, all in fp64, and rounds once.
//
// Backward (g = d loss / d m; kernel values are formed again, no (L, N, N) tensor is kept, so there is no L N^2 limit):
//   g_z[l,i] = 1/L [ sum_{j != i} (g_i + g_j)/(N-1) grad_1 k(z_i, z_j) - 2/N g_i sum_j grad_1 k(z_i, p_j) ]
//   g_p[l,j] = 1/L [ sum_{i != j} (g_i + g_j)/(N-1) grad_1 k(p_j, p_i) - 2/N sum_i g_i grad_2 k(z_i, p_j) ]
// with grad_1 k(a, b) = 2 k'(|a - b|^2) (a - b).  mmd_pair_kernel<true>: the same tiles with a fourth block (the row's p against
// the columns' z); the four pair weights w = coefficient x 2 k' of a step go through LDS to the second half of the step, where a
// thread owns a row and MMD_KW of the workgroup's MMD_KB coordinates and runs the fp64 chains acc = fma(w, a_k - b_k, acc) in
// ascending column order, the difference formed exactly in fp64.  The partial sums are stored per piece; mmd_bwd_finish_kernel
// (one workgroup per sample) adds the pieces in order, rounds g_z once and turns g_p (kept in fp64) into the sample's
// contributions to its class: g_means += g_p, g_T += -g_p e' / t^2 (summed over k for the scalar factor), which
// iw_class_fold_kernel (class_fold.h) folds in sample order.  Coincident points give a difference of exactly 0 and so a term of
// exactly 0; with g all zero every weight and every gradient is exactly 0.  No floating-point atomics: the same inputs give the
// same bits.  The number of pieces depends on (L, N, K) alone.
//
// A label outside [0, C) is never an index: NaN in every output of that sample, it is in nobody's set and adds to no class.
#include <math.h>
#include "common.h"
#include "jvae_hip.h"
#include "class_fold.h"

#define MMD_MAX_K 1024
#define MMD_MAX_N 8192
#define MMD_MAX_L 65535            // the draws are a grid dimension
#define MMD_MAX_S 8                // terms of the kernel
#define MMD_TI 64                  // rows of a workgroup: one per lane
#define MMD_TJ 32                  // columns of a step
#define MMD_CW (MMD_TJ / 4)        // ... of a wave
#define MMD_KC 16                  // coordinates of a staged chunk of the distance chain
#define MMD_KB 64                  // backward: coordinates of a workgroup
#define MMD_KW (MMD_KB / 4)        // ... of a wave
#define MMD_FWD_GRID 1024          // workgroups the column pieces are chosen to reach
#define MMD_BWD_GRID 512

namespace {

enum { VAR_SCALAR = 0, VAR_DIAG = 1 };
enum { MMD_IMQ = 0, MMD_RBF = 1 };

struct MmdKernel {
    int kind, S;
    float a[MMD_MAX_S];            // imq: C_s; rbf: -log2(e) / (2 h_s)
    float b[MMD_MAX_S];            // rbf: -1 / (2 h_s)
};

size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

bool mmd_in_range(int L, int N, int K) { return L >= 1 && L <= MMD_MAX_L && N >= 1 && N <= MMD_MAX_N && K >= 1 && K <= MMD_MAX_K; }

// the column steps of a piece: the pieces fill about `target` workgroups, a function of the shape alone
int mmd_piece_steps(int L, int N, int kchunks, int target) {
    const long tiles = (long)cdiv(N, MMD_TI) * L * kchunks;
    const int steps = cdiv(N, MMD_TJ);
    long pieces = (target + tiles - 1) / tiles;
    if (pieces < 1) pieces = 1;
    if (pieces > steps) pieces = steps;
    return cdiv(steps, pieces);
}
int mmd_pieces(int N, int piece_steps) { return cdiv(cdiv(N, MMD_TJ), piece_steps); }

struct MmdWs {
    float* p;                      // (L, N, K)
    int* group;                    // (N,)
    double* part;                  // forward: (pieces, L, N, 3); backward: (pieces, L, N, K, 2)
    double* gd;                    // backward: (N, K) the sample's contribution to its class mean
    double* gt;                    // backward: (N, K) | (N,) ... to its class factor
};

size_t mmd_ws_layout(MmdWs* w, char* base, int L, int N, int K, bool bwd) {
    const size_t M = (size_t)L * N;
    size_t o = 0;
    if (w) w->p = (float*)(base + o);
    o += up16(M * K * sizeof(float));
    if (w) w->group = (int*)(base + o);
    o += up16((size_t)N * sizeof(int));
    if (w) w->part = (double*)(base + o);
    if (!bwd) {
        const int pieces = mmd_pieces(N, mmd_piece_steps(L, N, 1, MMD_FWD_GRID));
        o += up16((size_t)pieces * M * 3 * sizeof(double));
        if (w) w->gd = w->gt = nullptr;
    } else {
        const int pieces = mmd_pieces(N, mmd_piece_steps(L, N, cdiv(K, MMD_KB), MMD_BWD_GRID));
        o += up16((size_t)pieces * M * K * 2 * sizeof(double));
        if (w) w->gd = (double*)(base + o);
        o += up16((size_t)N * K * sizeof(double));
        if (w) w->gt = (double*)(base + o);
        o += up16((size_t)N * K * sizeof(double));
    }
    return o;
}

__device__ __forceinline__ bool mmd_label_ok(long long cls, int C) { return cls >= 0 && cls < (long long)C; }

// One thread per element: p = means[y] + e' / T[y(, k)], each operation rounded on its own as ops.prior_sample rounds it (zeros
// for a bad label), and the groups by the first N threads.
__global__ __launch_bounds__(256) void mmd_prepare_kernel(const float* __restrict__ eps, const long long* __restrict__ y,
                                                          const float* __restrict__ means, const float* __restrict__ T,
                                                          float* __restrict__ p, int* __restrict__ group, int var_dim, int joint,
                                                          int L, int N, int K, int C) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t < N) {
        const long long cls = y[t];
        group[t] = mmd_label_ok(cls, C) ? (joint ? (int)cls : 0) : -1;
    }
    if (t >= (long)L * N * K) return;
    const long r = t / K;
    const int k = (int)(t - r * K);
    const long long cls = y[r % N];
    if (!mmd_label_ok(cls, C)) {
        p[t] = 0.f;
        return;
    }
    const float tt = var_dim == VAR_DIAG ? T[(size_t)cls * K + k] : T[cls];
    p[t] = __fadd_rn(means[(size_t)cls * K + k], __fdiv_rn(eps[t], tt));
}

// k(d2) and, with DERIV, k'(d2) = d k / d d2: the terms in the order of the scales, each sum in fp32
template <bool DERIV>
__device__ __forceinline__ float mmd_kernel_value(const MmdKernel& kn, float d2, float& deriv) {
    float v = 0.f, dv = 0.f;
    for (int s = 0; s < kn.S; ++s) {
        if (kn.kind == MMD_IMQ) {
            const float t = __fadd_rn(kn.a[s], d2);
            const float q = __fdiv_rn(kn.a[s], t);
            v = s ? __fadd_rn(v, q) : q;
            if (DERIV) {
                const float dq = -__fdiv_rn(q, t);
                dv = s ? __fadd_rn(dv, dq) : dq;
            }
        } else {
            const float q = __builtin_amdgcn_exp2f(__fmul_rn(kn.a[s], d2));      // v_exp_f32
            v = s ? __fadd_rn(v, q) : q;
            if (DERIV) {
                const float dq = __fmul_rn(q, kn.b[s]);
                dv = s ? __fadd_rn(dv, dq) : dq;
            }
        }
    }
    deriv = dv;
    return v;
}

// A workgroup: rows [blockIdx.y * MMD_TI, +MMD_TI) of draw blockIdx.z, the column steps of piece blockIdx.x (BWD: blockIdx.x =
// piece * kchunks + kchunk).  Rows and columns beyond N and coordinates beyond K are staged as zeros and never stored.
template <bool BWD>
__global__ __launch_bounds__(256) void mmd_pair_kernel(const float* __restrict__ z, const float* __restrict__ p,
                                                       const int* __restrict__ group, const float* __restrict__ g, MmdKernel kn,
                                                       int L, int N, int K, int piece_steps, int kchunks, float c_within,
                                                       float c_cross, double* __restrict__ part) {
    constexpr int NB = BWD ? 4 : 3;
    __shared__ __attribute__((aligned(16))) float colz[MMD_TJ * (BWD ? MMD_KB : MMD_KC)];
    __shared__ __attribute__((aligned(16))) float colp[MMD_TJ * (BWD ? MMD_KB : MMD_KC)];
    __shared__ int colgrp[MMD_TJ];
    __shared__ float colg[MMD_TJ];
    __shared__ float wgt[BWD ? 4 * MMD_TJ * MMD_TI : 1];
    __shared__ double red[BWD ? 1 : 3 * 4 * MMD_TI];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int l = blockIdx.z;
    const int piece = BWD ? blockIdx.x / kchunks : blockIdx.x;
    const int kb0 = BWD ? (blockIdx.x - piece * kchunks) * MMD_KB : 0;
    const int row = blockIdx.y * MMD_TI + lane;
    const bool row_in = row < N;
    const float* zl = z + (size_t)(l + 1) * N * K;             // the draw's rows of z
    const float* pl = p + (size_t)l * N * K;
    const float* zr = zl + (size_t)(row_in ? row : 0) * K;
    const float* pr = pl + (size_t)(row_in ? row : 0) * K;
    const int grp = row_in ? group[row] : -1;
    const float gr = (BWD && row_in && g) ? g[row] : 0.f;

    double sum[3] = {0., 0., 0.};                             // forward: zz, pp, zp of the thread's columns
    double gz[BWD ? MMD_KW : 1], gp[BWD ? MMD_KW : 1];         // backward: the thread's coordinates
    float za[BWD ? MMD_KW : 1], pa[BWD ? MMD_KW : 1];
    if (BWD) {
#pragma unroll
        for (int k = 0; k < MMD_KW; ++k) {
            const int kk = kb0 + wv * MMD_KW + k;
            gz[k] = 0.; gp[k] = 0.;
            za[k] = (row_in && kk < K) ? zr[kk] : 0.f;
            pa[k] = (row_in && kk < K) ? pr[kk] : 0.f;
        }
    }

    const int steps = (N + MMD_TJ - 1) / MMD_TJ;
    const int s0 = piece * piece_steps, s1 = min(steps, s0 + piece_steps);
    for (int s = s0; s < s1; ++s) {                           // block-uniform
        const int j0 = s * MMD_TJ;
        float d2[NB][MMD_CW];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int c = 0; c < MMD_CW; ++c) d2[b][c] = 0.f;
        // ---- the squared distances of the step, MMD_KC coordinates at a time
        for (int k0 = 0; k0 < K; k0 += MMD_KC) {
            __syncthreads();
            {
                const int arr = tid >> 7, c = (tid >> 2) & (MMD_TJ - 1), k4 = (tid & 3) * 4;
                const int j = j0 + c;
                const float* src = (arr ? pl : zl) + (size_t)(j < N ? j : 0) * K;
                float* dst = (arr ? colp : colz) + c * MMD_KC + k4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int kk = k0 + k4 + e;
                    dst[e] = (j < N && kk < K) ? src[kk] : 0.f;
                }
                if (k0 == 0 && tid < MMD_TJ) {
                    const int jj = j0 + tid;
                    colgrp[tid] = jj < N ? group[jj] : -2;
                    colg[tid] = (BWD && jj < N && g) ? g[jj] : 0.f;
                }
            }
            float zk[MMD_KC], pk[MMD_KC];
#pragma unroll
            for (int e = 0; e < MMD_KC; ++e) {
                const int kk = k0 + e;
                zk[e] = (row_in && kk < K) ? zr[kk] : 0.f;
                pk[e] = (row_in && kk < K) ? pr[kk] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < MMD_CW; ++c) {
                const f32x4* cz = reinterpret_cast<const f32x4*>(colz + (wv * MMD_CW + c) * MMD_KC);
                const f32x4* cp = reinterpret_cast<const f32x4*>(colp + (wv * MMD_CW + c) * MMD_KC);
#pragma unroll
                for (int q = 0; q < MMD_KC / 4; ++q) {
                    const f32x4 vz = cz[q], vp = cp[q];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float a = zk[4 * q + e], b = pk[4 * q + e];
                        float d = __fsub_rn(a, vz[e]);
                        d2[0][c] = fmaf(d, d, d2[0][c]);
                        d = __fsub_rn(b, vp[e]);
                        d2[1][c] = fmaf(d, d, d2[1][c]);
                        d = __fsub_rn(a, vp[e]);
                        d2[2][c] = fmaf(d, d, d2[2][c]);
                        if (BWD) {
                            d = __fsub_rn(b, vz[e]);
                            d2[3][c] = fmaf(d, d, d2[3][c]);
                        }
                    }
                }
            }
        }
        // ---- the kernel values of the thread's columns
#pragma unroll
        for (int c = 0; c < MMD_CW; ++c) {
            const int cc = wv * MMD_CW + c, j = j0 + cc;
            const bool in = grp >= 0 && colgrp[cc] == grp;     // a padding column has the group -2
            const bool off = in && j != row;
            float dv[NB];
            float kv[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) kv[b] = mmd_kernel_value<BWD>(kn, d2[b][c], dv[b]);
            if (!BWD) {
                if (off) {
                    sum[0] += (double)kv[0];
                    sum[1] += (double)kv[1];
                }
                if (in) sum[2] += (double)kv[2];
            } else {
                // w = coefficient x 2 k': c_within = 2 / ((N-1) L), c_cross = -4 / (N L)
                const float gc = colg[cc];
                const float cw = __fmul_rn(__fadd_rn(gr, gc), c_within);
                float* w = wgt + cc * MMD_TI + lane;
                w[0 * MMD_TJ * MMD_TI] = off ? __fmul_rn(cw, dv[0]) : 0.f;
                w[1 * MMD_TJ * MMD_TI] = in ? __fmul_rn(__fmul_rn(gr, c_cross), dv[2]) : 0.f;
                w[2 * MMD_TJ * MMD_TI] = off ? __fmul_rn(cw, dv[1]) : 0.f;
                w[3 * MMD_TJ * MMD_TI] = in ? __fmul_rn(__fmul_rn(gc, c_cross), dv[3]) : 0.f;
            }
        }
        if (BWD) {
            // ---- the step's columns, the workgroup's MMD_KB coordinates, then the fp64 chains in ascending column order
            __syncthreads();                                  // the weights are written, the chunk tiles are read
            for (int e = tid; e < MMD_TJ * MMD_KB; e += 256) {
                const int c = e / MMD_KB, k = e - c * MMD_KB, j = j0 + c, kk = kb0 + k;
                const bool in = j < N && kk < K;
                colz[e] = in ? zl[(size_t)j * K + kk] : 0.f;
                colp[e] = in ? pl[(size_t)j * K + kk] : 0.f;
            }
            __syncthreads();
            for (int c = 0; c < MMD_TJ; ++c) {
                const float* w = wgt + c * MMD_TI + lane;
                const double wzz = (double)w[0], wzp = (double)w[MMD_TJ * MMD_TI], wpp = (double)w[2 * MMD_TJ * MMD_TI],
                             wpz = (double)w[3 * MMD_TJ * MMD_TI];
                const float* cz = colz + c * MMD_KB + wv * MMD_KW;
                const float* cp = colp + c * MMD_KB + wv * MMD_KW;
#pragma unroll
                for (int k = 0; k < MMD_KW; ++k) {
                    const double a = (double)za[k], b = (double)pa[k], vz = (double)cz[k], vp = (double)cp[k];
                    gz[k] = fma(wzz, a - vz, gz[k]);
                    gz[k] = fma(wzp, a - vp, gz[k]);
                    gp[k] = fma(wpp, b - vp, gp[k]);
                    gp[k] = fma(wpz, b - vz, gp[k]);
                }
            }
        }
    }
    if (!BWD) {
        // the four waves' sums in wave order
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 3; ++b) red[(b * 4 + wv) * MMD_TI + lane] = sum[b];
        __syncthreads();
        if (wv == 0 && row_in) {
            double* out = part + (((size_t)piece * L + l) * N + row) * 3;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const double* r = red + b * 4 * MMD_TI + lane;
                out[b] = ((r[0] + r[MMD_TI]) + r[2 * MMD_TI]) + r[3 * MMD_TI];
            }
        }
    } else if (row_in) {
        double* out = part + ((((size_t)piece * L + l) * N + row) * K) * 2;
#pragma unroll
        for (int k = 0; k < MMD_KW; ++k) {
            const int kk = kb0 + wv * MMD_KW + k;
            if (kk < K) {
                out[2 * (size_t)kk] = gz[k];
                out[2 * (size_t)kk + 1] = gp[k];
            }
        }
    }
}

// m_i: the pieces in piece order, the draws in draw order, all in fp64, rounded once
__global__ __launch_bounds__(256) void mmd_finish_kernel(const double* __restrict__ part, const int* __restrict__ group, int pieces,
                                                         int L, int N, float* __restrict__ m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    if (group[i] < 0) {
        m[i] = NAN;
        return;
    }
    const double within = N > 1 ? 1. / (double)(N - 1) : 0., cross = 2. / (double)N;
    double acc = 0.;
    for (int l = 0; l < L; ++l) {
        double s[3] = {0., 0., 0.};
        for (int pc = 0; pc < pieces; ++pc) {
            const double* r = part + (((size_t)pc * L + l) * N + i) * 3;
            s[0] += r[0]; s[1] += r[1]; s[2] += r[2];
        }
        acc += (s[0] * within + s[1] * within) - s[2] * cross;
    }
    m[i] = (float)(acc / (double)L);
}

// One workgroup per sample: g_z of its draws (the pieces in piece order, rounded once; row 0 zero) and, from g_p in fp64, its
// contributions to its class, the draws in sequence.
__global__ __launch_bounds__(256) void mmd_bwd_finish_kernel(const double* __restrict__ part, const int* __restrict__ group,
                                                             const float* __restrict__ eps, const long long* __restrict__ y,
                                                             const float* __restrict__ T, int var_dim, int pieces, int L, int N,
                                                             int K, float* __restrict__ g_z, double* __restrict__ gd,
                                                             double* __restrict__ gt) {
    __shared__ double red[16];
    const int i = blockIdx.x, tid = threadIdx.x;
    const bool ok = group[i] >= 0;                            // block-uniform
    const long long cls = ok ? y[i] : 0;
    double tsum = 0.;
    for (int k = tid; k < K; k += 256) {
        g_z[(size_t)i * K + k] = 0.f;                         // the mean latent takes no part
        double sm = 0., sT = 0.;
        if (ok) {
            const double t = (double)(var_dim == VAR_DIAG ? T[(size_t)cls * K + k] : T[cls]);
            const double rt2 = 1. / (t * t);
            for (int l = 0; l < L; ++l) {
                double a = 0., b = 0.;
                for (int pc = 0; pc < pieces; ++pc) {
                    const double* r = part + ((((size_t)pc * L + l) * N + i) * K + k) * 2;
                    a += r[0]; b += r[1];
                }
                g_z[((size_t)(l + 1) * N + i) * K + k] = (float)a;
                sm += b;
                sT -= b * ((double)eps[((size_t)l * N + i) * K + k] * rt2);
            }
        } else {
            for (int l = 0; l < L; ++l) g_z[((size_t)(l + 1) * N + i) * K + k] = NAN;
        }
        if (gd) gd[(size_t)i * K + k] = sm;
        if (gt && var_dim == VAR_DIAG) gt[(size_t)i * K + k] = sT;
        tsum += sT;
    }
    if (gt && var_dim != VAR_DIAG) {                          // the scalar factor: the sample's sum over k, a fixed order
        const double s = block_sum64(tsum, red);
        if (tid == 0) gt[i] = s;
    }
}

// -1: a malformed call; -2: a configuration this file does not compute; 0: fine
int mmd_vet(MmdKernel* kn, const float* z, const float* eps, const long long* y, const float* means, const float* T, int var_dim,
            int kind, const float* scales, int n_scales, int joint, int L, int N, int K, int C) {
    if (L < 1 || K < 1 || N < 0 || C < 1) return JVAE_EINVAL;
    if (var_dim < 0 || var_dim > 2 || kind < 0 || kind > 1 || joint < 0 || joint > 1) return JVAE_EINVAL;
    if (!scales || n_scales < 1 || n_scales > MMD_MAX_S) return JVAE_EINVAL;
    for (int s = 0; s < n_scales; ++s)
        if (!(scales[s] > 0.f) || !(scales[s] < INFINITY)) return JVAE_EINVAL;
    if (!means || !T) return JVAE_EINVAL;
    if (N > 0 && (!z || !eps || !y)) return JVAE_EINVAL;      // an empty batch has no per-sample arrays
    if (var_dim > VAR_DIAG || K > MMD_MAX_K || N > MMD_MAX_N || L > MMD_MAX_L) return JVAE_ENOTSUP;
    if ((long)C * K > 0x7fffffffL) return JVAE_ENOTSUP;
    kn->kind = kind;
    kn->S = n_scales;
    for (int s = 0; s < MMD_MAX_S; ++s) {
        const double v = s < n_scales ? (double)scales[s] : 1.;
        kn->a[s] = kind == MMD_IMQ ? (float)v : (float)(-1.4426950408889634074 / (2. * v));
        kn->b[s] = (float)(-1. / (2. * v));
    }
    return 0;
}

}  // namespace

extern "C" {

int jvae_mmd_tile(void) { return MMD_TI; }

size_t jvae_mmd_fwd_workspace_bytes(int L, int N, int K) { return mmd_in_range(L, N, K) ? mmd_ws_layout(nullptr, nullptr, L, N, K, false) : 0; }

size_t jvae_mmd_bwd_workspace_bytes(int L, int N, int K) { return mmd_in_range(L, N, K) ? mmd_ws_layout(nullptr, nullptr, L, N, K, true) : 0; }

int jvae_mmd_objective_fwd_f32(const float* z, const float* eps_p, const long long* y, const float* means, const float* T,
                               int var_dim, int kind, const float* scales, int n_scales, int joint, int L, int N, int K, int C,
                               float* m, void* ws, size_t ws_bytes, void* stream) {
    MmdKernel kn;
    const int rc = mmd_vet(&kn, z, eps_p, y, means, T, var_dim, kind, scales, n_scales, joint, L, N, K, C);
    if (rc) return rc;
    if (N == 0) return 0;
    if (!m || !ws || ((uintptr_t)ws & 15)) return JVAE_EINVAL;
    if (ws_bytes < jvae_mmd_fwd_workspace_bytes(L, N, K)) return JVAE_EWORKSPACE;
    MmdWs w;
    mmd_ws_layout(&w, (char*)ws, L, N, K, false);
    hipStream_t st = (hipStream_t)stream;
    const long elems = (long)L * N * K;
    mmd_prepare_kernel<<<cdiv(elems > N ? elems : N, 256), 256, 0, st>>>(eps_p, y, means, T, w.p, w.group, var_dim, joint, L, N, K, C);
    JVAE_LAUNCH_CHECK();
    const int piece_steps = mmd_piece_steps(L, N, 1, MMD_FWD_GRID), pieces = mmd_pieces(N, piece_steps);
    const dim3 grid((unsigned)pieces, (unsigned)cdiv(N, MMD_TI), (unsigned)L);
    mmd_pair_kernel<false><<<grid, 256, 0, st>>>(z, w.p, w.group, nullptr, kn, L, N, K, piece_steps, 1, 0.f, 0.f, w.part);
    JVAE_LAUNCH_CHECK();
    mmd_finish_kernel<<<cdiv(N, 256), 256, 0, st>>>(w.part, w.group, pieces, L, N, m);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_mmd_objective_bwd_f32(const float* g_m, const float* z, const float* eps_p, const long long* y, const float* means,
                               const float* T, int var_dim, int kind, const float* scales, int n_scales, int joint, int L, int N,
                               int K, int C, float* g_z, float* g_means, float* g_T, void* ws, size_t ws_bytes, void* stream) {
    MmdKernel kn;
    const int rc = mmd_vet(&kn, z, eps_p, y, means, T, var_dim, kind, scales, n_scales, joint, L, N, K, C);
    if (rc) return rc;
    if (N > 0 && !g_z) return JVAE_EINVAL;
    const bool fold = g_means || g_T;
    if (N > 0 || fold) {
        if (!ws || ((uintptr_t)ws & 15)) return N > 0 ? JVAE_EINVAL : JVAE_EWORKSPACE;
        if (N > 0 && ws_bytes < jvae_mmd_bwd_workspace_bytes(L, N, K)) return JVAE_EWORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    MmdWs w = {};
    if (N > 0) {
        mmd_ws_layout(&w, (char*)ws, L, N, K, true);
        const long elems = (long)L * N * K;
        mmd_prepare_kernel<<<cdiv(elems > N ? elems : N, 256), 256, 0, st>>>(eps_p, y, means, T, w.p, w.group, var_dim, joint, L, N, K,
                                                                             C);
        JVAE_LAUNCH_CHECK();
        const int kchunks = cdiv(K, MMD_KB);
        const int piece_steps = mmd_piece_steps(L, N, kchunks, MMD_BWD_GRID), pieces = mmd_pieces(N, piece_steps);
        const float c_within = N > 1 ? (float)(2. / ((double)(N - 1) * (double)L)) : 0.f;
        const float c_cross = (float)(-4. / ((double)N * (double)L));
        const dim3 grid((unsigned)(pieces * kchunks), (unsigned)cdiv(N, MMD_TI), (unsigned)L);
        mmd_pair_kernel<true><<<grid, 256, 0, st>>>(z, w.p, w.group, g_m, kn, L, N, K, piece_steps, kchunks, c_within, c_cross, w.part);
        JVAE_LAUNCH_CHECK();
        mmd_bwd_finish_kernel<<<N, 256, 0, st>>>(w.part, w.group, eps_p, y, T, var_dim, pieces, L, N, K, g_z, g_means ? w.gd : nullptr,
                                                 g_T ? w.gt : nullptr);
        JVAE_LAUNCH_CHECK();
    }
    else {
        w.gd = w.gt = (double*)ws;                            // N = 0: the class sums are empty sums, zeros are written, nothing is read
    }
    if (g_means) {
        iw_class_fold_kernel<<<dim3(cdiv((long)C * K, 64), 1), dim3(1024), 0, st>>>((const double*)w.gd, g_means, nullptr, nullptr, y, N, C, K);
        JVAE_LAUNCH_CHECK();
    }
    if (g_T) {
        const int KT = var_dim == VAR_DIAG ? K : 1;
        iw_class_fold_kernel<<<dim3(cdiv((long)C * KT, 64), 1), dim3(1024), 0, st>>>((const double*)w.gt, g_T, nullptr, nullptr, y, N, C, KT);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

}  // extern "C"
