// 2-D pictures of recorded latents (reference ft/inspection.py::proj2d, there through scikit-learn's PCA and TSNE): the exact
// t-SNE of N <= 16384 points and the moments / projection of a PCA, on the device.
//
// Pairwise squared distances   x (N, K) fp32 -> d (N, N) fp32, d_ij = fp32(sum_k (double(x_ik) - double(x_jk))^2), k ascending,
//                              every difference, square and sum rounded on its own: (a - b)^2 == (b - a)^2, so d is exactly
//                              symmetric and its diagonal exactly 0.
// Perplexity search            scikit-learn's _binary_search_perplexity in fp64, one workgroup per row with the row of distances in
//                              LDS (64 KiB at the cap of N): beta from 1, at most 100 steps, p_j = exp(-d_ij beta) (j != i),
//                              S = sum p_j (0 -> 1e-8f), H = log S + beta sum d_ij p_j / S, stop at |H - log perplexity| <= 1e-5f
//                              (both constants are C floats there and are widened as such here), else double / halve beta while
//                              the other bound is infinite, else bisect.  Out: beta_i, S_i - never an N^2 fp64 matrix.
// Joint probabilities          P_ij = max((p_j|i + p_i|j) / max(sum P, eps), eps), eps = 2^-52, formed in fp64 from d, beta, S and
//                              stored as fp32 (N, N); sum P = 2 sum_i (sum_j p_j|i) from the rows' fp64 sums.  The diagonal is 0
//                              before the floor (eps after it) and is never read by the gradient.
// Gradient                     qn_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} qn_ij,
//                              g_i = 4 (f sum_j P_ij qn_ij (y_i - y_j) - sum_j qn_ij^2 (y_i - y_j) / Z): the separable form, Z
//                              applied at the end, all in fp64, one rounding to fp32.  As in scikit-learn, the distance inside
//                              qn is taken on the widened y (pdist), the FACTOR y_i - y_j is the fp32 difference, widened
//                              (`X_embedded[i] - X_embedded` on the fp32 embedding).  scikit-learn's floor Q >= eps is not
//                              applied (it moves a term by at most eps qn |dy|).  One wave per row i, the y_j in LDS tiles.
// KL and norm (on request)     KL = sum_{i != j} f P_ij log(max(f P_ij, eps) / max(qn_ij / Z, eps)) and |g|_2, two fp64 words.
// Update                       scikit-learn's _gradient_descent step as numpy executes it on fp32 arrays, bit for bit.
// PCA moments                  column means and the centred covariance / (N - 1), fp64, over a split of N that hangs on N alone.
// Projection                   (x - mean) V^T, fp64 accumulation with k ascending, fp32 out.
//
// Every sum is a fixed-order reduction: per-thread strided partials, xor butterfly inside a wave, the waves in sequence, the
// tiles and slabs in ascending order.  No float atomics: the same bits run to run.  Floating-point contraction is off for the
// whole file (the Makefile says so as well): the pairwise distances and the update are held to numpy's roundings bit for bit.
#include "common.h"
#include "jvae_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int EMB_MAX_N = 16384;       // a row of fp32 distances in LDS: 64 KiB
constexpr int EMB_MAX_K = 1024;
constexpr int EMB_MAX_COMPONENTS = 16;
constexpr long EMB_MAX_ROWS = 1L << 24;    // PCA rows
constexpr double EMB_EPS = 2.220446049250313e-16;
constexpr int EMB_BLOCK = 256;
constexpr int EMB_YTILE = 1024;        // y_j per LDS tile of the gradient passes
constexpr int EMB_PCA_SLAB = 1024;     // rows per slab of the PCA sums, at most EMB_PCA_MAX_SLABS slabs
constexpr int EMB_PCA_MAX_SLABS = 8;

inline size_t emb_align(size_t b) { return (b + 255) & ~(size_t)255; }

// ------------------------------------------------------------------------------------------------- pairwise distances
constexpr int PD_TILE = 16, PD_KC = 64;
__global__ __launch_bounds__(PD_TILE* PD_TILE) void emb_sqdist_kernel(const float* __restrict__ x, float* __restrict__ d, int N,
                                                                       int K) {
    __shared__ float xi[PD_TILE][PD_KC + 1], xj[PD_TILE][PD_KC + 1];
    const int tx = threadIdx.x % PD_TILE, ty = threadIdx.x / PD_TILE;
    const int i0 = blockIdx.y * PD_TILE, j0 = blockIdx.x * PD_TILE;
    double acc = 0.;
    for (int k0 = 0; k0 < K; k0 += PD_KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < PD_TILE * PD_KC; e += PD_TILE * PD_TILE) {
            const int r = e / PD_KC, k = e % PD_KC;
            const bool kin = k0 + k < K;
            xi[r][k] = kin && i0 + r < N ? x[(size_t)(i0 + r) * K + k0 + k] : 0.f;
            xj[r][k] = kin && j0 + r < N ? x[(size_t)(j0 + r) * K + k0 + k] : 0.f;
        }
        __syncthreads();
        const int kn = K - k0 < PD_KC ? K - k0 : PD_KC;
        for (int k = 0; k < kn; ++k) {
            const double t = (double)xi[ty][k] - (double)xj[tx][k];
            const double s = t * t;
            acc = acc + s;
        }
    }
    const int i = i0 + ty, j = j0 + tx;
    if (i < N && j < N) d[(size_t)i * N + j] = (float)acc;
}

// ---------------------------------------------------------------------------------------------------- perplexity search
__global__ __launch_bounds__(EMB_BLOCK) void emb_search_kernel(const float* __restrict__ d, double* __restrict__ beta_out,
                                                               double* __restrict__ s_out, double* __restrict__ rowsum, int N,
                                                               double desired_entropy) {
    extern __shared__ float emb_row[];
    __shared__ double red[2][4];
    const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int j = t; j < N; j += EMB_BLOCK) emb_row[j] = d[(size_t)i * N + j];
    __syncthreads();
    const double tol = (double)1e-5f, s_floor = (double)1e-8f;
    double beta = 1., used = 1., bmin = -INFINITY, bmax = INFINITY, S = 1.;
    for (int step = 0; step < 100; ++step) {
        double s = 0., sd = 0.;
        for (int j = t; j < N; j += EMB_BLOCK) {
            if (j == i) continue;
            const float dist = emb_row[j];
            const double p = exp((double)(-dist) * beta);
            s += p;
            sd += (double)dist * p;
        }
        s = wave_sum64(s);
        sd = wave_sum64(sd);
        __syncthreads();
        if (lane == 0) { red[0][w] = s; red[1][w] = sd; }
        __syncthreads();
        S = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double SD = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        if (S == 0.) S = s_floor;
        used = beta;
        const double diff = log(S) + beta * (SD / S) - desired_entropy;
        if (fabs(diff) <= tol) break;
        if (diff > 0.) {
            bmin = beta;
            beta = bmax == INFINITY ? beta * 2. : (beta + bmax) / 2.;
        } else {
            bmax = beta;
            beta = bmin == -INFINITY ? beta / 2. : (beta + bmin) / 2.;
        }
    }
    double rs = 0.;
    for (int j = t; j < N; j += EMB_BLOCK)
        if (j != i) rs += exp((double)(-emb_row[j]) * used) / S;
    rs = wave_sum64(rs);
    __syncthreads();
    if (lane == 0) red[0][w] = rs;
    __syncthreads();
    if (t == 0) {
        beta_out[i] = used;
        s_out[i] = S;
        rowsum[i] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    }
}

// out[0] = scale * sum_i v[i * stride] in a fixed order (one workgroup of 1024)
__global__ __launch_bounds__(1024) void emb_total_kernel(const double* __restrict__ v, double* __restrict__ out, int n, int stride,
                                                         double scale) {
    __shared__ double red[16];
    double s = 0.;
    for (int i = threadIdx.x; i < n; i += 1024) s += v[(size_t)i * stride];
    s = block_sum64(s, red);
    if (threadIdx.x == 0) out[0] = scale * s;
}

__global__ __launch_bounds__(EMB_BLOCK) void emb_joint_kernel(const float* __restrict__ d, const double* __restrict__ beta,
                                                              const double* __restrict__ S, const double* __restrict__ total,
                                                              float* __restrict__ P, int N) {
    const int j = blockIdx.x * EMB_BLOCK + threadIdx.x, i = blockIdx.y;
    if (j >= N) return;
    const double sum_p = fmax(total[0], EMB_EPS);
    double both = 0.;
    if (i != j) {
        const float dist = d[(size_t)i * N + j];
        const double a = exp((double)(-dist) * beta[i]) / S[i], b = exp((double)(-dist) * beta[j]) / S[j];
        both = i < j ? a + b : b + a;
    }
    P[(size_t)i * N + j] = (float)fmax(both / sum_p, EMB_EPS);
}

// -------------------------------------------------------------------------------------------------------------- gradient
// One wave per row i, four rows per workgroup; the y_j in LDS tiles.  KL = false: rows[5 i ..] = sum_j f P qn dy (2), sum_j
// qn^2 dy (2), sum_j qn.  KL = true: rows[i] = sum_j f P log(max(f P, eps) / max(qn / Z, eps)).
template <bool KL>
__global__ __launch_bounds__(EMB_BLOCK) void emb_pairs_kernel(const float* __restrict__ P, const float* __restrict__ y,
                                                              double* __restrict__ rows, const double* __restrict__ zsum, int N,
                                                              double f) {
    __shared__ float ys[EMB_YTILE][2];
    const int t = threadIdx.x, lane = t & 63, i = blockIdx.x * (EMB_BLOCK / 64) + (t >> 6);
    const bool valid = i < N;
    const float yf0 = valid ? y[2 * (size_t)i] : 0.f, yf1 = valid ? y[2 * (size_t)i + 1] : 0.f;
    const double yi0 = (double)yf0, yi1 = (double)yf1;
    const double Z = KL ? zsum[0] : 1.;
    double a0 = 0., a1 = 0., b0 = 0., b1 = 0., z = 0.;
    for (int j0 = 0; j0 < N; j0 += EMB_YTILE) {
        __syncthreads();
        for (int e = t; e < EMB_YTILE; e += EMB_BLOCK)
            if (j0 + e < N) { ys[e][0] = y[2 * (size_t)(j0 + e)]; ys[e][1] = y[2 * (size_t)(j0 + e) + 1]; }
        __syncthreads();
        if (!valid) continue;
        const int jn = N - j0 < EMB_YTILE ? N - j0 : EMB_YTILE;
        for (int jj = lane; jj < jn; jj += 64) {
            const int j = j0 + jj;
            if (j == i) continue;
            const double d0 = yi0 - (double)ys[jj][0], d1 = yi1 - (double)ys[jj][1];
            const double qn = 1. / (1. + (d0 * d0 + d1 * d1));
            const double fp = f * (double)P[(size_t)i * N + j];
            if (KL) {
                a0 += fp * log(fmax(fp, EMB_EPS) / fmax(qn / Z, EMB_EPS));
            } else {
                // the factor y_i - y_j of the gradient is scikit-learn's `X_embedded[i] - X_embedded`: an fp32 difference
                const double e0 = (double)(yf0 - ys[jj][0]), e1 = (double)(yf1 - ys[jj][1]);
                const double pq = fp * qn, q2 = qn * qn;
                a0 += pq * e0; a1 += pq * e1;
                b0 += q2 * e0; b1 += q2 * e1;
                z += qn;
            }
        }
    }
    a0 = wave_sum64(a0);
    if (KL) {
        if (valid && lane == 0) rows[i] = a0;
        return;
    }
    a1 = wave_sum64(a1); b0 = wave_sum64(b0); b1 = wave_sum64(b1); z = wave_sum64(z);
    if (valid && lane == 0) {
        double* r = rows + 5 * (size_t)i;
        r[0] = a0; r[1] = a1; r[2] = b0; r[3] = b1; r[4] = z;
    }
}

// Z = sum_i rows[5 i + 4] in a fixed order, then g_i = fp32(4 (A_i - B_i / Z))
__global__ __launch_bounds__(1024) void emb_grad_fold_kernel(const double* __restrict__ rows, double* __restrict__ zsum,
                                                             float* __restrict__ g, int N) {
    __shared__ double red[16];
    double s = 0.;
    for (int i = threadIdx.x; i < N; i += 1024) s += rows[5 * (size_t)i + 4];
    const double Z = block_sum64(s, red);
    if (threadIdx.x == 0) zsum[0] = Z;
    for (int i = threadIdx.x; i < N; i += 1024) {
        const double* r = rows + 5 * (size_t)i;
        g[2 * (size_t)i] = (float)(4. * (r[0] - r[2] / Z));
        g[2 * (size_t)i + 1] = (float)(4. * (r[1] - r[3] / Z));
    }
}

// stats[0] = sum_i kl[i] (when kl), stats[1] = |g|_2 over n values: fixed order, one workgroup
__global__ __launch_bounds__(1024) void emb_stats_kernel(const double* __restrict__ kl, const float* __restrict__ g,
                                                         double* __restrict__ stat_kl, double* __restrict__ stat_norm, int N,
                                                         long n) {
    __shared__ double red[16];
    if (stat_kl) {
        double s = 0.;
        for (int i = threadIdx.x; i < N; i += 1024) s += kl[i];
        s = block_sum64(s, red);
        if (threadIdx.x == 0) stat_kl[0] = s;
    }
    double q = 0.;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const double v = (double)g[i];
        q += v * v;
    }
    q = block_sum64(q, red);
    if (threadIdx.x == 0) stat_norm[0] = sqrt(q);
}

// ---------------------------------------------------------------------------------------------------------------- update
__global__ __launch_bounds__(EMB_BLOCK) void emb_update_kernel(float* __restrict__ y, float* __restrict__ update,
                                                               float* __restrict__ gains, float* __restrict__ g, float momentum,
                                                               float lr, long n) {
    const long i = (long)blockIdx.x * EMB_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float u = update[i], gr = g[i];
    const float sign = u * gr;                     // numpy's `update * grad < 0.0`: an fp32 product (it may underflow to 0)
    float gain = gains[i];
    gain = sign < 0.f ? gain + 0.2f : gain * 0.8f;
    gain = gain < 0.01f ? 0.01f : gain;            // np.clip(gains, 0.01, inf): a NaN stays
    const float scaled = gr * gain;
    const float mu = momentum * u, step = lr * scaled;
    const float nu = mu - step;
    gains[i] = gain;
    g[i] = scaled;
    update[i] = nu;
    y[i] = y[i] + nu;
}

// ------------------------------------------------------------------------------------------------------------------- PCA
inline int pca_slabs(long N) {
    const long s = (N + EMB_PCA_SLAB - 1) / EMB_PCA_SLAB;
    return (int)(s < 1 ? 1 : (s > EMB_PCA_MAX_SLABS ? EMB_PCA_MAX_SLABS : s));
}
struct SlabRange { long nb, ne; };
__host__ __device__ __forceinline__ SlabRange pca_range(long N, int slabs, int s) {
    const long per = (N + slabs - 1) / slabs, b = (long)s * per, e = b + per;
    SlabRange r;
    r.nb = b < N ? b : N;
    r.ne = e < N ? e : N;
    return r;
}

__global__ __launch_bounds__(EMB_BLOCK) void pca_colsum_kernel(const float* __restrict__ x, double* __restrict__ part, long N, int K,
                                                               int slabs) {
    const int k = blockIdx.x * EMB_BLOCK + threadIdx.x, s = blockIdx.y;
    if (k >= K) return;
    const SlabRange r = pca_range(N, slabs, s);
    double acc = 0.;
    for (long n = r.nb; n < r.ne; ++n) acc += (double)x[(size_t)n * K + k];
    part[(size_t)s * K + k] = acc;
}

__global__ __launch_bounds__(EMB_BLOCK) void pca_mean_kernel(const double* __restrict__ part, double* __restrict__ mean, long N,
                                                             int K, int slabs) {
    const int k = blockIdx.x * EMB_BLOCK + threadIdx.x;
    if (k >= K) return;
    double acc = 0.;
    for (int s = 0; s < slabs; ++s) acc += part[(size_t)s * K + k];
    mean[k] = acc / (double)N;
}

constexpr int PCA_TILE = 16, PCA_RC = 16;
__global__ __launch_bounds__(PCA_TILE* PCA_TILE) void pca_cov_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                                      double* __restrict__ part, long N, int K, int slabs) {
    __shared__ double xa[PCA_RC][PCA_TILE], xb[PCA_RC][PCA_TILE + 1];
    const int tx = threadIdx.x % PCA_TILE, ty = threadIdx.x / PCA_TILE;
    const int a0 = blockIdx.y * PCA_TILE, b0 = blockIdx.x * PCA_TILE, s = blockIdx.z;
    const SlabRange r = pca_range(N, slabs, s);
    const double ma = a0 + tx < K ? mean[a0 + tx] : 0., mb = b0 + tx < K ? mean[b0 + tx] : 0.;
    double acc = 0.;
    for (long n0 = r.nb; n0 < r.ne; n0 += PCA_RC) {
        __syncthreads();
        {   // thread (ty, tx) stages row n0 + ty, columns a0 + tx and b0 + tx, centred in fp64
            const long n = n0 + ty;
            const bool in = n < r.ne;
            xa[ty][tx] = in && a0 + tx < K ? (double)x[(size_t)n * K + a0 + tx] - ma : 0.;
            xb[ty][tx] = in && b0 + tx < K ? (double)x[(size_t)n * K + b0 + tx] - mb : 0.;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < PCA_RC; ++rr) {
            const double p = xa[rr][ty] * xb[rr][tx];
            acc = acc + p;
        }
    }
    const int a = a0 + ty, b = b0 + tx;
    if (a < K && b < K) part[((size_t)s * K + a) * K + b] = acc;
}

__global__ __launch_bounds__(EMB_BLOCK) void pca_cov_fold_kernel(const double* __restrict__ part, double* __restrict__ cov, long N,
                                                                 int K, int slabs) {
    const size_t e = (size_t)blockIdx.x * EMB_BLOCK + threadIdx.x, KK = (size_t)K * K;
    if (e >= KK) return;
    double acc = 0.;
    for (int s = 0; s < slabs; ++s) acc += part[(size_t)s * KK + e];
    cov[e] = acc / (double)(N - 1);
}

__global__ __launch_bounds__(EMB_BLOCK) void emb_project_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                                const double* __restrict__ V, float* __restrict__ out, long N, int K,
                                                                int C) {
    const long e = (long)blockIdx.x * EMB_BLOCK + threadIdx.x;
    if (e >= N * C) return;
    const long n = e / C;
    const int c = (int)(e % C);
    const float* xr = x + (size_t)n * K;
    const double* v = V + (size_t)c * K;
    double acc = 0.;
    for (int k = 0; k < K; ++k) {
        const double p = ((double)xr[k] - mean[k]) * v[k];
        acc = acc + p;
    }
    out[e] = (float)acc;
}

struct PcaWs { size_t colsum, cov, total; };
inline PcaWs pca_ws(long N, int K) {
    const int S = pca_slabs(N);
    PcaWs w;
    w.colsum = 0;
    w.cov = emb_align(sizeof(double) * (size_t)S * K);
    w.total = w.cov + emb_align(sizeof(double) * (size_t)S * K * K);
    return w;
}

// rows (5 N), Z (1), KL rows (N)
struct GradWs { size_t rows, z, kl, total; };
inline GradWs grad_ws(int N) {
    GradWs w;
    w.rows = 0;
    w.z = emb_align(sizeof(double) * 5 * (size_t)N);
    w.kl = w.z + 256;
    w.total = w.kl + emb_align(sizeof(double) * (size_t)N);
    return w;
}

inline int emb_check_n(long N) { return N < 2 ? JVAE_EINVAL : (N > EMB_MAX_N ? JVAE_ENOTSUP : 0); }

}  // namespace

extern "C" {

int jvae_pairwise_sqdist_f32(const float* x, float* d, int N, int K, void* stream) {
    if (!x || !d || K < 1) return JVAE_EINVAL;
    if (const int rc = emb_check_n(N)) return rc;
    if (K > EMB_MAX_K) return JVAE_ENOTSUP;
    const unsigned tiles = (unsigned)cdiv(N, PD_TILE);
    emb_sqdist_kernel<<<dim3(tiles, tiles), PD_TILE * PD_TILE, 0, (hipStream_t)stream>>>(x, d, N, K);
    JVAE_LAUNCH_CHECK();
    return 0;
}

size_t jvae_tsne_affinities_workspace_bytes(int N) {
    if (emb_check_n(N)) return 0;
    return emb_align(sizeof(double) * (size_t)N) + 256;
}

int jvae_tsne_affinities_f32(const float* d, float* P, double* beta, double* S, float perplexity, int N, void* ws, size_t ws_bytes,
                             void* stream) {
    if (!d || !P || !beta || !S || !ws || !(perplexity > 0.f)) return JVAE_EINVAL;
    if (const int rc = emb_check_n(N)) return rc;
    if (ws_bytes < jvae_tsne_affinities_workspace_bytes(N)) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 7) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double* rowsum = (double*)ws;
    double* total = (double*)((char*)ws + emb_align(sizeof(double) * (size_t)N));
    const int lds = (int)(sizeof(float) * (size_t)N);
    static int lds_set = 0;
    if (lds > lds_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&emb_search_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * EMB_MAX_N));
        if (e != hipSuccess) return (int)e;
        lds_set = (int)(sizeof(float) * EMB_MAX_N);
    }
    emb_search_kernel<<<N, EMB_BLOCK, lds, st>>>(d, beta, S, rowsum, N, log((double)perplexity));
    JVAE_LAUNCH_CHECK();
    emb_total_kernel<<<1, 1024, 0, st>>>(rowsum, total, N, 1, 2.);
    JVAE_LAUNCH_CHECK();
    emb_joint_kernel<<<dim3((unsigned)cdiv(N, EMB_BLOCK), (unsigned)N), EMB_BLOCK, 0, st>>>(d, beta, S, total, P, N);
    JVAE_LAUNCH_CHECK();
    return 0;
}

size_t jvae_tsne_gradient_workspace_bytes(int N) {
    if (emb_check_n(N)) return 0;
    return grad_ws(N).total;
}

int jvae_tsne_gradient_f32(const float* P, const float* y, float* g, float exaggeration, int N, double* stats, void* ws,
                           size_t ws_bytes, void* stream) {
    if (!P || !y || !g || !ws || !(exaggeration > 0.f)) return JVAE_EINVAL;
    if (const int rc = emb_check_n(N)) return rc;
    const GradWs w = grad_ws(N);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 7) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double* rows = (double*)((char*)ws + w.rows);
    double* z = (double*)((char*)ws + w.z);
    double* kl = (double*)((char*)ws + w.kl);
    const unsigned blocks = (unsigned)cdiv(N, EMB_BLOCK / 64);
    emb_pairs_kernel<false><<<blocks, EMB_BLOCK, 0, st>>>(P, y, rows, z, N, (double)exaggeration);
    JVAE_LAUNCH_CHECK();
    emb_grad_fold_kernel<<<1, 1024, 0, st>>>(rows, z, g, N);
    JVAE_LAUNCH_CHECK();
    if (stats) {
        emb_pairs_kernel<true><<<blocks, EMB_BLOCK, 0, st>>>(P, y, kl, z, N, (double)exaggeration);
        JVAE_LAUNCH_CHECK();
        emb_stats_kernel<<<1, 1024, 0, st>>>(kl, g, stats, stats + 1, N, 2L * N);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

int jvae_tsne_update_f32(float* y, float* update, float* gains, float* g, float momentum, float lr, int N, double* norm,
                         void* stream) {
    if (!y || !update || !gains || !g) return JVAE_EINVAL;
    if (const int rc = emb_check_n(N)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const long n = 2L * N;
    emb_update_kernel<<<(unsigned)cdiv(n, EMB_BLOCK), EMB_BLOCK, 0, st>>>(y, update, gains, g, momentum, lr, n);
    JVAE_LAUNCH_CHECK();
    if (norm) {
        emb_stats_kernel<<<1, 1024, 0, st>>>(nullptr, g, nullptr, norm, N, n);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}

size_t jvae_pca_moments_workspace_bytes(long N, int K) {
    if (N < 2 || N > EMB_MAX_ROWS || K < 1 || K > EMB_MAX_K) return 0;
    return pca_ws(N, K).total;
}

int jvae_pca_moments_f32(const float* x, double* mean, double* cov, long N, int K, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !mean || !cov || !ws || K < 1 || N < 2) return JVAE_EINVAL;
    if (K > EMB_MAX_K || N > EMB_MAX_ROWS) return JVAE_ENOTSUP;
    const PcaWs w = pca_ws(N, K);
    if (ws_bytes < w.total) return JVAE_EWORKSPACE;
    if (((uintptr_t)ws & 7) != 0) return JVAE_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int S = pca_slabs(N);
    double* colsum = (double*)((char*)ws + w.colsum);
    double* part = (double*)((char*)ws + w.cov);
    const unsigned kb = (unsigned)cdiv(K, EMB_BLOCK), kt = (unsigned)cdiv(K, PCA_TILE);
    pca_colsum_kernel<<<dim3(kb, (unsigned)S), EMB_BLOCK, 0, st>>>(x, colsum, N, K, S);
    JVAE_LAUNCH_CHECK();
    pca_mean_kernel<<<kb, EMB_BLOCK, 0, st>>>(colsum, mean, N, K, S);
    JVAE_LAUNCH_CHECK();
    pca_cov_kernel<<<dim3(kt, kt, (unsigned)S), PCA_TILE * PCA_TILE, 0, st>>>(x, mean, part, N, K, S);
    JVAE_LAUNCH_CHECK();
    pca_cov_fold_kernel<<<(unsigned)cdiv((long)K * K, EMB_BLOCK), EMB_BLOCK, 0, st>>>(part, cov, N, K, S);
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_project_f32(const float* x, const double* mean, const double* V, float* out, long N, int K, int n_components,
                     void* stream) {
    if (!x || !mean || !V || !out || K < 1 || N < 1 || n_components < 1) return JVAE_EINVAL;
    if (K > EMB_MAX_K || N > EMB_MAX_ROWS || n_components > EMB_MAX_COMPONENTS) return JVAE_ENOTSUP;
    emb_project_kernel<<<(unsigned)cdiv(N * n_components, EMB_BLOCK), EMB_BLOCK, 0, (hipStream_t)stream>>>(x, mean, V, out, N, K,
                                                                                                           n_components);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
