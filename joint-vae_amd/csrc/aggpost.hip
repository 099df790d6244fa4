// The aggregate posterior of a bank of N diagonal Gaussians (Hoffman & Johnson 2016, "ELBO surgery"; Chen et al. 2018, beta-TCVAE;
// DESIGN.md section 7u): log q(z) = log 1/|S| sum_{n in S} N(z; mu_n, diag e^{lv_n}) at M queries, and optionally the same for every
// coordinate alone, with S the whole bank or the rows of the query's group.  No (M, N) or (M, N, K) array exists anywhere.
//
// Stored operands (jvae_aggpost_prepare_f32, once per bank).  w = fp32(exp(-(double)lv)), c_n = fp32(sum_k (double)lv_nk), k
// ascending; mu, w and lv are stored k-major, (K, Np) with Np = N rounded up to AGP_TILE (padding rows are zeros and are masked,
// never read as terms), so that a tile of bank rows is a run of floats for every k.
//
// Arithmetic.  A pair (query m, bank row n) has Q = c_n + sum_k (z_mk - mu_nk)^2 w_nk: the fmaf chain acc = fmaf(d * d, w, acc)
// from acc = c_n on, k ascending, d = z - mu and d * d rounded on their own (built with -ffp-contract=off) - the direct form; its
// bits hang on (z_m, row n, K) alone, whichever tile, wave or piece meets the pair.  The pair's term is 2^(kk (Q - a)) with kk =
// -log2(e) / 2 and a the smallest Q of the sum: the DIFFERENCE is taken before the product (kk Q itself is only known to 2^-24 of
// its size, thousands of units for a far query), so the largest term of every sum is exactly 1, no exponent is positive and the
// sum is finite and >= 1 however far the query is.  A coordinate's term is the same with Q = fmaf(d * d, w, lv).
//
// Partition.  The bank is cut into pieces of AGP_PART rows whatever M and the grid are.  A workgroup owns AGP_QT queries (one per
// lane) and ONE piece; wave v of its four takes rows 16 v .. 16 v + 15 of every 64-row tile of the piece (joint launch) or rows
// 64 v .. 64 v + 63 of every 256-row tile (marginal launch).  A wave forms the terms of 16 (8) rows at a time: their smallest Q
// (exact, no order), the terms against it added as a tree, and the result folded into its running (a, s):
//   a' = min(a, a_t),  s' = s 2^(kk (a - a')) + s_t 2^(kk (a_t - a'))      (one of the two factors is exactly 1)
// in the tiles' order; the four waves meet through LDS as a tree, a piece leaves (a, s) and the number of rows of the query's
// group in the workspace, and the merge launch folds the pieces in their order the same way (pairwise: a binary counter) and ends
// in fp64: log q = -a / 2 + ln s - ln |S| - (K / 2) ln 2 pi, rounded once.  No floating-point atomics: a second run, another M or
// a subset of the queries give the same bits.
//
// Masked rows (padding, another group) have Q = +inf: their term is exactly +0 and they are in no minimum.  A query whose group has
// no row gets -inf and AGP_STATUS_EMPTY.  A query with a NaN gets NaN, one with an infinite element -inf, and so does a finite
// query so far away that every Q overflows fp32; they set AGP_STATUS_QUERY.  A non-finite stored operand sets AGP_STATUS_BANK (the
// workgroups of the first query tile look at what they stage).  The status word only ever takes an integer OR.
//
// Limits: 1 <= K <= AGP_MAX_K, 1 <= N <= AGP_MAX_BANK (so at most AGP_MAX_BANK / AGP_PART = 16384 pieces, the binary counter of
// the merge holds 2^AGP_STACK), 1 <= M < 2^31.
// The prepare, joint and marginal kernels and the fold live in aggpost_core.h: csrc/tcvae.hip launches them on a batch.
#include "common.h"
#include "jvae_hip.h"
#include "aggpost_core.h"
#include <math.h>

// One thread per output: R = 1 (out (M,), the whole row of z is looked at) or R = K (out (M, K), coordinate r of query q).
// pair[((piece, r), q)], cnt[(piece, q)]
__global__ __launch_bounds__(AGP_BLOCK) void agp_merge_kernel(const float* __restrict__ z, const float2* __restrict__ pair,
                                                              const int* __restrict__ cnt, float* __restrict__ out, long M,
                                                              int K, int R, int pieces, int* status) {
    const long i = (long)blockIdx.x * AGP_BLOCK + threadIdx.x;
    if (i >= (long)R * M) return;
    const long r = i / M, q = i - r * M;
    const float2* w = pair + (size_t)r * M + q;
    const size_t step = (size_t)R * M;
    float A = INFINITY;
    long rows = 0;
    for (int p = 0; p < pieces; ++p) {
        A = fminf(A, w[p * step].x);
        rows += cnt[(size_t)p * M + q];
    }
    float stack[AGP_STACK];
#pragma unroll
    for (int l = 0; l < AGP_STACK; ++l) stack[l] = 0.f;
    const float As = A < INFINITY ? A : 0.f;
    for (int p = 0; p < pieces; ++p) {
        const float2 v = w[p * step];
        float carry = v.y * exp2f(AGP_KK * (v.x - As));
        bool open = true;
#pragma unroll
        for (int l = 0; l < AGP_STACK; ++l) {          // a binary counter: level l holds the sum of 2^l pieces
            const bool full = (p >> l) & 1;
            if (open && full) carry = stack[l] + carry;
            if (open && !full) {
                stack[l] = carry;
                open = false;
            }
        }
    }
    float total = 0.f;
    bool first = true;
#pragma unroll
    for (int l = 0; l < AGP_STACK; ++l)                // the levels left, the fewest pieces first
        if ((pieces >> l) & 1) {
            total = first ? stack[l] : total + stack[l];
            first = false;
        }
    bool isn = false, isi = false;
    if (R == 1) {
        for (int k = 0; k < K; ++k) {
            const float v = z[(size_t)q * K + k];
            isn |= v != v;
            isi |= fabsf(v) == INFINITY;
        }
    } else {
        const float v = z[(size_t)q * K + r];
        isn = v != v;
        isi = fabsf(v) == INFINITY;
    }
    const double half_log2pi = 0.91893853320467274178;
    const double val = -0.5 * (double)A + log((double)total) - log((double)rows) - (R == 1 ? K : 1) * half_log2pi;
    const bool empty = rows == 0, lost = !(fabs(val) < INFINITY);      // lost: every Q overflowed, or a non-finite operand
    out[R == 1 ? q : q * K + r] = isn ? NAN : (isi || empty || lost ? -INFINITY : (float)val);
    if (isn || isi || (lost && !empty)) atomicOr(status, AGP_STATUS_QUERY);
    else if (empty) atomicOr(status, AGP_STATUS_EMPTY);
}

static bool agp_in_range(long M, long N, int K) {
    return M >= 1 && M < (1L << 31) && N >= 1 && N <= AGP_MAX_BANK && K >= 1 && K <= AGP_MAX_K;
}

extern "C" int jvae_aggpost_partition(void) { return AGP_PART; }

extern "C" long jvae_aggpost_padded_rows(long N) { return N >= 1 && N <= AGP_MAX_BANK ? agp_padded(N) : 0; }

extern "C" int jvae_aggpost_prepare_f32(const float* mu, const float* log_var, float* muT, float* wT, float* lvT, float* c, long N,
                                        int K, void* stream) {
    if (N < 1 || K < 1) return JVAE_EINVAL;
    if (N > AGP_MAX_BANK || K > AGP_MAX_K) return JVAE_ENOTSUP;
    if (!mu || !log_var || !muT || !wT || !lvT || !c) return JVAE_EINVAL;
    const long Np = agp_padded(N);
    agp_prepare_kernel<<<cdiv(Np, AGP_BLOCK), AGP_BLOCK, 0, (hipStream_t)stream>>>(mu, log_var, muT, wT, lvT, c, N, Np, K);
    JVAE_LAUNCH_CHECK();
    return 0;
}

// pieces * M (a, s) pairs and counts; with dims, pieces * K * M pairs more
extern "C" size_t jvae_aggpost_workspace_bytes(long M, long N, int K, int dims) {
    if (!agp_in_range(M, N, K)) return 0;
    const size_t pm = (size_t)agp_pieces(N) * M;
    return pm * (sizeof(float2) + sizeof(int)) + (dims ? pm * K * sizeof(float2) : 0);
}

extern "C" int jvae_aggpost_logdensity_f32(const float* z, const int* zgroup, const float* muT, const float* wT, const float* lvT,
                                           const float* c, const int* group, float* logq, float* logq_dims, long M, long N, int K,
                                           int conditional, int* status, void* ws, size_t ws_bytes, void* stream) {
    if (M < 0 || N < 1 || K < 1) return JVAE_EINVAL;
    if (M == 0) return 0;
    if (!agp_in_range(M, N, K)) return JVAE_ENOTSUP;
    if (!z || !muT || !wT || !lvT || !c || !logq || !status || !ws || ((uintptr_t)ws & 7)) return JVAE_EINVAL;
    if (conditional && (!zgroup || !group)) return JVAE_EINVAL;
    const int dims = logq_dims != nullptr;
    if (ws_bytes < jvae_aggpost_workspace_bytes(M, N, K, dims)) return JVAE_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int pieces = agp_pieces(N);
    const long Np = agp_padded(N);
    const size_t pm = (size_t)pieces * M;
    float2* pair = (float2*)ws;
    float2* dpair = pair + pm;
    int* cnt = (int*)(dpair + (dims ? pm * K : 0));
    const dim3 grid((unsigned)cdiv(M, AGP_QT), (unsigned)pieces);
    if (conditional)
        agp_joint_kernel<true, false><<<grid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, c, group, pair, cnt, M, N, Np, K, status, nullptr);
    else
        agp_joint_kernel<false, false><<<grid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, c, group, pair, cnt, M, N, Np, K, status, nullptr);
    JVAE_LAUNCH_CHECK();
    agp_merge_kernel<<<cdiv(M, AGP_BLOCK), AGP_BLOCK, 0, st>>>(z, pair, cnt, logq, M, K, 1, pieces, status);
    JVAE_LAUNCH_CHECK();
    if (dims) {
        const dim3 dgrid(grid.x, grid.y, (unsigned)cdiv(K, AGP_KD));
        if (conditional)
            agp_dims_kernel<true><<<dgrid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, lvT, group, dpair, M, N, Np, K);
        else
            agp_dims_kernel<false><<<dgrid, AGP_BLOCK, 0, st>>>(z, zgroup, muT, wT, lvT, group, dpair, M, N, Np, K);
        JVAE_LAUNCH_CHECK();
        agp_merge_kernel<<<cdiv((long)M * K, AGP_BLOCK), AGP_BLOCK, 0, st>>>(z, dpair, cnt, logq_dims, M, K, K, pieces, status);
        JVAE_LAUNCH_CHECK();
    }
    return 0;
}
