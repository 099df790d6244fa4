// The ordered class fold of the loss tails that learn the prior (csrc/iwae.hip, csrc/tcvae.hip).
#pragma once
#include "common.h"

// out[cls][k] = fp32 of the fp64 sum over the samples n of class cls of part[n][k]: 16 contiguous sample chunks per output are
// summed in sample order by 16 threads, the 16 partial sums are folded in chunk order (the partition of means_grad_kernel,
// csrc/latent.hip).  blockIdx.y picks the job: 0 the class means, 1 the whitening factors.  A label outside [0, C) matches no class.
static __global__ __launch_bounds__(1024) void iw_class_fold_kernel(const double* __restrict__ part0, float* __restrict__ out0,
                                                                    const double* __restrict__ part1, float* __restrict__ out1,
                                                                    const long long* __restrict__ y, int N, int C, int K) {
    __shared__ double part[16][64];
    const double* __restrict__ src = blockIdx.y ? part1 : part0;
    float* __restrict__ dst = blockIdx.y ? out1 : out0;
    if (!src || !dst) return;                                 // block-uniform
    const int ix = threadIdx.x & 63, chunk = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + ix;
    const int per = (N + 15) / 16, n0 = chunk * per, n1 = min(N, n0 + per);
    double s = 0.;
    if (i < C * K) {
        const int cls = i / K, k = i % K;
        for (int n = n0; n < n1; ++n)
            if (y[n] == (long long)cls) s += src[(long)n * K + k];
    }
    part[chunk][ix] = s;
    __syncthreads();
    if (chunk == 0 && i < C * K) {
        double t = 0.;
#pragma unroll
        for (int c = 0; c < 16; ++c) t += part[c][ix];
        dst[i] = (float)t;
    }
}
