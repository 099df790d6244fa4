// BatchNorm partial sums in the epilogue of the forward-type convolution kernels (conv_mfma, conv_t2_mfma, conv_x3, conv_t2_x3,
// conv_b8, conv_t2_b8): per workgroup and output channel the sum and the sum of squares of (out - bias) over the tile's pixels,
// written to stats[channel][tile][2].  Pixels of images beyond N contribute exact zeros (zero patch, no bias in the sums).
// A kernel builds the lane's sv[] = [sums | sums of squares] from its own accumulators, stages them with the form of its MFMA
// shape, places its own barrier (__syncthreads or lds_barrier) and folds:
//     red = float[waves][WCOLS][2] in LDS; slot 0 = sum, 1 = sum of squares
#pragma once
#include "common.h"

// 32x32 MFMA tiles: sv[r] / sv[16 + r] of the lane's 16 register rows r of ONE 32-channel tile whose first channel is column
// ch0 of the workgroup's WCOLS; lane l31 of a half-wave receives the half-wave total of sv[l31]
template <int WCOLS>
__device__ __forceinline__ void stats_stage32(const float (&sv)[32], float* red, int wave, int ch0, int l31, int half) {
    const float tot = half_wave_reduce32(sv);
    const int e = l31 & 15, ch = ch0 + (e & 3) + 8 * (e >> 2) + 4 * half;
    red[(wave * WCOLS + ch) * 2 + (l31 >> 4)] = tot;
}

// 16x16 MFMA tiles: sv[ct * 4 + r] / sv[8 + ct * 4 + r] of the lane's registers r of the two 16-channel tiles ct; lane l15 of
// every 16-lane row (kq = the row) receives the row total of sv[l15]
__device__ __forceinline__ void stats_stage16(const float (&sv)[16], float* red, int wave, int l15, int kq) {
    const float tot = row_reduce16(sv);
    const int j = l15 & 7, ch = (j >> 2) * 16 + kq * 4 + (j & 3);
    red[(wave * 32 + ch) * 2 + (l15 >> 3)] = tot;
}

// behind the barrier: thread tid < WCOLS adds the NW waves' entries of channel o0 + tid in wave order and writes the pair to
// the slot of the TILE (of ntiles), so the order of the partials does not depend on the workgroup -> tile mapping
template <int NW, int WCOLS>
__device__ __forceinline__ void stats_fold(const float* red, float* stats, int tid, int o0, int cout, int ntiles, int tile) {
    if (tid < WCOLS && o0 + tid < cout) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) { s1 += red[(w * WCOLS + tid) * 2]; s2 += red[(w * WCOLS + tid) * 2 + 1]; }
        float* dst = stats + ((long)(o0 + tid) * ntiles + tile) * 2;
        dst[0] = s1; dst[1] = s2;
    }
}
