// Input-complexity OOD scores (Serra et al. 2020): the exact length in bits of an achievable lossless code
// of every image of a batch, in ONE launch.  Nothing is encoded.
//
// An image (C, H, W) fp32 is quantised to q = clamp(rint(255 x), 0, 255).  Its planes are the channels as they are; at C == 3 the
// planes (R - G) mod 256 and (B - G) mod 256 as well, for the second colour space (G, R - G, B - G).  A plane has six predictors
// over a = left, b = up, c = up-left (0 outside the image): 0, a, b, (a + b) >> 1, PNG's Paeth, the LOCO-I median edge detector;
// the residual is (v - pred) mod 256.  A residual plane with histogram n_s over k used symbols costs
//   8 + (T[256] - T[k] - T[256 - k]) + T[n + k - 1] - T[k - 1] - sum_s T[n_s],  T[m] = log2(m!) from the caller's fp64 table:
// the count of used symbols, which they are, and an adaptive add-one arithmetic code over them.  A seventh mode stores the plane
// at 8 n bits.  The image costs min over the colour spaces of sum over the planes of (3 + min over the modes), + 1 at C == 3.
//
// A workgroup of 256 threads owns one image.  (1) The quantised planes are staged in LDS as bytes where they fit (IC_STAGE_BYTES),
// else every neighbour is quantised again from global memory.  (2) One sweep over (plane, pixel) adds every pixel to the six
// histograms of its plane with integer LDS atomics on 32-bit counters (n <= 2^20 fits): 5 x 6 histograms at C == 3, C x 6
// otherwise, 30 KB at most.  Equal residuals are NOT aggregated within a wave: a constant image sends every lane to one bin and
// is the slow case.  (3) In rounds of IC_ROUND histograms thread s looks T[n_s] up for every histogram of the round (independent
// loads) and parks it in LDS, the used symbols are counted by ballot, then ONE lane per histogram adds its 256 terms ascending in
// fp64 - the restatement's order - and forms the length.  (4) Thread 0 takes the minima; a tie goes to the lower index.  The counts
// are exact integers and every fp64 sum has one order: no floating-point atomics, the same bits on every call.
#include "common.h"
#include "jvae_hip.h"
#include <math.h>

#define IC_BLOCK 256
#define IC_MAX_C 4
#define IC_MAX_PIXELS (1L << 20)
#define IC_MODES 6                  // predictors with a histogram; mode 6 is "stored"
#define IC_MAX_HIST 30              // 5 planes x 6 predictors
#define IC_ROUND 15                 // histograms whose terms are parked in LDS at a time
#define IC_TERM_LD 257              // doubles between two histograms' terms: the summing lanes read different banks
#define IC_STAGE_BYTES 32768        // the quantised planes are staged in LDS up to this size
#define IC_STATUS_INEXACT 1
#define IC_STATUS_NONFINITE 2

struct IcLds { size_t terms, hist, small, img, total; };
static IcLds ic_lds(int planes, long n) {
    IcLds l;
    l.terms = 0;
    l.hist = (size_t)IC_ROUND * IC_TERM_LD * sizeof(double);
    l.small = l.hist + (size_t)planes * IC_MODES * 256 * sizeof(unsigned);
    l.img = l.small + 40 * sizeof(double);                     // bits of the histograms (32 doubles), their symbol counts, the flags
    l.total = l.img + ((size_t)planes * n <= IC_STAGE_BYTES ? (((size_t)planes * n + 15) & ~(size_t)15) : 0);
    return l;
}

__device__ __forceinline__ int ic_quant(float x, int& flags) {
    const float t = __fmul_rn(255.f, x);                       // rounded on its own: never fused with the subtraction below
    if (!(fabsf(t) < INFINITY)) {                              // the image is refused: its levels do not matter
        flags |= IC_STATUS_NONFINITE;
        return 0;
    }
    const float q = fminf(fmaxf(rintf(t), 0.f), 255.f);
    if (fabsf(t - q) > 0.015625f) flags |= IC_STATUS_INEXACT;
    return (int)q;
}

// plane p of the pixel at `o` of an image in global memory, quantised again (no status: the staging sweep has seen every pixel)
__device__ __forceinline__ int ic_plane_global(const float* __restrict__ xi, int C, long n, int p, long o) {
    int f = 0;
    if (C != 3 || p < 3) return ic_quant(xi[(size_t)p * n + o], f);
    const int g = ic_quant(xi[(size_t)n + o], f), v = ic_quant(xi[(size_t)(p == 3 ? 0 : 2) * n + o], f);
    return (v - g) & 255;
}

__device__ __forceinline__ int ic_abs(int v) { return v < 0 ? -v : v; }

__global__ __launch_bounds__(IC_BLOCK) void ic_code_length_kernel(const float* __restrict__ x, const double* __restrict__ T,
                                                                  double* __restrict__ bits, float* __restrict__ bits32,
                                                                  int* __restrict__ choice, int C, int H, int W, int staged,
                                                                  IcLds lay, int* status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ic_raw[];
    double* s_term = reinterpret_cast<double*>(ic_raw + lay.terms);
    unsigned* s_hist = reinterpret_cast<unsigned*>(ic_raw + lay.hist);
    double* s_bits = reinterpret_cast<double*>(ic_raw + lay.small);
    int* s_k = reinterpret_cast<int*>(s_bits + 32);            // 15 ints, then the flags
    int* s_flags = s_k + IC_ROUND;
    unsigned char* s_img = ic_raw + lay.img;
    const int tid = threadIdx.x, lane = tid & 63;
    const long n = (long)H * W;
    const int planes = C == 3 ? 5 : C, nh = planes * IC_MODES;
    const float* xi = x + (size_t)blockIdx.x * C * n;

    for (int i = tid; i < nh * 256; i += IC_BLOCK) s_hist[i] = 0u;
    if (tid == 0) *s_flags = 0;
    __syncthreads();

    // (1) quantise every pixel once: the flags, and the staged planes
    int flags = 0;
    if (C == 3) {
        for (long o = tid; o < n; o += IC_BLOCK) {
            const int r = ic_quant(xi[o], flags), g = ic_quant(xi[n + o], flags), b = ic_quant(xi[2 * n + o], flags);
            if (staged) {
                s_img[o] = (unsigned char)r;
                s_img[n + o] = (unsigned char)g;
                s_img[2 * n + o] = (unsigned char)b;
                s_img[3 * n + o] = (unsigned char)((r - g) & 255);
                s_img[4 * n + o] = (unsigned char)((b - g) & 255);
            }
        }
    } else {
        for (long o = tid; o < C * n; o += IC_BLOCK) {
            const int q = ic_quant(xi[o], flags);
            if (staged) s_img[o] = (unsigned char)q;
        }
    }
    if (flags) atomicOr(s_flags, flags);
    __syncthreads();
    flags = *s_flags;
    if (flags & IC_STATUS_NONFINITE) {                         // uniform over the workgroup
        if (tid == 0) {
            bits[blockIdx.x] = NAN;
            bits32[blockIdx.x] = NAN;
            choice[blockIdx.x] = -1;
            atomicOr(status, flags);
        }
        return;
    }

    // (2) the histograms of every (plane, predictor)
    for (long item = tid; item < planes * n; item += IC_BLOCK) {
        const int p = (int)(item / n);
        const long o = item - (long)p * n;
        const int yy = (int)(o / W), xx = (int)(o - (long)yy * W);
        int v, a = 0, b = 0, c = 0;
        if (staged) {
            const unsigned char* pl = s_img + (size_t)p * n;
            v = pl[o];
            if (xx) a = pl[o - 1];
            if (yy) b = pl[o - W];
            if (xx && yy) c = pl[o - W - 1];
        } else {
            v = ic_plane_global(xi, C, n, p, o);
            if (xx) a = ic_plane_global(xi, C, n, p, o - 1);
            if (yy) b = ic_plane_global(xi, C, n, p, o - W);
            if (xx && yy) c = ic_plane_global(xi, C, n, p, o - W - 1);
        }
        const int pp = a + b - c, pa = ic_abs(pp - a), pb = ic_abs(pp - b), pc = ic_abs(pp - c);
        const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        const int med = c >= hi ? lo : (c <= lo ? hi : pp);
        unsigned* h = s_hist + (size_t)p * IC_MODES * 256;
        atomicAdd(h + v, 1u);
        atomicAdd(h + 256 + ((v - a) & 255), 1u);
        atomicAdd(h + 512 + ((v - b) & 255), 1u);
        atomicAdd(h + 768 + ((v - ((a + b) >> 1)) & 255), 1u);
        atomicAdd(h + 1024 + ((v - paeth) & 255), 1u);
        atomicAdd(h + 1280 + ((v - med) & 255), 1u);
    }
    __syncthreads();

    // (3) the length of every residual plane
    for (int h0 = 0; h0 < nh; h0 += IC_ROUND) {
        const int hn = nh - h0 < IC_ROUND ? nh - h0 : IC_ROUND;
        if (tid < IC_ROUND) s_k[tid] = 0;
        __syncthreads();
        for (int j = 0; j < hn; ++j) {
            const unsigned cnt = s_hist[(h0 + j) * 256 + tid];  // <= n: inside the table
            s_term[j * IC_TERM_LD + tid] = T[cnt];
            const unsigned long long used = __ballot(cnt != 0u);
            if (lane == 0) atomicAdd(s_k + j, __popcll(used));
        }
        __syncthreads();
        if (tid < hn) {
            const double* tp = s_term + tid * IC_TERM_LD;
            double sum = 0.;
#pragma unroll 16
            for (int s = 0; s < 256; ++s) sum += tp[s];
            const int k = s_k[tid];                            // 1 <= k <= min(n, 256)
            double b = 8. + ((T[256] - T[k]) - T[256 - k]);
            b += T[n + k - 1];
            b -= T[k - 1];
            b -= sum;
            s_bits[h0 + tid] = b;
        }
        __syncthreads();
    }

    // (4) the minima: modes of a plane, planes of a space, spaces
    if (tid == 0) {
        const double stored = 8. * (double)n;
        double plane_bits[5];
        int plane_mode[5];
        for (int p = 0; p < planes; ++p) {
            double best = s_bits[p * IC_MODES];
            int bm = 0;
            for (int m = 1; m < IC_MODES; ++m)
                if (s_bits[p * IC_MODES + m] < best) {
                    best = s_bits[p * IC_MODES + m];
                    bm = m;
                }
            if (stored < best) {
                best = stored;
                bm = IC_MODES;
            }
            plane_bits[p] = 3. + best;
            plane_mode[p] = bm;
        }
        double total = 0.;
        int word = 0;                                          // space 0
        for (int p = 0; p < C; ++p) {
            total += plane_bits[p];
            word |= (plane_mode[p] + 1) << (4 + 3 * p);
        }
        if (C == 3) {
            total += 1.;
            const int sp[3] = {1, 3, 4};
            double other = 0.;
            int w1 = 1;
            for (int p = 0; p < 3; ++p) {
                other += plane_bits[sp[p]];
                w1 |= (plane_mode[sp[p]] + 1) << (4 + 3 * p);
            }
            other += 1.;
            if (other < total) {
                total = other;
                word = w1;
            }
        }
        bits[blockIdx.x] = total;
        bits32[blockIdx.x] = (float)total;
        choice[blockIdx.x] = word;
        if (flags) atomicOr(status, flags);
    }
}

extern "C" int jvae_image_code_length_f32(const float* x, long N, int C, int H, int W, const double* table, long table_len,
                                          double* bits, float* bits32, int* choice, int* status, void* stream) {
    if (N < 0) return JVAE_EINVAL;
    if (C < 1 || C > IC_MAX_C || H < 1 || W < 1 || (long)H * W > IC_MAX_PIXELS || N >= (1L << 31)) return JVAE_ENOTSUP;
    const long n = (long)H * W;
    if (table_len < n + 257) return JVAE_EINVAL;
    if (N == 0) return 0;
    if (!x || !table || !bits || !bits32 || !choice || !status) return JVAE_EINVAL;
    const int planes = C == 3 ? 5 : C;
    const IcLds lay = ic_lds(planes, n);
    static bool lds_set = false;
    if (!lds_set) {
        const IcLds most = ic_lds(5, IC_STAGE_BYTES / 5);
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&ic_code_length_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)most.total);
        if (e != hipSuccess) return (int)e;
        lds_set = true;
    }
    const int staged = (size_t)planes * n <= IC_STAGE_BYTES;
    ic_code_length_kernel<<<(unsigned)N, IC_BLOCK, lay.total, (hipStream_t)stream>>>(x, table, bits, bits32, choice, C, H, W, staged,
                                                                                      lay, status);
    JVAE_LAUNCH_CHECK();
    return 0;
}
