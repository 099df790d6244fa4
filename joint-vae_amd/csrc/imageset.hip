// Device-resident image sets (jvae_compat/torch_load.py): a list of sample indices -> a ready float32 NCHW batch and its
// int64 labels in ONE launch, with the static transform chain of the set (utils/torch_load.py:347-426) and, when asked, the
// random flip / edge-padded crop of augment.hip.  The set's raw uint8 images stay on the device; nothing but the index list
// comes from the host per batch.
//
// The chain is walked BACKWARDS from the output coordinate, stage by stage, in integer arithmetic:
//   output <- post transform (zero pad 2 | centre crop | none) <- random part (crop at (dy, dx) of the edge-padded image, flip)
//          <- g2c <- quarter-turn/flip element B <- zero padding p0 <- resize (PIL 8-bit bilinear, two passes) <- element A
//          <- data[idx[i]]
// A coordinate that lands in zero padding is 0.0f; everything else is (float)v / 255.0f of one source byte, or of the resized
// byte.  The result is a pure function of its inputs: bit-exact against the torchvision chain.
#include "common.h"
#include "jvae_internal.h"

namespace {

constexpr int IMAGESET_DESC_WORDS = 20;
constexpr int IMAGESET_MAX_TAPS = 8;

// One of the eight compositions of k counter-clockwise quarter turns followed by a horizontal flip, as the map from a
// coordinate of its OUTPUT to the coordinate of its input: ys = ay * y + by * x + cy, xs = ax * y + bx * x + cx.
struct Turn { int ay, by, cy, ax, bx, cx; };

struct Chain {
    int nhwc, Hs, Ws, Cs;      // source layout and extents
    Turn A;                    // first element, input (Hs, Ws)
    int H1, W1;                // extents after A
    int Hr, Wr, kh, kv;        // resize target and taps per axis (RESIZE only)
    int p0;                    // zero padding on all four sides
    int H2, W2;                // extents after resize (or H1, W1) and before p0
    Turn B;                    // second element, input (H2 + 2 p0, W2 + 2 p0)
    int g2c;                   // one source channel repeated
    int H6, W6;                // extents after B = extents of the random part
    int pa;                    // edge padding of the random crop
    int py, px;                // post transform: output (y, x) -> (y + py, x + px) of the (H6, W6) image, outside = zero
    int C, H, W;               // output
};

__host__ __device__ inline Turn make_turn(int e, int Hi, int Wi, int* Ho, int* Wo) {
    const int k = e & 3, f = e >> 2;
    *Ho = (k & 1) ? Wi : Hi;
    *Wo = (k & 1) ? Hi : Wi;
    // rot90^k: out[y][x] = in[ys][xs]
    Turn t;
    switch (k) {
        case 0: t = {1, 0, 0, 0, 1, 0}; break;
        case 1: t = {0, 1, 0, -1, 0, Wi - 1}; break;
        case 2: t = {-1, 0, Hi - 1, 0, -1, Wi - 1}; break;
        default: t = {0, -1, Hi - 1, 1, 0, 0}; break;
    }
    if (f) {                   // the flip acts on the turned image: x -> Wo - 1 - x in front of the turn
        t.cy += t.by * (*Wo - 1); t.by = -t.by;
        t.cx += t.bx * (*Wo - 1); t.bx = -t.bx;
    }
    return t;
}

__device__ inline int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// byte (c, y, x) of image `img` as it is after element A
__device__ inline int fetch_a(const Chain& ch, const unsigned char* __restrict__ img, int c, int y, int x) {
    const int ys = ch.A.ay * y + ch.A.by * x + ch.A.cy;
    const int xs = ch.A.ax * y + ch.A.bx * x + ch.A.cx;
    const long src = ch.nhwc ? ((long)ys * ch.Ws + xs) * ch.Cs + c : ((long)c * ch.Hs + ys) * ch.Ws + xs;
    return img[src];
}

template <bool RESIZE>
__global__ __launch_bounds__(256) void imageset_kernel(const unsigned char* __restrict__ data, const long long* __restrict__ idx,
                                                       const long long* __restrict__ targets, const long long* __restrict__ lut,
                                                       const int* __restrict__ coef_h, const int* __restrict__ bounds_h,
                                                       const int* __restrict__ coef_v, const int* __restrict__ bounds_v,
                                                       const unsigned char* __restrict__ flip, const int* __restrict__ dy,
                                                       const int* __restrict__ dx, float* __restrict__ out,
                                                       long long* __restrict__ yout, int N, Chain ch) {
    const long per_image = (long)ch.Cs * ch.Hs * ch.Ws;
    const long total = (long)N * ch.C * ch.H * ch.W;
    const long stride = (long)gridDim.x * blockDim.x;
    const long first = (long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long i = first; i < N; i += stride) {
        const long long t = targets[idx[i]];
        yout[i] = lut ? lut[t] : t;
    }
    for (long i = first; i < total; i += stride) {
        int x = (int)(i % ch.W);
        long r = i / ch.W;
        int y = (int)(r % ch.H); r /= ch.H;
        int c = (int)(r % ch.C);
        const int n = (int)(r / ch.C);
        // post transform
        y += ch.py; x += ch.px;
        if (y < 0 || y >= ch.H6 || x < 0 || x >= ch.W6) { out[i] = 0.0f; continue; }
        // random part: crop of the edge-padded image, then the flip that came before the padding
        y += (dy ? dy[n] : ch.pa) - ch.pa;
        x += (dx ? dx[n] : ch.pa) - ch.pa;
        y = y < 0 ? 0 : (y >= ch.H6 ? ch.H6 - 1 : y);
        x = x < 0 ? 0 : (x >= ch.W6 ? ch.W6 - 1 : x);
        if (flip && flip[n]) x = ch.W6 - 1 - x;
        if (ch.g2c) c = 0;
        // element B, then the zero padding in front of it
        const int yb = ch.B.ay * y + ch.B.by * x + ch.B.cy - ch.p0;
        const int xb = ch.B.ax * y + ch.B.bx * x + ch.B.cx - ch.p0;
        if (yb < 0 || yb >= ch.H2 || xb < 0 || xb >= ch.W2) { out[i] = 0.0f; continue; }
        const unsigned char* img = data + (long)idx[n] * per_image;
        int v;
        if constexpr (RESIZE) {
            // PIL's two passes for this one pixel: the horizontal pass of every source row the vertical pass reads, each
            // rounded and clipped to 8 bits, then the vertical pass; 22-bit fixed-point coefficients, sums in int32
            const int y0 = bounds_v[2 * yb], ny = bounds_v[2 * yb + 1];
            const int x0 = bounds_h[2 * xb], nx = bounds_h[2 * xb + 1];
            int acc = 1 << 21;
            for (int a = 0; a < ny; ++a) {
                int row = 1 << 21;
                for (int b = 0; b < nx; ++b) row += coef_h[xb * ch.kh + b] * fetch_a(ch, img, c, y0 + a, x0 + b);
                acc += coef_v[yb * ch.kv + a] * clip8(row >> 22);
            }
            v = clip8(acc >> 22);
        } else {
            v = fetch_a(ch, img, c, yb, xb);
        }
        out[i] = (float)v / 255.0f;
    }
}

// desc (host): [0] nhwc [1] Hs [2] Ws [3] Cs [4] A [5] resize [6] Hr [7] Wr [8] kh [9] kv [10] p0 [11] B [12] g2c [13] pa
//              [14] post (0 none, 1 zero pad 2, 2 centre crop) [15] oy [16] ox (crop offsets) [17] C [18] H [19] W
int chain_from_desc(const int* d, Chain* out) {
    Chain ch{};
    ch.nhwc = d[0]; ch.Hs = d[1]; ch.Ws = d[2]; ch.Cs = d[3];
    const int A = d[4], resize = d[5], B = d[11], post = d[14];
    if ((ch.nhwc != 0 && ch.nhwc != 1) || ch.Hs <= 0 || ch.Ws <= 0 || (ch.Cs != 1 && ch.Cs != 3)) return JVAE_EINVAL;
    if (A < 0 || A > 7 || B < 0 || B > 7 || (resize != 0 && resize != 1) || d[10] < 0 || d[13] < 0) return JVAE_EINVAL;
    if (post < 0 || post > 2 || (d[12] != 0 && d[12] != 1) || (d[12] && ch.Cs != 1)) return JVAE_EINVAL;
    ch.A = make_turn(A, ch.Hs, ch.Ws, &ch.H1, &ch.W1);
    ch.H2 = ch.H1; ch.W2 = ch.W1;
    if (resize) {
        ch.Hr = d[6]; ch.Wr = d[7]; ch.kh = d[8]; ch.kv = d[9];
        if (ch.Hr <= 0 || ch.Wr <= 0 || ch.kh <= 0 || ch.kv <= 0) return JVAE_EINVAL;
        if (ch.kh > IMAGESET_MAX_TAPS || ch.kv > IMAGESET_MAX_TAPS) return JVAE_ENOTSUP;
        ch.H2 = ch.Hr; ch.W2 = ch.Wr;
    }
    ch.p0 = d[10];
    ch.B = make_turn(B, ch.H2 + 2 * ch.p0, ch.W2 + 2 * ch.p0, &ch.H6, &ch.W6);
    ch.g2c = d[12];
    ch.pa = d[13];
    ch.C = ch.g2c ? 3 : ch.Cs;
    if (post == 1) {
        ch.py = ch.px = -2;
        ch.H = ch.H6 + 4; ch.W = ch.W6 + 4;
    } else if (post == 2) {                        // offsets as torchvision rounds them, worked out by the caller
        ch.py = d[15]; ch.px = d[16];
        ch.H = d[18]; ch.W = d[19];
        if (ch.H <= 0 || ch.W <= 0 || ch.py < 0 || ch.px < 0 || ch.py + ch.H > ch.H6 || ch.px + ch.W > ch.W6) return JVAE_EINVAL;
    } else {
        ch.H = ch.H6; ch.W = ch.W6;
    }
    if (d[17] != ch.C || d[18] != ch.H || d[19] != ch.W) return JVAE_EINVAL;      // the caller allocated another output
    *out = ch;
    return 0;
}

}  // namespace

extern "C" int jvae_imageset_desc_words(void) { return IMAGESET_DESC_WORDS; }

extern "C" int jvae_imageset_batch_u8_f32(const unsigned char* data, const long long* idx, const long long* targets,
                                          const long long* lut, const int* desc, const int* coef_h, const int* bounds_h,
                                          const int* coef_v, const int* bounds_v, const unsigned char* flip, const int* dy,
                                          const int* dx, float* x, long long* y, long n, int N, void* stream) {
    if (!data || !idx || !targets || !desc || !x || !y || n <= 0 || N < 0) return JVAE_EINVAL;
    Chain ch;
    const int rc = chain_from_desc(desc, &ch);
    if (rc) return rc;
    if (desc[5] && (!coef_h || !bounds_h || !coef_v || !bounds_v)) return JVAE_EINVAL;
    if ((dy == nullptr) != (dx == nullptr)) return JVAE_EINVAL;
    if (N == 0) return 0;
    const long total = (long)N * ch.C * ch.H * ch.W;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (desc[5])
        hipLaunchKernelGGL(imageset_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, data, idx, targets,
                           lut, coef_h, bounds_h, coef_v, bounds_v, flip, dy, dx, x, y, N, ch);
    else
        hipLaunchKernelGGL(imageset_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, data, idx, targets,
                           lut, coef_h, bounds_h, coef_v, bounds_v, flip, dy, dx, x, y, N, ch);
    JVAE_LAUNCH_CHECK();
    return 0;
}
