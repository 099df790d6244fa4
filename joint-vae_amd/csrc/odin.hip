// The two ends of the ODIN loop (reference cvae.py:1645-1663): between them sit the model's own forward / input-gradient kernels.
//
//   head      logits of F batched forwards -> score[f][n] = max_c softmax_c(mean_{l>=1} logits[f][l][n][:] / T_f)
//             (+ for the gradient pass d(sum_n score)/d(logits): p_max (delta_{c,argmax} - p_c) / (L T) for l >= 1, 0 for l = 0)
//   perturb   acc += g;  out[e][i] = x[i] + eps_e * sign(acc[i]) for all E perturbation sizes in one launch
//
// Head: a group of G = 8 .. 64 lanes per (forward, sample) - 64 / G samples per wave - lanes stride the classes; max / arg-max /
// sum are shuffles inside the group.  Ties in the max resolve to the FIRST index, as torch.max does.
#include "common.h"
#include "jvae_internal.h"

namespace {

struct HeadP {
    const float* logits;    // element (f, l, n, c) at f * sf + l * sl + n * C + c
    const float* temps;     // (F)
    float* scores;          // (F, N)
    float* dlogits;         // same layout as logits, or null
    int F, L, N, C;         // L draws: rows 1 .. L enter the mean, row 0 (the mean latent) does not
    long sf, sl;
};

template <int G>
__global__ __launch_bounds__(256) void odin_head_kernel(HeadP p) {
    const int sub = threadIdx.x % G;
    const long items = (long)p.F * p.N;
    const long item0 = (long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = item0 < items;
    const long item = live ? item0 : items - 1;          // every lane stays in the shuffles; only live groups write
    const int f = (int)(item / p.N), n = (int)(item % p.N);
    const float T = p.temps[f];
    const float* base = p.logits + (long)f * p.sf + (long)n * p.C;
    auto value = [&](int c) {                              // (sum over the draws / L) / T, as the reference divides
        float s = 0.f;
        for (int l = 1; l <= p.L; ++l) s += base[(long)l * p.sl + c];
        return s / (float)p.L / T;
    };
    float best = -INFINITY;
    int arg = 0x7fffffff;
    for (int c = sub; c < p.C; c += G) {
        const float v = value(c);
        if (v > best || (v == best && c < arg) || arg == 0x7fffffff) { best = v; arg = c; }
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(arg, o, 64);
        if (oa != 0x7fffffff && (arg == 0x7fffffff || ob > best || (ob == best && oa < arg))) { best = ob; arg = oa; }
    }
    float sum = 0.f;
    for (int c = sub; c < p.C; c += G) sum += __expf(value(c) - best);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float pmax = 1.f / sum;                          // exp(best - best) / sum
    if (!live) return;
    if (sub == 0) p.scores[item] = pmax;
    if (p.dlogits) {
        float* d = p.dlogits + (long)f * p.sf + (long)n * p.C;
        const float k = pmax / ((float)p.L * T);
        for (int c = sub; c < p.C; c += G) {
            const float pc = __expf(value(c) - best) / sum;
            const float gv = k * ((c == arg ? 1.f : 0.f) - pc);
            d[c] = 0.f;
            for (int l = 1; l <= p.L; ++l) d[(long)l * p.sl + c] = gv;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void odin_perturb_kernel(float* __restrict__ acc, const float* __restrict__ g,
                                                           const float* __restrict__ x, const float* __restrict__ eps,
                                                           float* __restrict__ out, long numel, int E) {
    constexpr int V = VEC ? 4 : 1;
    typedef float vec_t __attribute__((ext_vector_type(V)));
    const long units = numel / V;
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long)gridDim.x * 256) {
        vec_t a = *reinterpret_cast<const vec_t*>(acc + u * V);
        const vec_t xv = *reinterpret_cast<const vec_t*>(x + u * V);
        if (g) {
            a += *reinterpret_cast<const vec_t*>(g + u * V);
            *reinterpret_cast<vec_t*>(acc + u * V) = a;
        }
        vec_t s;
#pragma unroll
        for (int j = 0; j < V; ++j) s[j] = a[j] > 0.f ? 1.f : (a[j] < 0.f ? -1.f : 0.f);      // torch.sign: 0 where acc == 0
        for (int e = 0; e < E; ++e) {
            const float ev = eps[e];
            vec_t o;
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = xv[j] + ev * s[j];      // eps * (+-1 | 0) is exact: the bits of torch's x + eps * dx
            *reinterpret_cast<vec_t*>(out + (long)e * numel + u * V) = o;
        }
    }
}

}  // namespace

extern "C" {

int jvae_odin_head_f32(const float* logits, const float* temps, float* scores, float* dlogits,
                       int F, int L, int N, int C, long stride_f, long stride_l, void* stream) {
    if (!logits || !temps || !scores || F < 0 || L < 1 || N < 0 || C < 1 || stride_f < 0 || stride_l < 0) return JVAE_EINVAL;
    if (F == 0 || N == 0) return 0;
    HeadP p{logits, temps, scores, dlogits, F, L, N, C, stride_f, stride_l};
    const long items = (long)F * N;
    hipStream_t st = (hipStream_t)stream;
#define HEAD(G_) hipLaunchKernelGGL((odin_head_kernel<G_>), dim3((unsigned)((items + 256 / G_ - 1) / (256 / G_))), dim3(256), 0, st, p)
    if (C <= 8) HEAD(8);
    else if (C <= 16) HEAD(16);
    else if (C <= 32) HEAD(32);
    else HEAD(64);
#undef HEAD
    JVAE_LAUNCH_CHECK();
    return 0;
}

int jvae_odin_perturb_f32(float* acc, const float* g, const float* x, const float* eps, float* out, long numel, int E,
                          void* stream) {
    if (!acc || !x || !eps || !out || numel < 0 || E < 0) return JVAE_EINVAL;
    if (numel == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = numel % 4 == 0 && ((uintptr_t)acc | (uintptr_t)x | (uintptr_t)out | (uintptr_t)g) % 16 == 0;
    const long units = vec ? numel / 4 : numel;
    long blocks = (units + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (vec) hipLaunchKernelGGL((odin_perturb_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, acc, g, x, eps, out, numel, E);
    else hipLaunchKernelGGL((odin_perturb_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, acc, g, x, eps, out, numel, E);
    JVAE_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
