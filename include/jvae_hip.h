/* libjvae_hip.so — C ABI of the MI355X (gfx950) kernels behind the joint-CVAE training step.
 *
 * Drop-in boundary: the reference (moxime/joint-vae) has no FFI of its own — the path sits
 * behind a Python import surface (cvae.py:8-15) and bottoms out in PyTorch ops.  Each entry point below
 * names the PyTorch op / reference lines it replaces; the Python host in joint-vae_amd/ binds them with
 * ctypes (joint-vae_amd/jvae_hip/lib.py) — INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers to DEVICE memory (fp32 unless stated; class labels int64), sizes as int/long,
 *     `stream` is a hipStream_t passed as void*; everything is stream-ordered, nothing synchronises,
 *     nothing allocates: scratch comes from the caller (`ws`, size from the matching *_workspace_bytes).
 *   - tensors are dense, NCHW for images.
 *   - return 0 = ok, <0 = invalid argument (-1), unsupported (-2), workspace too small (-3),
 *     >0 = hipError_t of the failing launch.
 *   - thread-compatible: no global mutable state.
 */
#ifndef JVAE_HIP_H
#define JVAE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* jvae_version(void);

/* ---- dense products -------------------------------------------------------------------------------
 * C[b](m,n) (+)= sum_k A[b](m,k) B[b](k,n) [+ bias] [ReLU]; strides in elements; batch over b.
 * bias_mode 0 none / 1 per-n / 2 per-m.  flags: 1 accumulate into C, 2 ReLU, 4 add with float atomics
 * (C must hold the base value; implied by splitk > 1).
 * Replaces nn.Linear forward/backward (module/vae_layers/layers.py:283-296,380-394; cvae.py:291-301,319-326;
 * Classifier layers.py:456-483) and the GEMM inside every convolution. */
int jvae_gemm_f32(int M, int N, int K, int batch,
                  const float* A, long sAm, long sAk, long sAb,
                  const float* B, long sBk, long sBn, long sBb,
                  float* C, long sCm, long sCn, long sCb,
                  const float* bias, int bias_mode, int flags, int splitk, void* stream);

/* y[i] = [relu]([y[i] +] bias[i % N] + sum_{s<S} part[s][i]), i < MN (bias may be NULL): deterministic fold of a split-K product whose K slices were
 * computed by one batched jvae_gemm_f32 launch (used by the dense heads when M*N gives too few tiles, e.g. 256 x 200
 * with K = 7200 in the 64x64 model). */
int jvae_splitk_fold_f32(const float* part, const float* bias, float* y, int S, long MN, int N, int relu, int accumulate,
                         void* stream);

/* Independent products in ONE launch (two when the group holds both kernel families, see csrc/gemm.hip).  A descriptor is the
 * argument list of jvae_gemm_f32; want_splits > 0 asks instead for the deterministic split-K form: K is cut into at most
 * want_splits pieces whose partial products are STORED sCsplit elements apart (no bias, flags and splitk unused), and the number of
 * pieces made is written to *splits (required then; fold them with jvae_splitk_fold_f32).  Every product runs the kernel, the
 * tiles and the K slices that it gets when launched alone: the results are the same bits.  The products must not depend on each
 * other.  n == 0: nothing is done.  n > 8: -2.  A descriptor that jvae_gemm_f32 refuses, or two descriptors whose outputs
 * overlap (judged by the address ranges they span): -1, and nothing is launched. */
typedef struct JvaeGemmDesc {
    int M, N, K, batch;
    const float* A; long sAm, sAk, sAb;
    const float* B; long sBk, sBn, sBb;
    float* C; long sCm, sCn, sCb;
    const float* bias; int bias_mode, flags, splitk;
    int want_splits; long sCsplit; int* splits;
} JvaeGemmDesc;
int jvae_gemm_group_f32(const JvaeGemmDesc* descs, int n, void* stream);

/* Host-only query of the plan the dense entry points take for a descriptor (nothing is initialised on the device, nothing is
 * launched; the operand pointers are looked at for their alignment only, *d->splits is not written).  want_splits > 0 means the
 * stored-slices form, as in jvae_gemm_group_f32.  Reads the split-bf16 switch (jvae_conv2d_set_split_bf16) like every call.
 * variant: 0 ... 7 the fp32 MFMA tile kernel, 8 ... 15 the split-bf16 kernel (name: jvae_gemm_variant_name); gx, gy, gz the
 * grid (gz = batch * slices); slices the K slices made, kchunk the K elements of a slice (a multiple of 32; 0 when K = 0);
 * vecA / vecB whether the operand is read with 16-byte loads; lds the LDS bytes of a workgroup.  Returns what the launch entries
 * return for the descriptor: -1 for one they refuse; 0 with variant -1 (the other fields 0) for an empty product. */
typedef struct JvaeGemmRoute {
    int variant;
    int gx, gy, gz;
    int slices, kchunk;
    int vecA, vecB;
    int lds;
} JvaeGemmRoute;
int jvae_gemm_route(const JvaeGemmDesc* d, JvaeGemmRoute* out);
/* "TILE64_AM_BK" ... "X3_AK_BN_D3" for a variant of jvae_gemm_route: TILE64 / TILE128 the block tile of the fp32 kernel, X3 the
 * split-bf16 kernel with D1 / D3 K steps in flight; AK / AM: A is contiguous along k / treated as contiguous along m (sAk != 1),
 * BN / BK: B contiguous along n / treated as contiguous along k (sBn != 1).  NULL outside 0 ... 15. */
const char* jvae_gemm_variant_name(int variant);

/* Up to 8 folds (the arguments of jvae_splitk_fold_f32 each) in one launch; every element is folded by the same expression in
 * the same slice order.  n == 0: nothing; n > 8: -2; a descriptor that jvae_splitk_fold_f32 refuses or overlapping outputs: -1. */
typedef struct JvaeFoldDesc {
    const float* part; const float* bias; float* y;
    int S; long MN; int N, relu, accumulate;
} JvaeFoldDesc;
int jvae_splitk_fold_group_f32(const JvaeFoldDesc* descs, int n, void* stream);

/* ---- (transposed) convolution ---------------------------------------------------------------------
 * x: (N,Cin,H,W) layer input; y: (N,Cout,OH,OW) layer output; w in the PyTorch layout of the layer kind
 * ((Cout,Cin,KH,KW) for Conv2d, (Cin,Cout,KH,KW) for ConvTranspose2d); S stride, P padding,
 * OP output_padding (transposed only).  Replaces nn.Conv2d / nn.ConvTranspose2d built by
 * build_de_conv_layers (module/vae_layers/conv.py:186-196) and their autograd backward.
 * wgrad: accumulate != 0 adds into dw/dbias (autograd .grad accumulation), else overwrites.
 * ws / ws_bytes: device scratch of at least jvae_conv2d_workspace_bytes(...) bytes (every direction); an entry point given
 * less than its selected kernel needs returns -3 (JVAE_EWORKSPACE) - the kernel depends on the geometry, the call's arguments
 * and jvae_conv2d_set_split_bf16 only, never on the workspace size. */
size_t jvae_conv2d_workspace_bytes(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP,
                                   int transposed);
/* Arithmetic unit of the stride-1 5x5 layers with >= 16 input channels (forward, ConvTranspose2d forward, dgrad):
 * mode 1 (default, JVAE_X3=0 in the environment sets 0 at start-up) = bf16 matrix cores with every fp32 operand split
 * EXACTLY into three bf16 terms and six bf16 MFMA products per fp32 product (csrc/conv_x3.hip: fp32-accurate, error
 * below the fp32 FMA chain's own rounding); mode 0 = v_mfma_f32_32x32x2_f32 (csrc/conv_mfma.hip).  Same tensors, same
 * results to fp32 rounding; returns the previous mode.  Same reference ops as jvae_conv2d_fwd_f32. */
int jvae_conv2d_set_split_bf16(int mode);
/* MFMA shape of that split-bf16 kernel on maps up to 32 wide: on = 1 (default) =
 * v_mfma_f32_16x16x32_bf16 with K = 2 taps x 16 channels, on = 0 = v_mfma_f32_32x32x16_bf16 with K = 16 channels of one tap.
 * Same six products per fp32 product, same fp32 accumulation order per output up to the pairing of taps; returns the
 * previous setting (A/B switch for tests and benches). */
int jvae_conv2d_set_split_shape16(int on);
int jvae_conv2d_out_shape(int H, int W, int KH, int KW, int S, int P, int OP, int transposed, int* OH, int* OW);
/* Host-only query of the kernel selection (nothing is initialised on the device): the route the entry points take for a call
 * of direction dir (1 forward, 2 dgrad, 4 wgrad: the bits of jvae_conv2d_native_b8) in layout 0 (fp32 NCHW) or 1 (bf16 B8)
 * with these call facts: bias / stats given, y_f32 (the bf16 forward's fp32 output), aff_kind 0 / 1 / 2 (in_relu of the *_aff
 * entry points + 1 when a deferred BatchNorm is applied, 0 without).  Reads the split-bf16 switch like every call.  Outputs
 * (each may be NULL): *kernel the kernel family (0 = none: that bf16 entry point returns -2; name: jvae_conv2d_kernel_name),
 * *swap the role swap of the leaf, *ws_bytes the workspace the leaf needs (0: the generic path sizes itself by what it is
 * given), *splits the BatchNorm partial sums per channel a forward writes at most, *aff_ok whether the leaf applies a
 * deferred BatchNorm.  -1 for a geometry the entry points refuse. */
int jvae_conv2d_route(int dir, int layout, int bias, int stats, int y_f32, int aff_kind,
                      int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                      int* kernel, int* swap, size_t* ws_bytes, int* splits, int* aff_ok);
/* "CK_FWD5_X3", ... for a *kernel of jvae_conv2d_route; NULL beyond the last one */
const char* jvae_conv2d_kernel_name(int kernel);
/* N = 0 (an empty batch) is valid on every convolution entry point of both layouts: 0 is returned, no activation is read or
 * written (their pointers may be NULL), a weight gradient without `accumulate` zeroes dw / dbias and leaves them alone with it. */
int jvae_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y,
                        int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                        void* ws, size_t ws_bytes, void* stream);
/* Forward that also emits BatchNorm partial statistics of (y - bias) from the kernel's epilogue when the selected
 * kernel supports it.  stats: (Cout, cap, 2) floats with cap >= jvae_conv2d_stats_splits(...) (0 = this layer never
 * produces them); *nsplit (HOST int) = partials per channel actually written, laid out (Cout, *nsplit, 2). */
int jvae_conv2d_stats_splits(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed);
int jvae_conv2d_fwd_stats_f32(const float* x, const float* w, const float* bias, float* y, float* stats, int* nsplit,
                              int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                              void* ws, size_t ws_bytes, void* stream);
int jvae_conv2d_dgrad_f32(const float* dy, const float* w, float* dx,
                          int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                          void* ws, size_t ws_bytes, void* stream);
int jvae_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                          int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                          void* ws, size_t ws_bytes, void* stream);

/* ---- per-step cache of the re-packed convolution weights (csrc/pack_cache.hip; no reference counterpart: PyTorch re-lays
 * weights out inside its conv library).  The 5x5 kernels read their weights in a packed operand layout that depends on the
 * weights only; the host brackets the span in which the weights are constant (evaluate() ... end of backward of
 * cvae.py:2429-2461): begin() re-packs every registered (weight, layout) pair of `owner` in ONE launch and arms the lookups,
 * the convolution entry points then skip their own pack launch, end() disarms (backward is over / the optimiser is about to
 * change the weights).  Outside a bracket every convolution packs for itself, as without a cache.
 * configure(): caller-owned persistent device buffer (256-byte aligned; NULL = off), shared out in equal regions to at most
 * four owners.  owner: a value that changes whenever the set of weight ADDRESSES in use changes; weights[0..n): those addresses
 * - entries are only ever created for them (any other tensor, e.g. a temporary whose address is re-used later, packs per call).
 * pin(): the armed owner's region is never recycled for another owner (a HIP graph captured in the bracket has its slot
 * addresses baked in).  stats(): host-side counters for tests. */
int jvae_pack_cache_configure(void* buf, size_t bytes);
int jvae_pack_cache_begin(void* stream, long long owner, const void* const* weights, int n);
int jvae_pack_cache_end(void);
int jvae_pack_cache_pin(void);
int jvae_pack_cache_reset(void);
int jvae_pack_cache_stats(int* entries, long long* hits, long long* misses, long long* refreshes);

/* out[c] (+)= sum_{n,q} t[n][c][q]: bias gradient of a conv (P = OH*OW) or linear (P = 1) layer. */
size_t jvae_channel_sum_workspace_bytes(int C);
int jvae_channel_sum_f32(const float* t, float* out, int N, int C, int P, int accumulate, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- BatchNorm2d (+ fused ReLU) -------------------------------------------------------------------
 * x,y,dx,dy: (N,C,P) with P = H*W.  training != 0: batch statistics (biased variance in the forward,
 * unbiased into running_var, momentum update, num_batches_tracked += 1), else running statistics.
 * `relu` (here and as `in_relu` of the convolutions below) names the activation that follows the BatchNorm in the reference's stacks
 * (conv.py:214-220, misc.py:24-27), fused into these kernels: 0 none, 1 nn.ReLU, 2 nn.LeakyReLU() - negative slope 0.01, the
 * reference's activation='leaky' (round 5); any other non-zero value means ReLU.  Backward recomputes the mask from x.  The bf16
 * ("b8") entry points know 0 and 1 only and refuse 2 with JVAE_ENOTSUP (-2) before they launch anything, as the bf16 convolutions
 * refuse a leaky in_relu: nothing is written. */
size_t jvae_bn_workspace_bytes(int C);
/* Host-only (no GPU work): launch plan of the BatchNorm kernels - nsplit image parts for the reduction kernels, nchunk for the
 * apply kernels - and the image range [nb, ne) of part j out of `parts` (trailing parts may be EMPTY, nb == ne, never
 * negative: the reference keeps the ragged last batch, cvae.py:2245-2249, so every N must partition safely). */
int jvae_bn_plan(int N, int C, int P, int* nsplit, int* nchunk);
int jvae_image_range(int N, int parts, int j, int* nb, int* ne);
int jvae_bn_fwd_f32(const float* x, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, long long* num_batches_tracked,
                    float* y, float* save_mean, float* save_invstd,
                    int N, int C, int P, float momentum, float eps, int training, int relu,
                    void* ws, size_t ws_bytes, void* stream);
/* Same as jvae_bn_fwd_f32 with the batch statistics supplied by the producing convolution: ext_stats (C, ext_nsplit, 2)
 * = per-workgroup (sum, sum of squares) of (x - ext_pivot[c]), ext_pivot = the conv bias (NULL = 0). */
int jvae_bn_fwd_ext_f32(const float* x, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, long long* num_batches_tracked,
                        float* y, float* save_mean, float* save_invstd,
                        int N, int C, int P, float momentum, float eps, int training, int relu,
                        const float* ext_stats, int ext_nsplit, const float* ext_pivot,
                        void* ws, size_t ws_bytes, void* stream);
int jvae_bn_bwd_f32(const float* dy, const float* x, const float* gamma, const float* beta,
                    const float* save_mean, const float* save_invstd,
                    float* dx, float* dgamma, float* dbeta, int accumulate,
                    int N, int C, int P, int relu, void* ws, size_t ws_bytes, void* stream);
/* Backward of the EVAL-mode BatchNorm (+activation; running statistics are constants): dx = dy * gamma * rsqrt(running_var + eps)
 * * act'(y), the mask re-derived from x exactly as the forward computes y.  One elementwise pass; no parameter gradients.
 * Serves the materialised and the deferred form (x = the BatchNorm's input in both). */
int jvae_bn_eval_bwd_f32(const float* dy, const float* x, const float* gamma, const float* beta,
                         const float* running_mean, const float* running_var, float* dx,
                         int N, int C, int P, float eps, int relu, void* stream);

/* Deferred BatchNorm: statistics + per-channel coefficients only (scale, shift: C floats each, y = fmaf(x, scale, shift));
 * the normalisation (+ReLU) itself is applied by the CONSUMING convolution while it stages its input
 * (jvae_conv2d_fwd_aff_f32 / jvae_conv2d_wgrad_aff_f32), so the normalised activation is never written to HBM.  Backward
 * is the ordinary jvae_bn_bwd_f32.  Statistics arguments as jvae_bn_fwd_ext_f32 (ext_nsplit == 0: own statistics pass). */
int jvae_bn_finalize_f32(const float* x, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, long long* num_batches_tracked,
                         float* save_mean, float* save_invstd, float* scale, float* shift,
                         int N, int C, int P, float momentum, float eps, int training,
                         const float* ext_stats, int ext_nsplit, const float* ext_pivot,
                         void* ws, size_t ws_bytes, void* stream);
/* 1 when both the forward and the weight gradient of this geometry can apply in_scale / in_shift / in_relu to the layer
 * input (the implicit 5x5 kernels; the one for <= 4 output channels with at most 256 input channels); the *_aff entry points
 * return -2 otherwise. */
int jvae_conv2d_affine_ok(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed);
int jvae_conv2d_fwd_aff_f32(const float* x, const float* w, const float* bias, float* y, float* stats, int* nsplit,
                            const float* in_scale, const float* in_shift, int in_relu,
                            int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                            void* ws, size_t ws_bytes, void* stream);
int jvae_conv2d_wgrad_aff_f32(const float* x, const float* dy, float* dw, float* dbias, int accumulate,
                              const float* in_scale, const float* in_shift, int in_relu,
                              int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                              void* ws, size_t ws_bytes, void* stream);

/* Synchronised BatchNorm for data-parallel ranks (no counterpart in the single-process reference, it
 * reproduces what the reference's BatchNorm2d computes on the WHOLE global batch).  Forward: jvae_bn_sums_f32 ->
 * all-reduce(SUM) of the (C,2) sums by the host -> jvae_bn_fwd_sync_f32.  Backward: jvae_bn_bwd_sums_f32 ->
 * all-reduce(SUM) -> jvae_bn_bwd_sync_f32 (dx from the global means, dgamma/dbeta from the local sums).
 * pivot: (C) floats identical on all ranks (the running mean before the update). */
int jvae_bn_sums_f32(const float* x, const float* pivot, float* sums, int N, int C, int P,
                     void* ws, size_t ws_bytes, void* stream);
int jvae_bn_fwd_sync_f32(const float* x, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, long long* num_batches_tracked,
                         float* y, float* save_mean, float* save_invstd,
                         int N, int C, int P, float momentum, float eps, int relu,
                         const float* global_sums, const float* pivot, int world,
                         void* ws, size_t ws_bytes, void* stream);
int jvae_bn_bwd_sums_f32(const float* dy, const float* x, const float* gamma, const float* beta,
                         const float* save_mean, const float* save_invstd, float* local_sums,
                         int N, int C, int P, int relu, void* ws, size_t ws_bytes, void* stream);
int jvae_bn_bwd_sync_f32(const float* dy, const float* x, const float* gamma, const float* beta,
                         const float* save_mean, const float* save_invstd,
                         const float* local_sums, const float* global_sums, int world,
                         float* dx, float* dgamma, float* dbeta, int accumulate,
                         int N, int C, int P, int relu, void* stream);

/* ---- bf16 activation path ("B8" layout) --------------------------------------------------------------
 * BASELINE.json configs[4] ("bf16 ... 64x64 deeper conv CVAE"): no counterpart in the fp32 reference.  An activation
 * tensor (N, C, H, W) is stored as (N, ceil(C/8), H, W, 8) bf16: the 8 channels of a pixel are one 16-byte unit, which is
 * one lane's operand of v_mfma_f32_32x32x16_bf16; padding channels are 0.  Master weights (PyTorch layouts, as in the
 * fp32 entry points), biases, BatchNorm statistics / parameters and every gradient of a parameter stay fp32; products
 * are bf16 x bf16 accumulated in fp32.  Geometry arguments as in the *_f32 convolution entry points.
 * jvae_conv2d_native_b8 -> bit mask of the directions that have a bf16 kernel (1 forward, 2 dgrad, 4 wgrad: the 5x5
 * stride-1/2 "same"/"half"/"double" layers of conv32(+) / deconv32(+)); the other entry points return -2 (not
 * supported) for the rest and the host runs those layers on the fp32 kernels between two conversions. */
int jvae_b8_pack_f32(const float* x, void* y, int N, int C, long HW, void* stream);            /* fp32 NCHW -> B8 */
int jvae_b8_unpack_f32(const void* y, float* x, int N, int C, long HW, int accumulate, void* stream);
int jvae_conv2d_native_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed);
size_t jvae_conv2d_workspace_bytes_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP,
                                      int transposed);
int jvae_conv2d_stats_splits_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed);
/* y: B8, or fp32 NCHW when y_f32 (last layer of a stack).  stats / nsplit (both may be NULL): BatchNorm partial sums
 * of (y - bias) taken from the fp32 accumulators, laid out (Cout, *nsplit, 2) as in jvae_conv2d_fwd_stats_f32. */
int jvae_conv2d_fwd_b8(const void* x, const float* w, const float* bias, void* y, int y_f32, float* stats, int* nsplit,
                       int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                       void* ws, size_t ws_bytes, void* stream);
int jvae_conv2d_dgrad_b8(const void* dy, const float* w, void* dx,
                         int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                         void* ws, size_t ws_bytes, void* stream);
/* dw / dbias fp32 (dbias may be NULL); accumulate: add onto their current contents. */
int jvae_conv2d_wgrad_b8(const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                         int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                         void* ws, size_t ws_bytes, void* stream);
/* BatchNorm2d (+ReLU) on B8 tensors; arguments as jvae_bn_fwd_ext_f32 / jvae_bn_bwd_f32 with HW = pixels per image. */
size_t jvae_bn_workspace_bytes_b8(int C);
int jvae_bn_plan_b8(int N, int C, long HW, int* nsplit, int* nchunk);      /* host-only, see jvae_bn_plan */
int jvae_bn_fwd_b8(const void* x, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, long long* num_batches_tracked,
                   void* y, float* save_mean, float* save_invstd,
                   int N, int C, long HW, float momentum, float eps, int training, int relu,
                   const float* ext_stats, int ext_nsplit, const float* ext_pivot,
                   void* ws, size_t ws_bytes, void* stream);
int jvae_bn_bwd_b8(const void* dy, const void* x, const float* gamma, const float* beta,
                   const float* save_mean, const float* save_invstd,
                   void* dx, float* dgamma, float* dbeta, int accumulate,
                   int N, int C, long HW, int relu, void* ws, size_t ws_bytes, void* stream);
/* Deferred form (as jvae_bn_finalize_f32 / *_aff_f32 for fp32): statistics + coef = (2, ceil(C/8)*8) floats (scale, shift;
 * zero on the padding channels); the consuming bf16 convolution applies them (+ReLU) to its input while staging it. */
int jvae_bn_finalize_b8(const void* x, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, long long* num_batches_tracked,
                        float* save_mean, float* save_invstd, float* coef,
                        int N, int C, long HW, float momentum, float eps, int training,
                        const float* ext_stats, int ext_nsplit, const float* ext_pivot,
                        void* ws, size_t ws_bytes, void* stream);
/* Synchronised BatchNorm on B8 tensors (data-parallel ranks share the batch statistics): the bf16 counterpart of
 * jvae_bn_sums_f32 / jvae_bn_fwd_sync_f32 / jvae_bn_bwd_sums_f32 / jvae_bn_bwd_sync_f32 (same protocol: the host all-reduces
 * the (C,2) sums between the two calls of each direction; reference semantics: nn.BatchNorm2d of the single-process
 * reference on the GLOBAL batch, module/vae_layers/conv.py:214-220).  Workspace: jvae_bn_workspace_bytes_b8(C). */
int jvae_bn_sums_b8(const void* x, const float* pivot, float* sums, int N, int C, long HW,
                    void* ws, size_t ws_bytes, void* stream);
int jvae_bn_fwd_sync_b8(const void* x, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, long long* num_batches_tracked,
                        void* y, float* save_mean, float* save_invstd,
                        int N, int C, long HW, float momentum, float eps, int relu,
                        const float* global_sums, const float* pivot, int world,
                        void* ws, size_t ws_bytes, void* stream);
int jvae_bn_bwd_sums_b8(const void* dy, const void* x, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_invstd, float* local_sums,
                        int N, int C, long HW, int relu, void* ws, size_t ws_bytes, void* stream);
int jvae_bn_bwd_sync_b8(const void* dy, const void* x, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_invstd,
                        const float* local_sums, const float* global_sums, int world,
                        void* dx, float* dgamma, float* dbeta, int accumulate,
                        int N, int C, long HW, int relu, void* ws, size_t ws_bytes, void* stream);
/* Deferred BatchNorm(+ReLU) on the B8 layer input (as jvae_conv2d_affine_ok / *_aff_f32): in_scale / in_shift hold
 * ceil(Cin/8)*8 floats (jvae_bn_finalize_b8), ceil(Cin/8)*8 <= 256.  in_relu = 2 (leaky ReLU) has no bf16 kernel: both
 * *_aff_b8 entry points return -2 for it before writing anything. */
int jvae_conv2d_affine_ok_b8(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed);
int jvae_conv2d_fwd_aff_b8(const void* x, const float* w, const float* bias, void* y, int y_f32, float* stats, int* nsplit,
                           const float* in_scale, const float* in_shift, int in_relu,
                           int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                           void* ws, size_t ws_bytes, void* stream);
int jvae_conv2d_wgrad_aff_b8(const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                             const float* in_scale, const float* in_shift, int in_relu,
                             int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                             void* ws, size_t ws_bytes, void* stream);
int jvae_relu_fwd_b8(const void* x, void* y, long units, void* stream);                /* units of 8 bf16 */
int jvae_relu_bwd_b8(const void* dy, const void* y, void* dx, long units, void* stream);

/* ---- activations (kind 0 identity, 1 ReLU, 2 sigmoid, 3 leaky ReLU with slope 0.01); backward takes the forward OUTPUT ---------- */
int jvae_act_fwd_f32(const float* x, float* y, long n, int kind, void* stream);
int jvae_act_bwd_f32(const float* dy, const float* y, float* dx, long n, int kind, void* stream);

/* ---- latent: clip + reparameterise + KL to the class-conditional prior ----------------------------
 * Replaces Encoder.forward's clip (layers.py:388-394), Sampling.forward (layers.py:230-244; eps is an
 * input: eps (L+1,N,K) with eps[0] = 0), GaussianPrior.kl & helpers (priors.py:173-326),
 * TiltedGaussianPrior.kl (priors.py:389-408), UniformWithGaussianTailPrior.kl (priors.py:429-476) and
 * dzdist (cvae.py:747-753).
 * prior: 0 gaussian, 1 tilted, 2 uniform.  var_dim: 0 scalar T (C,), 1 diag (C,K), 2 full (C,K,K).
 * dict (K+1 floats from jvae_dict_stats_f32, or NULL): dictionary mean and its norm variance.
 * Outputs: lv (N,K) clipped log-variance, z (L+1,N,K), kl / zdist / var_kl / dzdist (N,). */
int jvae_dict_stats_f32(const float* means, float* dict, int C, int K, void* stream);
int jvae_latent_fwd_f32(const float* mu, const float* lv_raw, const float* eps, const long long* y,
                        const float* means, const float* T, const float* dict,
                        float* lv, float* z, float* kl, float* zdist, float* var_kl, float* dzdist,
                        int N, int K, int L, int C, int prior, int var_dim, float tau, float alpha, float w,
                        int sampled, int has_forced, float forced_lv, void* stream);
/* Upstream gradients (any may be NULL): gz (L+1,N,K), g_kl / g_zdist / g_vkl (N,), gmu_direct /
 * glv_direct (N,K).  gmeans (C,K) and gT (shape of T; diag/full only) are ADDED to: per-sample contributions go to
 * the workspace and are folded per class in sample order (deterministic, no float atomics).
 * ws: (4*N + 2*N*K) floats cover every mode. */
int jvae_latent_bwd_f32(const float* mu, const float* lv_raw, const float* lv, const float* eps, const long long* y,
                        const float* means, const float* T,
                        const float* gz, const float* g_kl, const float* g_zdist, const float* g_vkl,
                        const float* gmu_direct, const float* glv_direct,
                        float* gmu, float* glv_raw, float* gmeans, float* gT,
                        int N, int K, int L, int C, int prior, int var_dim, float tau, float alpha, float w,
                        int sampled, int has_forced, void* ws, size_t ws_bytes, void* stream);
/* The same two calls with the warm-up weight in DEVICE memory: w_dev (1 float; NULL: `w` is used, which is what the two entry
 * points above do) is read by the kernels instead of the launch argument, so a captured HIP graph of the training step follows
 * a weight that changes from epoch to epoch.  Same arithmetic on the same fp32 value: bit-identical results. */
int jvae_latent_fwd_wdev_f32(const float* mu, const float* lv_raw, const float* eps, const long long* y,
                             const float* means, const float* T, const float* dict,
                             float* lv, float* z, float* kl, float* zdist, float* var_kl, float* dzdist,
                             int N, int K, int L, int C, int prior, int var_dim, float tau, float alpha, float w,
                             int sampled, int has_forced, float forced_lv, const float* w_dev, void* stream);
int jvae_latent_bwd_wdev_f32(const float* mu, const float* lv_raw, const float* lv, const float* eps, const long long* y,
                             const float* means, const float* T,
                             const float* gz, const float* g_kl, const float* g_zdist, const float* g_vkl,
                             const float* gmu_direct, const float* glv_direct,
                             float* gmu, float* glv_raw, float* gmeans, float* gT,
                             int N, int K, int L, int C, int prior, int var_dim, float tau, float alpha, float w,
                             int sampled, int has_forced, const float* w_dev, void* ws, size_t ws_bytes, void* stream);
/* The latent kernel over ONE batch measured against TWO priors (the WIM fine-tuning step: labelled samples against the
 * class-conditional prior, mixture samples against the alternate one).  Sample n < split takes prior A (means_a (C_a,K), T_a,
 * prior_a, var_dim_a, tau_a, alpha_a) with class y[n]; sample n >= split takes prior B with class y[n].  `dict` belongs to
 * the A part; dzdist[n] = 0 for n >= split.  One launch, one wavefront per sample, the choice of prior wave-uniform; each
 * sample runs the per-sample body of the single-prior kernels, so its results are theirs bit for bit.  0 <= split <= N;
 * split = N / split = 0 is the single-prior kernel under A / B on the whole batch.  A label outside [0, C_a) resp. [0, C_b) is
 * never used as an index: every output of that sample is NaN.
 * Backward: both priors are frozen - gmeans and gT must be NULL (else -1); gmu and glv_raw only.  No workspace is needed
 * (ws may be NULL): nothing is folded per class, the uniform prior's two forward sums are recomputed in the wave.
 * Neither call allocates, synchronises or uses atomics. */
int jvae_latent_mixed_fwd_f32(const float* mu, const float* lv_raw, const float* eps, const long long* y,
                              const float* means_a, const float* T_a, const float* dict, const float* means_b, const float* T_b,
                              float* lv, float* z, float* kl, float* zdist, float* var_kl, float* dzdist,
                              int N, int K, int L, int split,
                              int C_a, int prior_a, int var_dim_a, float tau_a, float alpha_a,
                              int C_b, int prior_b, int var_dim_b, float tau_b, float alpha_b,
                              float w, int sampled, int has_forced, float forced_lv, void* stream);
int jvae_latent_mixed_bwd_f32(const float* mu, const float* lv_raw, const float* lv, const float* eps, const long long* y,
                              const float* means_a, const float* T_a, const float* means_b, const float* T_b,
                              const float* gz, const float* g_kl, const float* g_zdist, const float* g_vkl,
                              const float* gmu_direct, const float* glv_direct,
                              float* gmu, float* glv_raw, float* gmeans, float* gT,
                              int N, int K, int L, int split,
                              int C_a, int prior_a, int var_dim_a, float tau_a, float alpha_a,
                              int C_b, int prior_b, int var_dim_b, float tau_b, float alpha_b,
                              float w, int sampled, int has_forced, void* ws, size_t ws_bytes, void* stream);
/* One iteration of the posterior refinement behind the likelihood regret (Xiao, Yan, Amit 2020) in ONE launch, one wavefront
 * per sample, with the per-sample bodies of the latent kernels.  For sample n with class y[n], in this order:
 *   1. gradient of J_n = mean_l(-log p(x_n | z_ln)) + KL(q_n || p(z | y_n)) with respect to (mu_n, lv_raw_n): `dz` (L+1,N,K)
 *      is d(sum_n mean_l -log p)/dz at z = mu + exp(lv/2) eps_cur (row 0, the mean path, normally carries zeros), the KL part
 *      is analytic with KL weight 1 and warm-up weight 1; the +-20 clip gates the log-variance gradient as in training;
 *   2. torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, bias-corrected, no weight decay, no clipping) on mu_n and lv_raw_n IN
 *      PLACE with the state m_mu, v_mu, m_lv, v_lv (N,K each), step number `step` >= 1 and learning rate `lr`; with a forced
 *      variance only mu moves (lv_raw, m_lv, v_lv may be NULL);
 *   3. the latent forward at the moved posterior with eps_next (L+1,N,K): lv (clipped, N,K), z_next (L+1,N,K), kl, zdist,
 *      var_kl (N,).
 * `lv` is in/out: the clipped log-variance of the posterior on entry (step 3 of the previous call), of the moved one on exit.
 * flags: 1 skips 1 and 2 (the first draw of a loop: eps_cur, dz and the state may be NULL); 2 skips 3 (a last update: eps_next
 * and the outputs of 3 may be NULL); 3 is refused.  All priors of the latent kernel.  No atomics, no workspace; LDS only for
 * the full-variance prior (8 K floats per workgroup, -2 beyond 64 KiB); same inputs, same bits.  A label outside [0, C) is
 * never an index: that sample does not move and its outputs of step 3 are NaN. */
int jvae_latent_refine_f32(float* mu, float* lv_raw, float* lv, const float* eps_cur, const float* eps_next,
                           const long long* y, const float* means, const float* T, const float* dz,
                           float* m_mu, float* v_mu, float* m_lv, float* v_lv,
                           float* z_next, float* kl, float* zdist, float* var_kl,
                           int N, int K, int L, int C, int prior, int var_dim, float tau, float alpha,
                           int sampled, int has_forced, float forced_lv, float lr, long step, int flags, void* stream);

/* ---- reconstruction term ---------------------------------------------------------------------------
 * wmse[l][n] = mean_D((x_reco[l+1][n] - x[n])^2) / sigma^2   (mse_loss, module/losses.py:8-27, called at
 * cvae.py:649-652 on x_reco[1:]/sigma, x/sigma).  `sigma_is_log` selects the kind of sigma (cvae.py:626-670):
 *   0  sigma = 1 float on the device (fixed / decayed value)      1  the float is log(sigma) (learned, layers.py:84-89)
 *   2  sigma = N floats, log sigma_n coded by the encoder         3  sigma follows each sample's own rmse: no division here
 *      (cvae.py:631-634)                                             (the ELBO kernels normalise, cvae.py:662-666)
 * Backward fills ALL L+1 rows of g_x_reco (row 0 with zeros); gsigma (may be NULL): 1 float (modes 0/1) or N floats (2).
 * sigma_fwd (mode 0, may be NULL): the value sigma had in the forward pass - the reference's decay rule changes the
 * parameter in place between forward and backward and its backward divides by sigma_fwd * sigma_now (layers.py:168).
 * x_reco, x and g_x_reco 16-byte aligned when D % 4 == 0 (the float4 path; JVAE_EINVAL before any launch otherwise). */
int jvae_recon_fwd_f32(const float* x_reco, const float* x, const float* sigma, int sigma_is_log,
                       float* wmse, int L, int N, int D, void* stream);
int jvae_recon_bwd_f32(const float* x_reco, const float* x, const float* sigma, int sigma_is_log, const float* sigma_fwd,
                       const float* g_wmse, const float* wmse, float* g_x_reco, float* gsigma, int accumulate_sigma,
                       int L, int N, int D, void* ws, size_t ws_bytes, void* stream);

/* mse_loss(x_output, x_target, batch_mean=False) itself (module/losses.py:8-27) for EVERY row of x_output: rows (L,N,D),
 * x (N,D) -> wmse (L,N) = mean_D((rows[l][n] - x[n])^2); backward: g_rows = g_wmse * 2 (rows - x) / D.  (The jvae_recon_*
 * pair above skips row 0 of an (L+1)-row reconstruction; these take the rows as they are.)  16-byte aligned when D % 4 == 0. */
int jvae_mse_rows_fwd_f32(const float* rows, const float* x, float* wmse, int L, int N, int D, void* stream);
int jvae_mse_rows_bwd_f32(const float* rows, const float* x, const float* g_wmse, float* g_rows, int L, int N, int D, void* stream);

/* ---- ELBO assembly (cvae.py:773-791,887-902): wmse = mean_l wmse_s; cross_x = D/2 (2 log sigma + wmse + log 2pi);
 * total = cross_x + cw * ce + beta * kl   (ce may be NULL).  Backward takes the upstream gradients of the three
 * outputs (any may be NULL) and returns g_wmse_s (L,N), g_kl, g_ce (N,) and d/d sigma of the 2 log sigma term.
 * sigma_is_log: the kinds of jvae_recon_fwd_f32; kind 3 divides wmse_s by the sample's mean over l (sigma_n^2) and uses
 * log sigma_n = log(mean)/2; its backward takes the forward's wmse_s in the `sigma` argument.  mse (N, may be NULL)
 * receives wmse * sigma^2 per sample (the `mse` measure). */
int jvae_elbo_fwd_f32(const float* wmse_s, const float* kl, const float* ce, const float* sigma, int sigma_is_log,
                      float* wmse, float* cross_x, float* total, float* mse, int L, int N, int D, float beta, float cw,
                      void* stream);
int jvae_elbo_bwd_f32(const float* g_wmse, const float* g_cx, const float* g_tot, const float* sigma, int sigma_is_log,
                      float* g_wmse_s, float* g_kl, float* g_ce, float* gsigma, int accumulate_sigma,
                      int L, int N, int D, float beta, float cw, void* ws, size_t ws_bytes, void* stream);
/* ... with the weight of cross_y in DEVICE memory (cw_dev: 1 float; NULL: `cw`), as for the latent kernels above. */
int jvae_elbo_fwd_wdev_f32(const float* wmse_s, const float* kl, const float* ce, const float* sigma, int sigma_is_log,
                           float* wmse, float* cross_x, float* total, float* mse, int L, int N, int D, float beta, float cw,
                           const float* cw_dev, void* stream);
int jvae_elbo_bwd_wdev_f32(const float* g_wmse, const float* g_cx, const float* g_tot, const float* sigma, int sigma_is_log,
                           float* g_wmse_s, float* g_kl, float* g_ce, float* gsigma, int accumulate_sigma,
                           int L, int N, int D, float beta, float cw, const float* cw_dev, void* ws, size_t ws_bytes,
                           void* stream);

/* ---- nn.Dropout(p) of the dense trunks (module/vae_layers/layers.py:287-288, cvae.py:297-298), train mode:
 * y[i] = keep(seed, i) ? x[i] / (1 - p) : 0 with a counter-based mask (the backward pass calls it on dy with the same
 * seed).  The random stream is the kernel's own; the reference draws from torch's global generator. */
int jvae_dropout_f32(const float* x, float* y, long n, float p, long seed, void* stream);
/* the same with the seed in DEVICE memory (mask seed = *seed_dev + salt): nothing about the call depends on host state that
 * changes from step to step, so a captured HIP graph draws a fresh mask at every replay once the caller advances *seed_dev
 * on the stream. */
int jvae_dropout_dev_f32(const float* x, float* y, long n, float p, const long long* seed_dev, long salt, void* stream);

/* ---- importance-weighted bound of the evaluation path (cvae.py:672-676,793-873): li[l][c][n] = log p(x|z_l) +
 * log p(z_l|c) - log q(z_l|x) with log p(x|z_l) = -D/2 (wmse_s + 2 log sigma + log 2pi), -log q = (|eps_l|^2 + sum_k
 * log_var)/2 + K/2 log 2pi; iws[c][n] = mean_l exp(li - max_l li) + max_l li (as the reference writes it).
 * wmse_s (L,N); eps (L,N,K): rows 1..L of the sampling noise; log_var (N,K); log_pz (L,C,N) from the prior's
 * log-density (C = 1 for a non-conditional prior); rows: scratch of L*N floats. */
int jvae_iws_f32(const float* wmse_s, const float* eps, const float* log_var, const float* log_pz, const float* sigma,
                 int sigma_is_log, int L, int N, int K, int C, int D, float* rows, float* iws, void* stream);

/* ---- running measures of evaluate() in ONE device buffer (cvae.py:619-624,689-724,747-762; Encoder.capacity /
 * dict_min_distance layers.py:323-348): out[16]: [0..9] = sigma, mean x^2, mean mse, rmse, mean zdist, mean var_kl, ld-norm,
 * imut-zy, d-mind, optimiser non-finite flag; [10..15] = running means over `batch`+1 calls of xpow, mse, rmse, dB,
 * zdist, var_kl (prev = the previous call's out, NULL at batch 0); wmse has N entries, zdist / var_kl Nz (= N, or C*N
 * for the all-class evaluation).  sumsq_x = sum(x^2) from jvae_sqnorm_accum_f32; means may be NULL.  sigma_is_log >= 2
 * (coded / rmse sigma): `wmse` holds the per-sample MSE itself and sigma[0] the rms value to report. */
int jvae_measures_f32(const float* sumsq_x, long nx, const float* wmse, const float* zdist, const float* var_kl, int N, int Nz,
                      const float* sigma, int sigma_is_log, const float* means, int C, int K, const int* flag,
                      const float* prev, int batch, float* out, void* stream);
/* The same for a captured training step: the batch index is *counter (device int: read, then incremented by the kernel) and
 * `run` (16 floats) is both `prev` and `out` - the running means continue from replay to replay with no host value in the
 * launch.  Zero *counter at the start of an epoch (run is then ignored), or seed both from the last eager batch. */
int jvae_measures_dev_f32(const float* sumsq_x, long nx, const float* wmse, const float* zdist, const float* var_kl, int N, int Nz,
                          const float* sigma, int sigma_is_log, const float* means, int C, int K, const int* flag,
                          float* run, int* counter, void* stream);

/* ---- epoch sums of the batch-mean losses (the `acc += stack(means)` of the training loop, cvae.py:2463-2469) in ONE
 * launch: acc[r] += mean(rows[r][0 .. lens[r])) for r < nrows <= 16.  rows / lens are HOST arrays (device pointers of the
 * loss rows - (N,) or (L+1)*N floats each - and their lengths); acc: nrows device floats.  Fixed summation order, no
 * atomics (fp64 partial sums: each mean is exact to one fp32 rounding). */
int jvae_loss_sums_f32(const float* const* rows, const long* lens, int nrows, float* acc, void* stream);

/* ---- classification term: per-row cross entropy, target y[r % N] (x_loss, module/losses.py:52-86) -- */
int jvae_xent_fwd_f32(const float* logits, const long long* y, float* ce, int R, int N, int C, void* stream);
int jvae_xent_bwd_f32(const float* logits, const long long* y, const float* g_ce, float* g_logits, int R, int N, int C,
                      void* stream);

/* ---- optimiser: clip_grad_norm_ + Adam (module/optimizers.py:39-47,79-81,120-121; cvae.py:2454-2461)
 * jvae_sqnorm_accum_f32: *acc += sum g^2 (reset != 0 zeroes acc first).
 * jvae_adam_step_f32: g' = g*min(1, max_norm/(sqrt(*sqnorm)+1e-6)) + weight_decay*p, Adam with bias
 * correction for `step` (>= 1); *nonfinite_flag |= 1 when an updated parameter is NaN/Inf. */
size_t jvae_sqnorm_workspace_bytes(void);
int jvae_sqnorm_accum_f32(const float* g, long n, float* acc, int reset, void* ws, size_t ws_bytes, void* stream);
int jvae_clip_scale_f32(float* g, long n, const float* sqnorm, float max_norm, void* stream);
int jvae_adam_step_f32(float* p, const float* g, float* m, float* v, long n,
                       float lr, float beta1, float beta2, float eps, float weight_decay, long step,
                       float max_norm, const float* sqnorm, int* nonfinite_flag, void* stream);
/* The same update with step count / learning rate / betas in device memory (hyper: 6 floats [lr, beta1, beta2, completed
 * steps, 2 scratch]); advance != 0 increments the step and refreshes the bias corrections first.  No host state: the
 * whole training step can be captured into a HIP graph and replayed (ClassificationVariationalNetwork.graph_train_step). */
int jvae_adam_step_dev_f32(float* p, const float* g, float* m, float* v, long n, float* hyper, int advance,
                           float eps, float weight_decay, float max_norm, const float* sqnorm, int* nonfinite_flag,
                           void* stream);

/* torch.optim.SGD (module/optimizers.py:39-40; momentum / nesterov / weight_decay, dampening 0) with the same fused
 * clip coefficient and NaN/Inf flag as the Adam entry points; buf = momentum buffer (may be NULL when momentum == 0),
 * first_step != 0 initialises it with the gradient as torch does. */
int jvae_sgd_step_f32(float* p, const float* g, float* buf, long n, float lr, float momentum, int nesterov,
                      float weight_decay, int first_step, float max_norm, const float* sqnorm, int* nonfinite_flag,
                      void* stream);

/* ---- MaxPool2d / AvgPool2d / UpsamplingNearest2d: tokens M, A, U of the layer DSL (module/vae_layers/conv.py:201-212;
 * conv-models.ini:13-18,28-30).  Tensors are (planes = N*C, H, W) fp32.  mode 0 = max (idx: int32 (planes, OH, OW), flat
 * h*W + w of the first maximum, as nn.MaxPool2d's return_indices), 1 = average with count_include_pad (divisor K*K).
 * OH = (H + 2P - K)/S + 1.  Up-sampling by an integer factor: y (planes, H*scale, W*scale). */
int jvae_pool2d_out_shape(int H, int W, int K, int S, int P, int* OH, int* OW);
int jvae_pool2d_fwd_f32(const float* x, float* y, int* idx, long planes, int H, int W, int K, int S, int P, int mode,
                        void* stream);
int jvae_pool2d_bwd_f32(const float* dy, const int* idx, float* dx, long planes, int H, int W, int K, int S, int P,
                        int mode, void* stream);
int jvae_upsample_nearest_fwd_f32(const float* x, float* y, long planes, int H, int W, int scale, void* stream);
int jvae_upsample_nearest_bwd_f32(const float* dy, float* dx, long planes, int H, int W, int scale, void* stream);
/* The same four on bf16 B8 tensors (blocks = N*ceil(C/8) channel blocks of (H, W, 8) bf16; padding channels stay zero): per
 * channel the window order, tie rule and fp32 sums of the fp32 kernels, rounded to bf16 once.  idx: int32 (blocks, OH, OW, 8). */
int jvae_pool2d_fwd_b8(const void* x, void* y, int* idx, long blocks, int H, int W, int K, int S, int P, int mode, void* stream);
int jvae_pool2d_bwd_b8(const void* dy, const int* idx, void* dx, long blocks, int H, int W, int K, int S, int P, int mode,
                       void* stream);
int jvae_upsample_nearest_fwd_b8(const void* x, void* y, long blocks, int H, int W, int scale, void* stream);
int jvae_upsample_nearest_bwd_b8(const void* dy, void* dx, long blocks, int H, int W, int scale, void* stream);

/* ---- input pipeline in front of the path: uint8 batch (NHWC if nhwc else NCHW) -> horizontal flip
 * where flip[n] != 0 -> edge padding by `pad` + crop at offsets (dy[n], dx[n]) in [0, 2*pad] -> float32 NCHW / 255.
 * Replaces RandomHorizontalFlip + RandomCrop(padding_mode='edge') + ToTensor of utils/torch_load.py:405-426.
 * flip / dy / dx may be NULL (no flip / centred crop).  dy, dx: int32 on the device. */
int jvae_augment_u8_f32(const unsigned char* in, const unsigned char* flip, const int* dy, const int* dx,
                        float* out, int N, int C, int H, int W, int pad, int nhwc, void* stream);

/* ---- device-resident image sets (csrc/imageset.hip, jvae_compat/torch_load.py): sample indices -> float32 NCHW batch + labels
 * in ONE launch.  data: the whole set's raw uint8 images on the device, (n, Hs, Ws, Cs) or (n, Cs, Hs, Ws), Cs 1 or 3; idx: N
 * int64 indices on the device, any order, repeats allowed, every one in [0, n) - the CALLER checks them, there is no trap in the
 * kernel; y[i] = lut[targets[idx[i]]] (lut NULL: identity; the caller checks the targets against the table's length).
 * desc: jvae_imageset_desc_words ints in HOST memory, the static chain of the set in the order of utils/torch_load.py:347-426:
 *   [0] nhwc  [1] Hs  [2] Ws  [3] Cs
 *   [4] A     quarter-turn/flip element, k + 4 f: k counter-clockwise quarter turns, then a horizontal flip when f
 *   [5] resize (0 / 1)  [6] Hr  [7] Wr  [8] kh  [9] kv: PIL's 8-bit bilinear resampling, horizontal then vertical pass, the
 *       intermediate rounded and clipped to uint8: clip8((2^21 + sum k v) >> 22), int32 sums; coef_h (Wr, kh) / coef_v (Hr, kv)
 *       int32 22-bit fixed-point weights and bounds_h (Wr, 2) / bounds_v (Hr, 2) int32 (first source index, count <= ksize), all
 *       on the device and checked by the caller against the extents after A; kh or kv above 8: -2 (JVAE_ENOTSUP)
 *   [10] p0   zero padding on all four sides
 *   [11] B    second quarter-turn/flip element
 *   [12] g2c  one source channel repeated to 3 (Cs = 1)
 *   [13] pa   edge padding of the random part: flip[i] (uint8), then crop at (dy[i], dx[i]) in [0, 2 pa] (int32) of the padded
 *             image, exactly as jvae_augment_u8_f32; flip NULL: none, dy and dx NULL (both or neither): the centred crop
 *   [14] post 0 none, 1 zero padding 2, 2 centre crop at offsets [15] oy, [16] ox
 *   [17] C  [18] H  [19] W  the output extents; they must be what the chain gives, else -1 (JVAE_EINVAL)
 * then (float)v / 255.0f; padded zeros are 0.0f.  x: float32 (N, C, H, W), y: int64 (N,).  Neither allocates nor synchronises. */
int jvae_imageset_desc_words(void);
int jvae_imageset_batch_u8_f32(const unsigned char* data, const long long* idx, const long long* targets, const long long* lut,
                               const int* desc, const int* coef_h, const int* bounds_h, const int* coef_v, const int* bounds_v,
                               const unsigned char* flip, const int* dy, const int* dx, float* x, long long* y, long n, int N,
                               void* stream);

/* ---- mixed batches (the moving sets of jvae_compat/ft_datasets.py): N images taken from SEVERAL resident sets, and from the
 * synthetic const / uniform sets, in ONE launch.  One record per leaf (jvae_imageset_mix_leaf_bytes bytes each), the same
 * array in host memory (checked here, before the launch) and on the device (read by the kernel):
 *   int kind (0 image set, 1 const, 2 uniform); int border (synthetic leaves: zero border of 2, the 'pad' transformer);
 *   seven device pointers: data, targets, lut (or NULL), coef_h, bounds_h, coef_v, bounds_v (NULL without a resize);
 *   the leaf's jvae_imageset_desc_words descriptor words, [13] pa = 0 (a mixed batch has no random part); a synthetic leaf
 *   sets only [17..19].  Every leaf must end in the same (C, H, W), else -1 (JVAE_EINVAL).
 * leaf (int32), index, tag (int64): per item of the resolved set, on the device, the number of its leaf, the sample inside
 * that leaf and its class position; pos: N int64 positions into these arrays, on the device.  The CALLER checks pos against
 * the arrays' length, leaf against n_leaves and index against the leaf's length: there is no trap in the kernel.
 * x[i] = image index[pos[i]] of leaf leaf[pos[i]] through that leaf's chain (the resize is chosen per image), tagout[i] =
 * tag[pos[i]], y[i] = lut[targets[index[pos[i]]]] of the leaf (0 for a synthetic leaf).  Synthetic leaves take their values
 * from u, float32 on the device drawn by the caller: u_dims 2 = (N, C), const leaves only, x[i, c, :, :] = u[i, c];
 * u_dims 4 = (N, C, H, W), x[i] = u[i] for a uniform leaf and u[i, c, 0, 0] for a const one; NULL when there is no synthetic
 * leaf.  vec: consecutive x per thread, 1 or 4 (W a multiple of it), 0 = the default.  Neither allocates nor synchronises. */
int jvae_imageset_mix_leaf_bytes(void);
int jvae_imageset_mixed_u8_f32(const void* leaves_host, const void* leaves_dev, int n_leaves, const int* leaf,
                               const long long* index, const long long* tag, const long long* pos, const float* u, int u_dims,
                               float* x, long long* tagout, long long* y, int N, int vec, void* stream);

/* ---- ROC of OOD scores: AUC and the FPR / thresholds at kept TPRs (csrc/roc.hip) -----------------------------------
 * Replaces utils/roc_curves.py:38-210 (roc_curve, a Python loop over every in-distribution score) as
 * ood_detection_rates calls it per method and OOD set (cvae.py:1843-1868), for M score rows in one call.
 * ins (M, n_in), outs (M, n_out): fp32 scores, higher = more in-distribution.  kept_tpr: K doubles, ascending.
 * two_sided: M int32 mode words on the device, one per row, mixed freely in one call:
 *   0                               one-sided test (roc_curves.py:85-88)
 *   1                               'around-mean' (roc_curves.py:68-72)
 *   2 | f_low << 8 | f_up << 16     strided quantiles, the tuple mode two_sided=(f_low, f_up) of roc_curves.py:74-83, both
 *                                   factors in [1, 255], bits 24-31 zero: with s the ascending in-scores widened to fp64,
 *                                   low = [-inf, s[0], s[f_low], s[2 f_low], ..., +inf], up = [-inf, s[0], s[f_up], ..., +inf],
 *                                   nt = min(len(low), len(up)), iteration `it` uses low[it] and up[len(up) - 1 - it] while
 *                                   low[it] < up[-1 - it] and it < nt - 1; counts, cursor, kept values and AUC as in the
 *                                   other modes.  In-scores of +-inf are legal, as in mode 0.
 *   The reference takes these thresholds from UnivariateSpline(k=3, s=0) through s, evaluated at its own knots: s again up
 *   to FITPACK's rounding (about 1e-15 relative), which its loop then compares with the scores themselves.  Mode 2 is that
 *   loop on the noise-free thresholds, bit for bit; the rounding noise is not reproduced.
 *   Any other word decodes to nothing.  The words live on the device and the call neither copies nor synchronises, so such
 *   a row is reported through status bit 2 rather than through the return value; it is computed as a mode-0 row.
 * Outputs (fp64): auc (M), kept_fpr / kept_tpr_out / thr_low / thr_up (M, K): what the reference returns, the rates and
 * thresholds bit for bit (same fp64 expressions over integer counts and exactly widened scores), the AUC summed exactly
 * over the counts and divided once.  status (M int32): bit 0 = a NaN score was seen, bit 1 = around-mean row with a
 * non-finite in-score, bit 2 = malformed mode word; the other outputs of such a row are meaningless (never out of bounds).
 * n_in, n_out in [1, 2^24]; M <= 65535; ws 8-byte aligned, jvae_roc_workspace_bytes(...) bytes (0 = invalid sizes). */
size_t jvae_roc_workspace_bytes(int M, long n_in, long n_out);
int jvae_roc_curve_f32(const float* ins, const float* outs, const double* kept_tpr, const int* two_sided,
                       double* auc, double* kept_fpr, double* kept_tpr_out, double* thr_low, double* thr_up, int* status,
                       int M, long n_in, long n_out, int K, void* ws, size_t ws_bytes, void* stream);

/* ---- Precision-recall figures of OOD scores: AUPR-in / -out, AUCPR, detection error (csrc/prc.hip) ------------------
 * The companions of the ROC in the tables of the OOD literature, for M score rows in one call.  ins (M, n_in), outs
 * (M, n_out): fp32 scores, higher = more in-distribution; modes: M int32 mode words on the device, those of
 * jvae_roc_curve_f32.  figures (M, 5) fp64, defined by scikit-learn's functions on the scores widened exactly to fp64:
 *   0  aupr_in    average_precision_score, in = positive: sum dR * P over the distinct in-scores v, with
 *                 tp = #{ins >= v}, fp = #{outs >= v}, tp' = #{ins > v}, fp' = #{outs > v}, dR = (tp - tp') / n_in,
 *                 P = tp / (tp + fp), P' = tp' / (tp' + fp') (1 when tp' + fp' = 0)
 *   1  aupr_out   the same with out = positive and the score negated: the sweep over the distinct out-scores with the rows
 *                 swapped and <= / <
 *   2  aucpr_in   auc(recall, precision) of precision_recall_curve, the trapezoid: sum dR * (P + P') / 2
 *   3  aucpr_out  its out-side twin
 *   4  dete       the smallest detection error: min(0.5, min_v 0.5 * (n_in - tp) / n_in + 0.5 * fp / n_out)
 * Mode 0: scores equal under IEEE comparison are one tie group (-0 = +0); infinities are ordinary values.  Mode 1: the score
 * of a sample is -|s - c| in fp64, c the fp64 mean of the row's in-scores exactly as jvae_roc_curve_f32 forms it.  Mode 2
 * (quantile rows) has no scalar score: five NaNs, status 0.  A malformed word: status bit 2, computed as a mode-0 row.
 * status (M int32, cleared by the call): the bits of jvae_roc_curve_f32 (0 = NaN score, 1 = non-finite in-score of an
 * around-mean row, 2 = malformed mode word); the figures of such a row are meaningless (never out of bounds).
 * Sums in fp64 in a fixed order, no float atomics: the same bits run to run, and a row's figures do not depend on the other
 * rows of the call.  Neither copies to the host nor synchronises.
 * n_in, n_out in [1, 2^24]; M <= 65535; ws 8-byte aligned, jvae_pr_workspace_bytes(...) bytes (0 = sizes out of range). */
size_t jvae_pr_workspace_bytes(int M, long n_in, long n_out);
int jvae_pr_metrics_f32(const float* ins, const float* outs, const int* modes, double* figures, int* status,
                        int M, long n_in, long n_out, void* ws, size_t ws_bytes, void* stream);

/* ---- SCOD: selective classification with OOD data, score rows and risk curves (csrc/scod.hip) ----------------------
 * Replaces tests/scod.py of the reference (scoring_r, scoring_g, scoring, scrisk and the figures of its command-line block).
 * Scores: M <= 32 variants of ONE recorded set of N samples in one launch, row m of out (row stride out_stride >= N) =
 * r + weights[m] * g.  r_src / r_aux / g_src / g_alt: HOST arrays of M device pointers (NULL where the kind reads nothing),
 * kinds: HOST array of M pairs (r kind, g kind), weights: HOST array of M floats, y_est: (N,) int64 labels on the device.
 *   r kind  0  0.                             1  0.5 * r_src[y]   (r_src (C, N): zdist for `dist`, pre-zdist for `predist`)
 *           2  0.5 * r_src[y] - r_aux         (`logmsp`: r_src = zdist, r_aux (N,) = logsumexp_c(-0.5 zdist), computed by torch)
 *           3  1 - r_src                      (r_src (N,): a recorded `odin-*` row)
 *   g kind  0  0.     1  0.5 * (g_src[y] - g_alt)  (`elbo`)     2  -(g_src[y] - g_alt)  (`iws`)     3  g_src[y] - g_alt
 *           (g_src (C, N) the all-class loss, g_alt (N,) its `@` partner under the alternate prior; a 2-D partner: its row 0)
 *   kind -1 on one side: the row is the OTHER side alone (r, or the unweighted g), nothing is added.
 * Every product, difference and sum is rounded on its own: the reference's fp32 torch expressions bit for bit.  A label
 * outside [0, C) is never used as an index: that sample is NaN and *status (device int32, owned and cleared by the caller)
 * is set to 1, as for jvae_wim_scores_f32.  Neither allocates nor synchronises.  Malformed arguments: -1 (JVAE_EINVAL).
 * Curves: scores (M, n) fp32, the HIGHer the more likely to reject; y_true (n,) int64, the class of an in-distribution sample
 * and a negative value for an OOD one; y_est (n,) int64; n_in = the number of in-distribution samples (known to the host:
 * nothing is read back), 1 <= n_in < n <= 2^24, M <= 65535.  Each row is sorted ascending, stable by position, and scanned:
 *   curves (3, M, n) fp32 or NULL: tpr = in_cum / n_in, selective_risk = wrong_cum / in_cum (0 / 0 -> 0), fpr = ood_cum / n_ood
 *     - correctly rounded fp32 quotients of integers below 2^24, what scrisk returns bit for bit on tie-free scores;
 *   figures (M, 5) fp64 or NULL: fpr95, sr95 (the minimum of fpr and of selective_risk over tpr >= 0.95f), then the trapezoid
 *     areas AuROC (fpr, tpr), AuST (tpr, selective_risk), AuSCODT (tpr, 0.5 sr + 0.5 fpr formed in fp32), summed in fp64 over
 *     the fp32 curve values in a fixed order.
 * status (M int32, cleared by the call): bit 0 = a NaN score was seen, bit 1 = y_true does not hold n_in non-negative
 * entries; the outputs of such a row are meaningless (never out of bounds).  No float atomics; the same bits run to run.
 * ws 16-byte aligned, jvae_scod_workspace_bytes(M, n) bytes (0 = invalid sizes). */
int jvae_scod_scores_f32(const float* const* r_src, const float* const* r_aux, const float* const* g_src,
                         const float* const* g_alt, const int* kinds, const float* weights, const long long* y_est,
                         float* out, long out_stride, int M, int C, long N, int* status, void* stream);
size_t jvae_scod_workspace_bytes(int M, long n);
int jvae_scod_curve_f32(const float* scores, const long long* y_true, const long long* y_est, float* curves, double* figures,
                        int* status, int M, long n, long n_in, void* ws, size_t ws_bytes, void* stream);

/* ---- Misclassification detection: score rows, split by correctness, confusion counts (csrc/misclass.hip) ----------
 * What surrounds jvae_roc_curve_f32 in misclassification_detection_rates (reference cvae.py:1913-2079).
 * Scores: src (C, N) fp32 (all-class kl / zdist / iws losses, or the logits as the recorder stores them), C <= 128, read once;
 * row r of the R requested rows goes to out + rows[r] * out_stride (out_stride >= N), with kinds[r] / temps[r] (device arrays):
 *   0  max_c softmax_c(-v / T)   1  max_c softmax_c(v / T)   2  max_c (-v)   3  max_c v   4  sum_c p log p, p = softmax_c(v / T)
 * and, with l = -v, d = l - max_c l, e = exp d and temps[r] an additive constant (any finite value):
 *   5  log sum_c e + max_c l + temps[r]   6  kind 5 on l = +v   7  log mean_c e + max_c l   8  unbiased std_c l (C = 1: NaN)
 *   9  (std_c e / mean_c e)^2, unbiased   10  max_c l - median_c l (lower middle element)
 *   11  sum_c(d e) / (C mean_c e) - log mean_c e   12  -v   13  v   (12, 13: row 0 of the source, meant for C = 1)
 * (batch_dist_measures, cvae.py:985-1068), fp32 with the max-subtracted softmax; a NaN propagates as in torch; any other kind
 * above 4 gives a NaN row.
 * Split: scores (M, N), mask (N bytes, non-zero = correctly classified) -> out (M * N floats): ins (M, n_correct) followed by
 * outs (M, N - n_correct), each row in its original order; *n_correct (device int32) receives the count.  One scan of the mask
 * serves all rows.  ws: 4-byte aligned, jvae_misclass_split_workspace_bytes(N) bytes (0 = invalid N).
 * Confusion: thr (M, K) fp64 (thr_low of the ROC), K <= 16 -> tp / fp (M, K) int32: the correct / missed samples whose exactly
 * widened score is >= thr[m][k] (cvae.py:2009-2015).  Integer counts: independent of any order.
 * N in [1, 2^24], M <= 65535 (the limits of jvae_roc_curve_f32); beyond a bound: -1 (JVAE_EINVAL). */
int jvae_misclass_scores_f32(const float* src, const int* kinds, const float* temps, const int* rows, float* out,
                             int R, int C, long N, long out_stride, void* stream);
size_t jvae_misclass_split_workspace_bytes(long N);
int jvae_misclass_split_f32(const float* scores, const unsigned char* mask, float* out, int* n_correct, int M, long N,
                            void* ws, size_t ws_bytes, void* stream);
int jvae_misclass_confusion_f32(const float* scores, const unsigned char* mask, const double* thr, int* tp, int* fp,
                                int M, long N, int K, void* stream);

/* ODIN out-of-distribution scores (csrc/odin.hip; reference cvae.py:1645-1663): the two ends of the loop.
 * Head: logits of F batched forwards, element (f, l, n, c) at f * stride_f + l * stride_l + n * C + c with l = 0 .. L (row 0, the mean
 * latent, is left out of the mean), temps (F) -> scores (F, N) = max_c softmax_c(mean_{l >= 1} logits / temps[f]); dlogits (same
 * layout, or NULL) receives d(sum_n scores)/d(logits) = p_max (delta_{c,argmax} - p_c) / (L temps[f]) for l >= 1 and 0 for l = 0.
 * Ties in the max resolve to the first index.
 * Perturb: acc (numel) += g (NULL: acc is left as it is), then out (E, numel): out[e][i] = x[i] + eps[e] * sign(acc[i]) with
 * sign(0) = 0; eps (E) in device memory. */
int jvae_odin_head_f32(const float* logits, const float* temps, float* scores, float* dlogits,
                       int F, int L, int N, int C, long stride_f, long stride_l, void* stream);
int jvae_odin_perturb_f32(float* acc, const float* g, const float* x, const float* eps, float* out, long numel, int E,
                          void* stream);

/* ---- WIM score rows: the scores of a model fine-tuned with an alternate prior (csrc/wim.hip) -------------------------
 * Replaces the torch expressions of WIMJob.batch_dist_measures (reference ft/wim.py:132-201): about ten small launches per
 * method and batch become ONE launch for every row of a batch.
 * srcs / alts / factors: HOST arrays of S <= 4 entries - srcs[s] a (C, N) fp32 device tensor (the all-class kl, zdist, iws or
 * total losses), factors[s] its factor f (-1, -1/2, +1; -1 on `total` stands for elbo), alts[s] the (N,) fp32 loss of the same
 * name under the alternate prior, or NULL.  y_est: (N,) int64 estimated labels on the device.  specs: HOST array of R <= 16
 * triples (source index, kind, out row); row r goes to out + row * out_stride (out_stride >= N, rows distinct).  With
 * x = f * v, y = y_est[n], a = alts[s][n]:
 *   0  Y       x[y]                    `k~`          1  SOFT_Y  softmax_c(x)[y]             `softk~`
 *   2  LSE_AT  logsumexp_c(x) - f a    `k@`          3  Y_AT    x[y] - f a                  `k~@`
 * Kinds 0 and 3 are the torch expressions bit for bit for the factors above (f v is exact); kinds 1 and 2 are the max-shifted
 * fp32 forms.  A source is read at most twice whatever the number of its rows; no atomics, one writer per output element.
 * A label outside [0, C) is never used as an index: kinds 0, 1, 3 of that sample are NaN and *status (device int32, owned and
 * cleared by the caller) is set to 1 (bit 0).  Non-finite losses give unspecified values, never an access out of bounds.
 * Neither allocates nor synchronises.  1 <= C <= 128, else -2 (JVAE_ENOTSUP); any other malformed argument (a kind 2 / 3 row
 * of a source without alternate, a repeated out row, S, R or N out of range): -1 (JVAE_EINVAL). */
int jvae_wim_scores_f32(const float* const* srcs, const float* const* alts, const float* factors, int S, const long long* y_est,
                        const int* specs, int R, float* out, long out_stride, int C, long N, int* status, void* stream);
/* Running tally of the losses the fine-tuning loop prints (reference ft/job.py:401-417 reads a masked .mean().item() per
 * group and batch: one host synchronisation per batch).  values (R, N) fp32 rows, group (N,) int32 in [0, G) - a value outside
 * it (negative: "skip") leaves the sample out.  sums (R, G) fp64 and counts (G,) int64 are DEVICE accumulators the caller
 * owns and clears: sums[r][g] += sum of values[r][n] over group[n] == g, counts[g] += their number.  One workgroup, each
 * sum taken in fp64 in a fixed order (a strided walk per thread, then a tree over the threads): the same bits run to run;
 * no atomics, no allocation, no synchronisation.  1 <= R, 1 <= G, 0 <= N, R * G <= 4096, else -1. */
int jvae_group_tally_f32(const float* values, const int* group, double* sums, long long* counts, int R, int N, int G,
                         void* stream);

/* ---- Image generation: prior draws and the image grid (csrc/sample.hip) -------------------------------------------
 * The two ends of the reference's module/sample.py::sample(): noise -> latent draws of the prior, decoded rows -> the grid of
 * images, its cells and its 8-bit form.  Neither entry point allocates or synchronises; no atomics, one writer per output
 * element, the same bits run to run.
 * Draws: eps (R, K) fp32 noise, y (R,) int64 labels on the device or NULL (component 0 for every row), means (C, K), T the
 * whitening factor in the layout of GaussianPrior._var_parameter ((C,), (C, K) or (C, K, K): only the lower triangle is read;
 * NULL allowed in mode 0), t a temperature -> z (R, K) dense:
 *   0  UNIT    z = means[y] + t eps                 (module/sample.py:129-132: the prior's variance is ignored)
 *   1  SCALAR  z = means[y] + (t eps) / T[y]        2  DIAG  z = means[y] + (t eps) / T[y, k]
 *   3  FULL    z = means[y] + u, tril(T[y]) u = t eps        (the inverse of whiten(), module/priors.py:228-233)
 * Modes 0 - 2: each product, quotient and sum is rounded on its own, in that order - the fp32 torch expressions bit for bit
 * (t = 1, mode 0: the reference's z + mean).  Mode 3: one forward substitution per row in fp32 by one 64-lane wave; the order
 * of every sum depends on K alone, not on R or the launch.  A label outside [0, C) is never used as an index: its row is NaN
 * and *status (device int32, owned and cleared by the caller) is set to 1 (bit 0), as for jvae_wim_scores_f32.
 * 1 <= K <= 1024, 1 <= C, 0 <= R; any malformed argument: -1 (JVAE_EINVAL).
 * Grid: x_in (N, D, H, W) or NULL, decoded rows x_out (Rr, N, D, H, W), specs a DEVICE int32 array of Ncol triples
 * (kind, a, b) owned by the caller, specs_host the same values in host memory (checked there):
 *   0  INPUT    x_in[row]        1  DRAW  x_out[a, row]        2  AVERAGE  (sum_{l = a .. b} x_out[l, row]) / (b - a + 1)
 * (the sum in ascending l in fp32, then one division) -> cell (row, column) of grid_f32 (D, N H, Ncol W) and / or of
 * grid_u8 (N H, Ncol W, D), channel last (either may be NULL, not both).  The 8-bit value is
 * floor(min(max(v * 255 + 0.5, 0), 255)), product and sum rounded separately (torchvision's save_image:
 * mul(255).add_(0.5).clamp_(0, 255).to(uint8)); NaN gives 0.  INPUT and DRAW cells are copies.  16-byte accesses when W is a
 * multiple of 4 and the tensors are 16-byte aligned (grid_u8: 4-byte), a scalar path otherwise.
 * grid_u8 with D > 4: -2 (JVAE_ENOTSUP; any D for grid_f32 alone).  1 <= Ncol <= 1024; a kind-0 column without x_in, a kind
 * outside 0 .. 2, a or b of a kind-1 / kind-2 column outside [0, Rr), b < a in kind 2: -1 (JVAE_EINVAL). */
int jvae_prior_sample_f32(const float* eps, const long long* y, const float* means, const float* T, float* z, int* status,
                          long R, int K, int C, float t, int mode, void* stream);
int jvae_image_grid_f32(const float* x_in, const float* x_out, const int* specs, const int* specs_host, int Ncol, float* grid_f32,
                        unsigned char* grid_u8, int N, int D, int H, int W, int Rr, void* stream);

/* ---- Model ensembles: class posteriors of latent draws, pairwise latent mutual information, score aggregation
 * (csrc/aggregate.hip; reference module/aggregation.py, module/cascad.py, results/aggregation.py:321-374) -------------
 * None of the entry points allocates or synchronises; no atomics, one writer per output element, the order of every sum is
 * fixed by the shape: the same bits run to run.  temps: a HOST array of nT <= 16 temperatures; a NaN entry is a temperature of
 * the reference's NAN_TEMPS (None, -1, 0): its slot takes the logits unchanged.
 * Class posteriors: z (R, K) rows (the draws z[1:] of a model, R = L N), means (C, K), T the whitening factor in the layout
 * of GaussianPrior._var_parameter (var_dim 0 scalar (C,), 1 diag (C, K), 2 full (C, K, K): only the lower triangle is read),
 * log_det (C,) = log|Sigma_c| ->
 *   logp (C, R)      = (-(K / 2) log 2 pi - u / 2) - log_det[c] / 2,  u = |T_c (z_r - m_c)|^2 as jvae_latent_fwd_f32's zdist
 *   P    (nT, C, R)  = softmax_c(logp / temps[t]), max-shifted
 * (either may be NULL, not both; P needs nT >= 1).  Each row of z is read once whatever C and nT.  The quadratic form, logp and
 * the soft-max are taken in fp64 and rounded once: P is the soft-max of the unrounded logp.
 * 1 <= K <= 1024, 1 <= C <= 128, 0 <= R <= 2^30, else -1 (JVAE_EINVAL).
 * Latent mutual information: P0 (nT, C, L0, N), P1 (nT, C, L1, N) ->
 *   Im (nT, N),  Im[t, n] = 1 / (L0 L1) sum_{a < L0, b < L1} log sum_c P0[t, c, a, n] P1[t, c, b, n]
 * the class sum in fp32 (ascending c, fused multiply-adds), the logs added in fp64 in a fixed order, one division.  A draw
 * pair whose class sum is exactly 0 gives -inf, and so does its sample.  ws: device scratch of at least
 * jvae_latent_mi_workspace_bytes(nT, L0, N) bytes, 8-byte aligned (-3, JVAE_EWORKSPACE, when smaller).
 * 1 <= nT <= 16, 1 <= C <= 128, 1 <= L0, L1, else -1.
 * Score aggregation: srcs / factors HOST arrays of E <= 8 entries - srcs[e] a (C, N) fp32 device tensor x_e (mode 3: an (N,)
 * int64 tensor of predicted classes), factors[e] its factor f_e:
 *   0  MEAN       a = m + log((sum_e exp(f x_e - m)) / E), m = max_e f x_e       (log_mean_exp; iws, f = 1)
 *   1  JOINT      a = f_0 sum_e x_e, ascending e                                  (joint_posterior; zdist, f = -1/2)
 *   2  MEAN_SOFT  post[t] = (sum_e softmax_c(f x_e / T_t)) / E; NaN T_t: (sum_e f x_e) / E     (`mean~`; kl, f = -1; no a)
 *   3  VOTE       a = count_c / E; post[t] = a for every t
 * post (nT, C, N): softmax_c(a / T_t), or a for a NaN T_t; a (C, N); amax (N,) fp32 / argmax (N,) int64: maximum over c and
 * its lowest index of slot `slot` of post (-1: of a), a NaN kept.  Every output may be NULL, not all.  A vote outside [0, C)
 * is never used as an index: its sample is NaN in a / post and *status (device int32, owned and cleared by the caller; needed
 * in mode 3) is set to 1 (bit 0), as for jvae_wim_scores_f32.
 * 1 <= E <= 8, 1 <= C <= 128, 0 <= nT <= 16, -1 <= slot < nT, an unknown mode, a or slot -1 in mode 2: -1. */
int jvae_class_posterior_f32(const float* z, const float* means, const float* T, const float* log_det, const float* temps, int nT,
                             float* logp, float* P, long R, int K, int C, int var_dim, void* stream);
size_t jvae_latent_mi_workspace_bytes(int nT, int L0, long N);
int jvae_latent_mi_f32(const float* P0, const float* P1, float* Im, int nT, int C, int L0, int L1, long N, void* ws, size_t ws_bytes,
                       void* stream);
int jvae_aggregate_scores_f32(const void* const* srcs, const float* factors, int E, int mode, const float* temps, int nT, float* post,
                              float* a, float* amax, long long* argmax, int slot, int C, long N, int* status, void* stream);

/* ---- Chained models: stage-pair mean squared errors, sequential Bayesian update (csrc/cascad.hip; reference
 * module/cascad.py) ----------------------------------------------------------------------------------------------------
 * Neither entry point allocates or synchronises; no atomics, the order of every sum is fixed by the shape: the same bits run
 * to run.
 * Stage-pair MSE: x (N, D) fp32 is stage 0, stages a HOST array of M device pointers R_1 .. R_M, each (L, N, D) fp32 and
 * contiguous (any 4-byte aligned base: the views x_reco[1:] are taken as they are) ->
 *   mse (M (M + 1) / 2, N),  row p = i (i - 1) / 2 + j for 1 <= i <= M, 0 <= j < i (the reference's `for i: for j < i`):
 *   mse[p, n] = 1 / (L D) sum_{l, d} (R_i[l, n, d] - R_j[l, n, d])^2,  R_0[l] = x
 * in ONE pass: every stage element is loaded once, x once per (n, d); differences, squares and sums in fp64, one division,
 * one rounding.  16-byte loads where D % 4 == 0 and every base is 16-byte aligned, 4-byte loads otherwise - the same bits
 * either way.  ws: device scratch of at least jvae_cascade_mse_workspace_bytes(M, N, D) bytes, 8-byte aligned (-3,
 * JVAE_EWORKSPACE, when smaller).  1 <= M <= 8, 1 <= L, 0 <= N, 1 <= D <= 65535 * 256, N * ceil(D / 256) < 2^24 (the threads of
 * the launch stay below 2^32), else -1 (JVAE_EINVAL).
 * Sequential update: p (M, C, N) -> posterior (M, C, N) (another buffer than p), per sample
 *   prior_0 = 1 / C;  posterior[i] = p[i] prior / sum_c p[i] prior;  prior = posterior[i]
 * products and class sums in fp64, ascending c.  A stage whose class sum is 0 makes that sample NaN from that stage on.
 * 1 <= M <= 8, 1 <= C <= 128, 0 <= N <= 2^30, else -1. */
size_t jvae_cascade_mse_workspace_bytes(int M, long N, long D);
int jvae_cascade_mse_f32(const float* x, const void* const* stages, int M, float* mse, int L, long N, long D, void* ws,
                         size_t ws_bytes, void* stream);
int jvae_iterate_prior_f32(const float* p, float* posterior, int M, int C, long N, void* stream);

/* ---- Latent-space inspection: per-group posterior moments, nearest centroid, histogram (csrc/inspect.hip; reference
 * module/sample.py::zsample, ft/inspection.py, utils/inspection.py) ----------------------------------------------------
 * None of the entry points allocates or synchronises.  No floating-point atomics: every float result is the same bits run to
 * run and does not depend on the number of CUs; the exact counts are added with integer atomics.
 * Moments: mu, log_var (N, K) fp32, group (N,) int32 in [0, G) or NULL (every sample in group 0, G = 1) - a value outside
 * [0, G) leaves the sample out, as in jvae_group_tally_f32.  sums (G, 4, K) fp64 and counts (G,) int64 are DEVICE accumulators
 * the caller owns and clears:
 *   sums[g, 0..3, k] += sum over group[n] == g of mu, mu^2, v, v^2,  v = expf(log_var[n, k]) widened to fp64
 *   counts[g]        += the number of such n
 * Rows are summed in slabs of 256 (inside a slab: four interleaved runs, folded as (0 + 1) + (2 + 3)), the slabs in ascending
 * order: the order hangs on N alone.  ws: device scratch of at least jvae_latent_moments_workspace_bytes(N, K, G) bytes, 8-byte
 * aligned (-3, JVAE_EWORKSPACE, when smaller).  1 <= K <= 65536, 1 <= G <= 65536, 0 <= N <= 2^24, else -2 (JVAE_ENOTSUP).
 * Nearest centroid: mu (N, K), centroids (C, K) -> y_nearest (N,) int64 = argmin_c |mu_n - m_c|^2, d2 (N,) fp32 the winner's
 * squared distance.  Differences, squares and sums in fp64, one rounding; the comparison is made on the fp64 sums, ties go to
 * the lowest index and a NaN distance comes before every number (torch.argmin).  1 <= K <= 65536, 1 <= C <= 65536,
 * 0 <= N <= 2^30, else -2.
 * Histogram: values (n,) fp32, edges (B + 1,) fp64 ascending ON THE DEVICE, group (n,) int32 in [0, G) or NULL ->
 *   counts[g, b] += #{i: group[i] == g, edges[b] <= values[i] < edges[b + 1]}, the last bin closed on the right
 * (np.histogram's rule).  counts (G, B) int64 is the caller's accumulator.  Values outside [edges[0], edges[B]] are not counted;
 * neither are NaN and +-inf, whose number is added to *nonfinite (device int64, owned and cleared by the caller).  The bin is
 * found by bisection of the edges in fp64; edges that do not ascend give unspecified counts, never an access out of bounds.
 * B <= 4096 and G B <= 4096: edges and private counters in LDS.  G B <= 2^26, else -2.
 * Any other malformed argument: -1 (JVAE_EINVAL). */
size_t jvae_latent_moments_workspace_bytes(int N, int K, int G);
int jvae_latent_moments_f32(const float* mu, const float* log_var, const int* group, double* sums, long long* counts, int N, int K,
                            int G, void* ws, size_t ws_bytes, void* stream);
int jvae_nearest_centroid_f32(const float* mu, const float* centroids, long long* y_nearest, float* d2, long N, int K, int C,
                              void* stream);
int jvae_histogram_f32(const float* values, const double* edges, const int* group, long long* counts, long long* nonfinite, long n,
                       int B, int G, void* stream);

/* ---- 2-D projections of recorded latents: exact t-SNE and PCA (csrc/embed.hip; reference ft/inspection.py::proj2d, there
 * through scikit-learn) ------------------------------------------------------------------------------------------------
 * None of the entry points allocates or synchronises.  No floating-point atomics: every sum is a fixed-order reduction whose
 * order hangs on the sizes alone, the same bits run to run.  Pair arithmetic is fp64; tensors are fp32 unless stated.
 * Distances: x (N, K) -> d (N, N), d_ij = fp32(sum_k (double(x_ik) - double(x_jk))^2), k ascending, each operation rounded on
 * its own: d is exactly symmetric with an exactly zero diagonal.
 * Affinities: d (N, N) -> beta (N,) fp64, S (N,) fp64 and P (N, N): per row scikit-learn's search for the precision beta_i at
 * which the conditional distribution p_j|i = exp(-d_ij beta_i) / S_i (j != i) has the given perplexity (beta from 1, at most
 * 100 steps, stop at |H - log perplexity| <= 1e-5f, S = 0 replaced by 1e-8f), then
 *   P_ij = max((p_j|i + p_i|j) / max(sum P, eps), eps),  eps = 2^-52,
 * formed in fp64 and rounded once.  The diagonal holds eps.  ws: jvae_tsne_affinities_workspace_bytes(N) bytes, 8-byte aligned.
 * Gradient: P (N, N), y (N, 2) -> g (N, 2), with qn_ij = 1 / (1 + |y_i - y_j|^2) and Z = sum_{i != j} qn_ij
 *   g_i = 4 (exaggeration sum_j P_ij qn_ij (y_i - y_j) - sum_j qn_ij^2 (y_i - y_j) / Z)      (j != i)
 * rounded once to fp32; as in scikit-learn the distance in qn is taken on the widened y and the factor (y_i - y_j) is the fp32
 * difference, widened.  P itself is never rescaled.  stats (2 fp64 device words, or NULL): a second pass leaves
 *   stats[0] = sum_{i != j} f P_ij log(max(f P_ij, eps) / max(qn_ij / Z, eps)),  f = exaggeration;   stats[1] = |g|_2.
 * ws: jvae_tsne_gradient_workspace_bytes(N) bytes, 8-byte aligned.
 * Update: scikit-learn's gradient-descent step on the 2 N values, as numpy executes it in fp32 (each product and sum rounded):
 *   gains = max(update * g < 0 ? gains + 0.2 : gains * 0.8, 0.01);  g *= gains;  update = momentum * update - lr * g;  y += update
 * norm (one fp64 device word, or NULL) receives |g|_2 of the scaled g, which is what scikit-learn's stopping rule looks at.
 * 2 <= N <= 16384 (a row of distances in LDS) and 1 <= K <= 1024 for the above, else -2 (JVAE_ENOTSUP); N < 2: -1.
 * PCA moments: x (N, K) -> mean (K,) fp64 and cov (K, K) fp64 = (x - mean)^T (x - mean) / (N - 1), summed in fp64 over at most
 * 8 slabs of rows that are folded in ascending order; cov is exactly symmetric.  2 <= N <= 2^24, K <= 1024.
 * ws: jvae_pca_moments_workspace_bytes(N, K) bytes, 8-byte aligned (-3, JVAE_EWORKSPACE, when smaller).
 * Projection: out (N, n_components) = fp32((x - mean) V^T), V (n_components, K) fp64, k ascending.  n_components <= 16.
 * Any other malformed argument: -1 (JVAE_EINVAL).  A refused call launches nothing and writes nothing. */
int jvae_pairwise_sqdist_f32(const float* x, float* d, int N, int K, void* stream);
size_t jvae_tsne_affinities_workspace_bytes(int N);
int jvae_tsne_affinities_f32(const float* d, float* P, double* beta, double* S, float perplexity, int N, void* ws, size_t ws_bytes,
                             void* stream);
size_t jvae_tsne_gradient_workspace_bytes(int N);
int jvae_tsne_gradient_f32(const float* P, const float* y, float* g, float exaggeration, int N, double* stats, void* ws,
                           size_t ws_bytes, void* stream);
int jvae_tsne_update_f32(float* y, float* update, float* gains, float* g, float momentum, float lr, int N, double* norm,
                         void* stream);
size_t jvae_pca_moments_workspace_bytes(long N, int K);
int jvae_pca_moments_f32(const float* x, double* mean, double* cov, long N, int K, void* ws, size_t ws_bytes, void* stream);
int jvae_project_f32(const float* x, const double* mean, const double* V, float* out, long N, int K, int n_components,
                     void* stream);

/* ---- k nearest neighbours of query rows among the rows of a bank (csrc/knn.hip; the deep-nearest-neighbour OOD score of Sun,
 * Ming, Zhu and Li 2022 over the posterior means of a training set; no counterpart in the reference) ------------------------
 * None of the entry points allocates or synchronises.  No floating-point atomics: same inputs, same bits, run to run and
 * whatever `splits` is.
 * Norms: x (M, K) fp32 -> sq (M,) fp32, sq_m = fmaf chain over k ascending of x_mk^2.  Computed once per bank.
 * Neighbours: q (N, K), q_sq (N,), bank (M, K), bank_sq (M,) -> d2_out (N, k) fp32, the k smallest squared distances of each
 * query row, ascending, and idx_out (N, k) int32, their bank rows.  The dot product of a pair is one fmaf chain over k ascending
 * (the fp32 matrix instruction), then
 *   normalized = 0:  d2 = max(fmaf(-2, q.b, |q|^2 + |b|^2), 0)
 *   normalized = 1:  d2 = max(fmaf(-2, q.b / (max(sqrt|q|^2, 1e-12) * max(sqrt|b|^2, 1e-12)), 2), 0)
 * the squared distance of the F.normalize()d rows, of which no copy is made.  Equal distances are ordered by ascending bank row.
 * With M < k the unused slots hold +inf and -1.  A bank row whose distance is not finite is never selected and sets bit 0 of the
 * device word *status; a query row with a non-finite element (or norm) gets NaN and -1 in all k slots and sets bit 1.  The word
 * is only ever OR-ed into: the caller owns and clears it.
 * splits: the number of bank partitions that are selected independently and merged by a second, fixed-order launch; 0: chosen
 * here.  ws: device scratch of jvae_knn_workspace_bytes(N, M, K, k, splits) bytes, 4-byte aligned (-3, JVAE_EWORKSPACE, when
 * smaller).  1 <= k <= 64, 1 <= K <= 4096, M < 2^31, N < 2^31, else -2 (JVAE_ENOTSUP) and a workspace size of 0; splits outside
 * 0 .. 1024, a negative size or a missing pointer: -1 (JVAE_EINVAL).  N = 0 launches nothing. */
int jvae_knn_sqnorms_f32(const float* x, float* sq, long M, int K, void* stream);
size_t jvae_knn_workspace_bytes(long N, long M, int K, int k, int splits);
int jvae_knn_f32(const float* q, const float* q_sq, const float* bank, const float* bank_sq, float* d2_out, int* idx_out, long N,
                 long M, int K, int k, int normalized, int splits, int* status, void* ws, size_t ws_bytes, void* stream);

/* ---- Mahalanobis scores against Gaussians fitted on a bank (csrc/maha.hip; Lee et al. 2018, the relative form of Ren et al. 2021;
 * no counterpart in the reference) -------------------------------------------------------------------------------------------
 * None of the entry points allocates or synchronises.  No floating-point atomics: same inputs, same bits, run to run.
 * Moments: bank (M, K) fp32, labels (M,) int64 -> counts (C,) int64, means (C, K), mean0 (K,), Sw (K, K) and St (K, K) fp64:
 * the class sizes and means, the overall mean, and the scatter of the rows about the mean of their class (Sw) and about mean0
 * (St), each divided by the number of rows summed.  All sums are fp64 in a fixed order that hangs on M alone; Sw and St are
 * symmetric to the bit.  A row whose label is outside [0, C) sets bit 0 of *status, a row with a non-finite element bit 1; such
 * a row is in no sum and in no count.  An empty class has a mean of zeros.  ws: device scratch of
 * jvae_maha_moments_workspace_bytes(M, K, C) bytes, 8-byte aligned (-3 when smaller).  1 <= K <= 256, 1 <= C <= 128,
 * 1 <= M < 2^31, else -2 (a size below 1, a missing pointer: -1) and a workspace size of 0.
 * Scores: q (N, K) fp32; mu0 (K,) fp32; W (2K, K) fp32, the whitening matrix of Sw stacked on that of St; m (Cn, K) fp32, the
 * whitened, mu0-centred means of the Cn non-empty classes in ascending label order; m0 (K,) fp32, the overall mean treated the
 * same way (the whitened rounding error of mu0); cmap (Cn,) int32, the classes' labels in [0, C).
 * With x = q - mu0, y = W x (each y_k one fmaf chain over j ascending: the fp32 matrix instruction), d_c = sum_k (y_k - m_ck)^2
 * for k < K and d0 = sum_k (y_(K + k) - m0_k)^2 (fmaf chains over k ascending):
 *   d (N,) = min_c d_c, cls (N,) int32 = the label of the first class that attains it, rel (N,) = d - d0,
 *   per_class (N, C) or NULL: d_c in the column of its label, +inf in the column of an empty class.
 * A query row with a non-finite element gets NaN, -1, NaN (and NaN in all of per_class) and sets bit 2 of *status.  The word is
 * only ever OR-ed into: the caller owns and clears it.  ONE launch; neither y nor the (N, Cn) distances reach memory unless
 * per_class is given.  1 <= K <= 256, 1 <= Cn <= C <= 128, N < 2^31.  N = 0 launches nothing. */
size_t jvae_maha_moments_workspace_bytes(long M, int K, int C);
int jvae_maha_moments_f32(const float* bank, const long long* labels, long M, int K, int C, long long* counts, double* means,
                          double* mean0, double* Sw, double* St, int* status, void* ws, size_t ws_bytes, void* stream);
int jvae_maha_scores_f32(const float* q, const float* mu0, const float* W, const float* m, const float* m0, const int* cmap,
                         float* d, int* cls, float* rel, float* per_class, long N, int K, int Cn, int C, int* status, void* stream);

/* ---- Input complexity: the length of a lossless image code (csrc/ic.hip; Serra et al. 2020; no counterpart in the reference) ----
 * x (N, C, H, W) fp32 -> bits (N,) fp64, bits32 (N,) fp32 = (float)bits, choice (N,) int32.  Nothing is encoded: the exact
 * length of an achievable code is computed, in ONE launch, one workgroup per image; nothing is allocated or synchronised.
 * q = clamp(rint(255 x), 0, 255).  Planes: the channels; at C == 3 a second colour space (G, (R - G) mod 256, (B - G) mod 256).
 * Modes of a plane, over a = left, b = up, c = up-left (0 outside the image), residual (v - pred) mod 256:
 *   0: 0, 1: a, 2: b, 3: (a + b) >> 1, 4: PNG's Paeth, 5: the LOCO-I median edge detector, 6: stored at 8 n bits, n = H W.
 * A residual plane with histogram n_s over k used symbols costs, with table[m] = log2(m!) in fp64 for m = 0 .. table_len - 1,
 *   ((((8 + ((table[256] - table[k]) - table[256 - k])) + table[n + k - 1]) - table[k - 1]) - sum_s table[n_s]),
 * the sum over s ascending from 0 in fp64.  bits = min over the colour spaces of the sum over its planes, in their order, of
 * (3 + min over the modes), + 1 at C == 3; a tie goes to the lower index.  The counts are integers and every sum has one order:
 * the same bits on every call, no floating-point atomics.
 * choice = space | (mode of plane p + 1) << (4 + 3 p) for the planes of the chosen space.
 * A pixel with |255 x - q| > 1/64 sets bit 0 of *status (the length is that of the quantised image); a non-finite pixel sets
 * bit 1, and its image gets NaN, NaN, -1 while the other images are untouched.  The word is only ever OR-ed into: the caller
 * owns and clears it.  1 <= C <= 4, 1 <= H, W, H W <= 2^20, N < 2^31, else -2; N < 0, table_len < n + 257 or a missing pointer:
 * -1.  N = 0 launches nothing. */
int jvae_image_code_length_f32(const float* x, long N, int C, int H, int W, const double* table, long table_len, double* bits,
                               float* bits32, int* choice, int* status, void* stream);

/* ---- Density-of-states scores: a Gaussian kernel density estimate over a score bank (csrc/dose.hip; Morningstar et al. 2021,
 * Nalisnick et al. 2019; no counterpart in the reference) ------------------------------------------------------------------------
 * None of the entry points allocates or synchronises.  No floating-point atomics: same inputs, same bits, run to run.
 * Fit: bank (S, M) fp32, row s = statistic s of M samples.  factors: a HOST pointer to three doubles, read by the call itself:
 * bandwidth, scott1 = M^(-1/5), scottS = M^(-1/(S + 4)).  -> centre (S,), sigma (S,) (ddof = 1), h1 = bandwidth * sigma * scott1,
 * hS = bandwidth * sigma * scottS, lognorm (S + 1,): log(M h1_s) + log(2 pi) / 2 for s < S, then log M + sum_s log hS_s +
 * (S / 2) log(2 pi); all fp64, every sum in a fixed order that hangs on M alone.  z (S, M) fp32 = ((double)bank - centre) / h1,
 * rounded once.  A non-finite element of row s sets bit s of *status, a row whose sigma is not a positive finite number bit
 * 8 + s.  ws: device scratch of jvae_kde_fit_workspace_bytes(M, S) bytes, 8-byte aligned (-3 when smaller).  1 <= S <= 8,
 * 2 <= M <= 2^24, else -2 and a workspace size of 0; M < 2, S < 1, a factor that is not positive, a missing pointer: -1.
 * Scores: stats (S, N) fp32, raw -> out (2 S + 2, N) fp32.  With t = fp32(((double)stats - centre) / h1):
 *   rows 0 .. S - 1   the marginal log-densities logsumexp_m(-((t_s - z_sm)^2) / 2) - lognorm[s];
 *   row S             their sum over s ascending, in fp64, rounded once;
 *   row S + 1         the product-kernel log-density logsumexp_m(-(*ratio2 / 2) sum_s (t_s - z_sm)^2) - lognorm[S];
 *   rows S + 2 ..     the typicality -|stats_s - centre_s| / sigma_s.
 * ratio2: a HOST pointer to one double, (h1 / hS)^2, the same for every row.  Differences, squares and exponentials are fp32.
 * Every sum is shifted by its largest exponent, piece by piece of jvae_kde_partition() bank values - a partition that depends on
 * neither N nor the grid, so a query's bits do not depend on the batch it is in.  A query element that is +-inf gives -inf in the
 * rows that read it (its marginal and typicality row, rows S and S + 1); so does a finite element so far from the bank that a
 * square overflows fp32 (|t - z| above 2^63; its typicality row stays finite; where only the SUM of the squares overflows, row
 * S + 1 alone); a NaN gives NaN there.  All of them set bit 16 of *status and leave the other columns untouched.  The word is
 * only ever OR-ed into: the caller owns and clears it.  ONE scoring launch and one merge launch.  ws: device scratch of
 * jvae_kde_workspace_bytes(N, M, S) bytes, 8-byte aligned.  N = 0 launches nothing; N < 2^31. */
int jvae_kde_partition(void);
size_t jvae_kde_fit_workspace_bytes(long M, int S);
int jvae_kde_fit_f32(const float* bank, long M, int S, const double* factors, float* z, double* centre, double* sigma, double* h1,
                     double* hS, double* lognorm, int* status, void* ws, size_t ws_bytes, void* stream);
size_t jvae_kde_workspace_bytes(long N, long M, int S);
int jvae_kde_logdensity_f32(const float* stats, const float* z, const double* centre, const double* sigma, const double* h1,
                            const double* lognorm, float* out, long N, long M, int S, const double* ratio2, int* status, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- SSIM of images against their reconstructions (csrc/ssim.hip; Wang et al. 2004, Bergmann et al. 2018; no counterpart in the
 * reference) ----
 * x (N, C, H, W) fp32, y (R, N, C, H, W) fp32 -> ssim (R, N) fp32, cs (R, N) fp32 and, where map is not NULL, map (R, N, H - 10,
 * W - 10) fp32.  ONE launch; nothing is allocated or synchronised.  g: the 11 taps exp(-k^2 / 4.5), k = -5 .. 5, over their sum
 * (formed in fp64, rounded to fp32), applied separably over the valid region.  Per plane, with a = fp32(the fp64 mean of the
 * plane of x), x' = x - a and y' = y - a:
 *   mx = g*x', my = g*y', vx = g*x'^2 - mx^2, vy = g*y'^2 - my^2, cxy = g*x'y' - mx my   (products rounded, then fmaf chains),
 *   cs = ((cxy + cxy) + C2) / ((vx + vy) + C2), fx = a + mx, fy = a + my,
 *   l = ((fx fy + fx fy) + C1) / ((fx fx + fy fy) + C1), C1 = 1e-4, C2 = 9e-4 (data range 1),
 * every operation fp32, rounded as written.  ssim[r, n] = the mean of l cs over channels and valid pixels, cs[r, n] that of cs
 * (fp64 sums in a fixed order, one division, rounded once); map[r, n] = the channel mean of l cs (fp32, channels ascending).
 * This is scikit-image's structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=1) on its
 * interior.  A draw equal to its image scores exactly 1.  No output bit depends on N, R, the place of a sample or draw in the
 * batch, or on whether map is given.  A non-finite pixel in x[n] sets bit 0 of *status and makes ssim, cs (and map) of every
 * [r, n] NaN; one in y[r, n] sets bit 1 and makes that entry NaN.  The word is only ever OR-ed into: the caller owns and clears
 * it.  C >= 1, 11 <= H <= 32768, 11 <= W <= 128 (a strip of rows is staged at full width), N, R < 2^31, else -2; N < 0, R < 0 or
 * a missing pointer (map may be NULL): -1.  N = 0 or R = 0 launches nothing.
 * jvae_ssim_strip_rows: the output rows of one staged strip at this shape (0 for a refused shape): host only. */
int jvae_ssim_f32(const float* x, const float* y, long N, long R, int C, int H, int W, float* ssim, float* cs, float* map,
                  int* status, void* stream);
int jvae_ssim_strip_rows(int H, int W);

/* ---- log-density of the aggregate posterior of a bank of diagonal Gaussians (csrc/aggpost.hip; Hoffman & Johnson 2016, Chen et
 * al. 2018; no counterpart in the reference) ----
 * Bank: mu, log_var (N, K) fp32 and, for the conditional form, group (N,) int32 >= 0.  Prepare (once per bank): with Np =
 * jvae_aggpost_padded_rows(N) (N rounded up to the row tile; 0 for N out of range; host only), muT, wT, lvT (K, Np) fp32 = mu,
 * fp32(exp(-(double)log_var)) and log_var k-major (padding rows 0) and c (Np,) fp32 = fp32(sum_k (double)log_var), k ascending.
 * Scores: z (M, K) fp32, zgroup (M,) int32 ->
 *   logq (M,) fp32 = log 1/|S_m| sum_{n in S_m} N(z_m; mu_n, diag exp(log_var_n)), S_m all rows or, with conditional != 0, the rows
 *   with group == zgroup[m] (zgroup and group may be NULL otherwise);
 *   logq_dims (M, K) fp32 where not NULL: the same over S_m for each coordinate alone.
 * A pair's exponent is -Q / 2 with Q = c_n + sum_k (z - mu)^2 w, the fmaf chain acc = fmaf(d * d, w, acc) from acc = c_n on, k
 * ascending, d and d * d rounded on their own (a coordinate's: fmaf(d * d, w, log_var)).  Every sum is shifted by its smallest Q,
 * the difference taken before the scaling: its largest term is exactly 1 and every output is finite for every finite query whose
 * Q does not overflow fp32.  The bank is cut into pieces of jvae_aggpost_partition() rows whatever M is and every sum has a fixed
 * order: bits hang on (N, K, the piece size) alone, a subset of the queries gives the bits of its rows, there are no
 * floating-point atomics.  The end is fp64: -min Q / 2 + ln sum - ln |S_m| - (K / 2) ln 2 pi (K = 1 for a coordinate), rounded once.
 * *status takes an integer OR: bit 0 a non-finite stored operand (mu, exp(-log_var) or c), bit 1 a query with a non-finite
 * element (NaN -> NaN, +-inf -> -inf) or a finite one so far away that every Q overflows fp32 (-inf), bit 2 a query whose group
 * has no bank row (-inf).  The caller owns and clears the word.  Two launches for logq, two more for logq_dims.
 * ws: device scratch of jvae_aggpost_workspace_bytes(M, N, K, dims) = pieces M (8 + 4) + (dims ? pieces M K 8 : 0) bytes, pieces =
 * ceil(N / partition), 8-byte aligned (-3 when smaller).  1 <= K <= 1024, 1 <= N <= 2^24 (at most 16384 pieces), M < 2^31, else
 * -2 and a workspace size of 0; N < 1, K < 1, M < 0 or a missing pointer: -1.  M = 0 launches nothing. */
int jvae_aggpost_partition(void);
long jvae_aggpost_padded_rows(long N);
int jvae_aggpost_prepare_f32(const float* mu, const float* log_var, float* muT, float* wT, float* lvT, float* c, long N, int K,
                             void* stream);
size_t jvae_aggpost_workspace_bytes(long M, long N, int K, int dims);
int jvae_aggpost_logdensity_f32(const float* z, const int* zgroup, const float* muT, const float* wT, const float* lvT,
                                const float* c, const int* group, float* logq, float* logq_dims, long M, long N, int K,
                                int conditional, int* status, void* ws, size_t ws_bytes, void* stream);

/* ---- importance-weighted bound of the training step, forward and backward (csrc/iwae.hip; Burda et al. 2016; no counterpart in
 * the reference, whose `iws` (jvae_iws_f32) is an evaluation score without gradient) ----
 * For sample n of class y[n] and the draws l = 1..L (row 0 of z, the mean latent, takes no part):
 *   log w_l = -D/2 (wmse_s[l,n] + 2 log sigma + log 2pi) + beta (-1/2 |T_y (z_l - m_y)|^2 + sum_k log|t_yk| + 1/2 sum_k (eps_lk^2 + lv_k))
 *   bound[n] = logsumexp_l(log w_l) - log L,   wt[l,n] = softmax_l(log w_l),   ess[n] = 1 / sum_l wt^2
 * wmse_s (L, N), z (L+1, N, K), lv (N, K) the clipped log-variance, eps (L, N, K), y (N,) int64, means (C, K), T (C,) for var_dim 0
 * and (C, K) for var_dim 1 (the whitening factor of GaussianPrior), sigma as jvae_elbo_fwd_f32 takes it (kinds 0 value, 1 log, 2
 * coded).  log w is formed in fp64 (fixed-order sums) from these fp32 operands and never stored; what the fold reads is
 * fp32(log w - max).  (wmse_s itself is an fp32 row, magnified by D/2: a weight is as good as that row, not better.)  Forward: ONE
 * launch; the sum over l is shifted by its maximum, so every output is finite for finite inputs, and a draw that leads the others
 * beyond the fp32 exponent range gives a wt that is exactly one-hot and ess exactly 1.  state (may be NULL): (4, N) fp64 = (max,
 * shifted sum, shifted sum of squares, draws so far) of earlier slabs of draws, all zeros at the start; the slab is merged in
 * exactly (one of the two scale factors is exp(0) = 1) and bound / ess are those of all draws so far (wt stays the slab's own
 * softmax).
 * Backward: g_bound (N,) (NULL: zeros) and the forward's wt -> the DIRECT partial derivatives g_wmse_s (L, N) = -g wt D/2, g_z
 * (L+1, N, K) = -g wt beta T^T T (z - m) (row 0 zero), g_lv (N, K) = g beta/2 and, where not NULL, g_means (C, K), g_T (C, K; var_dim
 * 1 only, else -1) and g_sigma (1 value for kinds 0 / 1, N for kind 2), all overwritten.  The class sums run in sample order over a
 * fixed partition of 16 contiguous sample chunks and the sigma sum in a fixed order: no floating-point atomics, the same bits
 * from run to run (each product chain and each sum in fp64, rounded once).  ws: jvae_iw_bound_bwd_workspace_bytes(N, K) bytes,
 * 8-byte aligned, when any of the three is asked for (-3 when smaller).
 * A label outside [0, C) is never an index: NaN in every output of that sample, nothing added to any class.
 * prior != 0 (tilted, uniform), var_dim 2 (full) and sigma kind 3 (rmse): -2 before any launch.  L < 1, K < 1, C < 1, D < 1,
 * N < 0, an unknown kind or a missing pointer: -1.  N = 0 launches nothing in the forward. */
int jvae_iw_bound_fwd_f32(const float* wmse_s, const float* z, const float* lv, const float* eps, const long long* y,
                          const float* means, const float* T, const float* sigma, int sigma_is_log, int prior, int var_dim,
                          float beta, int L, int N, int K, int C, int D, float* bound, float* wt, float* ess, double* state,
                          void* stream);
size_t jvae_iw_bound_bwd_workspace_bytes(int N, int K);
int jvae_iw_bound_bwd_f32(const float* g_bound, const float* wt, const float* z, const long long* y, const float* means,
                          const float* T, const float* sigma, int sigma_is_log, int prior, int var_dim, float beta,
                          int L, int N, int K, int C, int D, float* g_wmse_s, float* g_z, float* g_lv, float* g_means,
                          float* g_T, float* g_sigma, void* ws, size_t ws_bytes, void* stream);

/* ---- beta-TCVAE split of the training step, forward and backward (csrc/tcvae.hip; Chen et al. 2018; no counterpart in the
 * reference) ----
 * For sample i of class y[i], its draws l = 1..L (row 0 of z takes no part) and S_i = the rows j of the batch with y[j] = y[i]:
 *   l_ijk = -1/2 (lv_jk + (z_lik - mu_jk)^2 e^(-lv_jk) + log 2pi),    c_i = log |S_i| + log n_i
 *   A = -1/2 sum_k (eps_lik^2 + lv_ik) - K/2 log 2pi,   J = logsumexp_{j in S_i} sum_k l_ijk - c_i,
 *   P = sum_k [logsumexp_{j in S_i} l_ijk - c_i],       Bp = log p(z_li | y_i) of the Gaussian prior (means, T as jvae_iw_bound_fwd_f32)
 *   mi = mean_l (A - J),  tc = mean_l (J - P),  dwkl = mean_l (P - Bp),  reg = alpha mi + beta_tc tc + gamma dwkl        each (N,)
 * z (L+1, N, K), mu, lv (N, K), eps (L, N, K), y (N,) int64, log_n (C,) fp64 = log of the training samples behind each class (NULL:
 * n_i = |S_i|).  The two logsumexp are the aggregate posterior of jvae_aggpost_logdensity_f32 with the batch as the bank and the
 * labels as the groups: the same kernels, the same bits for the same pair; every logarithm ends in fp64 and every output is
 * rounded once.  keep: jvae_tc_keep_bytes(L, N, K) bytes, 16-byte aligned, written by the forward and read by the backward (every
 * joint exponent Q_ij, the merged (min, 1 / sum) pairs, e^(-lv)); ws: jvae_tc_fwd_workspace_bytes(L, N, K) bytes of scratch, 16-byte
 * aligned.  Both queries answer 0 for a shape the file does not compute.
 * Backward: g_reg (N,) (NULL: zeros) -> the DIRECT partial derivatives g_z (L+1, N, K; row 0 zero), g_mu, g_lv (N, K) and, where not
 * NULL, g_means (C, K) and g_T (C, K; var_dim 1 only, else -1), all overwritten; ws: jvae_tc_bwd_workspace_bytes(N, K) bytes, 8-byte
 * aligned, when a class gradient is asked for.  Every sum has a fixed order (row pass: j ascending; column pass: i ascending, then l
 * ascending; class sums as jvae_iw_bound_bwd_f32) and runs in fp64: no floating-point atomics, the same bits from run to run.  With
 * alpha = beta_tc = gamma the mixture cancels and its weights are exactly 0.
 * A label outside [0, C) is never an index: NaN in every output of that sample, it is in nobody's set and adds to no class.
 * jvae_tc_joint_partition(): the rows of a piece of the joint sum (the error bound of the tests counts one merge step per piece).
 * K > 1024, N > 8192, L N^2 > 2^26 (256 MB of kept exponents), var_dim 2: -2 before any launch.  L < 1, K < 1, C < 1, N < 0, a NaN
 * weight or a missing pointer: -1; a short keep or ws: -3.  N = 0 launches nothing in the forward. */
int jvae_tc_joint_partition(void);
size_t jvae_tc_keep_bytes(int L, int N, int K);
size_t jvae_tc_fwd_workspace_bytes(int L, int N, int K);
size_t jvae_tc_bwd_workspace_bytes(int N, int K);
int jvae_tc_objective_fwd_f32(const float* z, const float* mu, const float* lv, const float* eps, const long long* y,
                              const float* means, const float* T, const double* log_n, int var_dim, float alpha, float beta_tc,
                              float gamma, int L, int N, int K, int C, float* reg, float* mi, float* tc, float* dwkl, void* keep,
                              size_t keep_bytes, void* ws, size_t ws_bytes, void* stream);
int jvae_tc_objective_bwd_f32(const float* g_reg, const float* z, const float* mu, const float* lv, const long long* y,
                              const float* means, const float* T, int var_dim, float alpha, float beta_tc, float gamma, int L,
                              int N, int K, int C, const void* keep, size_t keep_bytes, float* g_z, float* g_mu, float* g_lv,
                              float* g_means, float* g_T, void* ws, size_t ws_bytes, void* stream);

/* ---- class-marginal KL of the unlabelled rows of a training batch, forward and backward (csrc/semisup.hip; the bound of Hershey &
 * Olsen 2007; no counterpart in the reference) ----
 * mu, lv (N, K) (lv: the clipped log-variance), y (N,) int64, means (C, K), T ((C,) var_dim 0 / (C, K) var_dim 1) as
 * jvae_latent_fwd_f32 takes them, log_pi (C,) fp64 = the logarithms of the class weights (NULL: uniform), w the weight of var_kl.
 * A row with y >= 0 is labelled: kl / zdist / var_kl are its kl_in / zdist_in / var_kl_in bit for bit, its row of r is one-hot on
 * y (all zero for y >= C, which is never an index).  A row with y < 0 has no label:
 *   d_c = sum_k t_ck^2 (mu_k - m_ck)^2,   v_c = sum_k (e^lv_k t_ck^2 - lv_k - log t_ck^2 - 1),   KL_c = 1/2 (d_c + w v_c)
 *   kl = U = -log sum_c pi_c exp(-KL_c),   r_c = pi_c exp(-KL_c) / sum_c' pi_c' exp(-KL_c'),
 *   zdist = sum_c r_c d_c,   var_kl = sum_c r_c v_c
 * U is an upper bound of KL(q || sum_c pi_c p_c).  ONE launch; fp64 from the fp32 operands to the one rounding of each output; the
 * sum is shifted by min_c (KL_c - log pi_c).  r (N, C) fp32, jvae_semi_keep_bytes(N, C) bytes: returned, and read by the backward.
 * ws: jvae_semi_fwd_workspace_bytes(N, C) bytes of scratch, 8-byte aligned.  Both queries answer 0 for a shape the file does not
 * compute.
 * Backward: g_kl (N,) (NULL: zeros) -> g_kl_in (N,) (g_kl of a labelled row, 0 of an unlabelled one), g_mu, g_lv (N, K) (zero rows
 * for labelled samples) and, where not NULL, g_means (C, K) and g_T (C, K; var_dim 1 only, else -1), all overwritten.  Two launches
 * (one when no class gradient is asked for), fp64 sums of fp32 operands in fixed orders (rows: c ascending; classes: 16 contiguous
 * chunks of rows in row order, folded in chunk order), no atomics: the same bits from run to run.  zdist and var_kl carry no gradient.
 * -1 before any launch: a missing or misaligned pointer (4 bytes; y, log_pi and ws 8), var_dim other than 0 or 1, a non-finite w,
 * K < 1, K > 1024, C < 1, C > 1024, N < 0, N > 2^20; -3: a short r or ws.  N = 0 launches nothing in the forward. */
size_t jvae_semi_keep_bytes(int N, int C);
size_t jvae_semi_fwd_workspace_bytes(int N, int C);
int jvae_semi_class_marginal_fwd_f32(const float* mu, const float* lv, const long long* y, const float* means, const float* T,
                                     const double* log_pi, int var_dim, float w, int N, int K, int C, const float* kl_in,
                                     const float* zdist_in, const float* var_kl_in, float* kl, float* zdist, float* var_kl, float* r,
                                     size_t r_bytes, void* ws, size_t ws_bytes, void* stream);
int jvae_semi_class_marginal_bwd_f32(const float* g_kl, const float* mu, const float* lv, const long long* y, const float* means,
                                     const float* T, int var_dim, float w, int N, int K, int C, const float* r, size_t r_bytes,
                                     float* g_kl_in, float* g_mu, float* g_lv, float* g_means, float* g_T, void* stream);

/* ---- MMD-regularised bound of the training step, forward and backward (csrc/mmd.hip; InfoVAE, Zhao et al. 2019; WAE-MMD,
 * Tolstikhin et al. 2018; no counterpart in the reference) ----
 * For sample i of class y[i], its draws l = 1..L (row 0 of z takes no part) and S_i = the rows j of the batch with y[j] = y[i]
 * (joint = 0: the whole batch):
 *   p_li = means[y_i] + eps_p_li / T[y_i(, k)]     (the 'scalar' / 'diag' expression of jvae_prior_sample_f32, bit for bit)
 *   m_i  = mean_l [ 1/(N-1) sum_{j in S_i, j != i} k(z_li, z_lj) + 1/(N-1) sum_{j in S_i, j != i} k(p_li, p_lj)
 *                 - 2/N sum_{j in S_i} k(z_li, p_lj) ]                                (N = 1: the two within sums are 0)
 *   kind 0 (imq): k(a, b) = sum_s scales[s] / (scales[s] + |a - b|^2);  kind 1 (rbf): sum_s exp(-|a - b|^2 / (2 scales[s]))
 * mean_i m_i is the unbiased U-statistic of MMD^2 between q(z, y) and pi_hat(y) p(z | y).  z (L+1, N, K), eps_p (L, N, K), y (N,)
 * int64, means (C, K), T ((C,) var_dim 0 / (C, K) var_dim 1) on the device; scales: n_scales (1..8) positive finite floats in
 * HOST memory, read before the call returns.  Squared distances are direct fp32 chains over k (never |a|^2 + |b|^2 - 2ab); kernel
 * values are fp32; every sum over pairs is an fp64 chain in a fixed order, each output is rounded once.  m (N,).
 * Backward: g_m (N,) (NULL: zeros) -> the DIRECT partial derivatives g_z (L+1, N, K; row 0 zero) and, where not NULL, g_means
 * (C, K) and g_T ((C,) var_dim 0 / (C, K) var_dim 1) through p, all overwritten.  Kernel values are formed again: nothing is kept
 * between the two calls and there is no limit on L N^2.  The class sums run as those of jvae_iw_bound_bwd_f32.  No floating-point
 * atomics: the same bits from run to run.  Coincident points add exactly 0; with g_m all zero every gradient is exactly 0.
 * ws: jvae_mmd_fwd_workspace_bytes / jvae_mmd_bwd_workspace_bytes(L, N, K) bytes of scratch, 16-byte aligned; both queries answer
 * 0 for a shape the file does not compute.  jvae_mmd_tile: the rows of a workgroup's tile (host only).
 * A label outside [0, C) is never an index: NaN in every output of that sample, it is in nobody's set and adds to no class.
 * K > 1024, N > 8192, L > 65535, var_dim 2: -2 before any launch.  L < 1, K < 1, C < 1, N < 0, an unknown kind, joint other than
 * 0 / 1, n_scales outside 1..8, a scale that is not positive and finite or a missing pointer: -1; a short ws: -3.  N = 0 launches
 * nothing in the forward and writes zeros to the class gradients in the backward. */
int jvae_mmd_tile(void);
size_t jvae_mmd_fwd_workspace_bytes(int L, int N, int K);
size_t jvae_mmd_bwd_workspace_bytes(int L, int N, int K);
int jvae_mmd_objective_fwd_f32(const float* z, const float* eps_p, const long long* y, const float* means, const float* T,
                               int var_dim, int kind, const float* scales, int n_scales, int joint, int L, int N, int K, int C,
                               float* m, void* ws, size_t ws_bytes, void* stream);
int jvae_mmd_objective_bwd_f32(const float* g_m, const float* z, const float* eps_p, const long long* y, const float* means,
                               const float* T, int var_dim, int kind, const float* scales, int n_scales, int joint, int L, int N,
                               int K, int C, float* g_z, float* g_means, float* g_T, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* JVAE_HIP_H */
