// Kernel selection for one (transposed) convolution, both layouts: jvae_conv_route() (conv_dispatch.hip) is the only code
// that decides which leaf kernel runs; the queries and the entry points read its result.  Fast implicit kernels where the
// geometry matches, the generic unfold+GEMM path otherwise (fp32; the bf16 path has no generic kernel).  x = layer input,
// y = layer output, w = the layer's weight in its PyTorch layout ([Cout][Cin][KH][KW] for Conv2d, [Cin][Cout][KH][KW] for
// ConvTranspose2d).  The kernel-family functions declared below are plain launchers: they take what the route chose.
#pragma once
#include "common.h"
#include "jvae_internal.h"

// conv_generic.hip
size_t jvae_conv_generic_ws(const ConvGeom& g);
int jvae_fold_fwd(const ConvGeom& g, const float* xb, const float* w, const float* bias, float* ys,
                  float* ws, size_t ws_bytes, hipStream_t st);
int jvae_fold_bwd(const ConvGeom& g, const float* ys, const float* w, const float* bias, float* xb,
                  float* ws, size_t ws_bytes, hipStream_t st);
int jvae_fold_wgrad(const ConvGeom& g, const float* xb, const float* ys, float* dw,
                    float* ws, size_t ws_bytes, hipStream_t st);
size_t jvae_channel_sum_ws_bytes(int C);
int jvae_channel_sum(const float* t, float* out, int N, int C, int P, int accumulate, float* ws, size_t ws_bytes,
                     hipStream_t st);

// conv_mfma.hip: implicit-GEMM 5x5 kernels (forward-type) on the fp32 matrix cores
bool jvae_conv5_fwd_ok(int Cin, int H, int W, int Cout, int OH, int OW, int S, int P);
size_t jvae_conv5_pack_floats(int Cin, int Cout);
int jvae_conv5_fwd(const float* in, const float* w, int swap, int flip, const float* bias, float* out,
                   int N, int Cin, int H, int W, int Cout, int OW, int S, int P, float* ws, hipStream_t st,
                   float* stats = nullptr, int* nsplit = nullptr, const InAff* aff = nullptr);
int jvae_conv5_fwd_max_splits(int N, int OW);

int jvae_conv5_pack(const float* w, float* wp, int C, int O, int swap, int flip, hipStream_t st);

// conv_x3.hip: the same operator on the bf16 matrix cores, every fp32 operand split exactly into three bf16 terms
bool jvae_conv5_x3_ok(int Cin, int H, int W, int Cout, int OH, int OW, int S, int P);
size_t jvae_conv5_x3_pack_bytes(int Cin, int Cout);
int jvae_conv5_x3_set(int mode);
int jvae_conv5_x3_set_shape16(int on);
bool jvae_conv5_x3_enabled();
int jvae_conv5_x3_wpack(const float* w, float* ws, int C, int O, int swap, int flip, hipStream_t st);
// conv_t2_x3.hip: the 4-phase stride-2 transposed convolution in the same arithmetic (w = raw weight, [c][o][tap])
bool jvae_convt2_x3_ok(int N, int C, int WS, int O);
int jvae_convt2_x3(const float* in, const float* w, const float* bias, float* out, int N, int C, int WS, int O, float* ws,
                   hipStream_t st, float* stats = nullptr, int* nsplit = nullptr, const InAff* aff = nullptr);
int jvae_conv5_x3_fwd(const float* in, const float* w, int swap, int flip, const float* bias, float* out,
                      int N, int Cin, int H, int W, int Cout, int OW, int S, int P, float* ws, hipStream_t st,
                      float* stats = nullptr, int* nsplit = nullptr, const InAff* aff = nullptr);

// conv_t2_mfma.hip: stride-2 transposed 5x5 (4-phase): small (C,HS,WS) -> big (O,2HS,2WS), wpacked = (C,25,O)
bool jvae_convt2_ok(int C, int HS, int WS, int O, int HB, int WB, int KH, int KW, int S, int P);
int jvae_convt2(const float* in, const float* wpacked, const float* bias, float* out, int N, int C, int WS, int O,
                hipStream_t st, float* stats = nullptr, int* nsplit = nullptr, const InAff* aff = nullptr);

// conv_smallco.hip: 5x5 stride-1 'same' convolution with <= 4 output channels (vector ALUs)
bool jvae_conv5_smallco_ok(int Cin, int H, int W, int Cout, int KH, int KW, int S, int P);
int jvae_conv5_smallco(const float* in, const float* w, const float* bias, float* out, int N, int Cin, int W, int Cout,
                       hipStream_t st, const InAff* aff = nullptr);
// the data gradient of the mirror layer (Conv2d with <= 4 INPUT channels: the gradient with respect to the input image)
int jvae_conv5_smallco_dgrad(const float* dy, const float* w, float* dx, int N, int Cy, int W, int Cx, hipStream_t st);

// ... and with <= 4 INPUT channels (forward-type operator, any weight role: the first layer's forward, the head's dgrad)
bool jvae_conv5_smallci_ok(int Cin, int H, int W, int Cout, int OW, int S, int P, bool dgrad_role);
int jvae_conv5_smallci(const float* in, const float* w, int swap, int flip, const float* bias, float* out,
                       int N, int Cin, int W, int Cout, float* ws, hipStream_t st, float* stats = nullptr, int* nsplit = nullptr);

// conv_wgrad_mfma.hip (fp32 matrix cores): dW[a][b][tap] = sum Ps[n][a][u][v] Q[n][b][u*S+kh-P][v*S+kw-P]
bool jvae_conv5_wgrad_ok(int Ca, int HS, int WS, int Cb, int HB, int WB, int S, int P);
size_t jvae_conv5_wgrad_ws_floats(int N, int Ca, int Cb, int S, int WS);
int jvae_conv5_wgrad(const float* ps, const float* q, float* dw, int accumulate, int swapflip,
                     int N, int Ca, int WS, int Cb, int S, int P, float* ws, hipStream_t st,
                     const InAff* aff_p = nullptr, const InAff* aff_q = nullptr);

// conv_wgrad_x3.hip: the same operator on the bf16 matrix cores (3-way exact operand split), WS in {8, 16, 32}
bool jvae_conv5_wgrad_x3_ok(int Ca, int HS, int WS, int Cb, int HB, int WB, int S, int P);
size_t jvae_conv5_wgrad_x3_ws_floats(int N, int Ca, int Cb, int S);
int jvae_conv5_wgrad_x3(const float* ps, const float* q, float* dw, int accumulate, int swapflip,
                        int N, int Ca, int WS, int Cb, int S, int P, float* ws, hipStream_t st,
                        const InAff* aff_p = nullptr, const InAff* aff_q = nullptr);

// conv_dispatch.hip
// (x: the layer's input, y: the layer's output) -> big/small-side geometry; false for an invalid one
bool jvae_make_geom(int N, int Cin, int H, int W, int Cout, int KH, int KW, int S, int P, int OP, int transposed,
                    ConvGeom* g, int* OH, int* OW);

enum ConvDir { CONV_FWD = 1, CONV_DGRAD = 2, CONV_WGRAD = 4 };     // the bits of jvae_conv2d_native_b8
enum ConvLayout { CONV_F32, CONV_B8 };
enum ConvKernel {
    CK_NONE,                                  // no kernel: JVAE_ENOTSUP (the bf16 layout has no generic path)
    CK_GENERIC, CK_POINT,                     // unfold + GEMM (conv_generic.hip); the 1x1-input transposed layer as plain GEMMs
    CK_SMALLCO, CK_SMALLCI, CK_FWD5, CK_FWD5_X3, CK_T2, CK_T2_X3, CK_WG5, CK_WG5_X3,     // fp32
    CK_B8, CK_T2_B8, CK_WG_B8, CK_WG_B8X,                                                // bf16
    CK_SMALLCO_DG,                            // fp32, CONV_DGRAD only: the input-image gradient of a <= 4-input-channel 5x5 layer
};
// The per-call facts that change the choice
struct CallFlags {
    bool bias, stats;   // forward: a bias is added / BatchNorm partial sums are wanted (neither: the smallci "dgrad role")
    bool y_f32;         // bf16 forward with an fp32 NCHW output (the 4-phase kernel writes B8 only)
    int aff;            // input affine (InAff): 0 none, 1 BatchNorm (+ReLU), 2 BatchNorm + leaky ReLU (the AFF of the kernels)
};
struct ConvRoute {
    ConvKernel k;
    bool swap;          // forward / dgrad: the input is the SMALL side (weight read [c][o], taps flipped: swap = flip = 1);
                        // wgrad: roles swapped (ps = big side, swapflip = 1)
    int S, P;           // stride / padding of the operator the leaf computes (swap: 1, 4 - P)
    size_t ws;          // workspace bytes the leaf needs (CK_GENERIC chunks by what it is given and checks that itself)
    int splits;         // BatchNorm partial sums per channel the forward writes at most (0: none)
    bool aff_ok;        // the leaf applies the input affine of the call (flags.aff, or a plain one when 0)
};
// Reads the split-bf16 switch on every call (jvae_conv5_x3_enabled): nothing is cached.
ConvRoute jvae_conv_route(const ConvGeom& g, int transposed, ConvDir dir, ConvLayout layout, CallFlags f);
inline int jvae_aff_kind(const InAff* aff) { return !aff ? 0 : (aff->relu == JVAE_ACT_LEAKY ? 2 : 1); }
inline bool jvae_ws_short(const ConvRoute& r, const void* ws, size_t ws_bytes) { return r.ws && (!ws || ws_bytes < r.ws); }
// wgrad operands of a route: ps / q as the leaves take them.  The deferred BatchNorm belongs to the layer input x alone (the
// big side of a convolution, the small side of a transposed one), so at most one of aff_p / aff_q is set: the stride-2 forms of
// conv_wgrad_x3.hip keep a single coefficient set and rely on that.
template <class T>
inline void jvae_wgrad_operands(const ConvRoute& r, int transposed, T* x, T* dy, const InAff* aff, T** ps, T** q,
                                const InAff** aff_p, const InAff** aff_q) {
    const bool p_is_x = r.swap != (transposed != 0);           // ps = big side when swapped, small side otherwise
    *ps = p_is_x ? x : dy;
    *q = p_is_x ? dy : x;
    *aff_p = p_is_x ? aff : nullptr;
    *aff_q = p_is_x ? nullptr : aff;
}

// fp32 workspace of all three directions (never less than the generic path's, which chunks its images below it)
size_t jvae_conv_ws(const ConvGeom& g, int transposed);
// Execute an fp32 route: the forward-type directions (forward, dgrad) and the weight gradient (accumulates onto dw)
int jvae_conv_run_fwd(const ConvRoute& r, const ConvGeom& g, const float* in, const float* w, const float* bias, float* out,
                      float* ws, size_t ws_bytes, hipStream_t st, float* stats = nullptr, int* nsplit = nullptr,
                      const InAff* aff = nullptr);
int jvae_conv_run_wgrad(const ConvRoute& r, const ConvGeom& g, int transposed, const float* x, const float* dy, float* dw,
                        float* ws, size_t ws_bytes, hipStream_t st, const InAff* aff = nullptr);
