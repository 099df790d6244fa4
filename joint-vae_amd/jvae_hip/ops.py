"""Autograd-aware wrappers around the HIP kernels of libjvae_hip.so.

PyTorch is plumbing here (device memory, streams, the autograd tape); every FLOP of the training step is
executed by the hand-written gfx950 kernels.  Every function raises if its tensors are not on the GPU.
"""
import collections
import contextlib
import ctypes
import math
from ctypes import byref, c_int, c_size_t

import numpy as np
import torch

from . import lib as L

RELU, SIGMOID, IDENT, LEAKY = 1, 2, 0, 3          # jvae_act_* kinds (LEAKY: nn.LeakyReLU(), negative slope 0.01)
# the `relu` / `in_relu` argument of the BatchNorm and convolution entry points: 0 none, 1 ReLU, 2 leaky ReLU (jvae_hip.h)
BN_ACT = {IDENT: 0, RELU: 1, LEAKY: 2}
OVERLAP_WGRAD = True          # weight-gradient kernels on a second HIP stream (see _Conv.backward)
ACT_KIND = {'relu': RELU, 'sigmoid': SIGMOID, 'linear': IDENT, 'leaky': LEAKY, None: IDENT}


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _f32(t, what):
    if t.dtype != torch.float32:
        raise L.JvaeHipError(f'{what}: fp32 expected, got {t.dtype}')
    return t


def _grad_slot(param):
    """The tensor a parameter gradient can be accumulated into in place (its existing, dense .grad), or None.

    When the optimiser has flattened the model every .grad is a view of one zeroed flat buffer: the backward
    kernels then add their result straight into it (exactly what autograd's AccumulateGrad would do with one
    more elementwise kernel per parameter) and hand `None` back to autograd."""
    if param is None or not isinstance(param, torch.nn.Parameter):
        return None
    g = param.grad
    if g is None or not g.is_contiguous() or g.dtype != torch.float32 or g.shape != param.shape or not g.is_cuda:
        return None
    return g


def _join_after_backward():
    """When the autograd engine finishes this backward pass, the main stream waits for the side stream, so that
    whoever reads .grad next (optimiser, all-reduce, a test) sees the finished weight gradients.  Queued once per
    side-stream launch (an event wait each: cheap), so no state survives a backward pass that raised."""
    torch.autograd.Variable._execution_engine.queue_callback(L.join_side_stream)


def _close_span_after_backward():
    """The span of constant weights that a train-mode evaluate() / forward() opened (packed weights served from the step's
    cache, lib.pack_cache_begin) ends with the backward pass that needed it: the engine's end-of-backward callback disarms
    the cache, whether or not an optimiser step follows.  Queued by every convolution backward (a host-side flag flip each)."""
    if not L.span_hold:            # odin_scores: its input-gradient passes sit inside one span, which the call itself closes
        torch.autograd.Variable._execution_engine.queue_callback(L.pack_cache_end)


# ------------------------------------------------------------------------------------------- gemm
def gemm(M, N, K, A, sA, B, sB, C, sC, bias=None, bias_mode=0, flags=0, splitk=1, batch=1):
    """Raw strided product on the current stream.  sA = (sAm, sAk, sAb) etc. (elements)."""
    lib = L.load()
    rc = lib.jvae_gemm_f32(M, N, K, batch, L.ptr(A), *sA, L.ptr(B), *sB, L.ptr(C), *sC,
                           L.ptr(bias), bias_mode, flags, splitk, L.stream_ptr())
    L.check(rc, 'jvae_gemm_f32')


def gemm_desc(M, N, K, A, sA, B, sB, C, sC, bias=None, bias_mode=0, flags=0, splitk=1, batch=1):
    """The arguments of gemm() as one record of a grouped launch (gemm_group)."""
    return (M, N, K, batch, A, sA, B, sB, C, sC, bias, bias_mode, flags, splitk)


def _fill_gemm_desc(d, rec, ptr):
    """A gemm_desc record into the L.GemmDesc d; ptr turns an operand into its address."""
    M, N, K, batch, A, sA, B, sB, C, sC, bias, bias_mode, flags, splitk = rec
    d.M, d.N, d.K, d.batch = M, N, K, batch
    d.A, (d.sAm, d.sAk, d.sAb) = ptr(A), sA
    d.B, (d.sBk, d.sBn, d.sBb) = ptr(B), sB
    d.C, (d.sCm, d.sCn, d.sCb) = ptr(C), sC
    d.bias, d.bias_mode, d.flags, d.splitk = ptr(bias), bias_mode, flags, splitk


def gemm_group(descs):
    """Independent products (gemm_desc records, at most 8, outputs that do not overlap) in ONE launch on the current stream.
    Every product runs the kernel, tiles and K slices that gemm() gives it alone: the same bits."""
    lib = L.load()
    arr = (L.GemmDesc * max(len(descs), 1))()
    for d, rec in zip(arr, descs):
        _fill_gemm_desc(d, rec, L.ptr)
    L.check(lib.jvae_gemm_group_f32(arr, len(descs), L.stream_ptr()), 'jvae_gemm_group_f32')


GemmRoute = collections.namedtuple('GemmRoute', 'variant grid slices kchunk vecA vecB lds')


def gemm_route(M, N, K, A, sA, B, sB, C, sC, bias=None, bias_mode=0, flags=0, splitk=1, batch=1, want_splits=0, sCsplit=0):
    """The plan gemm() / a gemm_desc record of gemm_group takes for these arguments, asked from gemm_plan() through the host-only
    query: GemmRoute(variant='X3_AK_BK_D3', grid=(gx, gy, gz), slices, kchunk, vecA, vecB, lds); variant None for an empty
    product.  want_splits > 0: the stored-slices form of jvae_gemm_group_f32.  Nothing is launched and no operand is read: A, B,
    C and bias may be tensors or plain addresses (only their alignment matters).  Not memoised: the plan follows the split-bf16
    switch.  JvaeHipError for arguments the launch entries refuse."""
    lib = L.load()
    addr = lambda t: t if t is None or isinstance(t, int) else t.data_ptr()
    d, r, made = L.GemmDesc(), L.GemmRoute(), c_int(0)
    _fill_gemm_desc(d, gemm_desc(M, N, K, A, sA, B, sB, C, sC, bias, bias_mode, flags, splitk, batch), addr)
    d.want_splits, d.sCsplit = want_splits, sCsplit
    if want_splits > 0:
        d.splits = ctypes.pointer(made)
    L.check(lib.jvae_gemm_route(byref(d), byref(r)), 'jvae_gemm_route')
    name = lib.jvae_gemm_variant_name(r.variant)
    return GemmRoute(name.decode() if name is not None else None, (r.gx, r.gy, r.gz), r.slices, r.kchunk, bool(r.vecA), bool(r.vecB),
                     r.lds)


def splitk_fold_group(jobs):
    """jobs: (part, bias, y, S, MN, N, relu, accumulate) as for jvae_splitk_fold_f32, at most 8, in ONE launch."""
    lib = L.load()
    arr = (L.FoldDesc * max(len(jobs), 1))()
    for d, (part, bias, y, S, MN, N, relu, accumulate) in zip(arr, jobs):
        d.part, d.bias, d.y = L.ptr(part), L.ptr(bias), L.ptr(y)
        d.S, d.MN, d.N, d.relu, d.accumulate = S, MN, N, relu, accumulate
    L.check(lib.jvae_splitk_fold_group_f32(arr, len(jobs), L.stream_ptr()), 'jvae_splitk_fold_group_f32')


def _run_products(descs, folds):
    """The products of one dependency level, then their folds: one launch each when there is more than one."""
    if len(descs) == 1:
        M, N, K, batch, A, sA, B, sB, C, sC, bias, bias_mode, flags, splitk = descs[0]
        gemm(M, N, K, A, sA, B, sB, C, sC, bias=bias, bias_mode=bias_mode, flags=flags, splitk=splitk, batch=batch)
    elif descs:
        gemm_group(descs)
    if len(folds) == 1:
        part, bias, y, S, MN, N, relu, accumulate = folds[0]
        L.check(L.load().jvae_splitk_fold_f32(L.ptr(part), L.ptr(bias), L.ptr(y), S, MN, N, relu, accumulate, L.stream_ptr()),
                'jvae_splitk_fold_f32')
    elif folds:
        splitk_fold_group(folds)


def channel_sum(t, N, C, P, out=None, accumulate=False):
    lib = L.load()
    if out is None:
        out = torch.empty(C, device=t.device, dtype=torch.float32)
    ws = L.workspace(lib.jvae_channel_sum_workspace_bytes(C), t.device)
    L.check(lib.jvae_channel_sum_f32(L.ptr(t), L.ptr(out), N, C, P, int(accumulate), L.ptr(ws), ws.numel(), L.stream_ptr()),
            'channel_sum')
    return out


def _linear_split(R, O, I):
    """K slices for y = x W^T when the (R, O) output alone cannot fill the chip (64x64 tiles, 256 CUs)."""
    tiles = ((R + 63) // 64) * ((O + 63) // 64)
    if tiles >= 128 or I < 512:
        return 1
    for S in (32, 16, 8, 4, 2):
        if tiles * S <= 1024 and I % S == 0 and I // S >= 128:
            return S
    return 1


class _Linear(torch.autograd.Function):
    """y = x W^T + b (+ReLU / sigmoid).  nn.Linear + activation, layers.py:283-296, cvae.py:291-301."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        x2 = _c(_f32(x, 'linear').reshape(-1, x.shape[-1]))
        w_in = w
        w = _c(w)
        O = w.shape[0]
        descs, folds = [], []
        y = _linear_fwd_products(x2, w, b, act, descs, folds)
        _run_products(descs, folds)
        if act in (SIGMOID, LEAKY):           # (ReLU rides in the product's epilogue; these two are a pass of their own, in place)
            L.check(L.load().jvae_act_fwd_f32(L.ptr(y), L.ptr(y), y.numel(), act, L.stream_ptr()), 'act_fwd')
        ctx.save_for_backward(x2, w, y if act != IDENT else None)
        ctx.act = act
        ctx.has_bias = b is not None
        ctx.xshape = x.shape
        ctx.w_ref, ctx.b_ref = w_in, b
        return y.reshape(*x.shape[:-1], O)

    @staticmethod
    def backward(ctx, gy):
        x2, w, y = ctx.saved_tensors
        lib = L.load()
        R, I = x2.shape
        O = w.shape[0]
        gy = _c(gy.reshape(R, O))
        if ctx.act != IDENT:
            g = torch.empty_like(gy)
            L.check(lib.jvae_act_bwd_f32(L.ptr(gy), L.ptr(y), L.ptr(g), gy.numel(), ctx.act, L.stream_ptr()), 'act_bwd')
            gy = g
        descs, folds = [], []
        # the dgrad and the weight-gradient product share gy and nothing else: one launch when both are needed
        gx, gw = _linear_bwd_products(gy, x2, w, ctx.w_ref, ctx.needs_input_grad[0], ctx.needs_input_grad[1], descs, folds)
        _run_products(descs, folds)
        if gx is not None:
            gx = gx.reshape(ctx.xshape)
        gb = _linear_bias_grad(gy, ctx.b_ref) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb, None


def _linear_fwd_products(x2, w, b, act, descs, folds):
    """y = x2 W^T + b as records for _run_products: the product (K slices as the batch of the launch when the (R, O) output
    alone gives too few tiles) and, for the sliced form, the fixed-order fold (+bias, ReLU).  Returns y."""
    R, I = x2.shape
    O = w.shape[0]
    y = torch.empty((R, O), device=x2.device, dtype=torch.float32)
    S = _linear_split(R, O, I)
    if S > 1:
        part = torch.empty((S, R, O), device=x2.device, dtype=torch.float32)
        Ks = I // S
        descs.append(gemm_desc(R, O, Ks, x2, (I, 1, Ks), w, (1, I, Ks), part, (O, 1, R * O), batch=S))
        folds.append((part, b, y, S, R * O, O, int(act == RELU), 0))
    else:
        descs.append(gemm_desc(R, O, I, x2, (I, 1, 0), w, (1, I, 0), y, (O, 1, 0), bias=b, bias_mode=1 if b is not None else 0,
                               flags=2 if act == RELU else 0))
    return y


def _linear_bwd_products(gy, x2, w, w_ref, need_x, need_w, descs, folds):
    """The dgrad and weight-gradient products of one linear layer as records for _run_products.  Returns (gx, gw): gx (R, I) or
    None; gw None when it was not asked for or goes straight into the parameter's gradient slot."""
    R, I = x2.shape
    O = w.shape[0]
    gx = gw = None
    if need_x:
        gx = torch.empty((R, I), device=gy.device, dtype=torch.float32)
        descs.append(gemm_desc(R, I, O, gy, (O, 1, 0), w, (I, 1, 0), gx, (I, 1, 0)))
    if need_w:
        slot = _grad_slot(w_ref)
        gw = slot if slot is not None else torch.zeros((O, I), device=gy.device, dtype=torch.float32)
        S = _linear_split(O, I, R)
        if S > 1:           # few (O, I) tiles: batch rows sliced over the launch's batch dimension, fixed-order fold
            part = torch.empty((S, O, I), device=gy.device, dtype=torch.float32)
            Rs = R // S
            descs.append(gemm_desc(O, I, Rs, gy, (1, O, Rs * O), x2, (I, 1, Rs * I), part, (I, 1, O * I), batch=S))
            folds.append((part, None, gw, S, O * I, I, 0, 1))
        else:
            descs.append(gemm_desc(O, I, R, gy, (1, O, 0), x2, (I, 1, 0), gw, (I, 1, 0), flags=1))      # no atomics: deterministic
        if slot is not None:
            gw = None
    return gx, gw


def _linear_bias_grad(gy, b_ref):
    R, O = gy.shape
    slot = _grad_slot(b_ref)
    if slot is not None:
        channel_sum(gy, R, O, 1, out=slot, accumulate=True)
        return None
    return channel_sum(gy, R, O, 1)


def linear(x, w, b=None, act=IDENT):
    return _Linear.apply(x, w, b, act)


class _LinearPair(torch.autograd.Function):
    """Two linear layers without activation on the same input (the latent heads): (x W0^T + b0, x W1^T + b1).  The two forward
    products are one launch and their folds another; backward runs both dgrads and both weight-gradient products as one launch
    and the two weight folds as another.  Every product and fold is the one _Linear issues: the same bits."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1):
        x2 = _c(_f32(x, 'linear_pair').reshape(-1, x.shape[-1]))
        ws = (_c(w0), _c(w1))
        descs, folds = [], []
        ys = [_linear_fwd_products(x2, w, b, IDENT, descs, folds) for w, b in zip(ws, (b0, b1))]
        _run_products(descs, folds)
        ctx.save_for_backward(x2, *ws)
        ctx.xshape = x.shape
        ctx.refs = ((w0, b0), (w1, b1))
        ctx.set_materialize_grads(False)
        return tuple(y.reshape(*x.shape[:-1], y.shape[1]) for y in ys)

    @staticmethod
    def backward(ctx, g0, g1):
        x2, *ws = ctx.saved_tensors
        R = x2.shape[0]
        descs, folds = [], []
        out = []
        gxs = []
        gys = []
        for h, g in enumerate((g0, g1)):
            if g is None:           # this head's output was not used: no gradient from it, as with two linear() calls
                out += [None, None]
                gys.append(None)
                continue
            gy = _c(g.reshape(R, ws[h].shape[0]))
            gx, gw = _linear_bwd_products(gy, x2, ws[h], ctx.refs[h][0], ctx.needs_input_grad[0], ctx.needs_input_grad[1 + 2 * h],
                                          descs, folds)
            if gx is not None:
                gxs.append(gx)
            out += [gw, None]
            gys.append(gy)
        _run_products(descs, folds)
        for h, gy in enumerate(gys):
            b_ref = ctx.refs[h][1]
            if gy is not None and b_ref is not None and ctx.needs_input_grad[2 + 2 * h]:
                out[1 + 2 * h] = _linear_bias_grad(gy, b_ref)
        gx = None
        if gxs:
            gx = (gxs[0] if len(gxs) == 1 else torch.add(gxs[0], gxs[1])).reshape(ctx.xshape)
        return (gx, *out)


def linear_pair(x, w0, b0, w1, b1):
    """(linear(x, w0, b0), linear(x, w1, b1)) with the independent products of the two layers sharing their launches."""
    if w0 is w1:            # one gradient slot for both heads: their weight-gradient folds would depend on each other
        return linear(x, w0, b0), linear(x, w1, b1)
    return _LinearPair.apply(x, w0, b0, w1, b1)


# ------------------------------------------------------------------------------------------- conv
_GEOM_CACHE = {}          # pure functions of the layer geometry asked through the C ABI (host-side memo: every op asks)


def _geom_query(name, geom):
    key = (name, geom)
    r = _GEOM_CACHE.get(key)
    if r is None:
        _GEOM_CACHE[key] = r = getattr(L.load(), name)(*geom)
    return r


class ConvSpec:
    __slots__ = ('cin', 'cout', 'k', 's', 'p', 'op', 'transposed')

    def __init__(self, cin, cout, k, s, p, op=0, transposed=False):
        self.cin, self.cout, self.k, self.s, self.p, self.op, self.transposed = cin, cout, k, s, p, op, bool(transposed)

    def out_hw(self, H, W):
        key = ('hw', self.k, self.s, self.p, self.op, self.transposed, H, W)
        r = _GEOM_CACHE.get(key)
        if r is None:
            oh, ow = c_int(), c_int()
            rc = L.load().jvae_conv2d_out_shape(H, W, self.k, self.k, self.s, self.p, self.op, int(self.transposed),
                                                byref(oh), byref(ow))
            L.check(rc, 'jvae_conv2d_out_shape')
            _GEOM_CACHE[key] = r = (oh.value, ow.value)
        return r

    def geom(self, N, H, W):
        return (N, self.cin, H, W, self.cout, self.k, self.k, self.s, self.p, self.op, int(self.transposed))


def _conv_ws(geom, device):
    nbytes = _geom_query('jvae_conv2d_workspace_bytes', geom)
    ws = L.workspace(nbytes, device)
    return ws, ws.numel()


def conv_fwd_raw(x, w, b, spec):
    N, _, H, W = x.shape
    oh, ow = spec.out_hw(H, W)
    y = torch.empty((N, spec.cout, oh, ow), device=x.device, dtype=torch.float32)
    geom = spec.geom(N, H, W)
    ws, nb = _conv_ws(geom, x.device)
    rc = L.load().jvae_conv2d_fwd_f32(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), *geom, L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, 'jvae_conv2d_fwd_f32')
    return y


def conv_fwd_stats_raw(x, w, b, spec):
    """-> (y, stats, nsplit): forward + the BatchNorm partial sums of (y - bias) written by the conv epilogue
    (stats is None / nsplit 0 when the kernel selected for this geometry does not produce them)."""
    lib = L.load()
    N, _, H, W = x.shape
    geom = spec.geom(N, H, W)
    cap = _geom_query('jvae_conv2d_stats_splits', geom)
    if cap <= 0:
        return conv_fwd_raw(x, w, b, spec), None, 0
    oh, ow = spec.out_hw(H, W)
    y = torch.empty((N, spec.cout, oh, ow), device=x.device, dtype=torch.float32)
    stats = torch.empty((spec.cout * cap * 2,), device=x.device, dtype=torch.float32)
    ws, nb = _conv_ws(geom, x.device)
    ns = c_int(0)
    rc = lib.jvae_conv2d_fwd_stats_f32(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(stats), byref(ns), *geom,
                                       L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, 'jvae_conv2d_fwd_stats_f32')
    return y, (stats if ns.value > 0 else None), ns.value


def conv_affine_ok(spec, N, H, W):
    """Can this layer apply a deferred BatchNorm(+ReLU) to its input (forward and weight gradient kernels)?"""
    return bool(_geom_query('jvae_conv2d_affine_ok', spec.geom(N, H, W)))


ConvRoute = collections.namedtuple('ConvRoute', 'kernel swap ws splits aff_ok')
ROUTE_DIR = {'fwd': 1, 'dgrad': 2, 'wgrad': 4}
ROUTE_LAYOUT = {'f32': 0, 'b8': 1}


def conv_route(spec, N, H, W, direction, layout='f32', bias=False, stats=False, y_f32=False, aff=0):
    """The kernel the entry points of `layout` run for this call ('fwd' / 'dgrad' / 'wgrad'; aff: 0 none, 1 BatchNorm(+ReLU),
    2 leaky), asked from jvae_conv_route through the host-only query: ConvRoute(kernel='CK_FWD5_X3', swap, ws, splits, aff_ok).
    Not memoised: the route follows the split-bf16 switch.  JvaeHipError for a geometry the entry points refuse."""
    lib = L.load()
    k, sw, ns, ok, ws = c_int(), c_int(), c_int(), c_int(), c_size_t()
    rc = lib.jvae_conv2d_route(ROUTE_DIR[direction], ROUTE_LAYOUT[layout], int(bias), int(stats), int(y_f32), int(aff),
                               *spec.geom(N, H, W), byref(k), byref(sw), byref(ws), byref(ns), byref(ok))
    L.check(rc, 'jvae_conv2d_route')
    return ConvRoute(lib.jvae_conv2d_kernel_name(k.value).decode(), bool(sw.value), ws.value, ns.value, bool(ok.value))


class LaunchProbe:
    """HIP-event pairs around ONE convolution launch inside the running step (bench.py's `roofline`: the dominant kernel timed
    where it runs - same clocks, caches and neighbours as in the step - on the stream it is launched on).  `match(spec, N, H)`
    selects the launch; events are recorded on the current stream, read after the timed region."""

    def __init__(self, match):
        self.match, self.events, self.armed = match, [], False

    def times_ms(self):
        return [a.elapsed_time(b) for a, b in self.events]


FWD_AFF_PROBE = None          # set by bench.py only


def conv_fwd_aff_raw(x, w, b, spec, aff, want_stats):
    """Forward with a = [relu](x*scale[c] + shift[c]) applied to the input while it is staged; aff = (scale, shift, relu).
    -> (y, stats, nsplit) as conv_fwd_stats_raw."""
    lib = L.load()
    N, _, H, W = x.shape
    geom = spec.geom(N, H, W)
    oh, ow = spec.out_hw(H, W)
    y = torch.empty((N, spec.cout, oh, ow), device=x.device, dtype=torch.float32)
    stats, ns = None, c_int(0)
    if want_stats:
        cap = _geom_query('jvae_conv2d_stats_splits', geom)
        if cap > 0:
            stats = torch.empty((spec.cout * cap * 2,), device=x.device, dtype=torch.float32)
    ws, nb = _conv_ws(geom, x.device)
    probe = FWD_AFF_PROBE
    timed = probe is not None and probe.armed and probe.match(spec, N, H)
    if timed:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    rc = lib.jvae_conv2d_fwd_aff_f32(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), L.ptr(stats), byref(ns),
                                     L.ptr(aff[0]), L.ptr(aff[1]), int(aff[2]), *geom, L.ptr(ws), nb, L.stream_ptr())
    if timed:
        ev[1].record()
        probe.events.append(ev)
    L.check(rc, 'jvae_conv2d_fwd_aff_f32')
    return y, (stats if ns.value > 0 else None), ns.value


def conv_dgrad_raw(gy, w, spec, xshape):
    N, _, H, W = xshape
    gx = torch.empty(xshape, device=gy.device, dtype=torch.float32)
    geom = spec.geom(N, H, W)
    ws, nb = _conv_ws(geom, gy.device)
    rc = L.load().jvae_conv2d_dgrad_f32(L.ptr(gy), L.ptr(w), L.ptr(gx), *geom, L.ptr(ws), nb, L.stream_ptr())
    L.check(rc, 'jvae_conv2d_dgrad_f32')
    return gx


def conv_wgrad_raw(x, gy, spec, wshape, want_bias, w_slot=None, b_slot=None, aff=None):
    """-> (gw, gb).  With w_slot / b_slot (existing .grad tensors) the result is ADDED there and None is returned
    for that gradient.  The C entry point takes one accumulate flag: both slots or neither.
    aff = (scale, shift, relu): x is a pre-BatchNorm tensor whose normalisation is applied while it is staged."""
    N, _, H, W = x.shape
    inplace = w_slot is not None and (b_slot is not None or not want_bias)
    gw = w_slot if inplace else torch.empty(wshape, device=x.device, dtype=torch.float32)
    gb = None
    if want_bias:
        gb = b_slot if inplace else torch.empty(spec.cout, device=x.device, dtype=torch.float32)
    geom = spec.geom(N, H, W)
    ws, nb = _conv_ws(geom, x.device)
    if aff is not None:
        rc = L.load().jvae_conv2d_wgrad_aff_f32(L.ptr(x), L.ptr(gy), L.ptr(gw), L.ptr(gb), int(inplace),
                                                L.ptr(aff[0]), L.ptr(aff[1]), int(aff[2]), *geom, L.ptr(ws), nb,
                                                L.stream_ptr())
    else:
        rc = L.load().jvae_conv2d_wgrad_f32(L.ptr(x), L.ptr(gy), L.ptr(gw), L.ptr(gb), int(inplace), *geom, L.ptr(ws), nb,
                                            L.stream_ptr())
    L.check(rc, 'jvae_conv2d_wgrad_f32')
    return (None, None) if inplace else (gw, gb)


# ------------------------------------------------------------------------------------------- layouts
FWD, DGRAD, WGRAD = 1, 2, 4          # directions of a convolution (the bits of jvae_conv2d_native_b8)


class Layout:
    """What the convolution and BatchNorm ops below need to know about one activation layout.  This class is fp32 NCHW
    (F32); ops_b8.B8Layout overrides what differs for the bf16 B8 layout."""
    sfx = '_f32'                     # suffix of the C entry points
    ws_sfx = ''                      # suffix of the BatchNorm workspace query
    acts = BN_ACT                    # activations its kernels apply (in the BatchNorm kernels: the `relu` code)

    def dims(self, x, C):
        """-> (N, C, P); C is the caller's channel count (a B8 tensor cannot tell it)."""
        N, C = x.shape[0], x.shape[1]
        return N, C, x.numel() // max(N * C, 1)

    def coef_width(self, C):
        return C

    def prep(self, x, what):
        return _c(_f32(x, what))

    def to_f32(self, t, C):          # plain conversions between the kernels of one op (no autograd node)
        return t

    def from_f32(self, t):
        return t

    def native(self, spec, N, H, W):
        return FWD | DGRAD | WGRAD

    def affine_ok(self, spec, N, H, W):
        return conv_affine_ok(spec, N, H, W)

    def conv_fwd(self, x, w, b, spec, want_stats, aff, out_f32):
        """-> (y, stats, nsplit).  out_f32 only matters to a layout other than fp32."""
        if aff is not None:
            return conv_fwd_aff_raw(x, w, b, spec, aff, want_stats)
        if want_stats:
            return conv_fwd_stats_raw(x, w, b, spec)
        return conv_fwd_raw(x, w, b, spec), None, 0

    def conv_dgrad(self, gy, w, spec, N, H, W):
        return conv_dgrad_raw(gy, w, spec, (N, spec.cin, H, W))

    def conv_wgrad(self, *args):
        return conv_wgrad_raw(*args)

    def bn(self, name, *args, ws=None):
        """Call the BatchNorm entry point `name` of this layout on the current stream."""
        name += self.sfx
        extra = () if ws is None else (L.ptr(ws), ws.numel())
        L.check(getattr(L.load(), name)(*args, *extra, L.stream_ptr()), name)

    def bn_workspace(self, C, device):
        return L.workspace(getattr(L.load(), 'jvae_bn_workspace_bytes' + self.ws_sfx)(C), device)

    def bn_fwd(self, *args, ext, ws):
        """ext = (stats, nsplit, pivot) or nulls.  jvae_bn_fwd_f32 is jvae_bn_fwd_ext_f32 without the sums."""
        if ext[0] is None:
            self.bn('jvae_bn_fwd', *args, ws=ws)
        else:
            self.bn('jvae_bn_fwd_ext', *args, *ext, ws=ws)

    def coef_args(self, coef):
        return L.ptr(coef[0]), L.ptr(coef[1])          # jvae_bn_finalize_f32: separate scale and shift rows

    def bn_bwd_sync(self, *args, ws):
        self.bn('jvae_bn_bwd_sync', *args)              # jvae_bn_bwd_sync_f32 takes no workspace


F32 = Layout()


def layout_of(t):
    return _b8.B8 if _b8.is_b8(t) else F32


class _Conv(torch.autograd.Function):
    """nn.Conv2d / nn.ConvTranspose2d (conv.py:186-196) in the layout of its input.  A direction without a native kernel in
    that layout runs on the fp32 kernels between two conversions.  out_f32: a B8 input gives an fp32 NCHW output."""

    @staticmethod
    def forward(ctx, x, w, b, spec, dead_bias, stats_out, aff, out_f32):
        lay = layout_of(x)
        x = lay.prep(x, 'conv')
        if not L.span_depth:               # a convolution called outside forward() / evaluate() (net.imager(z), a raw module call):
            L.pack_cache_end()             # nobody vouches for the weights now - an armed cache (train-mode evaluate() without its
        ctx.w_ref, ctx.b_ref = w, b        # backward yet) may predate a change through .data; pack per call
        w = _c(w)
        native = lay.native(spec, x.shape[0], x.shape[2], x.shape[3])
        if aff is not None and (native & (FWD | WGRAD)) != FWD | WGRAD:
            raise L.JvaeHipError('a deferred BatchNorm needs native forward and weight-gradient kernels (conv_affine_ok)')
        want_stats = stats_out is not None           # the caller is a train-mode BatchNorm: let the conv epilogue do its sums
        if native & FWD:                   # with aff, x is a pre-BatchNorm tensor: normalise (+ReLU) while staging it
            y, st, ns = lay.conv_fwd(x, w, b, spec, want_stats, aff, out_f32)
        else:
            y, st, ns = F32.conv_fwd(lay.to_f32(x, spec.cin), w, b, spec, want_stats, None, False)
            y = y if out_f32 else lay.from_f32(y)
        if want_stats:
            stats_out['stats'], stats_out['nsplit'], stats_out['pivot'] = st, ns, b
        ctx.save_for_backward(x, w)
        ctx.lay, ctx.native, ctx.spec, ctx.out_f32, ctx.aff = lay, native, spec, out_f32, aff
        ctx.has_bias = b is not None
        ctx.dead_bias = dead_bias
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        lay, spec = ctx.lay, ctx.spec
        N, H, W = x.shape[0], x.shape[2], x.shape[3]
        gys = {F32 if ctx.out_f32 else lay: _c(gy)}      # gy in each layout it is needed in: converted once per layout

        def gy_in(want):
            if want not in gys:
                have, g = next(iter(gys.items()))
                gys[want] = want.from_f32(g) if have is F32 else have.to_f32(g, spec.cout)
            return gys[want]
        gx = gw = gb = None
        _close_span_after_backward()
        want_b = ctx.has_bias and ctx.needs_input_grad[2] and not ctx.dead_bias
        wgrad = ctx.needs_input_grad[1] or want_b
        on_side = False
        if wgrad:
            w_slot = _grad_slot(ctx.w_ref)
            b_slot = _grad_slot(ctx.b_ref) if want_b else None
            # the first layer of the model (its input needs no gradient) is the END of the backward chain: its weight
            # gradient stays on the main stream, where it runs beside the side stream's last kernels instead of behind them
            on_side = (OVERLAP_WGRAD and ctx.needs_input_grad[0] and w_slot is not None
                       and (b_slot is not None or not want_b))
        if ctx.needs_input_grad[0]:
            dl = lay if ctx.native & DGRAD else F32
            gyd = gy_in(dl)
        if on_side:
            # the weight gradient needs gy and x, not this layer's dgrad: the side stream forks off BEFORE the dgrad is
            # queued.  In a captured graph the dgrad is then the first successor of gy's producer and stays on the
            # launch queue (the runtime moves later successors to other queues: a 10 us hand-over per hop of the chain)
            side = L.side_stream(x.device)
            side.wait_stream(torch.cuda.current_stream(x.device))
        if ctx.needs_input_grad[0]:
            gx = dl.conv_dgrad(gyd, w, spec, N, H, W)
            gx = gx if dl is lay else lay.from_f32(gx)
        if wgrad:
            # on the side stream: in-place into the flat gradient buffer, nothing downstream of this node consumes the
            # result before the optimiser, so the kernel (and the conversions only it needs) overlaps the rest of backward
            with torch.cuda.stream(side) if on_side else contextlib.nullcontext():
                wl = lay if ctx.native & WGRAD else F32
                xw = x if wl is lay else lay.to_f32(x, spec.cin)
                gw, gb = wl.conv_wgrad(xw, gy_in(wl), spec, w.shape, want_b, w_slot, b_slot, ctx.aff)
            if on_side:
                for t in (x, xw, *gys.values(), *(ctx.aff[:2] if ctx.aff is not None else ())):
                    t.record_stream(side)
                _join_after_backward()
        if ctx.dead_bias and ctx.has_bias and ctx.needs_input_grad[2] and _grad_slot(ctx.b_ref) is None:
            gb = torch.zeros_like(ctx.b_ref)          # exact value; makes the bias a regular optimiser citizen
        return gx, gw, gb, None, None, None, None, None


def conv2d(x, w, b, spec, dead_bias=False, stats_out=None, aff=None, out_f32=False):
    """dead_bias: the bias feeds a train-mode BatchNorm, which removes the channel mean: its true gradient is
    exactly zero (what autograd would produce is rounding noise), so the channel reduction is skipped.
    aff: (scale, shift, relu) of a deferred BatchNorm on x (batchnorm_defer).  out_f32: see _Conv."""
    return _Conv.apply(x, w, b, spec, dead_bias, stats_out, aff, out_f32)


# ------------------------------------------------------------------------------------------- batch norm
def _ext_args(ext, training):
    """(stats, nsplit, pivot) of the producing convolution's BatchNorm sums (conv2d(..., stats_out=ext)), or nulls."""
    if ext is None or ext.get('stats') is None or not training:
        return None, 0, None
    return L.ptr(ext['stats']), int(ext['nsplit']), L.ptr(ext.get('pivot'))


def _bn_save(ctx, lay, training, relu, dims, x, gamma, beta, mean, invstd, rm, rv, eps):
    ctx.lay = lay
    ctx.relu, ctx.dims = relu, dims
    ctx.eval_eps = None if training else float(eps)
    if training:
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.g_ref, ctx.b_ref = gamma, beta
    else:                      # running statistics are constants: backward is one elementwise pass (jvae_bn_eval_bwd_f32)
        ctx.save_for_backward(x, gamma, beta, rm, rv)


def _bn_eval_backward(ctx, gy):
    """Input gradient of an eval-mode BatchNorm (+activation), materialised or deferred: gy * gamma * rsqrt(running_var + eps)
    * act'(y).  No parameter gradients (the ODIN gradient pass wants d/dx only)."""
    if ctx.lay is not F32:
        raise NotImplementedError('backward through an eval-mode BatchNorm is built for the fp32 layout only')
    x, gamma, beta, rm, rv = ctx.saved_tensors
    N, C, P = ctx.dims
    gy = _c(gy)
    gx = torch.empty_like(x)
    L.check(L.load().jvae_bn_eval_bwd_f32(L.ptr(gy), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(gx),
                                          N, C, P, ctx.eval_eps, int(ctx.relu), L.stream_ptr()), 'jvae_bn_eval_bwd_f32')
    return gx, None, None, None, None, None, None, None, None, None, None, None


def _bn_param_grads(ctx, C, device):
    """-> (ggamma, gbeta, inplace): the existing .grad slots when both exist, else new tensors."""
    sg, sb = _grad_slot(ctx.g_ref), _grad_slot(ctx.b_ref)
    if sg is not None and sb is not None:
        return sg, sb, True
    return torch.empty(C, device=device, dtype=torch.float32), torch.empty(C, device=device, dtype=torch.float32), False


class _BatchNormAct(torch.autograd.Function):
    """nn.BatchNorm2d (train or eval) + optional ReLU / leaky ReLU (conv.py:214-220) in the layout of its input; statistics
    and parameters fp32."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, training, relu, momentum, eps, ext, C):
        lay = layout_of(x)
        x = lay.prep(x, 'batchnorm')
        N, C, P = lay.dims(x, C)
        y = torch.empty_like(x)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        invstd = torch.empty(C, device=x.device, dtype=torch.float32)
        lay.bn_fwd(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(nbt), L.ptr(y), L.ptr(mean), L.ptr(invstd),
                   N, C, P, momentum, eps, int(training), int(relu), ext=_ext_args(ext, training),
                   ws=lay.bn_workspace(C, x.device))
        _bn_save(ctx, lay, training, relu, (N, C, P), x, gamma, beta, mean, invstd, rm, rv, eps)
        return y

    @staticmethod
    def backward(ctx, gy):
        if ctx.eval_eps is not None:
            return _bn_eval_backward(ctx, gy)
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        N, C, P = ctx.dims
        gy = _c(gy)
        gx = torch.empty_like(x)
        gg, gb, inplace = _bn_param_grads(ctx, C, x.device)
        ctx.lay.bn('jvae_bn_bwd', L.ptr(gy), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(invstd), L.ptr(gx),
                   L.ptr(gg), L.ptr(gb), int(inplace), N, C, P, int(ctx.relu), ws=ctx.lay.bn_workspace(C, x.device))
        if inplace:
            gg = gb = None
        return gx, gg, gb, None, None, None, None, None, None, None, None, None


def batchnorm_act(x, gamma, beta, running_mean, running_var, num_batches_tracked, training, relu,
                  momentum=0.1, eps=1e-5, ext=None, C=None):
    """ext: {'stats', 'nsplit', 'pivot'} filled by conv2d(..., stats_out=ext) for the tensor x.
    C: the channel count (needed for a B8 tensor)."""
    return _BatchNormAct.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, training, relu,
                               momentum, eps, ext, C)


class _BatchNormDefer(torch.autograd.Function):
    """nn.BatchNorm2d (train or eval) + optional ReLU whose arithmetic is deferred into the next convolution: forward
    only produces the statistics and the per-channel (scale, shift); the returned activation IS the input tensor (the
    consumer applies fmaf(x, scale, shift) [+ReLU] while staging it).  Backward is the ordinary BatchNorm backward on the
    gradient the consumer's dgrad returns (which is w.r.t. the normalised activation)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, training, relu, momentum, eps, ext, C):
        lay = layout_of(x)
        x = lay.prep(x, 'batchnorm')
        N, C, P = lay.dims(x, C)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        invstd = torch.empty(C, device=x.device, dtype=torch.float32)
        coef = torch.empty((2, lay.coef_width(C)), device=x.device, dtype=torch.float32)
        lay.bn('jvae_bn_finalize', L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(nbt), L.ptr(mean),
               L.ptr(invstd), *lay.coef_args(coef), N, C, P, momentum, eps, int(training), *_ext_args(ext, training),
               ws=lay.bn_workspace(C, x.device))
        _bn_save(ctx, lay, training, relu, (N, C, P), x, gamma, beta, mean, invstd, rm, rv, eps)
        ctx.mark_non_differentiable(coef)
        ctx.set_materialize_grads(False)        # no zero-fill launch for the (never used) gradient of `coef`
        return x.view_as(x), coef

    @staticmethod
    def backward(ctx, gy, _gcoef):
        return _BatchNormAct.backward(ctx, gy)


def batchnorm_defer(x, gamma, beta, running_mean, running_var, num_batches_tracked, training, relu,
                    momentum=0.1, eps=1e-5, ext=None, C=None):
    """-> (x_alias, (scale, shift, relu)): hand both to conv2d(..., aff=...) of a layer whose layout's conv_affine_ok()
    holds."""
    xa, coef = _BatchNormDefer.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, training, relu,
                                     momentum, eps, ext, C)
    return xa, (coef[0], coef[1], relu)


class _SyncBatchNormAct(torch.autograd.Function):
    """Train-mode BatchNorm2d (+ReLU) whose statistics span all data-parallel ranks (what the single-process reference
    computes on the whole global batch): two (C,2) fp32 all-reduces per layer, one in forward, one in backward."""

    @staticmethod
    def forward(ctx, x, gamma, beta, rm, rv, nbt, relu, momentum, eps, world, group, C):
        import torch.distributed as dist
        lay = layout_of(x)
        x = lay.prep(x, 'sync batchnorm')
        N, C, P = lay.dims(x, C)
        ws = lay.bn_workspace(C, x.device)
        pivot = rm.detach().clone()                       # identical on every rank; rm itself is updated by the kernel
        sums = torch.empty((C, 2), device=x.device, dtype=torch.float32)
        lay.bn('jvae_bn_sums', L.ptr(x), L.ptr(pivot), L.ptr(sums), N, C, P, ws=ws)
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=group)
        y = torch.empty_like(x)
        mean = torch.empty(C, device=x.device, dtype=torch.float32)
        invstd = torch.empty(C, device=x.device, dtype=torch.float32)
        lay.bn('jvae_bn_fwd_sync', L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(rm), L.ptr(rv), L.ptr(nbt), L.ptr(y),
               L.ptr(mean), L.ptr(invstd), N, C, P, momentum, eps, int(relu), L.ptr(sums), L.ptr(pivot), int(world), ws=ws)
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        ctx.lay, ctx.cfg = lay, (N, C, P, relu, int(world), group)
        ctx.g_ref, ctx.b_ref = gamma, beta
        return y

    @staticmethod
    def backward(ctx, gy):
        import torch.distributed as dist
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        N, C, P, relu, world, group = ctx.cfg
        lay = ctx.lay
        gy = _c(gy)
        ws = lay.bn_workspace(C, x.device)
        local = torch.empty((C, 2), device=x.device, dtype=torch.float32)
        lay.bn('jvae_bn_bwd_sums', L.ptr(gy), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(invstd), L.ptr(local),
               N, C, P, int(relu), ws=ws)
        glob = local.clone()
        dist.all_reduce(glob, op=dist.ReduceOp.SUM, group=group)
        gx = torch.empty_like(x)
        gg, gb, inplace = _bn_param_grads(ctx, C, x.device)
        lay.bn_bwd_sync(L.ptr(gy), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(invstd), L.ptr(local),
                        L.ptr(glob), world, L.ptr(gx), L.ptr(gg), L.ptr(gb), int(inplace), N, C, P, int(relu), ws=ws)
        if inplace:
            gg = gb = None
        return gx, gg, gb, None, None, None, None, None, None, None, None, None


def sync_batchnorm_act(x, gamma, beta, running_mean, running_var, num_batches_tracked, relu, momentum, eps, world, group=None,
                       C=None):
    return _SyncBatchNormAct.apply(x, gamma, beta, running_mean, running_var, num_batches_tracked, relu, momentum, eps,
                                   world, group, C)


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        x = _c(_f32(x, 'act'))
        y = torch.empty_like(x)
        L.check(L.load().jvae_act_fwd_f32(L.ptr(x), L.ptr(y), x.numel(), kind, L.stream_ptr()), 'act_fwd')
        ctx.save_for_backward(y)
        ctx.kind = kind
        return y

    @staticmethod
    def backward(ctx, gy):
        y, = ctx.saved_tensors
        gy = _c(gy)
        gx = torch.empty_like(gy)
        L.check(L.load().jvae_act_bwd_f32(L.ptr(gy), L.ptr(y), L.ptr(gx), gy.numel(), ctx.kind, L.stream_ptr()), 'act_bwd')
        return gx, None


def act(x, kind):
    if kind == IDENT:
        if not x.is_cuda:
            raise L.JvaeHipError('jvae_hip ops need tensors resident on the GPU (no CPU fallback)')
        return x
    return _Act.apply(x, kind)


# ------------------------------------------------------------------------------------------- dropout
class _Dropout(torch.autograd.Function):
    """nn.Dropout(p) in train mode (layers.py:287-288): counter-based mask, regenerated in backward from the seed.
    `seed`: a Python int, or a 1-element int64 DEVICE tensor (graph-capturable: no host value enters the launch)."""

    @staticmethod
    def forward(ctx, x, p, seed):
        x = _c(_f32(x, 'dropout'))
        y = torch.empty_like(x)
        if torch.is_tensor(seed):
            L.check(L.load().jvae_dropout_dev_f32(L.ptr(x), L.ptr(y), x.numel(), float(p), L.ptr(seed), 0, L.stream_ptr()),
                    'dropout')
        else:
            seed = int(seed)
            L.check(L.load().jvae_dropout_f32(L.ptr(x), L.ptr(y), x.numel(), float(p), seed, L.stream_ptr()), 'dropout')
        ctx.cfg = (float(p), seed)
        return y

    @staticmethod
    def backward(ctx, gy):
        p, seed = ctx.cfg
        gy = _c(gy)
        gx = torch.empty_like(gy)
        if torch.is_tensor(seed):
            L.check(L.load().jvae_dropout_dev_f32(L.ptr(gy), L.ptr(gx), gy.numel(), p, L.ptr(seed), 0, L.stream_ptr()),
                    'dropout_bwd')
        else:
            L.check(L.load().jvae_dropout_f32(L.ptr(gy), L.ptr(gx), gy.numel(), p, seed, L.stream_ptr()), 'dropout_bwd')
        return gx, None, None


def dropout(x, p, seed):
    return _Dropout.apply(x, p, seed)


# ------------------------------------------------------------------------------- pooling / up-sampling
POOL_MAX, POOL_AVG = 0, 1


class _Pool2d(torch.autograd.Function):
    """nn.MaxPool2d / nn.AvgPool2d of the layer DSL (tokens M / A; reference module/vae_layers/conv.py:201-206)."""

    @staticmethod
    def forward(ctx, x, K, S, P, mode):
        lib = L.load()
        x = _c(_f32(x, 'pool2d'))
        N, C, H, W = x.shape
        oh, ow = c_int(0), c_int(0)
        L.check(lib.jvae_pool2d_out_shape(H, W, K, S, P, byref(oh), byref(ow)), 'pool2d_out_shape')
        y = torch.empty((N, C, oh.value, ow.value), device=x.device, dtype=torch.float32)
        idx = torch.empty((N, C, oh.value, ow.value), device=x.device, dtype=torch.int32) if mode == POOL_MAX else None
        L.check(lib.jvae_pool2d_fwd_f32(L.ptr(x), L.ptr(y), L.ptr(idx), N * C, H, W, K, S, P, mode, L.stream_ptr()), 'pool2d_fwd')
        ctx.save_for_backward(idx)
        ctx.cfg = (N, C, H, W, K, S, P, mode)
        return y

    @staticmethod
    def backward(ctx, gy):
        idx, = ctx.saved_tensors
        N, C, H, W, K, S, P, mode = ctx.cfg
        gy = _c(gy)
        gx = torch.empty((N, C, H, W), device=gy.device, dtype=torch.float32)
        L.check(L.load().jvae_pool2d_bwd_f32(L.ptr(gy), L.ptr(idx), L.ptr(gx), N * C, H, W, K, S, P, mode, L.stream_ptr()),
                'pool2d_bwd')
        return gx, None, None, None, None


def pool2d(x, kernel_size, stride=None, padding=0, mode=POOL_MAX):
    return _Pool2d.apply(x, int(kernel_size), int(stride or kernel_size), int(padding), mode)


class _UpsampleNearest(torch.autograd.Function):
    """nn.UpsamplingNearest2d(scale_factor=int) (token U; reference module/vae_layers/conv.py:208-212)."""

    @staticmethod
    def forward(ctx, x, scale):
        x = _c(_f32(x, 'upsample_nearest'))
        N, C, H, W = x.shape
        y = torch.empty((N, C, H * scale, W * scale), device=x.device, dtype=torch.float32)
        L.check(L.load().jvae_upsample_nearest_fwd_f32(L.ptr(x), L.ptr(y), N * C, H, W, scale, L.stream_ptr()), 'upsample_fwd')
        ctx.cfg = (N, C, H, W, scale)
        return y

    @staticmethod
    def backward(ctx, gy):
        N, C, H, W, scale = ctx.cfg
        gy = _c(gy)
        gx = torch.empty((N, C, H, W), device=gy.device, dtype=torch.float32)
        L.check(L.load().jvae_upsample_nearest_bwd_f32(L.ptr(gy), L.ptr(gx), N * C, H, W, scale, L.stream_ptr()), 'upsample_bwd')
        return gx, None


def upsample_nearest(x, scale):
    if int(scale) != scale or scale < 1:
        raise L.JvaeHipError('nearest up-sampling is built for integer scale factors')
    return _UpsampleNearest.apply(x, int(scale))


# ------------------------------------------------------------------------------------------- latent
PRIOR_KIND = {'gaussian': 0, 'tilted': 1, 'uniform': 2}
VAR_KIND = {'scalar': 0, 'diag': 1, 'full': 2}


def _device_scalar(t, what):
    if not t.is_cuda or t.dtype != torch.float32 or t.numel() != 1 or t.requires_grad:
        raise L.JvaeHipError(what + ' as a tensor must be ONE fp32 value on the GPU without gradient')
    return t.detach()


class _Latent(torch.autograd.Function):
    """clip + reparameterise + KL terms; see csrc/latent.hip for the reference anchors."""

    @staticmethod
    def forward(ctx, mu, lv_raw, eps, y, means, T, cfg):
        lib = L.load()
        mu = _c(_f32(mu, 'latent'))
        lv_raw = _c(lv_raw)
        eps = _c(eps)
        means = _c(means)
        T = _c(T)
        y = _c(y)
        if y.dtype != torch.int64:
            raise L.JvaeHipError('class labels must be int64')
        N, K = mu.shape
        Ls = eps.shape[0] - 1
        C = means.shape[0]
        dev = mu.device
        dict_ = torch.empty(K + 1, device=dev, dtype=torch.float32)
        L.check(lib.jvae_dict_stats_f32(L.ptr(means), L.ptr(dict_), C, K, L.stream_ptr()), 'dict_stats')
        lv = torch.empty_like(mu)
        z = torch.empty((Ls + 1, N, K), device=dev, dtype=torch.float32)
        kl, zd, vkl, dzd = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(4))
        forced = cfg.get('forced_lv')
        args = (N, K, Ls, C, cfg['prior'], cfg['var_dim'], cfg['tau'], cfg['alpha'], cfg['w'], int(cfg['sampled']),
                int(forced is not None))
        w_dev = cfg.get('w_dev')             # the weight as a device scalar (captured step): the *_wdev entry points
        if w_dev is None:
            rc = lib.jvae_latent_fwd_f32(L.ptr(mu), L.ptr(lv_raw), L.ptr(eps), L.ptr(y), L.ptr(means), L.ptr(T), L.ptr(dict_),
                                         L.ptr(lv), L.ptr(z), L.ptr(kl), L.ptr(zd), L.ptr(vkl), L.ptr(dzd),
                                         *args, float(forced or 0.), L.stream_ptr())
        else:
            rc = lib.jvae_latent_fwd_wdev_f32(L.ptr(mu), L.ptr(lv_raw), L.ptr(eps), L.ptr(y), L.ptr(means), L.ptr(T),
                                              L.ptr(dict_), L.ptr(lv), L.ptr(z), L.ptr(kl), L.ptr(zd), L.ptr(vkl), L.ptr(dzd),
                                              *args, float(forced or 0.), L.ptr(w_dev), L.stream_ptr())
        L.check(rc, 'jvae_latent_fwd_f32')
        ctx.save_for_backward(mu, lv_raw, lv, eps, y, means, T)
        ctx.args = args
        ctx.w_dev = w_dev
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(dzd)
        return lv, z, kl, zd, vkl, dzd

    @staticmethod
    def backward(ctx, g_lv, g_z, g_kl, g_zd, g_vkl, _g_dzd):
        mu, lv_raw, lv, eps, y, means, T = ctx.saved_tensors
        lib = L.load()
        N, K, Ls, C, prior, var_dim = ctx.args[:6]
        dev = mu.device
        gmu = torch.empty_like(mu)
        glv = torch.empty_like(mu)
        need_means = ctx.needs_input_grad[4]
        need_T = ctx.needs_input_grad[5] and var_dim != 0
        gmeans = torch.zeros_like(means) if need_means else None
        gT = torch.zeros_like(T) if need_T else None
        nb = 16 * N + 8 * N * mu.shape[-1]
        ws = L.workspace(nb, dev)

        def opt(t):
            return None if t is None else _c(t)
        ptrs = (L.ptr(mu), L.ptr(lv_raw), L.ptr(lv), L.ptr(eps), L.ptr(y), L.ptr(means), L.ptr(T),
                L.ptr(opt(g_z)), L.ptr(opt(g_kl)), L.ptr(opt(g_zd)), L.ptr(opt(g_vkl)), None, L.ptr(opt(g_lv)),
                L.ptr(gmu), L.ptr(glv), L.ptr(gmeans), L.ptr(gT))
        if ctx.w_dev is None:
            rc = lib.jvae_latent_bwd_f32(*ptrs, *ctx.args, L.ptr(ws), ws.numel(), L.stream_ptr())
        else:
            rc = lib.jvae_latent_bwd_wdev_f32(*ptrs, *ctx.args, L.ptr(ctx.w_dev), L.ptr(ws), ws.numel(), L.stream_ptr())
        L.check(rc, 'jvae_latent_bwd_f32')
        return gmu, glv, None, None, gmeans, gT, None


def latent(mu, lv_raw, eps, y, means, T, *, prior='gaussian', var_dim='scalar', tau=0., alpha=0., w=1.,
           sampled=True, forced_lv=None):
    """-> (log_var (N,K), z (L+1,N,K), kl, zdist, var_kl, dzdist (N,)).  `w`: a float, or a 1-element fp32 DEVICE tensor that
    the kernels read at run time (a captured step whose warm-up weight changes between replays; bit-identical to the float)."""
    w_dev = None
    if torch.is_tensor(w):
        w_dev, w = _device_scalar(w, 'w'), 1.
    cfg = dict(prior=PRIOR_KIND[prior], var_dim=VAR_KIND[var_dim], tau=float(tau), alpha=float(alpha), w=float(w),
               sampled=bool(sampled), forced_lv=forced_lv, w_dev=w_dev)
    return _Latent.apply(mu, lv_raw, eps, y, means, T, cfg)


class _LatentMixed(torch.autograd.Function):
    """`_Latent` over one batch measured against two frozen priors: rows [0, split) against A, the rest against B."""

    @staticmethod
    def forward(ctx, mu, lv_raw, eps, y, means_a, T_a, means_b, T_b, cfg):
        lib = L.load()
        mu = _c(_f32(mu, 'latent_mixed'))
        lv_raw, eps, y = _c(lv_raw), _c(eps), _c(y)
        means_a, T_a, means_b, T_b = _c(means_a), _c(T_a), _c(means_b), _c(T_b)
        if y.dtype != torch.int64:
            raise L.JvaeHipError('class labels must be int64')
        N, K = mu.shape
        Ls = eps.shape[0] - 1
        dev = mu.device
        dict_ = torch.empty(K + 1, device=dev, dtype=torch.float32)
        L.check(lib.jvae_dict_stats_f32(L.ptr(means_a), L.ptr(dict_), means_a.shape[0], K, L.stream_ptr()), 'dict_stats')
        lv = torch.empty_like(mu)
        z = torch.empty((Ls + 1, N, K), device=dev, dtype=torch.float32)
        kl, zd, vkl, dzd = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(4))
        forced = cfg.get('forced_lv')
        args = (N, K, Ls, cfg['split'], means_a.shape[0], *cfg['a'], means_b.shape[0], *cfg['b'], cfg['w'], int(cfg['sampled']),
                int(forced is not None))
        rc = lib.jvae_latent_mixed_fwd_f32(L.ptr(mu), L.ptr(lv_raw), L.ptr(eps), L.ptr(y), L.ptr(means_a), L.ptr(T_a),
                                           L.ptr(dict_), L.ptr(means_b), L.ptr(T_b), L.ptr(lv), L.ptr(z), L.ptr(kl), L.ptr(zd),
                                           L.ptr(vkl), L.ptr(dzd), *args, float(forced or 0.), L.stream_ptr())
        L.check(rc, 'jvae_latent_mixed_fwd_f32')
        ctx.save_for_backward(mu, lv_raw, lv, eps, y, means_a, T_a, means_b, T_b)
        ctx.args = args
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(dzd)
        return lv, z, kl, zd, vkl, dzd

    @staticmethod
    def backward(ctx, g_lv, g_z, g_kl, g_zd, g_vkl, _g_dzd):
        mu, lv_raw, lv, eps, y, means_a, T_a, means_b, T_b = ctx.saved_tensors
        lib = L.load()
        gmu = torch.empty_like(mu)
        glv = torch.empty_like(mu)
        # both priors are frozen: a prior that asks for its gradient is handed to the kernel's own refusal (JVAE_EINVAL)
        gmeans = torch.zeros_like(means_a) if ctx.needs_input_grad[4] or ctx.needs_input_grad[6] else None
        gT = torch.zeros_like(T_a) if ctx.needs_input_grad[5] or ctx.needs_input_grad[7] else None

        def opt(t):
            return None if t is None else _c(t)
        rc = lib.jvae_latent_mixed_bwd_f32(L.ptr(mu), L.ptr(lv_raw), L.ptr(lv), L.ptr(eps), L.ptr(y), L.ptr(means_a), L.ptr(T_a),
                                           L.ptr(means_b), L.ptr(T_b), L.ptr(opt(g_z)), L.ptr(opt(g_kl)), L.ptr(opt(g_zd)),
                                           L.ptr(opt(g_vkl)), None, L.ptr(opt(g_lv)), L.ptr(gmu), L.ptr(glv), L.ptr(gmeans),
                                           L.ptr(gT), *ctx.args, None, 0, L.stream_ptr())
        L.check(rc, 'jvae_latent_mixed_bwd_f32')
        return gmu, glv, None, None, None, None, None, None, None


def latent_prior(means, T, *, prior='gaussian', var_dim='scalar', tau=0., alpha=0.):
    """One prior of `latent_mixed`: means (C, K), the whitening factor T in the layout of `var_dim`, and its kind."""
    return dict(means=means, T=T, kind=(PRIOR_KIND[prior], VAR_KIND[var_dim], float(tau), float(alpha)))


def latent_mixed(mu, lv_raw, eps, y, prior_a, prior_b, split, *, w=1., sampled=True, forced_lv=None):
    """`latent` for a batch whose rows [0, split) are measured against `prior_a` and whose rows [split, N) against `prior_b`
    (two `latent_prior` descriptions), in ONE launch; every sample's values are the single-prior kernel's, bit for bit.  The
    dictionary term belongs to the A part: dzdist is 0 from `split` on.  Both priors are frozen: the backward gives the
    gradients of mu and lv_raw only and raises if a prior's tensors require one.  Labels given on the HOST are checked against
    [0, C_A) resp. [0, C_B) here (JvaeHipError, the kernel's "invalid argument"); labels on the device are checked by the
    kernel, which never indexes with a bad one: that sample's outputs are NaN."""
    N, split = mu.shape[0], int(split)
    if not 0 <= split <= N:
        raise L.JvaeHipError(f'latent_mixed: split {split} outside [0, {N}]')
    if torch.is_tensor(w):
        raise L.JvaeHipError('latent_mixed: the warm-up weight is a host value here')
    if not y.is_cuda:
        C = torch.full((N,), prior_b['means'].shape[0], dtype=torch.int64)
        C[:split] = prior_a['means'].shape[0]
        if y.dtype != torch.int64 or tuple(y.shape) != (N,) or bool(((y < 0) | (y >= C)).any()):
            L.check(-1, 'latent_mixed: a label outside the classes of its prior')
        y = y.to(mu.device)
    cfg = dict(split=split, a=prior_a['kind'], b=prior_b['kind'], w=float(w), sampled=bool(sampled), forced_lv=forced_lv)
    return _LatentMixed.apply(mu, lv_raw, eps, y, prior_a['means'], prior_a['T'], prior_b['means'], prior_b['T'], cfg)


def _refine_operand(t, shape, what):
    """A tensor the refinement kernel reads or writes IN PLACE: fp32, on the GPU, contiguous (no copy can stand in), no graph."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.requires_grad \
            or tuple(t.shape) != tuple(shape):
        raise L.JvaeHipError(f'latent_refine: {what} must be a contiguous fp32 GPU tensor of shape {tuple(shape)} without '
                             'gradient (the kernel works in place)')
    return t


def latent_refine_state(mu, forced=False):
    """Zero Adam state of `latent_refine` for the posterior `mu` (N, K): (m_mu, v_mu, m_lv, v_lv); no lv pair when forced."""
    z = torch.zeros((4 - 2 * bool(forced),) + tuple(mu.shape), device=mu.device, dtype=torch.float32)
    return tuple(z) + (None, None) * bool(forced)


def latent_refine(mu, lv_raw, lv, y, means, T, *, eps_cur=None, dz=None, state=None, step=0, lr=0., eps_next=None,
                  prior='gaussian', var_dim='scalar', tau=0., alpha=0., sampled=True, forced_lv=None):
    """One iteration of the posterior refinement of the likelihood regret in ONE launch (csrc/latent.hip, latent_refine_kernel):

        dz given:        g = d[mean_l(-log p(x|z_l)) + KL(q || p(z|y))] / d(mu, lv_raw), `dz` (L+1, N, K) being the decoder's
                         part at z = mu + exp(lv/2) eps_cur; then one torch.optim.Adam step (betas (0.9, 0.999), eps 1e-8) of
                         number `step` >= 1 and learning rate `lr` on mu and lv_raw IN PLACE with `state` = (m_mu, v_mu, m_lv,
                         v_lv), updated in place as well (`latent_refine_state`); with forced_lv only mu moves;
        eps_next given:  the latent forward at the (moved) posterior -> (z_next (L+1, N, K), kl, zdist, var_kl (N,)); `lv` (N, K)
                         receives the clipped log-variance.  Without it: the update alone, returns None.

    `lv` must hold the clipped log-variance of the posterior on entry when dz is given (the previous call wrote it).  Labels
    given on the HOST are checked against [0, C) here; labels on the device are checked by the kernel, which never indexes with
    a bad one (that sample does not move, its outputs are NaN).  No autograd: the kernel IS the backward."""
    update, forward = dz is not None, eps_next is not None
    if not (update or forward):
        raise L.JvaeHipError('latent_refine: neither dz (an update) nor eps_next (a forward) was given')
    if not torch.is_tensor(mu) or mu.dim() != 2:
        raise L.JvaeHipError('latent_refine: mu must be (N, K)')
    N, K = mu.shape
    forced = forced_lv is not None
    _refine_operand(mu, (N, K), 'mu')
    _refine_operand(lv, (N, K), 'lv')
    if not forced:
        _refine_operand(lv_raw, (N, K), 'lv_raw')
    means, T = _c(means.detach()), _c(T.detach())
    if means.dim() != 2 or means.shape[1] != K or not means.is_cuda or means.dtype != torch.float32 or T.dtype != torch.float32:
        raise L.JvaeHipError(f'latent_refine: means must be (C, {K}) fp32 on the GPU')
    C = means.shape[0]
    if PRIOR_KIND[prior] != PRIOR_KIND['gaussian'] and var_dim != 'scalar':
        raise L.JvaeHipError('latent_refine: the tilted and uniform priors have a scalar variance')
    t_numel = {'scalar': C, 'diag': C * K, 'full': C * K * K}[var_dim]
    if T.numel() != t_numel:
        raise L.JvaeHipError(f'latent_refine: T has {T.numel()} elements, var_dim {var_dim!r} wants {t_numel}')
    if y.dtype != torch.int64 or tuple(y.shape) != (N,):
        raise L.JvaeHipError(f'latent_refine: class labels must be int64 of shape ({N},)')
    if not y.is_cuda:
        if bool(((y < 0) | (y >= C)).any()):
            L.check(-1, 'latent_refine: a label outside the classes of the prior')
        y = y.to(mu.device)
    y = _c(y)
    noise = eps_next if forward else eps_cur
    if not torch.is_tensor(noise) or noise.dim() != 3:
        raise L.JvaeHipError('latent_refine: the noise must be (L+1, N, K); an update needs eps_cur')
    Ls = noise.shape[0] - 1
    m_mu = v_mu = m_lv = v_lv = None
    if update:
        _refine_operand(eps_cur, (Ls + 1, N, K), 'eps_cur')
        _refine_operand(dz, (Ls + 1, N, K), 'dz')
        if state is None or len(state) != 4:
            raise L.JvaeHipError('latent_refine: an update needs state = (m_mu, v_mu, m_lv, v_lv)')
        m_mu, v_mu = (_refine_operand(t, (N, K), 'Adam state') for t in state[:2])
        if not forced:
            m_lv, v_lv = (_refine_operand(t, (N, K), 'Adam state') for t in state[2:])
        if int(step) < 1 or not math.isfinite(float(lr)):
            raise L.JvaeHipError(f'latent_refine: step {step} must be >= 1 and lr {lr} finite')
    out = None
    if forward:
        _refine_operand(eps_next, (Ls + 1, N, K), 'eps_next')
        z = torch.empty((Ls + 1, N, K), device=mu.device, dtype=torch.float32)
        out = (z,) + tuple(torch.empty((3, N), device=mu.device, dtype=torch.float32))
    o = out or (None,) * 4
    rc = L.load().jvae_latent_refine_f32(
        L.ptr(mu), L.ptr(None if forced else lv_raw), L.ptr(lv), L.ptr(eps_cur if update else None), L.ptr(eps_next),
        L.ptr(y), L.ptr(means), L.ptr(T), L.ptr(dz), L.ptr(m_mu), L.ptr(v_mu), L.ptr(m_lv), L.ptr(v_lv),
        L.ptr(o[0]), L.ptr(o[1]), L.ptr(o[2]), L.ptr(o[3]), N, K, Ls, C, PRIOR_KIND[prior], VAR_KIND[var_dim], float(tau),
        float(alpha), int(bool(sampled)), int(forced), float(forced_lv or 0.), float(lr), int(step) if update else 0,
        (0 if update else 1) | (0 if forward else 2), L.stream_ptr())
    L.check(rc, 'jvae_latent_refine_f32')
    return out


# ------------------------------------------------------------------------------------------- losses
SIGMA_VALUE,SIGMA_LOG, SIGMA_CODED, SIGMA_RMSE = 0, 1, 2, 3      # kinds of sigma the loss kernels know (csrc/loss.hip)


def _check_sigma(sigma, mode, N):
    want = N if mode == SIGMA_CODED else 1
    if mode not in (SIGMA_VALUE, SIGMA_LOG, SIGMA_CODED, SIGMA_RMSE) or (mode != SIGMA_RMSE and sigma.numel() != want):
        raise L.JvaeHipError('sigma must be one value, one log value, N coded log values or the rmse kind; per-dimension '
                             'sigma is not built (the reference itself fails on it: cvae.py:649 / 789 shapes)')


class _Recon(torch.autograd.Function):
    """wmse (L,N) of x_reco[1:] against x (losses.py:8-27; cvae.py:649-652); sigma kinds: csrc/loss.hip."""

    @staticmethod
    def forward(ctx, x_reco, x, sigma, mode, snapshot):
        x_reco = _c(_f32(x_reco, 'recon'))
        x = _c(x)
        sigma = _c(sigma)
        mode = int(mode)
        Lp1, N = x_reco.shape[0], x_reco.shape[1]
        _check_sigma(sigma, mode, N)
        D = x.numel() // max(N, 1)
        if D % 4 == 0:                                   # 16-byte loads: an odd view offset gets a copy (as _MseRows)
            x_reco = x_reco if x_reco.data_ptr() % 16 == 0 else x_reco.clone()
            x = x if x.data_ptr() % 16 == 0 else x.clone()
        wmse = torch.empty((Lp1 - 1, N), device=x.device, dtype=torch.float32)
        rc = L.load().jvae_recon_fwd_f32(L.ptr(x_reco), L.ptr(x), L.ptr(sigma), mode, L.ptr(wmse),
                                         Lp1 - 1, N, D, L.stream_ptr())
        L.check(rc, 'jvae_recon_fwd_f32')
        # snapshot: the caller's decay rule will change `sigma` in place before backward (see recon_bwd_kernel)
        ctx.sigma_fwd = sigma.detach().clone() if (snapshot and mode == SIGMA_VALUE) else None
        ctx.save_for_backward(x_reco, x, sigma, wmse)
        ctx.mode = mode
        ctx.dims = (Lp1 - 1, N, D)
        return wmse

    @staticmethod
    def backward(ctx, g):
        x_reco, x, sigma, wmse = ctx.saved_tensors
        Ls, N, D = ctx.dims
        g = _c(g)
        gxr = torch.empty_like(x_reco)
        gs = torch.empty_like(sigma) if (ctx.needs_input_grad[2] and ctx.mode != SIGMA_RMSE) else None
        ws = L.workspace(4 * Ls * N + 16, x.device)
        rc = L.load().jvae_recon_bwd_f32(L.ptr(x_reco), L.ptr(x), L.ptr(sigma), ctx.mode, L.ptr(ctx.sigma_fwd), L.ptr(g),
                                         L.ptr(wmse), L.ptr(gxr), L.ptr(gs), 0, Ls, N, D, L.ptr(ws), ws.numel(),
                                         L.stream_ptr())
        L.check(rc, 'jvae_recon_bwd_f32')
        return gxr, None, gs, None, None


def recon_wmse(x_reco, x, sigma, sigma_is_log, snapshot=False):
    """sigma_is_log: bool, or one of SIGMA_VALUE / SIGMA_LOG / SIGMA_CODED / SIGMA_RMSE."""
    return _Recon.apply(x_reco, x, sigma, int(sigma_is_log), snapshot)


class _MseRows(torch.autograd.Function):
    """The public `mse_loss(x_output, x_target, ndim, batch_mean=False)` of module/losses.py:8-27 on EVERY row of x_output:
    xo (L, N, D), x (N, D) -> (L, N) mean squares over D (jvae_mse_rows_{fwd,bwd}_f32: the reconstruction kernels told that
    there is no mean-path row in front of the rows - no copy, no padded row)."""

    @staticmethod
    def forward(ctx, xo, x):
        xo = _c(_f32(xo, 'mse_loss'))
        x = _c(_f32(x, 'mse_loss'))
        Ls, N, D = xo.shape
        if D % 4 == 0:                                   # the kernels use 16-byte loads: an odd view offset gets a copy
            xo = xo if xo.data_ptr() % 16 == 0 else xo.clone()
            x = x if x.data_ptr() % 16 == 0 else x.clone()
        wmse = torch.empty((Ls, N), device=x.device, dtype=torch.float32)
        rc = L.load().jvae_mse_rows_fwd_f32(L.ptr(xo), L.ptr(x), L.ptr(wmse), Ls, N, D, L.stream_ptr())
        L.check(rc, 'jvae_mse_rows_fwd_f32')
        ctx.save_for_backward(xo, x)
        return wmse

    @staticmethod
    def backward(ctx, g):
        xo, x = ctx.saved_tensors
        Ls, N, D = xo.shape
        g = _c(g)
        gx = torch.empty_like(xo)
        rc = L.load().jvae_mse_rows_bwd_f32(L.ptr(xo), L.ptr(x), L.ptr(g), L.ptr(gx), Ls, N, D, L.stream_ptr())
        L.check(rc, 'jvae_mse_rows_bwd_f32')
        return gx, None


def mse_rows(xo, x):
    """xo (L, N, D), x (N, D) -> (L, N) mean squares over D of every row (no copy of xo)."""
    return _MseRows.apply(xo, x)


class _Elbo(torch.autograd.Function):
    """wmse_s (L,N), kl (N,), ce (N,)|None, sigma -> (wmse, cross_x, total, mse) (cvae.py:662-670,773-791,887-902)."""

    @staticmethod
    def forward(ctx, wmse_s, kl, ce, sigma, mode, D, beta, cw, cw_dev=None):
        wmse_s, kl, sigma = _c(wmse_s), _c(kl), _c(sigma)
        ce = None if ce is None else _c(ce)
        mode = int(mode)
        Ls, N = wmse_s.shape
        _check_sigma(sigma, mode, N)
        wmse, cx, tot, mse = (torch.empty(N, device=kl.device, dtype=torch.float32) for _ in range(4))
        args = (L.ptr(wmse_s), L.ptr(kl), L.ptr(ce), L.ptr(sigma), mode, L.ptr(wmse), L.ptr(cx), L.ptr(tot), L.ptr(mse),
                Ls, N, int(D), float(beta), float(cw))
        if cw_dev is None:
            rc = L.load().jvae_elbo_fwd_f32(*args, L.stream_ptr())
        else:
            rc = L.load().jvae_elbo_fwd_wdev_f32(*args, L.ptr(cw_dev), L.stream_ptr())
        L.check(rc, 'jvae_elbo_fwd_f32')
        ctx.cw_dev = cw_dev
        ctx.save_for_backward(wmse_s if mode == SIGMA_RMSE else sigma)
        ctx.cfg = (mode, Ls, N, int(D), float(beta), float(cw), ce is not None)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mse)
        return wmse, cx, tot, mse

    @staticmethod
    def backward(ctx, g_wmse, g_cx, g_tot, _g_mse):
        sigma, = ctx.saved_tensors                  # kind 3: the forward's wmse_s
        mode, Ls, N, D, beta, cw, has_ce = ctx.cfg
        dev = sigma.device
        g_ws = torch.empty((Ls, N), device=dev, dtype=torch.float32)
        g_kl = torch.empty(N, device=dev, dtype=torch.float32)
        g_ce = torch.empty(N, device=dev, dtype=torch.float32) if has_ce else None
        gs = torch.empty_like(sigma) if (ctx.needs_input_grad[3] and mode != SIGMA_RMSE) else None
        ws = L.workspace(4 * N + 16, dev)

        def opt(t):
            return None if t is None else _c(t)
        args = (L.ptr(opt(g_wmse)), L.ptr(opt(g_cx)), L.ptr(opt(g_tot)), L.ptr(sigma), mode,
                L.ptr(g_ws), L.ptr(g_kl), L.ptr(g_ce), L.ptr(gs), 0, Ls, N, D, beta, cw)
        if ctx.cw_dev is None:
            rc = L.load().jvae_elbo_bwd_f32(*args, L.ptr(ws), ws.numel(), L.stream_ptr())
        else:
            rc = L.load().jvae_elbo_bwd_wdev_f32(*args, L.ptr(ctx.cw_dev), L.ptr(ws), ws.numel(), L.stream_ptr())
        L.check(rc, 'jvae_elbo_bwd_f32')
        return g_ws, g_kl, g_ce, gs, None, None, None, None, None


def elbo(wmse_s, kl, ce, sigma, sigma_is_log, D, beta, cw, with_mse=False):
    """`cw` (the weight of cross_y in `total`): a float, or a 1-element fp32 DEVICE tensor read by the kernels at run time."""
    cw_dev = None
    if torch.is_tensor(cw):
        cw_dev, cw = _device_scalar(cw, 'cw'), 0.
    wmse, cx, tot, mse = _Elbo.apply(wmse_s, kl, ce, sigma, int(sigma_is_log), D, beta, cw, cw_dev)
    return (wmse, cx, tot, mse) if with_mse else (wmse, cx, tot)


def iws(wmse_s, eps, log_var, log_pz, sigma, sigma_is_log, D):
    """Importance-weighted bound of the evaluation path (no gradient): wmse_s (L,N), eps (L,N,K), log_var (N,K),
    log_pz (L,C,N) or (L,N) -> (C,N) or (N,)  (reference cvae.py:793-873)."""
    Ls, N, K = eps.shape
    conditional = log_pz.dim() == 3
    C = log_pz.shape[1] if conditional else 1
    rows = torch.empty((Ls, N), device=eps.device, dtype=torch.float32)
    out = torch.empty((C, N), device=eps.device, dtype=torch.float32)
    rc = L.load().jvae_iws_f32(L.ptr(_c(_f32(wmse_s, 'iws'))), L.ptr(_c(eps)), L.ptr(_c(log_var)), L.ptr(_c(log_pz)), L.ptr(_c(sigma)),
                              int(sigma_is_log), Ls, N, K, C, int(D), L.ptr(rows), L.ptr(out), L.stream_ptr())
    L.check(rc, 'jvae_iws_f32')
    return out if conditional else out[0]


def _iw_operand(t, shape, what, dtype=torch.float32):
    """An operand of the importance-weighted bound as the kernels read it: this dtype and shape (lib.ptr then refuses a tensor
    that is off the device or not contiguous when its address is taken)."""
    if t.dtype != dtype:
        raise L.JvaeHipError(f'iw_bound: {what} must be {dtype}, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise L.JvaeHipError(f'iw_bound: {what} must have the shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


class _IwBound(torch.autograd.Function):
    """wmse_s (L,N), z (L+1,N,K), lv (N,K), eps (L,N,K), y, means, T, sigma -> (bound (N,), ess (N,)): csrc/iwae.hip."""

    @staticmethod
    def forward(ctx, wmse_s, z, lv, eps, y, means, T, sigma, cfg, state):
        mode, D, beta, var_dim = cfg
        Ls, N, K = eps.shape
        C = means.shape[0]
        _iw_operand(wmse_s, (Ls, N), 'wmse_s')
        _iw_operand(z, (Ls + 1, N, K), 'z')
        _iw_operand(lv, (N, K), 'lv')
        _iw_operand(eps, (Ls, N, K), 'eps')
        _iw_operand(y, (N,), 'y', torch.int64)
        _iw_operand(means, (C, K), 'means')
        _iw_operand(T, (C, K) if var_dim == VAR_KIND['diag'] else ((C, K, K) if var_dim == VAR_KIND['full'] else (C,)), 'T')
        _check_sigma(sigma, mode, N)
        _iw_operand(sigma, sigma.shape, 'sigma')
        dev = eps.device
        if state is not None:
            _iw_operand(state, (4, N), 'state', torch.float64)
        bound, ess = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(2))
        wt = torch.empty((Ls, N), device=dev, dtype=torch.float32)
        rc = L.load().jvae_iw_bound_fwd_f32(L.ptr(wmse_s), L.ptr(z), L.ptr(lv), L.ptr(eps), L.ptr(y), L.ptr(means), L.ptr(T),
                                            L.ptr(sigma), mode, PRIOR_KIND['gaussian'], var_dim, beta, Ls, N, K, C, D,
                                            L.ptr(bound), L.ptr(wt), L.ptr(ess), L.ptr(state), L.stream_ptr())
        L.check(rc, 'jvae_iw_bound_fwd_f32')
        ctx.save_for_backward(wt, z, y, means, T, sigma)
        ctx.cfg = (mode, D, beta, var_dim, Ls, N, K, C)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(ess)
        return bound, ess

    @staticmethod
    def backward(ctx, g_bound, _g_ess):
        wt, z, y, means, T, sigma = ctx.saved_tensors
        mode, D, beta, var_dim, Ls, N, K, C = ctx.cfg
        dev = wt.device
        lib = L.load()
        g_ws = torch.empty((Ls, N), device=dev, dtype=torch.float32)
        g_z = torch.empty((Ls + 1, N, K), device=dev, dtype=torch.float32)
        g_lv = torch.empty((N, K), device=dev, dtype=torch.float32)
        g_means = torch.empty_like(means) if ctx.needs_input_grad[5] else None
        g_T = torch.empty_like(T) if (ctx.needs_input_grad[6] and var_dim == VAR_KIND['diag']) else None
        g_sigma = torch.empty_like(sigma) if ctx.needs_input_grad[7] else None
        ws = L.workspace(lib.jvae_iw_bound_bwd_workspace_bytes(N, K), dev)
        g = None if g_bound is None else _c(g_bound)
        rc = lib.jvae_iw_bound_bwd_f32(L.ptr(g), L.ptr(wt), L.ptr(z), L.ptr(y), L.ptr(means), L.ptr(T), L.ptr(sigma), mode,
                                       PRIOR_KIND['gaussian'], var_dim, beta, Ls, N, K, C, D, L.ptr(g_ws), L.ptr(g_z), L.ptr(g_lv),
                                       L.ptr(g_means), L.ptr(g_T), L.ptr(g_sigma), L.ptr(ws), ws.numel(), L.stream_ptr())
        L.check(rc, 'jvae_iw_bound_bwd_f32')
        return g_ws, g_z, g_lv, None, None, g_means, g_T, g_sigma, None, None


def iw_bound(wmse_s, z, lv, eps, y, means, T, sigma, sigma_is_log, D, beta=1., var_dim='scalar', state=None):
    """The importance-weighted bound of Burda et al. and its effective sample size -> (bound (N,), ess (N,)), csrc/iwae.hip:

        log w_l = log p(x | z_l) + beta (log p(z_l | y) - log q(z_l | x)),  bound = logsumexp_l(log w_l) - log L,  ess = 1 / sum_l wt_l^2

    wmse_s (L, N) of recon_wmse, z (L+1, N, K) and lv (N, K) of latent (row 0 of z takes no part), eps (L, N, K) the noise of the
    draws, y (N,) int64, means (C, K) and T ((C,) 'scalar' / (C, K) 'diag') of the Gaussian prior, sigma and its kind as elbo takes
    them.  Differentiable in wmse_s, z, lv, means, T ('diag') and sigma with the DIRECT partial derivatives; autograd carries z and lv
    on through latent's backward.  ess carries no gradient.  Operands must be fp32 (y int64), contiguous and on the device.
    var_dim 'full', the rmse sigma kind: refused by the library (unsupported configuration); the tilted and uniform priors have
    no entry here at all.  log w is formed in fp64 inside the kernels.  state (4, N) fp64, zeros at first: the bound over slabs of draws - each call merges its slab in and
    returns bound / ess of all draws so far; no gradient flows through a call with a state."""
    if var_dim not in VAR_KIND:
        raise L.JvaeHipError(f'iw_bound: var_dim {var_dim!r} unknown')
    if state is not None and torch.is_grad_enabled() and any(t.requires_grad for t in (wmse_s, z, lv, means, T, sigma)):
        raise L.JvaeHipError('iw_bound: a call with a state carries no gradient: run it under no_grad')
    return _IwBound.apply(wmse_s, z, lv, eps, y, means, T, sigma, (int(sigma_is_log), int(D), float(beta), VAR_KIND[var_dim]), state)


TC_MAX_K, TC_MAX_N, TC_MAX_Q = 1024, 8192, 1 << 26       # the limits of csrc/tcvae.hip (L N^2 <= 2^26: 256 MB of kept exponents)


def tc_joint_partition():
    """Rows of a piece of tc_objective's joint sum (host only): the pieces are merged one after the other."""
    return int(L.load().jvae_tc_joint_partition())


def _tc_operand(t, shape, what, dtype=torch.float32):
    if t.dtype != dtype:
        raise L.JvaeHipError(f'tc_objective: {what} must be {dtype}, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise L.JvaeHipError(f'tc_objective: {what} must have the shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


class _TcObjective(torch.autograd.Function):
    """z (L+1,N,K), mu (N,K), lv (N,K), eps (L,N,K), y, means, T -> (reg, mi, tc, dwkl), each (N,): csrc/tcvae.hip."""

    @staticmethod
    def forward(ctx, z, mu, lv, eps, y, means, T, log_n, cfg):
        alpha, beta_tc, gamma, var_dim = cfg
        Ls, N, K = eps.shape
        C = means.shape[0]
        _tc_operand(z, (Ls + 1, N, K), 'z')
        _tc_operand(mu, (N, K), 'mu')
        _tc_operand(lv, (N, K), 'log_var')
        _tc_operand(eps, (Ls, N, K), 'eps')
        _tc_operand(y, (N,), 'y', torch.int64)
        _tc_operand(means, (C, K), 'means')
        _tc_operand(T, (C, K) if var_dim == VAR_KIND['diag'] else ((C, K, K) if var_dim == VAR_KIND['full'] else (C,)), 'T')
        if log_n is not None:
            _tc_operand(log_n, (C,), 'log_n', torch.float64)
        if Ls < 1 or K < 1:
            raise L.JvaeHipError(f'tc_objective: at least one draw and one coordinate expected, got L={Ls}, K={K}')
        if K > TC_MAX_K or N > TC_MAX_N:
            raise L.JvaeHipError(f'tc_objective: K <= {TC_MAX_K} and N <= {TC_MAX_N} expected, got N={N}, K={K} (unsupported configuration)')
        if Ls * N * N > TC_MAX_Q:
            raise L.JvaeHipError(f'tc_objective: the kept exponents (L, N, N) would take more than 256 MB (L N^2 = {Ls * N * N} > 2^26): '
                                 'unsupported configuration, use a smaller batch or fewer draws')
        operands = [L.ptr(t) for t in (z, mu, lv, eps, y, means, T, log_n)]      # on the device and contiguous, before anything is allocated
        dev = eps.device
        lib = L.load()
        reg, mi, tc, dwkl = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(4))
        keep = None
        if N:
            keep = torch.empty(lib.jvae_tc_keep_bytes(Ls, N, K), device=dev, dtype=torch.uint8)
            nbytes = lib.jvae_tc_fwd_workspace_bytes(Ls, N, K)
            ws = _aligned_ws(nbytes, dev, align=16, what='tc_objective')
        else:
            ws = (None, 0)
        rc = lib.jvae_tc_objective_fwd_f32(*operands, var_dim, alpha, beta_tc, gamma, Ls, N, K, C, L.ptr(reg), L.ptr(mi), L.ptr(tc), L.ptr(dwkl),
                                           L.ptr(keep), keep.numel() if N else 0, *ws, L.stream_ptr())
        L.check(rc, 'jvae_tc_objective_fwd_f32')
        ctx.save_for_backward(z, mu, lv, y, means, T, keep)
        ctx.cfg = (alpha, beta_tc, gamma, var_dim, Ls, N, K, C)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(mi, tc, dwkl)
        return reg, mi, tc, dwkl

    @staticmethod
    def backward(ctx, g_reg, _g_mi, _g_tc, _g_dwkl):
        z, mu, lv, y, means, T, keep = ctx.saved_tensors
        alpha, beta_tc, gamma, var_dim, Ls, N, K, C = ctx.cfg
        dev = z.device
        lib = L.load()
        g_z = torch.empty((Ls + 1, N, K), device=dev, dtype=torch.float32)
        g_mu = torch.empty((N, K), device=dev, dtype=torch.float32)
        g_lv = torch.empty((N, K), device=dev, dtype=torch.float32)
        g_means = torch.empty_like(means) if ctx.needs_input_grad[5] else None
        g_T = torch.empty_like(T) if (ctx.needs_input_grad[6] and var_dim == VAR_KIND['diag']) else None
        ws = L.workspace(lib.jvae_tc_bwd_workspace_bytes(N, K), dev)
        g = None if g_reg is None else _c(g_reg)
        rc = lib.jvae_tc_objective_bwd_f32(L.ptr(g), L.ptr(z), L.ptr(mu), L.ptr(lv), L.ptr(y), L.ptr(means), L.ptr(T), var_dim, alpha,
                                           beta_tc, gamma, Ls, N, K, C, L.ptr(keep), keep.numel() if N else 0, L.ptr(g_z),
                                           L.ptr(g_mu), L.ptr(g_lv), L.ptr(g_means), L.ptr(g_T), L.ptr(ws), ws.numel(), L.stream_ptr())
        L.check(rc, 'jvae_tc_objective_bwd_f32')
        return g_z, g_mu, g_lv, None, None, g_means, g_T, None, None


def tc_objective(z, mu, log_var, eps, y, means, T, weights=(1., 6., 1.), log_n=None, var_dim='scalar'):
    """The beta-TCVAE split of the KL over the batch's own posteriors (Chen et al. 2018) -> (reg, mi, tc, dwkl), each (N,),
    csrc/tcvae.hip:

        mi = A - J,  tc = J - P,  dwkl = P - Bp  (means over the L draws),   reg = alpha mi + beta_tc tc + gamma dwkl
        A = log q(z_l | x),  J = logsumexp_{j in S} sum_k l_jk - c,  P = sum_k [logsumexp_{j in S} l_jk - c],  Bp = log p(z_l | y)

    with S the rows of the batch that carry the sample's label (one class: the whole batch) and c = log |S| + log n.  z (L+1, N, K)
    and log_var (N, K) of latent (row 0 of z takes no part), mu (N, K), eps (L, N, K) the noise of the draws, y (N,) int64, means
    (C, K) and T ((C,) 'scalar' / (C, K) 'diag') of the Gaussian prior, weights = (alpha, beta_tc, gamma), log_n (C,) fp64 on the
    device = log of the number of training samples behind each class (None: n = |S|, the plain minibatch estimator; it moves the
    three terms by constants and enters no gradient).  Differentiable in z, mu, log_var, means and T ('diag') with the DIRECT
    partial derivatives; autograd carries z and log_var on through latent's backward.  mi, tc and dwkl carry no gradient.  Operands
    must be fp32 (y int64), contiguous and on the device.  K <= 1024, N <= 8192 and L N^2 <= 2^26; var_dim 'full' is refused by the
    library.  A label outside [0, C): NaN in every output of that sample, which is in nobody's set."""
    if var_dim not in VAR_KIND:
        raise L.JvaeHipError(f'tc_objective: var_dim {var_dim!r} unknown')
    a, b, g = (float(w) for w in weights)
    return _TcObjective.apply(z, mu, log_var, eps, y, means, T, log_n, (a, b, g, VAR_KIND[var_dim]))


MMD_MAX_K, MMD_MAX_N, MMD_MAX_L, MMD_MAX_SCALES = 1024, 8192, 65535, 8       # the limits of csrc/mmd.hip
MMD_KINDS = {'imq': 0, 'rbf': 1}
MMD_WAE_SCALES = (.1, .2, .5, 1., 2., 5., 10.)       # WAE's seven scales, times 2 K for a unit-variance prior


def mmd_tile():
    """Rows of a workgroup's tile of mmd_objective's pair sums (host only)."""
    return int(L.load().jvae_mmd_tile())


def mmd_scales(kernel, K):
    """(kind, scales) of a kernel = (kind, scales | None) as the library takes them: kind 'imq' | 'rbf', scales a tuple of 1..8
    positive finite floats read as absolute C_s / h_s, None: 2 K s for WAE's seven s.  Plain numbers: they carry no gradient."""
    try:
        kind, scales = kernel
    except (TypeError, ValueError):
        raise L.JvaeHipError(f'mmd_objective: kernel is (kind, scales), got {kernel!r}') from None
    if kind not in MMD_KINDS:
        raise L.JvaeHipError(f'mmd_objective: kernel kind {kind!r} unknown (one of {sorted(MMD_KINDS)})')
    if scales is None:
        scales = tuple(2. * K * s for s in MMD_WAE_SCALES)
    try:
        scales = tuple(float(s) for s in scales)
    except (TypeError, ValueError):
        raise L.JvaeHipError(f'mmd_objective: scales is a tuple of numbers or None, got {scales!r}') from None
    # positive and finite as the fp32 values the kernels read
    if not 1 <= len(scales) <= MMD_MAX_SCALES or not all(0. < ctypes.c_float(s).value < float('inf') for s in scales):
        raise L.JvaeHipError(f'mmd_objective: 1 to {MMD_MAX_SCALES} positive finite scales expected, got {scales!r}')
    return kind, scales


def _mmd_operand(t, shape, what, dtype=torch.float32):
    if t.dtype != dtype:
        raise L.JvaeHipError(f'mmd_objective: {what} must be {dtype}, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise L.JvaeHipError(f'mmd_objective: {what} must have the shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


class _MmdObjective(torch.autograd.Function):
    """z (L+1,N,K), eps_p (L,N,K), y, means, T -> m (N,): csrc/mmd.hip."""

    @staticmethod
    def forward(ctx, z, eps_p, y, means, T, cfg):
        kind, scales, joint, var_dim = cfg
        if eps_p.dim() != 3:
            raise L.JvaeHipError(f'mmd_objective: eps_p must have the shape (L, N, K), got {tuple(eps_p.shape)}')
        Ls, N, K = eps_p.shape
        C = means.shape[0] if means.dim() else 0
        _mmd_operand(z, (Ls + 1, N, K), 'z')
        _mmd_operand(eps_p, (Ls, N, K), 'eps_p')
        _mmd_operand(y, (N,), 'y', torch.int64)
        _mmd_operand(means, (C, K), 'means')
        _mmd_operand(T, (C, K) if var_dim == VAR_KIND['diag'] else ((C, K, K) if var_dim == VAR_KIND['full'] else (C,)), 'T')
        if Ls < 1 or K < 1 or C < 1:
            raise L.JvaeHipError(f'mmd_objective: at least one draw, one coordinate and one class expected, got L={Ls}, K={K}, C={C}')
        if K > MMD_MAX_K or N > MMD_MAX_N or Ls > MMD_MAX_L:
            raise L.JvaeHipError(f'mmd_objective: K <= {MMD_MAX_K}, N <= {MMD_MAX_N} and L <= {MMD_MAX_L} expected, got N={N}, K={K}, '
                                 f'L={Ls} (unsupported configuration)')
        operands = [L.ptr(t) for t in (z, eps_p, y, means, T)]      # on the device and contiguous, before anything is allocated
        dev = eps_p.device
        lib = L.load()
        sc = (ctypes.c_float * len(scales))(*scales)
        m = torch.empty(N, device=dev, dtype=torch.float32)
        ws = _aligned_ws(lib.jvae_mmd_fwd_workspace_bytes(Ls, N, K), dev, align=16, what='mmd_objective') if N else (None, 0)
        rc = lib.jvae_mmd_objective_fwd_f32(*operands, var_dim, MMD_KINDS[kind], sc, len(scales), int(joint), Ls, N, K, C, L.ptr(m),
                                            *ws, L.stream_ptr())
        L.check(rc, 'jvae_mmd_objective_fwd_f32')
        ctx.save_for_backward(z, eps_p, y, means, T)
        ctx.cfg = (kind, scales, joint, var_dim, Ls, N, K, C)
        ctx.set_materialize_grads(False)
        return m

    @staticmethod
    def backward(ctx, g_m):
        z, eps_p, y, means, T = ctx.saved_tensors
        kind, scales, joint, var_dim, Ls, N, K, C = ctx.cfg
        dev = z.device
        lib = L.load()
        g_z = torch.empty((Ls + 1, N, K), device=dev, dtype=torch.float32)
        g_means = torch.empty_like(means) if ctx.needs_input_grad[3] else None
        g_T = torch.empty_like(T) if ctx.needs_input_grad[4] else None
        sc = (ctypes.c_float * len(scales))(*scales)
        nbytes = lib.jvae_mmd_bwd_workspace_bytes(Ls, N, K) if N else 16
        ws = _aligned_ws(nbytes, dev, align=16, what='mmd_objective')
        g = None if g_m is None else _c(g_m)
        rc = lib.jvae_mmd_objective_bwd_f32(L.ptr(g), L.ptr(z), L.ptr(eps_p), L.ptr(y), L.ptr(means), L.ptr(T), var_dim, MMD_KINDS[kind],
                                            sc, len(scales), int(joint), Ls, N, K, C, L.ptr(g_z), L.ptr(g_means), L.ptr(g_T), *ws,
                                            L.stream_ptr())
        L.check(rc, 'jvae_mmd_objective_bwd_f32')
        return g_z, None, None, g_means, g_T, None


def mmd_objective(z, eps_p, y, means, T, kernel=('imq', None), joint=True, var_dim='scalar'):
    """The per-row terms of the unbiased U-statistic of MMD^2 between the step's draws and draws of the class-conditional Gaussian
    prior (InfoVAE, Zhao et al. 2019; WAE-MMD, Tolstikhin et al. 2018) -> m (N,), csrc/mmd.hip:

        p_li = means[y_i] + eps_p_li / T[y_i]                    (prior_sample's 'scalar' / 'diag' expression, bit for bit)
        m_i = mean_l [ 1/(N-1) sum_{j in S_i, j != i} k(z_li, z_lj) + 1/(N-1) sum_{j in S_i, j != i} k(p_li, p_lj)
                       - 2/N sum_{j in S_i} k(z_li, p_lj) ]

    with S_i the rows of the batch that carry the sample's label (joint=False or one class: the whole batch), so that mean_i m_i
    estimates the MMD between the joint laws q(z, y) and pi_hat(y) p(z | y).  z (L+1, N, K) of latent (row 0 takes no part: its
    gradient is 0), eps_p (L, N, K) the noise of the prior draws, y (N,) int64, means (C, K) and T ((C,) 'scalar' / (C, K) 'diag')
    of the Gaussian prior.  kernel = (kind, scales): 'imq' sum_s C_s / (C_s + d^2) or 'rbf' sum_s exp(-d^2 / (2 h_s)), scales a
    tuple of at most 8 positive floats or None (2 K s for WAE's seven s); d^2 is the direct sum of squared differences.
    Differentiable in z, means and T with the DIRECT partial derivatives (kernel values are formed again in the backward, nothing
    of size (L, N, N) is kept); autograd carries z on through latent's backward.  Operands must be fp32 (y int64), contiguous and
    on the device.  K <= 1024, N <= 8192; var_dim 'full' is refused by the library.  A label outside [0, C): NaN in every output
    of that sample, which is in nobody's set."""
    if var_dim not in VAR_KIND:
        raise L.JvaeHipError(f'mmd_objective: var_dim {var_dim!r} unknown')
    if eps_p.dim() != 3:
        raise L.JvaeHipError(f'mmd_objective: eps_p must have the shape (L, N, K), got {tuple(eps_p.shape)}')
    kind, scales = mmd_scales(kernel, eps_p.shape[-1])
    return _MmdObjective.apply(z, eps_p, y, means, T, (kind, scales, bool(joint), VAR_KIND[var_dim]))


SEMI_MAX_K, SEMI_MAX_C, SEMI_MAX_N = 1024, 1024, 1 << 20       # the limits of csrc/semisup.hip


def _semi_operand(t, shape, what, dtype=torch.float32):
    if t.dtype != dtype:
        raise L.JvaeHipError(f'class_marginal_kl: {what} must be {dtype}, got {t.dtype}')
    if tuple(t.shape) != tuple(shape):
        raise L.JvaeHipError(f'class_marginal_kl: {what} must have the shape {tuple(shape)}, got {tuple(t.shape)}')
    return t


class _ClassMarginalKl(torch.autograd.Function):
    """mu, lv (N,K), y, means, T, log_pi, the labelled rows' (kl, zdist, var_kl) -> merged (kl, zdist, var_kl), r (N,C): csrc/semisup.hip."""

    @staticmethod
    def forward(ctx, mu, lv, y, means, T, log_pi, kl_in, zd_in, vkl_in, cfg):
        w, var_dim = cfg
        if mu.dim() != 2 or means.dim() != 2:
            raise L.JvaeHipError(f'class_marginal_kl: mu (N, K) and means (C, K) expected, got {tuple(mu.shape)} and {tuple(means.shape)}')
        N, K = mu.shape
        C = means.shape[0]
        _semi_operand(mu, (N, K), 'mu')
        _semi_operand(lv, (N, K), 'log_var')
        _semi_operand(y, (N,), 'y', torch.int64)
        _semi_operand(means, (C, K), 'means')
        _semi_operand(T, (C, K) if var_dim == VAR_KIND['diag'] else (C,), 'T')
        if log_pi is not None:
            _semi_operand(log_pi, (C,), 'log_pi', torch.float64)
        for t, what in ((kl_in, 'kl'), (zd_in, 'zdist'), (vkl_in, 'var_kl')):
            _semi_operand(t, (N,), what)
        if not math.isfinite(w):
            raise L.JvaeHipError(f'class_marginal_kl: a finite w expected, got {w}')
        if K < 1 or C < 1:
            raise L.JvaeHipError(f'class_marginal_kl: at least one coordinate and one class expected, got K={K}, C={C}')
        if K > SEMI_MAX_K or C > SEMI_MAX_C or N > SEMI_MAX_N:
            raise L.JvaeHipError(f'class_marginal_kl: K <= {SEMI_MAX_K}, C <= {SEMI_MAX_C} and N <= {SEMI_MAX_N} expected, got N={N}, K={K}, '
                                 f'C={C} (unsupported configuration)')
        operands = [L.ptr(t) for t in (mu, lv, y, means, T, log_pi)]       # on the device and contiguous, before anything is allocated
        rows = [L.ptr(t) for t in (kl_in, zd_in, vkl_in)]
        dev = mu.device
        lib = L.load()
        kl, zd, vkl = (torch.empty(N, device=dev, dtype=torch.float32) for _ in range(3))
        r = torch.empty((N, C), device=dev, dtype=torch.float32)
        ws = _aligned_ws(lib.jvae_semi_fwd_workspace_bytes(N, C), dev, what='class_marginal_kl') if N else (None, 0)
        rc = lib.jvae_semi_class_marginal_fwd_f32(*operands, var_dim, w, N, K, C, *rows, L.ptr(kl), L.ptr(zd), L.ptr(vkl), L.ptr(r),
                                                  4 * N * C, *ws, L.stream_ptr())
        L.check(rc, 'jvae_semi_class_marginal_fwd_f32')
        ctx.save_for_backward(mu, lv, y, means, T, r)
        ctx.cfg = (w, var_dim, N, K, C)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(zd, vkl, r)
        return kl, zd, vkl, r

    @staticmethod
    def backward(ctx, g_kl, _g_zd, _g_vkl, _g_r):
        mu, lv, y, means, T, r = ctx.saved_tensors
        w, var_dim, N, K, C = ctx.cfg
        dev = mu.device
        lib = L.load()
        g_in = torch.empty(N, device=dev, dtype=torch.float32)
        g_mu = torch.empty((N, K), device=dev, dtype=torch.float32)
        g_lv = torch.empty((N, K), device=dev, dtype=torch.float32)
        g_means = torch.empty_like(means) if ctx.needs_input_grad[3] else None
        g_T = torch.empty_like(T) if (ctx.needs_input_grad[4] and var_dim == VAR_KIND['diag']) else None
        g = None if g_kl is None else _c(g_kl)
        rc = lib.jvae_semi_class_marginal_bwd_f32(L.ptr(g), L.ptr(mu), L.ptr(lv), L.ptr(y), L.ptr(means), L.ptr(T), var_dim, w, N, K, C,
                                                  L.ptr(r), 4 * N * C, L.ptr(g_in), L.ptr(g_mu), L.ptr(g_lv), L.ptr(g_means), L.ptr(g_T),
                                                  L.stream_ptr())
        L.check(rc, 'jvae_semi_class_marginal_bwd_f32')
        return g_mu, g_lv, None, g_means, g_T, None, g_in, None, None, None


def class_marginal_kl(mu, log_var, y, means, T, kl, zdist, var_kl, log_pi=None, w=1., var_dim='scalar'):
    """The KL of a batch in which a NEGATIVE label means "no label" -> (kl, zdist, var_kl (N,), r (N, C)), csrc/semisup.hip.

    A row with y >= 0 keeps the kl, zdist and var_kl given (those of ops.latent), bit for bit; its row of r is one-hot on y.  A row
    with y < 0 is measured against every class of the Gaussian prior at once:

        KL_c = 1/2 (d_c + w v_c)        d_c, v_c: GaussianPrior.kl's distance and var_kl against class c
        kl = U = -log sum_c pi_c exp(-KL_c),   r_c = pi_c exp(-KL_c) / sum_c' pi_c' exp(-KL_c'),   zdist = r . d,   var_kl = r . v

    U is an upper bound of KL(q || sum_c pi_c p_c) (Hershey & Olsen 2007), r the optimal q(y | x).  mu, log_var (N, K) (the CLIPPED
    log-variance), y (N,) int64, means (C, K), T ((C,) 'scalar' / (C, K) 'diag'), log_pi (C,) fp64 on the device (None: uniform
    weights), w a finite float.  Differentiable in kl only - through mu, log_var, means, T ('diag') for the unlabelled rows and
    through the incoming kl for the labelled ones; zdist, var_kl and r carry no gradient.  No (N, C, K) tensor exists.  Operands must
    be fp32 (y int64, log_pi fp64), contiguous and on the device.  K <= 1024, C <= 1024, N <= 2^20; var_dim 'full' has no entry."""
    if var_dim not in ('scalar', 'diag'):
        raise L.JvaeHipError(f"class_marginal_kl: var_dim 'scalar' or 'diag' expected, got {var_dim!r}")
    if torch.is_tensor(w):
        raise L.JvaeHipError('class_marginal_kl: w is a host float here, not a tensor')
    return _ClassMarginalKl.apply(mu, log_var, y, means, T, log_pi, kl, zdist, var_kl, (float(w), VAR_KIND[var_dim]))


def measures(x, wmse, zdist, var_kl, sigma, sigma_is_log, means, flag, scratch, prev=None, batch=0, run=None, counter=None):
    """-> device tensor of 16 floats (layout in csrc/loss.hip measures_kernel); `scratch`: 1-float device tensor;
    `prev`: the tensor returned for the previous batch (running means are continued on the device).
    run (16 fp32) + counter (1 int32), both on the device: the captured-step form - the batch index is *counter (incremented
    by the kernel), `run` is the previous result and receives this one (returned); prev / batch are not used."""
    lib = L.load()
    x = _c(x)
    sqnorm_accum(x, scratch, True)
    C, K = (means.shape if means is not None else (0, 0))
    if run is not None:
        if run.dtype != torch.float32 or run.numel() != 16 or counter is None or counter.dtype != torch.int32 or counter.numel() != 1:
            raise L.JvaeHipError('measures: run must hold 16 fp32 values and counter one int32')
        rc = lib.jvae_measures_dev_f32(L.ptr(scratch), x.numel(), L.ptr(_c(wmse)), L.ptr(_c(zdist)), L.ptr(_c(var_kl)), wmse.numel(),
                                       zdist.numel(), L.ptr(_c(sigma)), int(sigma_is_log),
                                       L.ptr(None if means is None else _c(means)), C, K, L.ptr(flag), L.ptr(run), L.ptr(counter),
                                       L.stream_ptr())
        L.check(rc, 'jvae_measures_dev_f32')
        return run
    out = torch.empty(16, device=x.device, dtype=torch.float32)
    rc = lib.jvae_measures_f32(L.ptr(scratch), x.numel(), L.ptr(_c(wmse)), L.ptr(_c(zdist)), L.ptr(_c(var_kl)), wmse.numel(), zdist.numel(),
                               L.ptr(_c(sigma)), int(sigma_is_log), L.ptr(None if means is None else _c(means)), C, K,
                               L.ptr(flag), L.ptr(prev), int(batch), L.ptr(out), L.stream_ptr())
    L.check(rc, 'jvae_measures_f32')
    return out


LOSS_ROWS_MAX = 16


def loss_sums(rows, acc):
    """acc[r] += mean(rows[r]) for every r, in ONE launch (csrc/loss.hip loss_sums_kernel): `rows` - up to 16 fp32 device
    tensors of any shapes (the loss rows of a step, (N,) or (L+1, N)); `acc` - fp32 device vector of at least len(rows)
    entries, updated in place.  Fixed summation order: repeatable bit for bit."""
    n = len(rows)
    if n > LOSS_ROWS_MAX:
        raise L.JvaeHipError('loss_sums takes at most {} rows, got {}'.format(LOSS_ROWS_MAX, n))
    if acc.dtype != torch.float32 or acc.numel() < n:
        raise L.JvaeHipError('loss_sums: acc must be fp32 with one entry per row')
    rows = [_c(_f32(r.detach(), 'loss_sums')) for r in rows]
    if any(r.numel() == 0 for r in rows):
        raise L.JvaeHipError('loss_sums: empty row')
    ptrs = (ctypes.c_void_p * max(n, 1))(*[L.ptr(r) for r in rows])
    lens = (ctypes.c_long * max(n, 1))(*[r.numel() for r in rows])
    rc = L.load().jvae_loss_sums_f32(ptrs, lens, n, L.ptr(acc), L.stream_ptr())
    L.check(rc, 'jvae_loss_sums_f32')
    return acc


class _Xent(torch.autograd.Function):
    """Row-wise cross entropy, target y[r % N] (F.cross_entropy(reduction='none'), losses.py:76-86)."""

    @staticmethod
    def forward(ctx, logits, y):
        lg = _c(_f32(logits, 'xent').reshape(-1, logits.shape[-1]))
        y = _c(y)
        R, C = lg.shape
        ce = torch.empty(R, device=lg.device, dtype=torch.float32)
        L.check(L.load().jvae_xent_fwd_f32(L.ptr(lg), L.ptr(y), L.ptr(ce), R, y.numel(), C, L.stream_ptr()), 'xent_fwd')
        ctx.save_for_backward(lg, y)
        ctx.shape = logits.shape
        return ce.reshape(logits.shape[:-1])

    @staticmethod
    def backward(ctx, g):
        lg, y = ctx.saved_tensors
        R, C = lg.shape
        g = _c(g.reshape(-1))
        gl = torch.empty_like(lg)
        L.check(L.load().jvae_xent_bwd_f32(L.ptr(lg), L.ptr(y), L.ptr(g), L.ptr(gl), R, y.numel(), C, L.stream_ptr()),
                'xent_bwd')
        return gl.reshape(ctx.shape), None


def cross_entropy_rows(logits, y):
    return _Xent.apply(logits, y)


# ------------------------------------------------------------------------------------------- optimiser
def sqnorm_accum(g, acc, reset):
    lib = L.load()
    ws = L.workspace(lib.jvae_sqnorm_workspace_bytes(), g.device)
    L.check(lib.jvae_sqnorm_accum_f32(L.ptr(g), g.numel(), L.ptr(acc), int(reset), L.ptr(ws), ws.numel(), L.stream_ptr()), 'sqnorm')


def clip_scale(g, sqnorm, max_norm):
    L.check(L.load().jvae_clip_scale_f32(L.ptr(g), g.numel(), L.ptr(sqnorm), float(max_norm), L.stream_ptr()), 'clip_scale')


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, max_norm=0., sqnorm=None, flag=None):
    rc = L.load().jvae_adam_step_f32(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), lr, beta1, beta2, eps,
                                     weight_decay, step, float(max_norm or 0.), L.ptr(sqnorm), L.ptr(flag), L.stream_ptr())
    L.check(rc, 'jvae_adam_step_f32')


def sgd_step(p, g, buf, lr, momentum, nesterov, weight_decay, first, max_norm=0., sqnorm=None, flag=None):
    """torch.optim.SGD update of one flat buffer (clip coefficient and NaN/Inf flag fused as for Adam)."""
    L.check(L.load().jvae_sgd_step_f32(L.ptr(p), L.ptr(g), L.ptr(buf), p.numel(), float(lr), float(momentum), int(bool(nesterov)),
                                      float(weight_decay), int(bool(first)), float(max_norm or 0.), L.ptr(sqnorm), L.ptr(flag),
                                      L.stream_ptr()), 'jvae_sgd_step_f32')


def adam_step_dev(p, g, m, v, hyper, advance, eps, weight_decay, max_norm=0., sqnorm=None, flag=None):
    """Adam with step count / lr / betas read from the 6-float device block `hyper` (capturable: no host state)."""
    rc = L.load().jvae_adam_step_dev_f32(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(hyper), int(advance),
                                         eps, weight_decay, float(max_norm or 0.), L.ptr(sqnorm), L.ptr(flag),
                                         L.stream_ptr())
    L.check(rc, 'jvae_adam_step_dev_f32')


# ------------------------------------------------------------------------------------------- ROC of OOD scores
def roc_curve(ins, outs, kept_tpr, two_sided=False):
    """AUC and the FPR / thresholds at the kept TPRs of M score rows in one call (utils/roc_curves.py:38-210; csrc/roc.hip).
    ins (M, n_in) or (n_in,), outs (M, n_out) or (n_out,): fp32 scores on the device, higher = more in-distribution.
    kept_tpr: ascending floats (list or fp64 device tensor of K).  two_sided: per row (or one value for all rows) False / True
    = one-sided test, 'around-mean' = two-sided around the mean of the in-scores, ('quantile', f_low, f_up) = the reference's
    two_sided=(f_low, f_up) on the sorted in-scores themselves (every f_low-th as a lower, every f_up-th as an upper threshold,
    factors in [1, 255]; include/jvae_hip.h says how this differs from the reference's spline); an int32 device tensor of the
    mode words of include/jvae_hip.h (`roc_mode_word`) is accepted.  A bare tuple such as (4, 1) is read as per-row values.
    -> dict of DEVICE tensors: 'auc' (M,), 'fpr' / 'tpr' / 'low' / 'up' (M, K) fp64 and 'status' (M,) int32 (bit 0: NaN score,
    bit 1: non-finite in-score of an around-mean row, bit 2: malformed mode word in a tensor; `roc_check_status` raises on
    them).  (n,) inputs drop the M axis.
    Nothing is synchronised or copied to the host."""
    lib = L.load()
    single = ins.dim() == 1
    ins, outs = _c(_f32(ins, 'roc_curve')), _c(_f32(outs, 'roc_curve'))
    L.ptr(ins), L.ptr(outs)                                    # off the GPU: JvaeHipError, before anything else is looked at
    if single:
        ins, outs = ins[None], outs[None]
    if ins.dim() != 2 or outs.dim() != 2 or ins.shape[0] != outs.shape[0] or ins.shape[1] < 1 or outs.shape[1] < 1:
        raise L.JvaeHipError(f'roc_curve: (M, n_in) and (M, n_out) score rows expected, got {tuple(ins.shape)} and {tuple(outs.shape)}')
    M, n_in, n_out, dev = ins.shape[0], ins.shape[1], outs.shape[1], ins.device
    if torch.is_tensor(kept_tpr):
        kept = _c(kept_tpr.to(device=dev, dtype=torch.float64))
    else:
        kept = torch.tensor(sorted(float(t) for t in kept_tpr), dtype=torch.float64, device=dev)
    modes = _roc_modes(two_sided, M, dev, 'roc_curve')
    K = kept.numel()
    out = torch.empty((4, M, max(K, 1)), dtype=torch.float64, device=dev)
    auc = torch.empty(M, dtype=torch.float64, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    nbytes = lib.jvae_roc_workspace_bytes(M, n_in, n_out)
    if not nbytes:
        raise L.JvaeHipError(f'roc_curve: sizes out of range (M={M}, n_in={n_in}, n_out={n_out})')
    ws = L.workspace(nbytes, dev)
    rc = lib.jvae_roc_curve_f32(L.ptr(ins), L.ptr(outs), L.ptr(kept), L.ptr(modes), L.ptr(auc), L.ptr(out[0]), L.ptr(out[1]),
                                L.ptr(out[2]), L.ptr(out[3]), L.ptr(status), M, n_in, n_out, K, L.ptr(ws), ws.numel(),
                                L.stream_ptr())
    L.check(rc, 'jvae_roc_curve_f32')
    res = {'auc': auc, 'fpr': out[0, :, :K], 'tpr': out[1, :, :K], 'low': out[2, :, :K], 'up': out[3, :, :K], 'status': status}
    return {k: v[0] for k, v in res.items()} if single else res


def _roc_modes(two_sided, M, dev, what):
    """The `two_sided` argument of `roc_curve` / `pr_metrics` -> (M,) int32 mode words on the device."""
    if torch.is_tensor(two_sided):
        modes = _c(two_sided.to(device=dev, dtype=torch.int32))
    else:
        for_all = not isinstance(two_sided, (list, tuple)) or two_sided[:1] == ('quantile',)
        rows = [two_sided] * M if for_all else list(two_sided)
        modes = torch.tensor([roc_mode_word(t) for t in rows], dtype=torch.int32, device=dev)
    if modes.numel() != M:
        raise L.JvaeHipError(f'{what}: {modes.numel()} modes for {M} rows')
    return modes


def roc_mode_word(t):
    """One row's `two_sided` value -> its int32 mode word (include/jvae_hip.h): 0 one-sided, 1 'around-mean',
    2 | f_low << 8 | f_up << 16 for ('quantile', f_low, f_up)."""
    if isinstance(t, tuple) and t[:1] == ('quantile',):
        if len(t) != 3 or any(isinstance(f, bool) or not isinstance(f, int) or not 1 <= f <= 255 for f in t[1:]):
            raise L.JvaeHipError(f'roc_curve: two_sided={t!r}: two integer factors in [1, 255] expected')
        return 2 | t[1] << 8 | t[2] << 16
    if isinstance(t, tuple) or t not in (False, True, 0, 1, None, 'around-mean'):
        raise NotImplementedError(f'roc_curve: two_sided={t!r} (the spline thresholds of the reference are not built)')
    return 1 if t == 'around-mean' else 0


PR_FIGURES = ('aupr_in', 'aupr_out', 'aucpr_in', 'aucpr_out', 'dete')


def pr_metrics(ins, outs, two_sided=False):
    """The precision-recall side of M score rows in one call (csrc/prc.hip): AUPR-in and AUPR-out (scikit-learn's
    average_precision_score with in, resp. out and the negated score, as the positive class), the trapezoid AUCPR of both
    (auc(recall, precision) of precision_recall_curve) and the smallest detection error over all thresholds,
    min 0.5 (1 - tpr) + 0.5 fpr.  ins, outs and two_sided as for `roc_curve`; with 'around-mean' the score of a sample is
    -|s - mean(ins)|; a ('quantile', f_low, f_up) row has no scalar score and gets NaN figures.
    -> dict of DEVICE tensors: the five PR_FIGURES (M,) fp64 and 'status' (M,) int32 with the bits of `roc_curve`
    (`roc_check_status` reads it).  (n,) inputs drop the M axis.  Nothing is synchronised or copied to the host."""
    lib = L.load()
    single = ins.dim() == 1
    ins, outs = _c(_f32(ins, 'pr_metrics')), _c(_f32(outs, 'pr_metrics'))
    L.ptr(ins), L.ptr(outs)                                    # off the GPU: JvaeHipError, before anything else is looked at
    if single:
        ins, outs = ins[None], outs[None]
    if ins.dim() != 2 or outs.dim() != 2 or ins.shape[0] != outs.shape[0] or ins.shape[1] < 1 or outs.shape[1] < 1:
        raise L.JvaeHipError(f'pr_metrics: (M, n_in) and (M, n_out) score rows expected, got {tuple(ins.shape)} and {tuple(outs.shape)}')
    M, n_in, n_out, dev = ins.shape[0], ins.shape[1], outs.shape[1], ins.device
    modes = _roc_modes(two_sided, M, dev, 'pr_metrics')
    figures =torch.empty((M, len(PR_FIGURES)), dtype=torch.float64, device=dev)
    status = torch.empty(M, dtype=torch.int32, device=dev)
    nbytes = lib.jvae_pr_workspace_bytes(M, n_in, n_out)
    if not nbytes:
        raise L.JvaeHipError(f'pr_metrics: sizes out of range (M={M}, n_in={n_in}, n_out={n_out})')
    ws = L.workspace(nbytes, dev)
    L.check(lib.jvae_pr_metrics_f32(L.ptr(ins), L.ptr(outs), L.ptr(modes), L.ptr(figures), L.ptr(status), M, n_in, n_out,
                                    L.ptr(ws), ws.numel(), L.stream_ptr()), 'jvae_pr_metrics_f32')
    res = dict({k: figures[:, j] for j, k in enumerate(PR_FIGURES)}, status=status)
    return {k: v[0] for k, v in res.items()} if single else res


def roc_check_status(status):
    """Raise for the rows `roc_curve` flagged (host values of its 'status' word): JvaeHipError for a malformed mode word,
    ValueError for what the scores hold."""
    for m, s in enumerate(status if hasattr(status, '__len__') else [status]):
        if int(s) & 4:
            raise L.JvaeHipError(f'roc_curve: malformed mode word in row {m}')
        if int(s) & 1:
            raise ValueError(f'roc_curve: NaN score in row {m}')
        if int(s) & 2:
            raise ValueError(f'roc_curve: non-finite in-distribution score in around-mean row {m}')


def read_back(fields):
    """{name: device tensor} -> {name: fp64 numpy array of that tensor's shape}, in ONE copy to the host: every field is widened
    to fp64 (exact for fp64 and fp32 values and for the int32 status words and counts), flattened and concatenated on the device,
    and the host copy is cut by numel() and reshaped."""
    host = torch.cat([v.double().reshape(-1) for v in fields.values()]).cpu().numpy()
    ends = np.cumsum([v.numel() for v in fields.values()]).tolist()
    return {k: host[end - v.numel():end].reshape(tuple(v.shape)) for (k, v), end in zip(fields.items(), ends)}


# ------------------------------------------------------------------------------------------- status words, aligned workspace
# ONE mechanism for the device status words of the flagging ops: a family ('wim', 'knn', 'maha', 'ic', 'ssim', 'kde', 'aggpost') has one
# default word per device for the calls made without a word of their own; an op takes its word through `_status_word`, a
# family's `X_check_status` reads through `_read_status` and raises for its own bits.
_status = {}                 # (family, device index) -> the int32 default word, created cleared on first use


def _status_word(family, device, status=None, what=None, noun=None):
    """The word an op hands to its kernel: the family's default word on `device`, or the caller's `status` - an int32 tensor with
    at least one element on that device, else JvaeHipError in the name of the op `what`, whose inputs are the `noun`."""
    if status is None:
        key = family, device.index if device.index is not None else torch.cuda.current_device()
        if key not in _status:
            _status[key] = torch.zeros(1, dtype=torch.int32, device=device)
        return _status[key]
    if not torch.is_tensor(status) or status.dtype != torch.int32 or status.numel() < 1 or status.device != device:
        raise L.JvaeHipError(f'{what}: an int32 status word on the device of the {noun} expected')
    return status


def _read_status(family, status=None):
    """status: the word given to an op (a tensor: read here - this is the synchronisation - and cleared when it was not zero), a
    host value, or None for every default word of the family -> the OR of what was read.  Every word is read and cleared before
    the caller raises anything."""
    words = [w for (f, _), w in _status.items() if f == family] if status is None else [status]
    seen = 0
    for w in words:
        v = int(w.reshape(-1)[0]) if torch.is_tensor(w) else int(w)
        if torch.is_tensor(w) and v:
            w.zero_()
        seen |= v
    return seen


def _aligned_ws(nbytes, device, align=8, what=None):
    """(pointer, bytes) of at least `nbytes` of the stream's workspace from an `align`-byte boundary on.  With `what`, the name
    of an op whose library call answers 0 bytes for sizes out of range, that answer is refused here."""
    if what and not nbytes:
        raise L.JvaeHipError(f'{what}: sizes out of range (unsupported configuration)')
    ws = L.workspace(nbytes + align, device)
    off = (-ws.data_ptr()) % align
    return ws.data_ptr() + off, ws.numel() - off


# ------------------------------------------------------------------------------------------- SCOD risk curves (csrc/scod.hip)
SCOD_R_KINDS = {None: -1, 'zero': 0, 'half_y': 1, 'logmsp': 2, 'odin': 3}
SCOD_G_KINDS = {None: -1, 'zero': 0, 'half': 1, 'neg': 2, 'plain': 3}
SCOD_MAX_ROWS = 32           # variants per launch (more are dealt to further launches)
SCOD_MAX_N = 1 << 24         # ROC_MAX_N of csrc/roc_sort.h: counts are exact in fp32 below it
SCOD_FIGURES = ('fpr95', 'sr95', 'auroc', 'aust', 'auscodt')


def scod_scores(specs, y_est, C, N, out=None, col=0, status=None):
    """The SCOD score rows r + weight * g of M variants of one recorded set in ONE launch per 32 variants (tests/scod.py:60-144 of
    the reference; csrc/scod.hip).  specs: M tuples (r_kind, r_src, r_aux, g_kind, g_src, g_alt, weight) - r_kind in
    SCOD_R_KINDS: 'zero' 0., 'half_y' 0.5 * r_src[y_est] (r_src (C, N)), 'logmsp' 0.5 * r_src[y_est] - r_aux (r_aux (N,), the
    class-axis logsumexp(-0.5 r_src) the caller took with torch), 'odin' 1 - r_src (r_src (N,)); g_kind in SCOD_G_KINDS: 'zero'
    0., 'half' / 'neg' / 'plain': 0.5 / -1 / 1 times (g_src[y_est] - g_alt), g_src (C, N), g_alt (N,) or (R, N) (its row 0);
    a kind None: the row is the other side alone.  Tensors a kind does not read may be None.  y_est (N,) int64 or None when no
    kind gathers.  out: a dense (>= M, >= col + N) fp32 device buffer whose rows 0 .. M - 1 are written at columns col .. col + N;
    without: a new (M, N) tensor.  Each operation is rounded on its own (the torch expressions bit for bit).  status as for
    `wim_scores`: set to 1 when a label is outside [0, C) (that sample is NaN); `wim_check_status` raises on it."""
    M = len(specs)
    dev = None
    rows = []
    for rk, r_src, r_aux, gk, g_src, g_alt, weight in specs:
        if rk not in SCOD_R_KINDS or gk not in SCOD_G_KINDS or (rk is None and gk is None):
            raise L.JvaeHipError(f'scod_scores: unknown variant ({rk!r}, {gk!r})')
        need = {'r_src': (r_src, SCOD_R_KINDS[rk] > 0, (N,) if rk == 'odin' else (C, N)), 'r_aux': (r_aux, rk == 'logmsp', (N,)),
                'g_src': (g_src, SCOD_G_KINDS[gk] > 0, (C, N)), 'g_alt': (g_alt, SCOD_G_KINDS[gk] > 0, (N,))}
        ptrs = []
        for name, (t, used, shape) in need.items():
            if not used:
                ptrs.append(None)
                continue
            if t is None:
                raise L.JvaeHipError(f'scod_scores: ({rk!r}, {gk!r}) needs {name}')
            if name == 'g_alt' and t.dim() == 2:
                t = t[0]
            t = _c(_f32(t, 'scod_scores'))
            L.ptr(t)
            if tuple(t.shape) != shape or (dev is not None and t.device != dev):
                raise L.JvaeHipError(f'scod_scores: {name} of shape {shape} on one device expected, got {tuple(t.shape)} on {t.device}')
            dev = t.device
            ptrs.append(t)
        rows.append((ptrs, SCOD_R_KINDS[rk], SCOD_G_KINDS[gk], float(weight)))
    gathers = any(rk in (1, 2) or gk > 0 for _, rk, gk, _ in rows)
    if y_est is not None:
        L.ptr(y_est)
        dev = dev or y_est.device
        if y_est.dtype != torch.int64 or tuple(y_est.shape) != (N,) or y_est.device != dev:
            raise L.JvaeHipError(f'scod_scores: ({N},) int64 labels on {dev} expected, got {tuple(y_est.shape)} {y_est.dtype}')
        y_est = _c(y_est)
    elif gathers:
        raise L.JvaeHipError('scod_scores: the variants gather at the estimated labels: y_est expected')
    if dev is None:
        dev = out.device if out is not None else torch.device('cuda', torch.cuda.current_device())
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
    col = int(col)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < M or not 0 <= col <= out.shape[1] - N \
            or not out.is_contiguous() or out.device != dev:
        raise L.JvaeHipError(f'scod_scores: a dense (>= {M}, >= {col} + {N}) fp32 buffer on {dev} expected')
    L.ptr(out)
    status = _status_word('wim', dev, status, 'scod_scores', 'sources')
    lib = L.load()
    for m0 in range(0, M, SCOD_MAX_ROWS):
        part = rows[m0:m0 + SCOD_MAX_ROWS]
        n = len(part)
        arrays = [(ctypes.c_void_p * n)(*[None if p[j] is None else p[j].data_ptr() for p, _, _, _ in part]) for j in range(4)]
        kinds = (ctypes.c_int * (2 * n))(*[k for _, rk, gk, _ in part for k in (rk, gk)])
        weights = (ctypes.c_float * n)(*[w for _, _, _, w in part])
        L.check(lib.jvae_scod_scores_f32(*arrays, kinds, weights, L.ptr(y_est), out.data_ptr() + 4 * (m0 * out.shape[1] + col),
                                         out.shape[1], n, int(C), int(N), L.ptr(status), L.stream_ptr()), 'jvae_scod_scores_f32')
    return out[:M, col:col + N]


def scod_curve(scores, y_true, y_est, curves=True, figures=True, n_in=None):
    """The SCOD risk curves of M score rows in one call (scrisk and the figures of the reference's tests/scod.py; csrc/scod.hip).
    scores (M, n) or (n,) fp32 on the device, the HIGHer the more likely to reject; y_true (n,) int64: the class of an
    in-distribution sample, negative for an OOD one; y_est (n,) int64.  Each row is sorted ascending (stable by position) and
    scanned.  -> dict of DEVICE tensors: with `curves` 'tpr', 'selective_risk', 'fpr' (M, n) fp32 - the reference's, bit for bit
    on tie-free scores; with `figures` 'figures' (M, 5) fp64 in the order of SCOD_FIGURES: the minimum of fpr / selective_risk
    over tpr >= 0.95 and the trapezoid areas AuROC, AuST, AuSCODT, summed in fp64 in a fixed order; 'status' (M,) int32, bit 0:
    NaN score, bit 1: `n_in` is not the number of non-negative y_true (`scod_check_status` raises on them).  (n,) scores drop
    the M axis.  n_in: the number of in-distribution samples when the caller knows it - nothing is then read back or
    synchronised; None: counted here, which reads one value back.  An empty in or OOD side (the reference returns NaN curves),
    n > SCOD_MAX_N, scores that are not fp32 or not on the device: JvaeHipError before any launch."""
    lib = L.load()
    single = scores.dim() == 1
    _f32(scores, 'scod_curve')
    for t in (scores, y_true, y_est):                          # off the GPU: JvaeHipError, before anything else is looked at
        if not t.is_cuda:
            raise L.JvaeHipError(f'scod_curve: tensors resident on the GPU expected (no CPU fallback); got device {t.device}')
    if single:
        scores = scores[None]
    if scores.dim() != 2 or scores.shape[0] < 1:
        raise L.JvaeHipError(f'scod_curve: (M, n) score rows expected, got {tuple(scores.shape)}')
    M, n = scores.shape
    dev = scores.device
    for name, y in (('y_true', y_true), ('y_est', y_est)):
        if y.dtype != torch.int64 or tuple(y.shape) != (n,) or y.device != dev:
            raise L.JvaeHipError(f'scod_curve: {name}: ({n},) int64 on {dev} expected, got {tuple(y.shape)} {y.dtype} on {y.device}')
    if not (curves or figures):
        raise L.JvaeHipError('scod_curve: nothing asked for')
    if n > SCOD_MAX_N or M > 65535:
        raise L.JvaeHipError(f'scod_curve: sizes out of range (M={M}, n={n}, at most {SCOD_MAX_N} samples)')
    if n_in is None:
        n_in = int((y_true >= 0).sum())
    n_in = int(n_in)
    if n_in < 1 or n_in >= n:
        raise L.JvaeHipError(f'scod_curve: {n_in} in-distribution and {n - n_in} OOD samples: neither side may be empty')
    scores, y_true, y_est = _c(scores), _c(y_true), _c(y_est)
    out = torch.empty((3, M, n), dtype=torch.float32, device=dev) if curves else None
    fig = torch.empty((M, len(SCOD_FIGURES)), dtype=torch.float64, device=dev) if figures else None
    status = torch.empty(M, dtype=torch.int32, device=dev)
    nbytes = lib.jvae_scod_workspace_bytes(M, n)
    if not nbytes:
        raise L.JvaeHipError(f'scod_curve: sizes out of range (M={M}, n={n})')
    ws = L.workspace(nbytes, dev)
    rc = lib.jvae_scod_curve_f32(L.ptr(scores), L.ptr(y_true), L.ptr(y_est), L.ptr(out), L.ptr(fig), L.ptr(status), M, n, n_in,
                                 L.ptr(ws), ws.numel(), L.stream_ptr())
    L.check(rc, 'jvae_scod_curve_f32')
    res = {'status': status}
    if curves:
        res.update(tpr=out[0], selective_risk=out[1], fpr=out[2])
    if figures:
        res['figures'] = fig
    return {k: v[0] for k, v in res.items()} if single else res


def scod_check_status(status):
    """Raise for the rows `scod_curve` flagged (host values of its 'status' word: a tensor, a list or one value)."""
    for m, s in enumerate(torch.as_tensor(status).reshape(-1).tolist()):
        if int(s) & 1:
            raise ValueError(f'scod_curve: NaN score in row {m}')
        if int(s) & 2:
            raise L.JvaeHipError(f'scod_curve: n_in is not the number of in-distribution samples of y_true (row {m})')


# ------------------------------------------------------------------------------------------- misclassification (csrc/misclass.hip)
MISCLASS_KINDS = {'soft-': 0, 'soft+': 1, 'max-': 2, 'max+': 3, 'hyz': 4, 'lse-': 5, 'lse+': 6, 'mean': 7, 'std': 8, 'nstd': 9,
                  'mag': 10, 'IYx': 11, 'neg': 12, 'id': 13}
MISCLASS_MAX_CLASSES = 128
MISCLASS_MAX_KEPT = 16


def _mask_u8(mask, N, what):
    if mask.dim() != 1 or mask.numel() != N:
        raise L.JvaeHipError(f'{what}: a mask of {N} samples expected, got {tuple(mask.shape)}')
    return _c(mask if mask.dtype == torch.uint8 else (mask != 0).to(torch.uint8))


def _rows_into(out, rows, col, R, N, dev, what):
    """The `out` / `rows` / `col` arguments of the score-row ops, checked -> (out, rows, col): a new (R, N) buffer without `out`,
    else columns col .. col + N of R distinct rows of a dense fp32 (M, n) buffer on `dev`."""
    if out is None:
        out, rows = torch.empty((R, N), dtype=torch.float32, device=dev), range(R)
    rows, col = [int(r) for r in rows], int(col)
    if out.dtype != torch.float32 or out.dim() != 2 or not 0 <= col <= out.shape[1] - N or not out.is_contiguous() \
            or out.device != dev or len(rows) != R or len(set(rows)) != R or any(not 0 <= r < out.shape[0] for r in rows):
        raise L.JvaeHipError(f'{what}: a dense (M, >= {col} + {N}) fp32 buffer and {R} distinct rows inside it expected')
    return out, rows, col


_misclass_specs = {}         # (kinds, constants, rows, device) -> their three device arrays: a pass repeats one launch per batch


def misclass_scores(src, specs, out=None, rows=None, col=0):
    """Score rows of one (C, N) fp32 source (all-class losses, or the logits as the recorder stores them) in ONE launch.
    specs: [(kind, T)] with kind in MISCLASS_KINDS - 'soft-': max_c softmax_c(-v / T), 'soft+': max_c softmax_c(v / T),
    'max-': max_c(-v), 'max+': max_c v, 'hyz': sum_c p log p with p = softmax_c(v / T) (batch_dist_measures, cvae.py:1024-1063).
    The class-axis rows of cvae.py:985-1068, with l = -v, d = l - max_c l, e = exp d; their T is not a temperature - 'lse-':
    log sum_c e + max_c l + T (`sum`: T = 0), 'lse+': the same on l = v (all-class `iws`: T = log C), 'mean': log mean_c e +
    max_c l, 'std': torch.std of l over the classes (C = 1: NaN), 'nstd': (std_c e / mean_c e)^2, 'mag': max_c l - torch.median
    of l, 'IYx': sum_c(d e) / (C mean_c e) - log mean_c e; the other new kinds ignore T.  'neg' / 'id': -v / v of a (1, N) source.
    out (M, n >= col + N) fp32 on the source's device with `rows` = the row of each spec, all distinct: columns col .. col + N of
    those rows are written in place; without: a new (len(specs), N) tensor.  C <= 128."""
    src = _c(_f32(src, 'misclass_scores'))
    L.ptr(src)
    if src.dim() != 2 or not 1 <= src.shape[0] <= MISCLASS_MAX_CLASSES:
        raise L.JvaeHipError(f'misclass_scores: a (C, N) source with C <= {MISCLASS_MAX_CLASSES} expected, got {tuple(src.shape)}')
    C, N = src.shape
    R, dev = len(specs), src.device
    out, rows, col = _rows_into(out, rows, col, R, N, dev, 'misclass_scores')
    for kind, T in specs:
        if kind not in MISCLASS_KINDS or not (float(T) > 0 if MISCLASS_KINDS[kind] < 5 else math.isfinite(float(T))):
            raise L.JvaeHipError(f'misclass_scores: unknown row ({kind!r}, {T!r})')
        if kind in ('neg', 'id') and C != 1:
            raise L.JvaeHipError(f'misclass_scores: {kind!r} is a row of a (1, N) source, got {tuple(src.shape)}')
    if R and N:
        key = (tuple(MISCLASS_KINDS[k] for k, _ in specs), tuple(float(T) for _, T in specs), tuple(rows), dev)
        if key not in _misclass_specs:
            if len(_misclass_specs) >= 256:
                _misclass_specs.clear()
            _misclass_specs[key] = (torch.tensor(key[0], dtype=torch.int32, device=dev),
                                    torch.tensor(key[1], dtype=torch.float32, device=dev),
                                    torch.tensor(key[2], dtype=torch.int32, device=dev))
        kinds, temps, rows_d = _misclass_specs[key]
        L.ptr(out)
        L.check(L.load().jvae_misclass_scores_f32(L.ptr(src), L.ptr(kinds), L.ptr(temps), L.ptr(rows_d), out.data_ptr() + 4 * col,
                                                  R, C, N, out.shape[1], L.stream_ptr()), 'jvae_misclass_scores_f32')
    return out


# ------------------------------------------------------------------------------------------- WIM score rows (csrc/wim.hip)
WIM_KINDS = {'Y': 0, 'SOFT_Y': 1, 'LSE_AT': 2, 'Y_AT': 3}
WIM_MAX_SOURCES = 4


def wim_status(device):
    """The per-device status word of `wim_scores` calls made without one of their own (created cleared, on first use)."""
    return _status_word('wim', device)


def wim_scores(sources, y_est, specs, out=None, rows=None, col=0, status=None):
    """Every WIM score row of a batch in ONE launch (ft/wim.py:132-201).  sources: up to 4 triples (src, f, alt) - src a (C, N)
    fp32 all-class loss, f its factor (-1 kl, -1/2 zdist, +1 iws, -1 on `total` for elbo), alt the (N,) fp32 loss under the
    alternate prior or None; y_est (N,) int64; specs: [(source index, kind)] with kind in WIM_KINDS and x = f * src -
    'Y': x[y_est], 'SOFT_Y': softmax_c(x)[y_est], 'LSE_AT': logsumexp_c(x) - f * alt, 'Y_AT': x[y_est] - f * alt.
    out / rows / col as for `misclass_scores`: columns col .. col + N of the given rows of a dense (M, n) fp32 buffer are written
    in place; without `out` a new (len(specs), N) tensor.  status: an int32 device word the kernel sets to 1 when a label is
    outside [0, C) (those samples' 'Y', 'SOFT_Y', 'Y_AT' values are NaN); default `wim_status(device)`; `wim_check_status`
    raises on it.  Nothing is synchronised.  C outside 1 .. MISCLASS_MAX_CLASSES: JvaeHipError (unsupported configuration)."""
    S, R = len(sources), len(specs)
    if not 1 <= S <= WIM_MAX_SOURCES:
        raise L.JvaeHipError(f'wim_scores: 1 .. {WIM_MAX_SOURCES} sources expected, got {S}')
    srcs = [_c(_f32(s, 'wim_scores')) for s, _, _ in sources]
    for s in srcs:
        L.ptr(s)
    if any(s.dim() != 2 or s.shape != srcs[0].shape for s in srcs):
        raise L.JvaeHipError(f'wim_scores: (C, N) sources of one shape expected, got {[tuple(s.shape) for s in srcs]}')
    C, N = srcs[0].shape
    dev = srcs[0].device
    alts = [None if a is None else _c(_f32(a, 'wim_scores')) for _, _, a in sources]
    if any(a is not None and (tuple(a.shape) != (N,) or a.device != dev) for a in alts):
        raise L.JvaeHipError(f'wim_scores: ({N},) alternate losses on {dev} expected')
    if y_est.dtype != torch.int64 or tuple(y_est.shape) != (N,) or y_est.device != dev:
        raise L.JvaeHipError(f'wim_scores: ({N},) int64 labels on {dev} expected, got {tuple(y_est.shape)} {y_est.dtype}')
    y_est = _c(y_est)
    out, rows, col = _rows_into(out, rows, col, R, N, dev, 'wim_scores')
    flat = []
    for (s, kind), r in zip(specs, rows):
        if kind not in WIM_KINDS or not 0 <= int(s) < S or (kind in ('LSE_AT', 'Y_AT') and alts[int(s)] is None):
            raise L.JvaeHipError(f'wim_scores: unknown row ({s!r}, {kind!r}) or no alternate loss for it')
        flat += [int(s), WIM_KINDS[kind], r]
    status = _status_word('wim', dev, status, 'wim_scores', 'sources')
    src_p = (ctypes.c_void_p * S)(*[s.data_ptr() for s in srcs])
    alt_p = (ctypes.c_void_p * S)(*[None if a is None else a.data_ptr() for a in alts])
    fac = (ctypes.c_float * S)(*[float(f) for _, f, _ in sources])
    spec = (ctypes.c_int * max(len(flat), 1))(*flat)
    L.check(L.load().jvae_wim_scores_f32(src_p, alt_p, fac, S, L.ptr(y_est), spec, R, out.data_ptr() + 4 * col, out.shape[1], C, N,
                                         L.ptr(status), L.stream_ptr()), 'jvae_wim_scores_f32')
    return out


def wim_check_status(status=None):
    """Raise JvaeHipError when a launch that takes a status word (`wim_scores`, `prior_sample`, `aggregate_scores` on votes) met
    a label outside [0, C).  status: the word given to the op (a device tensor: read here - this is the synchronisation - and
    cleared), a host value, or None for the per-device default words."""
    if _read_status('wim', status) & 1:
        raise L.JvaeHipError('a label outside [0, C) was met by wim_scores, prior_sample or aggregate_scores (the rows of '
                             'that sample are NaN)')


def group_tally(values, group, sums, counts):
    """sums (R, G) fp64 and counts (G,) int64, device accumulators of the caller, take this batch's per-group sums of the rows
    `values` (R, N) fp32 and the group sizes; group (N,) int32 in [0, G), anything else (negative: skip) leaves the sample out.
    One launch, fp64 sums in a fixed order, nothing synchronised (the fine-tuning loop's printed losses, ft/job.py:401-417)."""
    values = _c(_f32(values, 'group_tally'))
    if values.dim() != 2 or sums.dim() != 2 or counts.dim() != 1 or sums.shape[0] != values.shape[0] \
            or sums.shape[1] != counts.shape[0] or sums.dtype != torch.float64 or counts.dtype != torch.int64 \
            or group.dtype != torch.int32 or tuple(group.shape) != (values.shape[1],) \
            or any(t.device != values.device for t in (group, sums, counts)):
        raise L.JvaeHipError('group_tally: values (R, N) fp32, group (N,) int32, sums (R, G) fp64 and counts (G,) int64 on one '
                             'device expected')
    R, N = values.shape
    L.check(L.load().jvae_group_tally_f32(L.ptr(values), L.ptr(_c(group)), L.ptr(sums), L.ptr(counts), R, N, counts.shape[0],
                                          L.stream_ptr()), 'jvae_group_tally_f32')
    return sums, counts


# ------------------------------------------------------------------------- image generation (csrc/sample.hip)
SAMPLE_MODES = {'unit': 0, 'scalar': 1, 'diag': 2, 'full': 3}
GRID_KINDS = {'input': 0, 'draw': 1, 'average': 2}
GRID_MAX_COLUMNS = 1024


def prior_sample(eps, y, means, T, mode='unit', temperature=1., out=None, status=None):
    """Latent draws of a Gaussian prior from noise, ONE launch: eps (..., K) fp32, y (...) int64 labels or None (component 0),
    means (C, K), T the whitening factor ((C,), (C, K) or (C, K, K) by mode; unused by 'unit') -> z of eps's shape:
    'unit' means[y] + t eps (the reference's draw, module/sample.py:129-132) | 'scalar' / 'diag' means[y] + (t eps) / T[y(, k)]
    | 'full' means[y] + tril(T[y])^-1 (t eps).  The first three are the fp32 torch expressions bit for bit.  out: a dense fp32
    tensor of eps's shape to write into.  status as for `wim_scores`: bit 0 is set when a label is outside [0, C) (that row is
    NaN); default `wim_status(device)`, read and raised on by `wim_check_status`.  Nothing is synchronised."""
    if mode not in SAMPLE_MODES:
        raise L.JvaeHipError(f'prior_sample: mode {mode!r} unknown (one of {sorted(SAMPLE_MODES)})')
    eps = _c(_f32(eps, 'prior_sample'))
    means = _c(_f32(means, 'prior_sample'))
    L.ptr(eps)
    dev = eps.device
    if means.dim() != 2 or eps.dim() < 1 or eps.shape[-1] != means.shape[1] or means.device != dev:
        raise L.JvaeHipError(f'prior_sample: eps (..., K) and means (C, K) on one device expected, got {tuple(eps.shape)}, '
                             f'{tuple(means.shape)}')
    C, K = means.shape
    R = eps.numel() // K
    if mode != 'unit':
        T = _c(_f32(T, 'prior_sample'))
        want = {'scalar': (C,), 'diag': (C, K), 'full': (C, K, K)}[mode]
        if tuple(T.shape) != want or T.device != dev:
            raise L.JvaeHipError(f'prior_sample: a {want} factor on {dev} expected for mode {mode!r}, got {tuple(T.shape)}')
    else:
        T = None
    if y is not None:
        if y.dtype != torch.int64 or y.numel() != R or y.device != dev:
            raise L.JvaeHipError(f'prior_sample: {R} int64 labels on {dev} expected, got {tuple(y.shape)} {y.dtype}')
        y = _c(y)
    if out is None:
        out = torch.empty_like(eps)
    elif out.dtype != torch.float32 or out.shape != eps.shape or not out.is_contiguous() or out.device != dev:
        raise L.JvaeHipError(f'prior_sample: a dense fp32 output of shape {tuple(eps.shape)} on {dev} expected')
    status = _status_word('wim', dev, status, 'prior_sample', 'noise')
    L.check(L.load().jvae_prior_sample_f32(L.ptr(eps), L.ptr(y), L.ptr(means), L.ptr(T), L.ptr(out), L.ptr(status), R, K, C,
                                           float(temperature), SAMPLE_MODES[mode], L.stream_ptr()), 'jvae_prior_sample_f32')
    return out


def grid_columns(columns, device):
    """The column specs of `image_grid` in both forms the kernel takes: [('input',) | ('draw', a) | ('average', a, b)] ->
    (host ctypes array, (Ncol, 3) int32 device tensor).  Build once for a layout that is launched repeatedly."""
    flat = []
    for col in columns:
        kind = col[0]
        if kind not in GRID_KINDS or len(col) != {'input': 1, 'draw': 2, 'average': 3}[kind]:
            raise L.JvaeHipError(f'image_grid: column {col!r} is not (input,), (draw, a) or (average, a, b)')
        a = int(col[1]) if len(col) > 1 else 0
        flat += [GRID_KINDS[kind], a, int(col[2]) if len(col) > 2 else a]
    if not 1 <= len(columns) <= GRID_MAX_COLUMNS:
        raise L.JvaeHipError(f'image_grid: 1 .. {GRID_MAX_COLUMNS} columns expected, got {len(columns)}')
    host = (ctypes.c_int * len(flat))(*flat)
    return host, torch.tensor(flat, dtype=torch.int32, device=device).view(-1, 3)


def image_grid(x_in, x_out, columns, f32=True, u8=True):
    """The grid of images of module/sample.py in ONE launch.  x_in (N, D, H, W) or None, x_out (Rr, N, D, H, W) decoded rows,
    columns: a list [('input',) | ('draw', a) | ('average', a, b)] (x_in[n] | x_out[a, n] | the mean of x_out[a .. b, n], b
    included) or the pair `grid_columns` made of one -> (grid_f32 (D, N H, Ncol W) or None, grid_u8 (N H, Ncol W, D) uint8,
    channel last, or None): cell (n, c) is rows n H .. (n + 1) H, columns c W .. (c + 1) W.  The 8-bit value is
    floor(clamp(v * 255 + 0.5, 0, 255)) (torchvision's save_image), NaN -> 0; it needs D <= 4."""
    x_out = _c(_f32(x_out, 'image_grid'))
    L.ptr(x_out)
    dev = x_out.device
    if x_out.dim() != 5:
        raise L.JvaeHipError(f'image_grid: decoded rows (Rr, N, D, H, W) expected, got {tuple(x_out.shape)}')
    Rr, N, D, H, W = x_out.shape
    if x_in is not None:
        x_in = _c(_f32(x_in, 'image_grid'))
        if tuple(x_in.shape) != (N, D, H, W) or x_in.device != dev:
            raise L.JvaeHipError(f'image_grid: inputs {(N, D, H, W)} on {dev} expected, got {tuple(x_in.shape)}')
    host, specs = columns if isinstance(columns, tuple) and torch.is_tensor(columns[1]) else grid_columns(columns, dev)
    Ncol = specs.shape[0]
    if specs.dtype != torch.int32 or specs.device != dev or len(host) != 3 * Ncol:
        raise L.JvaeHipError('image_grid: column specs as made by grid_columns on the device of the rows expected')
    if not (f32 or u8):
        raise L.JvaeHipError('image_grid: nothing to write')
    gf = torch.empty((D, N * H, Ncol * W), dtype=torch.float32, device=dev) if f32 else None
    gu = torch.empty((N * H, Ncol * W, D), dtype=torch.uint8, device=dev) if u8 else None      # D > 4: the entry point refuses
    L.check(L.load().jvae_image_grid_f32(L.ptr(x_in), L.ptr(x_out), L.ptr(_c(specs)), host, Ncol, L.ptr(gf), L.ptr(gu), N, D, H, W,
                                         Rr, L.stream_ptr()), 'jvae_image_grid_f32')
    return gf, gu


# ------------------------------------------------------------------------- model ensembles (csrc/aggregate.hip)
AGG_MODES = {'mean': 0, 'joint': 1, 'mean_soft': 2, 'vote': 3}
AGG_MAX_SOURCES = 8
AGG_MAX_TEMPS = 16
AGG_MAX_K = 1024
AGG_NAN_TEMPS = (None, -1, 0)          # the reference's NAN_TEMPS: such a temperature passes the logits through


def _temps_array(temps, what, least=0):
    """Temperatures -> the host float array the entry points take (NaN for a temperature of AGG_NAN_TEMPS)."""
    temps = list(temps)
    if not least <= len(temps) <= AGG_MAX_TEMPS:
        raise L.JvaeHipError(f'{what}: {least} .. {AGG_MAX_TEMPS} temperatures expected, got {len(temps)}')
    vals = [float('nan') if any(t is n or (t is not None and n is not None and t == n) for n in AGG_NAN_TEMPS) else float(t)
            for t in temps]
    return (ctypes.c_float * max(len(vals), 1))(*vals)


def class_posterior(z, means, T, log_det, var_dim='scalar', temps=(1,), logp=True, post=True):
    """log p(z | c) of latent draws for EVERY class of a conditional Gaussian prior, and its soft-max over the classes, in ONE
    launch: z (..., K) fp32 (each row is read once), means (C, K), T the whitening factor ((C,), (C, K) or (C, K, K) by
    var_dim, the layout of GaussianPrior._var_parameter), log_det (C,) = log|Sigma_c| (GaussianPrior.log_det_per_class()) ->
    (logp (C, ...) or None, P (nT, C, ...) or None): logp = (-(K / 2) log 2 pi - u / 2) - log_det[c] / 2 with u the quadratic
    form of GaussianPrior.mahala, P[t] = softmax_c(logp / temps[t]) (a temperature of AGG_NAN_TEMPS: logp itself).  No tensor of
    C * rows * K elements is made.  C <= MISCLASS_MAX_CLASSES, K <= AGG_MAX_K.  Nothing is synchronised."""
    if var_dim not in VAR_KIND:
        raise L.JvaeHipError(f'class_posterior: var_dim {var_dim!r} unknown (one of {sorted(VAR_KIND)})')
    z, means = _c(_f32(z, 'class_posterior')), _c(_f32(means, 'class_posterior'))
    T, log_det = _c(_f32(T, 'class_posterior')), _c(_f32(log_det, 'class_posterior'))
    L.ptr(z)
    dev = z.device
    if means.dim() != 2 or z.dim() < 1 or z.shape[-1] != means.shape[1]:
        raise L.JvaeHipError(f'class_posterior: z (..., K) and means (C, K) expected, got {tuple(z.shape)}, {tuple(means.shape)}')
    C, K = means.shape
    want = {'scalar': (C,), 'diag': (C, K), 'full': (C, K, K)}[var_dim]
    if tuple(T.shape) != want or tuple(log_det.shape) != (C,) or any(t.device != dev for t in (means, T, log_det)):
        raise L.JvaeHipError(f'class_posterior: a {want} factor and ({C},) log-determinants on {dev} expected for var_dim '
                             f'{var_dim!r}, got {tuple(T.shape)}, {tuple(log_det.shape)}')
    if not 1 <= C <= MISCLASS_MAX_CLASSES or not 1 <= K <= AGG_MAX_K:
        raise L.JvaeHipError(f'class_posterior: 1 <= C <= {MISCLASS_MAX_CLASSES} and 1 <= K <= {AGG_MAX_K} expected, got C = {C}, '
                             f'K = {K}')
    if not (logp or post):
        raise L.JvaeHipError('class_posterior: nothing to write')
    tarr = _temps_array(temps if post else (), 'class_posterior', 1 if post else 0)
    nT = len(list(temps)) if post else 0
    lead = tuple(z.shape[:-1])
    R = z.numel() // K
    lp = torch.empty((C,) + lead, dtype=torch.float32, device=dev) if logp else None
    P = torch.empty((nT, C) + lead, dtype=torch.float32, device=dev) if post else None
    L.check(L.load().jvae_class_posterior_f32(L.ptr(z), L.ptr(means), L.ptr(T), L.ptr(log_det), tarr, nT, L.ptr(lp), L.ptr(P), R, K,
                                              C, VAR_KIND[var_dim], L.stream_ptr()), 'jvae_class_posterior_f32')
    return lp, P


def latent_mutual_info(P0, P1):
    """Pairwise latent mutual information of two models' class posteriors: P0 (nT, C, L0, N), P1 (nT, C, L1, N) fp32 ->
    Im (nT, N), Im[t, n] = 1 / (L0 L1) sum_{a, b} log sum_c P0[t, c, a, n] P1[t, c, b, n] (reference
    module/aggregation.py::compute_latent_mutual_info without its (C, L1, L0, N) tensors).  The logs are added in fp64 in a
    fixed order; a pair of draws with no class in common (class sum exactly 0) makes its sample -inf.  The only allocation
    beside Im is nT * ceil(L0 / 4) * N fp64 partial sums.  Nothing is synchronised."""
    P0, P1 = _c(_f32(P0, 'latent_mutual_info')), _c(_f32(P1, 'latent_mutual_info'))
    L.ptr(P0)
    L.ptr(P1)
    if P0.dim() != 4 or P1.dim() != 4 or P0.shape[:2] != P1.shape[:2] or P0.shape[3] != P1.shape[3] or P0.device != P1.device:
        raise L.JvaeHipError(f'latent_mutual_info: (nT, C, L0, N) and (nT, C, L1, N) on one device expected, got '
                             f'{tuple(P0.shape)}, {tuple(P1.shape)}')
    nT, C, L0, N = P0.shape
    L1 = P1.shape[2]
    if not 1 <= nT <= AGG_MAX_TEMPS or not 1 <= C <= MISCLASS_MAX_CLASSES or L0 < 1 or L1 < 1:
        raise L.JvaeHipError(f'latent_mutual_info: 1 <= nT <= {AGG_MAX_TEMPS}, 1 <= C <= {MISCLASS_MAX_CLASSES} and at least one '
                             f'draw per model expected, got {tuple(P0.shape)}, {tuple(P1.shape)}')
    lib = L.load()
    Im = torch.empty((nT, N), dtype=torch.float32, device=P0.device)
    nbytes = lib.jvae_latent_mi_workspace_bytes(nT, L0, N)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=P0.device)
    L.check(lib.jvae_latent_mi_f32(L.ptr(P0), L.ptr(P1), L.ptr(Im), nT, C, L0, L1, N, L.ptr(ws), ws.numel() * 8, L.stream_ptr()),
            'jvae_latent_mi_f32')
    return Im


def aggregate_scores(sources, mode, factors=None, temps=(), post=True, a=False, amax=False, argmax=False, slot=None,
                     num_classes=None, status=None):
    """The ensemble rows of several models' recorded scores in ONE launch (reference results/aggregation.py:321-374).
    sources: 1 .. 8 (C, N) fp32 tensors x_e - for mode 'vote' (N,) int64 predicted classes and `num_classes` = C;
    factors: one float per source (or one for all; default 1).  mode, with a the (C, N) aggregated row:
    'mean': a = log_mean_exp_e(f x_e) | 'joint': a = f sum_e x_e (ascending e) | 'mean_soft': no a, post[t] = mean_e
    softmax_c(f x_e / T_t) ((sum_e f x_e) / E for a temperature of AGG_NAN_TEMPS) | 'vote': a = count_c / E.
    -> (post, a, amax, argmax), None where not asked for: post (nT, C, N) = softmax_c(a / T_t), a itself for a temperature of
    AGG_NAN_TEMPS and for votes; amax (N,) fp32 and argmax (N,) int64 of slot `slot` of post (None: of a) - equal maxima give
    the lowest class, a NaN is kept.  status as for `wim_scores`: bit 0 is set when a vote is outside [0, C) (that sample is
    NaN); default `wim_status(device)`, read and raised on by `wim_check_status`.  Nothing is synchronised."""
    if mode not in AGG_MODES:
        raise L.JvaeHipError(f'aggregate_scores: mode {mode!r} unknown (one of {sorted(AGG_MODES)})')
    sources = list(sources)
    E = len(sources)
    if not 1 <= E <= AGG_MAX_SOURCES:
        raise L.JvaeHipError(f'aggregate_scores: 1 .. {AGG_MAX_SOURCES} sources expected, got {E}')
    vote = mode == 'vote'
    for s in sources:
        if not s.is_cuda:
            L.ptr(s)                   # raises: no CPU fallback
    dev = sources[0].device
    if vote:
        if num_classes is None:
            raise L.JvaeHipError('aggregate_scores: votes need num_classes')
        if any(s.dtype != torch.int64 or s.dim() != 1 or s.shape != sources[0].shape or s.device != dev for s in sources):
            raise L.JvaeHipError(f'aggregate_scores: (N,) int64 votes of one length on {dev} expected, got '
                                 f'{[(tuple(s.shape), s.dtype) for s in sources]}')
        C, N = int(num_classes), sources[0].shape[0]
    else:
        if any(s.dim() != 2 or s.shape != sources[0].shape or s.device != dev for s in sources):
            raise L.JvaeHipError(f'aggregate_scores: (C, N) sources of one shape on {dev} expected, got '
                                 f'{[tuple(s.shape) for s in sources]}')
        sources = [_f32(s, 'aggregate_scores') for s in sources]
        C, N = sources[0].shape
    sources = [_c(s) for s in sources]
    if not 1 <= C <= MISCLASS_MAX_CLASSES:
        raise L.JvaeHipError(f'aggregate_scores: 1 <= C <= {MISCLASS_MAX_CLASSES} expected, got {C}')
    if factors is None:
        factors = [1.] * E
    elif not isinstance(factors, (list, tuple)):
        factors = [float(factors)] * E
    if len(factors) != E or (mode == 'joint' and any(float(f) != float(factors[0]) for f in factors)):
        raise L.JvaeHipError(f'aggregate_scores: {E} factors expected (one value for mode joint), got {factors!r}')
    temps = list(temps)
    tarr = _temps_array(temps, 'aggregate_scores', 1 if post else 0)
    nT = len(temps)
    if slot is None:
        slot = -1
    if not -1 <= int(slot) < nT or not (post or a or amax or argmax) or (mode == 'mean_soft' and (a or ((amax or argmax) and slot < 0))):
        raise L.JvaeHipError(f'aggregate_scores: nothing to write, slot {slot} outside the {nT} temperatures, or the aggregated '
                             'row of mode mean_soft (it has none) asked for')
    status = _status_word('wim', dev, status, 'aggregate_scores', 'sources')
    o_post = torch.empty((nT, C, N), dtype=torch.float32, device=dev) if post else None
    o_a = torch.empty((C, N), dtype=torch.float32, device=dev) if a else None
    o_max = torch.empty((N,), dtype=torch.float32, device=dev) if amax else None
    o_arg = torch.empty((N,), dtype=torch.int64, device=dev) if argmax else None
    src_p = (ctypes.c_void_p * E)(*[s.data_ptr() for s in sources])
    fac = (ctypes.c_float * E)(*[float(f) for f in factors])
    L.check(L.load().jvae_aggregate_scores_f32(src_p, fac, E, AGG_MODES[mode], tarr, nT, L.ptr(o_post), L.ptr(o_a), L.ptr(o_max),
                                               L.ptr(o_arg), int(slot), C, N, L.ptr(status), L.stream_ptr()),
            'jvae_aggregate_scores_f32')
    return o_post, o_a, o_max, o_arg


# ------------------------------------------------------------------------- chained models (csrc/cascad.hip)
CASCADE_MAX_MODELS = 8


def cascade_mse(x, stages):
    """The mean squared errors of EVERY pair of stages of a cascade in ONE pass (reference module/cascad.py::evaluate, which
    forms them pair by pair): x (N, ...) fp32 is stage 0, stages 1 .. 8 tensors R_1 .. R_M of one shape (L, N, ...) - the sampled
    reconstructions x_reco[1:] of the models, taken as the views they are: contiguous, any 4-byte aligned base, never copied ->
    mse (M (M + 1) / 2, N), row p = i (i - 1) / 2 + j for 1 <= i <= M, 0 <= j < i (`for i: for j < i`):
    mse[p, n] = mean over l and the image axes of (R_i[l, n] - R_j[l, n])^2, R_0[l] = x.  Every stage element is loaded once;
    differences, squares and sums in fp64 in an order (L, D) fixes.  The only allocation beside mse is
    ceil(D / 256) * M (M + 1) / 2 * N fp64 partial sums.  Nothing is synchronised."""
    stages = list(stages)
    M = len(stages)
    if not 1 <= M <= CASCADE_MAX_MODELS:
        raise L.JvaeHipError(f'cascade_mse: 1 .. {CASCADE_MAX_MODELS} stages expected, got {M}')
    for t in [x] + stages:
        _f32(t, 'cascade_mse')
        L.ptr(t)                       # raises on a CPU or a strided tensor: no CPU fallback, no hidden copy
    if x.dim() < 1 or any(s.dim() != x.dim() + 1 or s.shape != stages[0].shape or s.device != x.device for s in stages) \
            or tuple(stages[0].shape[1:]) != tuple(x.shape):
        raise L.JvaeHipError(f'cascade_mse: x (N, ...) and stages of one shape (L, N, ...) on one device expected, got '
                             f'{tuple(x.shape)} and {[tuple(s.shape) for s in stages]}')
    Ls, N = stages[0].shape[0], x.shape[0]
    D = math.prod(x.shape[1:])
    if Ls < 1 or D < 1:
        raise L.JvaeHipError(f'cascade_mse: at least one draw and one element per sample expected, got {tuple(stages[0].shape)}')
    lib = L.load()
    mse = torch.empty((M * (M + 1) // 2, N), dtype=torch.float32, device=x.device)
    if N == 0:                         # an empty batch has no storage to point at
        return mse
    nbytes = lib.jvae_cascade_mse_workspace_bytes(M, N, D)
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=x.device)
    src_p = (ctypes.c_void_p * M)(*[s.data_ptr() for s in stages])
    L.check(lib.jvae_cascade_mse_f32(L.ptr(x), src_p, M, L.ptr(mse), Ls, N, D, L.ptr(ws), ws.numel() * 8, L.stream_ptr()),
            'jvae_cascade_mse_f32')
    return mse


def iterate_prior(p):
    """The sequential Bayesian update of module/cascad.py::iterate_with_prior in one launch: p (M, C, N) fp32, the class
    likelihoods of M <= 8 chained models -> posterior (M, C, N): prior_0 = 1 / C, posterior[i] = p[i] prior / sum_c p[i] prior,
    prior = posterior[i].  A stage whose class sum is 0 makes that sample NaN from that stage on (0 / 0, as in the reference).
    C <= MISCLASS_MAX_CLASSES.  Nothing is synchronised."""
    p = _c(_f32(p, 'iterate_prior'))
    L.ptr(p)
    if p.dim() != 3:
        raise L.JvaeHipError(f'iterate_prior: (M, C, N) expected, got {tuple(p.shape)}')
    M, C, N = p.shape
    if not 1 <= M <= CASCADE_MAX_MODELS or not 1 <= C <= MISCLASS_MAX_CLASSES:
        raise L.JvaeHipError(f'iterate_prior: 1 <= M <= {CASCADE_MAX_MODELS} and 1 <= C <= {MISCLASS_MAX_CLASSES} expected, got '
                             f'M = {M}, C = {C}')
    post = torch.empty_like(p)
    L.check(L.load().jvae_iterate_prior_f32(L.ptr(p), L.ptr(post), M, C, N, L.stream_ptr()), 'jvae_iterate_prior_f32')
    return post


# ------------------------------------------------------------------------- latent-space inspection (csrc/inspect.hip)
def latent_moments(mu, log_var, group, sums, counts):
    """sums (G, 4, K) fp64 and counts (G,) int64, device accumulators of the caller, take this batch's per-group, per-dimension
    sums of mu, mu^2, v and v^2 (v = exp(log_var) in fp32, widened) of the posterior mu, log_var (N, K) fp32 and the group sizes;
    group (N,) int32 in [0, G) - anything else leaves the sample out - or None (G = 1).  Two launches (slabs of 256 rows, then their
    fold in ascending order), no floating-point atomics: the same bits run to run whatever the device.  Nothing is
    synchronised (reference module/sample.py::zsample with the class mask it forgets to apply)."""
    mu, log_var = _c(_f32(mu, 'latent_moments')), _c(_f32(log_var, 'latent_moments'))
    L.ptr(mu), L.ptr(log_var)
    if mu.dim() != 2 or log_var.shape != mu.shape or sums.dim() != 3 or counts.dim() != 1 \
            or tuple(sums.shape) != (counts.shape[0], 4, mu.shape[1]) or sums.dtype != torch.float64 \
            or counts.dtype != torch.int64 or not sums.is_contiguous() or not counts.is_contiguous() \
            or (group is None and counts.shape[0] != 1) \
            or (group is not None and (group.dtype != torch.int32 or tuple(group.shape) != (mu.shape[0],))) \
            or any(t.device != mu.device for t in (log_var, sums, counts) + (() if group is None else (group,))):
        raise L.JvaeHipError('latent_moments: mu and log_var (N, K) fp32, group (N,) int32 (None: one group), sums (G, 4, K) fp64 '
                             'and counts (G,) int64, dense and on one device, expected')
    N, K = mu.shape
    G = counts.shape[0]
    if N == 0:
        return sums, counts
    lib = L.load()
    ws = _aligned_ws(lib.jvae_latent_moments_workspace_bytes(N, K, G), mu.device)
    L.check(lib.jvae_latent_moments_f32(L.ptr(mu), L.ptr(log_var), None if group is None else L.ptr(_c(group)), L.ptr(sums),
                                        L.ptr(counts), N, K, G, *ws, L.stream_ptr()),
            'jvae_latent_moments_f32')
    return sums, counts


def nearest_centroid(mu, centroids):
    """mu (N, K), centroids (C, K) fp32 -> (y_nearest (N,) int64, d2 (N,) fp32): the centroid with the smallest squared distance
    to each row and that distance (reference ft/inspection.py::estimate_y, which goes through an (N, C, K) temporary).  The
    distances are summed and compared in fp64; ties go to the lowest index, as torch.argmin.  One launch, nothing synchronised."""
    mu, centroids = _c(_f32(mu, 'nearest_centroid')), _c(_f32(centroids, 'nearest_centroid'))
    L.ptr(mu), L.ptr(centroids)
    if mu.dim() != 2 or centroids.dim() != 2 or centroids.shape[1] != mu.shape[1] or centroids.shape[0] < 1 or mu.shape[1] < 1 \
            or centroids.device != mu.device:
        raise L.JvaeHipError(f'nearest_centroid: mu (N, K) and centroids (C, K) on one device expected, got {tuple(mu.shape)} and '
                             f'{tuple(centroids.shape)}')
    N, K = mu.shape
    y = torch.empty(N, dtype=torch.int64, device=mu.device)
    d2 = torch.empty(N, dtype=torch.float32, device=mu.device)
    if N:
        L.check(L.load().jvae_nearest_centroid_f32(L.ptr(mu), L.ptr(centroids), L.ptr(y), L.ptr(d2), N, K, centroids.shape[0],
                                                   L.stream_ptr()), 'jvae_nearest_centroid_f32')
    return y, d2


_hist_nonfinite = {}


def histogram(values, edges, group=None, counts=None, G=None, check=False):
    """Counts of `values` (n,) fp32 in the bins of `edges` (B + 1 ascending numbers: a numpy array or a sequence, checked and
    uploaded as fp64; or an fp64 device tensor, taken as it is) -> counts (G, B) int64, added to when given.  Bin b holds
    edges[b] <= x < edges[b + 1], the last bin is closed on the right, values outside [edges[0], edges[B]] are not counted:
    np.histogram's rule, so that with edges = np.histogram_bin_edges(np.empty(0, np.float32), bins=B, range=(lo, hi)) the counts
    are np.histogram(values, bins=B, range=(lo, hi))'s.  group (n,) int32 in [0, G) - anything else leaves the value out - or
    None (G = 1); G is taken from `counts`, or given.  NaN and +-inf are not counted; their number goes to a device word that
    `check=True` reads (a synchronisation) and turns into ValueError.  One launch; exact integer counts."""
    values = _c(_f32(values, 'histogram')).reshape(-1)
    L.ptr(values)
    dev = values.device
    if not torch.is_tensor(edges):
        import numpy as np
        e = np.asarray(edges, dtype=np.float64).reshape(-1)
        if e.size < 2 or not np.all(np.isfinite(e)) or np.any(np.diff(e) < 0):
            raise ValueError('histogram: at least two finite, ascending edges expected')
        edges = torch.from_numpy(e).to(dev)
    if edges.dtype != torch.float64 or edges.dim() != 1 or edges.shape[0] < 2 or edges.device != dev:
        raise L.JvaeHipError('histogram: edges (B + 1,) fp64 on the device of the values expected')
    B = edges.shape[0] - 1
    if counts is None:
        G = 1 if G is None else int(G)
        if G < 1:
            raise L.JvaeHipError('histogram: at least one group expected')
        counts = torch.zeros((G, B), dtype=torch.int64, device=dev)
    if counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[1] != B or counts.device != dev or not counts.is_contiguous() \
            or (G is not None and counts.shape[0] != G) or (group is None and counts.shape[0] != 1) \
            or (group is not None and (group.dtype != torch.int32 or tuple(group.shape) != (values.shape[0],) or group.device != dev)):
        raise L.JvaeHipError('histogram: counts (G, B) int64 and group (n,) int32 (None: G = 1) on the device of the values expected')
    key = (dev.index if dev.index is not None else torch.cuda.current_device())
    word = _hist_nonfinite.get(key)
    if word is None:
        _hist_nonfinite[key] = word = torch.zeros(1, dtype=torch.int64, device=dev)
    L.check(L.load().jvae_histogram_f32(L.ptr(values), L.ptr(_c(edges)), None if group is None else L.ptr(_c(group)), L.ptr(counts),
                                        L.ptr(word), values.shape[0], B, counts.shape[0], L.stream_ptr()), 'jvae_histogram_f32')
    if check:
        histogram_check(dev)
    return counts


def histogram_check(device=None):
    """Read (and clear) the non-finite word(s) of `histogram`: ValueError when a NaN or an infinity was met since the last check."""
    for key, word in _hist_nonfinite.items():
        if device is not None and device.index not in (None, key):
            continue
        bad = int(word[0])
        if bad:
            word.zero_()
            raise ValueError(f'histogram: {bad} non-finite value(s) were met (they are in no bin)')


# ------------------------------------------------------------ k nearest neighbours over a latent bank (csrc/knn.hip)
KNN_MAX_K = 64              # neighbours: one list slot per lane
KNN_MAX_DIM = 4096          # columns of the rows
KNN_MAX_SPLITS = 1024
KNN_STATUS_BANK = 1         # a bank row with a distance that is not finite was met (it is in no list)
KNN_STATUS_QUERY = 2        # a query row with a non-finite element was met (its slots are NaN / -1)


def knn_status(device):
    """The per-device status word of `knn` calls made without one of their own (created cleared, on first use)."""
    return _status_word('knn', device)


def _knn_sqnorms(x):
    sq = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    if x.shape[0]:
        L.check(L.load().jvae_knn_sqnorms_f32(L.ptr(x), L.ptr(sq), x.shape[0], x.shape[1], L.stream_ptr()), 'jvae_knn_sqnorms_f32')
    return sq


def knn_bank(x):
    """x (M, K) -> (bank, sq): the rows as contiguous fp32 (x itself when it already is; a bf16 / fp16 x is widened) and their
    squared norms (M,) fp32, summed over k ascending in a fixed order - what `knn` wants of a bank, computed once.
    1 <= K <= KNN_MAX_DIM.  One launch."""
    if not x.is_floating_point():
        raise L.JvaeHipError(f'knn_bank: floating-point rows expected, got {x.dtype}')
    bank = _c(x.float())
    L.ptr(bank)
    if bank.dim() != 2 or not 1 <= bank.shape[1] <= KNN_MAX_DIM:
        raise L.JvaeHipError(f'knn_bank: (M, K) with 1 <= K <= {KNN_MAX_DIM} expected, got {tuple(bank.shape)}')
    return bank, _knn_sqnorms(bank)


def knn(q, bank, sq, k, normalized=True, splits=0, status=None):
    """The k nearest rows of `bank` (M, K) to each row of q (N, K), all fp32 on one device; sq (M,): the bank's norms from
    `knn_bank` -> (d2 (N, k) fp32, the squared distances ascending, idx (N, k) int32, their bank rows).  normalized: the
    distance between the F.normalize()d rows, 2 - 2 cos (no normalised copy is made), else |q|^2 + |b|^2 - 2 q.b; both clamped
    at 0.  The products are exact-fp32 matrix instructions fused with the selection (csrc/knn.hip): no (N, M) matrix exists.
    Ties go to the lower bank row; with M < k the unused slots hold +inf / -1.  splits: bank partitions selected independently
    and merged in a fixed order (0: the library's choice); the result's bits do not depend on it.  status: an int32 device word
    that takes bit KNN_STATUS_BANK when a bank row's distance is not finite (the row is never selected) and KNN_STATUS_QUERY
    when a query row is not finite (its slots are NaN / -1); default `knn_status(device)`; `knn_check_status` raises on them.
    1 <= k <= KNN_MAX_K, 1 <= K <= KNN_MAX_DIM.  N = 0 returns empties.  Three launches, nothing synchronised."""
    q, bank, sq = _c(_f32(q, 'knn')), _c(_f32(bank, 'knn')), _c(_f32(sq, 'knn'))
    L.ptr(q), L.ptr(bank), L.ptr(sq)
    if q.dim() != 2 or bank.dim() != 2 or bank.shape[1] != q.shape[1] or tuple(sq.shape) != (bank.shape[0],) \
            or bank.device != q.device or sq.device != q.device:
        raise L.JvaeHipError(f'knn: q (N, K), bank (M, K) and sq (M,) on one device expected, got {tuple(q.shape)}, '
                             f'{tuple(bank.shape)} and {tuple(sq.shape)}')
    k, splits = int(k), int(splits)
    (N, K), M = q.shape, bank.shape[0]
    if not 1 <= k <= KNN_MAX_K or not 1 <= K <= KNN_MAX_DIM or not 0 <= splits <= KNN_MAX_SPLITS:
        raise L.JvaeHipError(f'knn: 1 <= k <= {KNN_MAX_K}, 1 <= K <= {KNN_MAX_DIM} and 0 <= splits <= {KNN_MAX_SPLITS} expected, '
                             f'got k={k}, K={K}, splits={splits} (unsupported configuration)')
    dev = q.device
    d2 = torch.empty((N, k), dtype=torch.float32, device=dev)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    if not N:
        return d2, idx
    status = _status_word('knn', dev, status, 'knn', 'rows')
    lib = L.load()
    nbytes = lib.jvae_knn_workspace_bytes(N, M, K, k, splits)
    if not nbytes:
        raise L.JvaeHipError(f'knn: sizes out of range (N={N}, M={M}, K={K}, k={k})')
    L.check(lib.jvae_knn_f32(L.ptr(q), L.ptr(_knn_sqnorms(q)), L.ptr(bank), L.ptr(sq), L.ptr(d2), L.ptr(idx), N, M, K, k,
                             1 if normalized else 0, splits, L.ptr(status), *_aligned_ws(nbytes, dev, 4), L.stream_ptr()),
            'jvae_knn_f32')
    return d2, idx


def knn_check_status(status=None):
    """Raise ValueError for what `knn` flagged.  status: the word given to the op (a device tensor: read here - this is the
    synchronisation - and cleared), a host value, or None for the per-device default words."""
    word = _read_status('knn', status)
    if word & KNN_STATUS_QUERY:
        raise ValueError('knn: a query row with a non-finite element was met (its distances are NaN, its indices -1)')
    if word & KNN_STATUS_BANK:
        raise ValueError('knn: a bank row at a non-finite distance was met (it is in no list)')


# ------------------------------------------------------------ Mahalanobis scores over a latent bank (csrc/maha.hip)
MAHA_MAX_DIM = 256          # columns of the rows
MAHA_STATUS_LABEL = 1       # a bank row with a label outside [0, C) was met (it is in no sum)
MAHA_STATUS_BANK = 2        # a bank row with a non-finite element was met (it is in no sum)
MAHA_STATUS_QUERY = 4       # a query row with a non-finite element was met (its scores are NaN, its class -1)
MAHA_FIT_KEYS = ('counts', 'means', 'mean0', 'W', 'W0', 'mu0_32', 'W32', 'm32', 'm0_32', 'cmap', 'shrinkage')


def maha_status(device):
    """The per-device status word of `maha_moments` / `maha_scores` calls made without one of their own (created cleared)."""
    return _status_word('maha', device)


def maha_moments(bank, labels, num_classes, status=None):
    """bank (M, K) fp32 and labels (M,) int64 on one device -> {'counts' (C,) int64, 'means' (C, K), 'mean0' (K,), 'Sw' (K, K),
    'St' (K, K) fp64}: the class sizes and means, the overall mean, Sw = sum_i (b_i - means[y_i]) (b_i - means[y_i])^T / M and St,
    the same about mean0.  Every sum is fp64 in a fixed order that hangs on M alone, without floating-point atomics: a second call
    returns the same bits; Sw and St are symmetric to the bit.  A row with a label outside [0, C) sets MAHA_STATUS_LABEL in the
    device word `status` (default `maha_status(device)`), a row with a non-finite element MAHA_STATUS_BANK; such a row is in no
    sum and in no count, and the divisor M is the number of rows kept.  An empty class has a mean of zeros.
    1 <= K <= MAHA_MAX_DIM, 1 <= C <= MISCLASS_MAX_CLASSES, 1 <= M < 2^31, refused here before any launch.  Nothing is
    synchronised (csrc/maha.hip)."""
    if not torch.is_tensor(bank) or not torch.is_tensor(labels) or bank.dim() != 2 or tuple(labels.shape) != (bank.shape[0],):
        raise L.JvaeHipError('maha_moments: bank (M, K) and labels (M,) expected')
    if labels.dtype != torch.int64:
        raise L.JvaeHipError(f'maha_moments: int64 labels expected, got {labels.dtype}')
    bank = _c(_f32(bank, 'maha_moments'))
    (M, K), C = bank.shape, int(num_classes)
    if not 1 <= K <= MAHA_MAX_DIM or not 1 <= C <= MISCLASS_MAX_CLASSES or not 1 <= M < 1 << 31:
        raise L.JvaeHipError(f'maha_moments: 1 <= K <= {MAHA_MAX_DIM}, 1 <= C <= {MISCLASS_MAX_CLASSES} and 1 <= M < 2^31 expected, '
                             f'got K={K}, C={C}, M={M} (unsupported configuration)')
    L.ptr(bank), L.ptr(labels)
    dev = bank.device
    if labels.device != dev:
        raise L.JvaeHipError('maha_moments: bank and labels on one device expected')
    status = _status_word('maha', dev, status, 'maha_moments', 'rows')
    out = {'counts': torch.empty(C, dtype=torch.int64, device=dev), 'means': torch.empty((C, K), dtype=torch.float64, device=dev),
           'mean0': torch.empty(K, dtype=torch.float64, device=dev), 'Sw': torch.empty((K, K), dtype=torch.float64, device=dev),
           'St': torch.empty((K, K), dtype=torch.float64, device=dev)}
    lib = L.load()
    L.check(lib.jvae_maha_moments_f32(L.ptr(bank), L.ptr(_c(labels)), M, K, C, *(L.ptr(out[k]) for k in out), L.ptr(status),
                                      *_aligned_ws(lib.jvae_maha_moments_workspace_bytes(M, K, C), dev), L.stream_ptr()),
            'jvae_maha_moments_f32')
    return out


def _maha_whitener(S, shrinkage, what):
    """fp64 numpy: L^-1 (lower triangular) of the Cholesky factor L of S + shrinkage * (trace S / K) * I."""
    import numpy as np
    K = S.shape[0]
    A = S + shrinkage * (np.trace(S) / K) * np.eye(K)
    refusal = (f'maha_fit: {what} is not positive definite (fewer independent rows than dimensions, or a constant dimension): '
               f'a larger `shrinkage` is needed (now {shrinkage})')
    if not np.all(np.isfinite(A)):
        raise ValueError(refusal)
    try:
        chol = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        raise ValueError(refusal) from None
    # a pivot at the rounding level of the matrix: positive by accident
    if np.min(np.diag(chol)) ** 2 <= K * 2. ** -52 * np.max(np.diag(A)):
        raise ValueError(refusal)
    return np.tril(np.linalg.inv(chol))


def maha_fit(moments, shrinkage=0., device=None):
    """The Gaussians of `maha_moments`' result (device or host tensors, or numpy arrays), factored on the host in numpy fp64 -
    once per fit, as the eigenvectors of `pca_moments`' covariance are: for Sw and for St, S + shrinkage * (trace S / K) * I =
    L L^T and W = L^-1 (`W`, `W0`, lower triangular).  -> the fit of `maha_scores`, on `device` (default: the moments' own):
    'counts' int64, 'means', 'mean0', 'W', 'W0' fp64, and the operands rounded ONCE to fp32: 'mu0_32' = fp32(mean0), 'W32' (2K, K)
    = W stacked on W0, 'm32' (Cn, K) = fp32(W (means[c] - mu0_32)) for the Cn non-empty classes in ascending label order, 'm0_32'
    (K,) = fp32(W0 (mean0 - mu0_32)), the whitened rounding error of mu0_32, 'cmap' (Cn,) int32 the classes' labels; 'shrinkage'.  ValueError, naming `shrinkage`, for a matrix that is not positive definite."""
    import numpy as np
    if device is None:
        device = next((v.device for v in moments.values() if torch.is_tensor(v)), torch.device('cpu'))
    tensors = {k: torch.as_tensor(moments[k]) for k in ('counts', 'means', 'mean0', 'Sw', 'St')}
    if tensors['means'].dim() != 2 or any(tensors[k].dtype != torch.float64 for k in ('means', 'mean0', 'Sw', 'St')) \
            or tensors['counts'].dtype != torch.int64:
        raise L.JvaeHipError('maha_fit: the result of maha_moments expected (counts int64; means, mean0, Sw, St fp64)')
    C, K = tensors['means'].shape
    if tuple(tensors['counts'].shape) != (C,) or tuple(tensors['mean0'].shape) != (K,) \
            or any(tuple(tensors[k].shape) != (K, K) for k in ('Sw', 'St')):
        raise L.JvaeHipError('maha_fit: counts (C,), means (C, K), mean0 (K,), Sw and St (K, K) expected')
    shrinkage = float(shrinkage)
    if not shrinkage >= 0.:
        raise ValueError(f'maha_fit: a shrinkage >= 0 expected, got {shrinkage}')
    host = read_back(tensors)                                       # ONE copy; the counts are exact in fp64
    counts = host['counts'].astype(np.int64)
    kept = np.flatnonzero(counts > 0)
    if not kept.size:
        raise ValueError('maha_fit: no row was kept, every class is empty')
    W = _maha_whitener(host['Sw'], shrinkage, 'the within-class scatter Sw')
    W0 = _maha_whitener(host['St'], shrinkage, 'the total scatter St')
    mu0_32 = host['mean0'].astype(np.float32)
    m = (host['means'][kept] - mu0_32.astype(np.float64)) @ W.T
    m0 = W0 @ (host['mean0'] - mu0_32.astype(np.float64))

    def put(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return {'counts': put(counts), 'means': put(host['means']), 'mean0': put(host['mean0']), 'W': put(W), 'W0': put(W0),
            'mu0_32': put(mu0_32), 'W32': put(np.concatenate([W, W0]).astype(np.float32)), 'm32': put(m.astype(np.float32)),
            'm0_32': put(m0.astype(np.float32)), 'cmap': put(kept.astype(np.int32)), 'shrinkage': shrinkage}


def maha_check_fit(fit, what='maha_scores'):
    """Keys, dtypes and shapes of a fit of `maha_fit` -> (K, Cn, C); ValueError otherwise."""
    def bad(why):
        return ValueError(f'{what}: not a fit of maha_fit ({why})')
    if not isinstance(fit, dict) or not set(MAHA_FIT_KEYS) <= set(fit):
        raise bad('keys ' + ', '.join(MAHA_FIT_KEYS) + ' expected')
    dtypes = {'counts': torch.int64, 'means': torch.float64, 'mean0': torch.float64, 'W': torch.float64, 'W0': torch.float64,
              'mu0_32': torch.float32, 'W32': torch.float32, 'm32': torch.float32, 'm0_32': torch.float32, 'cmap': torch.int32}
    for k, dt in dtypes.items():
        if not torch.is_tensor(fit[k]) or fit[k].dtype != dt:
            raise bad(f'{k}: a {dt} tensor expected')
    if fit['means'].dim() != 2 or fit['m32'].dim() != 2:
        raise bad('means (C, K) and m32 (Cn, K) expected')
    (C, K), Cn = fit['means'].shape, fit['m32'].shape[0]
    shapes = {'counts': (C,), 'mean0': (K,), 'W': (K, K), 'W0': (K, K), 'mu0_32': (K,), 'W32': (2 * K, K), 'm32': (Cn, K), 'm0_32': (K,),
              'cmap': (Cn,)}
    for k, shape in shapes.items():
        if tuple(fit[k].shape) != shape:
            raise bad(f'{k}: {shape} expected, got {tuple(fit[k].shape)}')
    if not 1 <= K <= MAHA_MAX_DIM or not 1 <= Cn <= C <= MISCLASS_MAX_CLASSES:
        raise bad(f'1 <= K <= {MAHA_MAX_DIM} and 1 <= non-empty classes <= C <= {MISCLASS_MAX_CLASSES} expected')
    if not isinstance(fit['shrinkage'], float):
        raise bad('shrinkage: a float expected')
    return K, Cn, C


def maha_scores(q, fit, per_class=False, status=None):
    """q (N, K) fp32 against the fit of `maha_fit` -> (d (N,) fp32, cls (N,) int32, rel (N,) fp32[, per_class (N, C) fp32]):
    with x = q - mu0_32 and y = W32 x (ONE product against the stacked matrix on the fp32 matrix cores, every y_k the fmaf chain
    over j ascending), d_c = sum_k (y_k - m_ck)^2 and d0 = sum_k (y0_k - m0_k)^2 as fmaf chains over k ascending; d = min_c d_c over the
    non-empty classes, cls the label that attains it (the lower one of a tie), rel = min_c (d_c - d0) - the relative distance of
    Ren et al. 2021.  per_class: also d_c for every label, +inf in the column of an empty class.  A query row with a non-finite
    element gets NaN / -1 and sets MAHA_STATUS_QUERY in `status` (default `maha_status(device)`; `maha_check_status`).
    N = 0 returns empties without a launch.  ONE launch; neither y nor the (N, C) distances are written to memory unless
    `per_class` asks for them.  Nothing is synchronised."""
    K, Cn, C = maha_check_fit(fit)
    if not torch.is_tensor(q) or q.dim() != 2 or q.shape[1] != K:
        raise L.JvaeHipError(f'maha_scores: q (N, {K}) expected, got {tuple(q.shape) if torch.is_tensor(q) else type(q)}')
    q = _c(_f32(q, 'maha_scores'))
    N = q.shape[0]
    if N >= 1 << 31:
        raise L.JvaeHipError(f'maha_scores: N < 2^31 expected, got {N} (unsupported configuration)')
    L.ptr(q)
    dev = q.device
    ops_ = [fit[k] for k in ('mu0_32', 'W32', 'm32', 'm0_32', 'cmap')]
    if any(t.device != dev for t in ops_):
        raise L.JvaeHipError('maha_scores: the fit on the device of the rows expected')
    d = torch.empty(N, dtype=torch.float32, device=dev)
    cls = torch.empty(N, dtype=torch.int32, device=dev)
    rel = torch.empty(N, dtype=torch.float32, device=dev)
    pc = torch.empty((N, C), dtype=torch.float32, device=dev) if per_class else None
    if N:
        status = _status_word('maha', dev, status, 'maha_scores', 'rows')
        L.check(L.load().jvae_maha_scores_f32(L.ptr(q), *(L.ptr(_c(t)) for t in ops_), L.ptr(d), L.ptr(cls), L.ptr(rel), L.ptr(pc),
                                              N, K, Cn, C, L.ptr(status), L.stream_ptr()), 'jvae_maha_scores_f32')
    return (d, cls, rel, pc) if per_class else (d, cls, rel)


def maha_check_status(status=None):
    """Raise ValueError for what `maha_moments` / `maha_scores` flagged.  status: the word given to the op (a device tensor: read
    here - this is the synchronisation - and cleared), a host value, or None for the per-device default words."""
    word = _read_status('maha', status)
    if word & MAHA_STATUS_QUERY:
        raise ValueError('maha: a query row with a non-finite element was met (its scores are NaN, its class -1)')
    if word & MAHA_STATUS_LABEL:
        raise ValueError('maha: a bank row with a label outside [0, num_classes) was met (it is in no sum)')
    if word & MAHA_STATUS_BANK:
        raise ValueError('maha: a bank row with a non-finite element was met (it is in no sum)')


# ------------------------------------------------------------ input complexity: a lossless image code length (csrc/ic.hip)
IC_MAX_CHANNELS = 4
IC_MAX_PIXELS = 1 << 20     # H W of an image: the 32-bit counters of a histogram hold it
IC_MODES = ('none', 'sub', 'up', 'average', 'paeth', 'med', 'stored')
IC_STATUS_INEXACT = 1       # a pixel further than 1/64 from its 8-bit level was met (the length is the quantised image's)
IC_STATUS_NONFINITE = 2     # an image with a non-finite pixel was met (its bits are NaN, its choice -1)
_ic_tables = {}             # n = H W -> the host table log2(m!), m = 0 .. n + 256; (n, device) -> its upload


def ic_status(device):
    """The per-device status word of `image_code_length` calls made without one of their own (created cleared)."""
    return _status_word('ic', device)


def ic_table(n, device=None):
    """T[m] = log2(m!) for m = 0 .. n + 256 in fp64, math.lgamma(m + 1) / math.log(2) entry by entry, built once per n on the
    host and kept; with `device` the (cached) upload of it."""
    n = int(n)
    if n not in _ic_tables:
        ln2 = math.log(2)
        _ic_tables[n] = torch.tensor([math.lgamma(m + 1) / ln2 for m in range(n + 257)], dtype=torch.float64)
    if device is None:
        return _ic_tables[n]
    key = (n, str(device))
    if key not in _ic_tables:
        _ic_tables[key] = _ic_tables[n].to(device)
    return _ic_tables[key]


def image_code_length(x, status=None):
    """x (N, C, H, W) fp32 -> (bits (N,) fp64, bits32 (N,) fp32, choice (N,) int32): the length in bits of every image under a
    lossless coder - the exact length of an achievable code, nothing is encoded (csrc/ic.hip, ONE launch, one workgroup per
    image).  q = clamp(rint(255 x), 0, 255); per plane the best of six predictors (`IC_MODES`: none, left, up, their mean, Paeth,
    the LOCO-I median) and the stored mode, a residual plane at 8 + log2 C(256, k) + log2[(n + k - 1)! / ((k - 1)! prod n_s!)]
    bits for its histogram n_s over k used symbols, 3 bits per plane for the mode; at C == 3 the better of (R, G, B) and
    (G, R - G, B - G), and 1 bit for it.  Integer histograms and one fixed-order fp64 sum per histogram over the table
    `ic_table(H W)`: the bits are those of the numpy restatement (tests/test_ic_restatement.py) and the same on every call.
    bits32 = fp32(bits); `ic_choice` decodes `choice`.  status: an int32 device word that takes IC_STATUS_INEXACT when a pixel is
    further than 1/64 from its 8-bit level and IC_STATUS_NONFINITE when one is not finite (that image: NaN, NaN, -1; the others
    are untouched); default `ic_status(device)`; `ic_check_status` raises on the second.  1 <= C <= IC_MAX_CHANNELS,
    H W <= IC_MAX_PIXELS.  N = 0 returns empties without a launch.  Nothing is synchronised."""
    if not torch.is_tensor(x) or x.dim() != 4:
        raise L.JvaeHipError(f'image_code_length: x (N, C, H, W) expected, got {tuple(x.shape) if torch.is_tensor(x) else type(x)}')
    x = _c(_f32(x, 'image_code_length'))
    N, C, H, W = x.shape
    if not 1 <= C <= IC_MAX_CHANNELS or H < 1 or W < 1 or H * W > IC_MAX_PIXELS or N >= 1 << 31:
        raise L.JvaeHipError(f'image_code_length: 1 <= C <= {IC_MAX_CHANNELS}, 1 <= H, W, H W <= 2^20 and N < 2^31 expected, got '
                             f'{tuple(x.shape)} (unsupported configuration)')
    L.ptr(x)
    dev = x.device
    bits = torch.empty(N, dtype=torch.float64, device=dev)
    bits32 = torch.empty(N, dtype=torch.float32, device=dev)
    choice = torch.empty(N, dtype=torch.int32, device=dev)
    if N:
        status = _status_word('ic', dev, status, 'image_code_length', 'images')
        table = ic_table(H * W, dev)
        L.check(L.load().jvae_image_code_length_f32(L.ptr(x), N, C, H, W, L.ptr(table), table.numel(), L.ptr(bits), L.ptr(bits32),
                                                    L.ptr(choice), L.ptr(status), L.stream_ptr()), 'jvae_image_code_length_f32')
    return bits, bits32, choice


def ic_check_status(status=None):
    """Read and clear what `image_code_length` flagged and raise ValueError for a non-finite pixel; pixels off the 8-bit grid
    (IC_STATUS_INEXACT) are not an error.  status: the word given to the op (a device tensor: read here - this is the
    synchronisation - and cleared), a host value, or None for the per-device default words.  -> the OR of the words read."""
    seen = _read_status('ic', status)
    if seen & IC_STATUS_NONFINITE:
        raise ValueError('image_code_length: an image with a non-finite pixel was met (its bits are NaN, its choice -1)')
    return seen


def ic_choice(word):
    """The `choice` word of an image -> (space, [mode per plane of that space]): space 0 = the planes as they are, 1 =
    (G, R - G, B - G); modes index `IC_MODES`.  -1 (a refused image) -> (-1, [])."""
    word = int(word)
    if word < 0:
        return -1, []
    modes, rest = [], word >> 4
    while rest & 7:
        modes.append((rest & 7) - 1)
        rest >>= 3
    return word & 15, modes


def ic_choice_word(space, modes):
    """The inverse of `ic_choice`."""
    word = int(space)
    for p, m in enumerate(modes):
        word |= (int(m) + 1) << (4 + 3 * p)
    return word


# ------------------------------------------------------------ SSIM of images against their reconstructions (csrc/ssim.hip)
SSIM_WINDOW = 11            # taps of the Gaussian window (sigma 1.5); min(H, W) of an image
SSIM_MAX_W = 128            # a strip of rows is staged at full width
SSIM_MAX_H = 32768
SSIM_STATUS_X = 1           # an image x[n] with a non-finite pixel was met (every [r, n] is NaN)
SSIM_STATUS_Y = 2           # a draw y[r, n] with a non-finite pixel was met (that entry is NaN)


def ssim_status(device):
    """The per-device status word of `ssim` calls made without one of their own (created cleared)."""
    return _status_word('ssim', device)


def ssim_strip_rows(H, W):
    """The output rows of one staged strip of csrc/ssim.hip at this image size (a property of the build; 0: a refused size)."""
    return int(L.load().jvae_ssim_strip_rows(int(H), int(W)))


def ssim(x, x_reco, maps=False, status=None):
    """x (N, C, H, W) fp32, x_reco (R, N, C, H, W) fp32 -> (ssim (R, N), cs (R, N)) fp32, with `maps` also map (R, N, H - 10,
    W - 10): the structural similarity (Wang et al. 2004) of every image to each of its R reconstructions under the 11-tap
    Gaussian window of sigma 1.5 over the valid region, data range 1 - scikit-image's structural_similarity(gaussian_weights=
    True, use_sample_covariance=False, data_range=1) on its interior.  ssim: the mean over channels and valid pixels of
    l * cs; cs: the same mean of the contrast-structure term alone; map: the channel mean of l * cs per pixel.  ONE launch
    (csrc/ssim.hip): x is staged and its local moments are formed once per sample and chunk of draws; the second moments are
    those of x - a and y - a, a the plane mean of x.  A draw equal to its image scores exactly 1; no bit depends on the batch
    or on `maps`.  status: an int32 device word that takes SSIM_STATUS_X for a non-finite pixel in x[n] (every [r, n] NaN)
    and SSIM_STATUS_Y for one in x_reco[r, n] (that entry NaN); default `ssim_status(device)`; `ssim_check_status` raises on
    either.  SSIM_WINDOW <= H <= SSIM_MAX_H, SSIM_WINDOW <= W <= SSIM_MAX_W, C >= 1.  N = 0 or R = 0 returns empties without a
    launch.  Nothing is synchronised."""
    if not torch.is_tensor(x) or not torch.is_tensor(x_reco) or x.dim() != 4 or x_reco.dim() != 5 \
            or tuple(x_reco.shape[1:]) != tuple(x.shape):
        raise L.JvaeHipError('ssim: x (N, C, H, W) and x_reco (R, N, C, H, W) expected, got '
                             + ' and '.join(str(tuple(t.shape)) if torch.is_tensor(t) else str(type(t)) for t in (x, x_reco)))
    x, y = _c(_f32(x, 'ssim')), _c(_f32(x_reco, 'ssim'))
    N, C, H, W = x.shape
    R = y.shape[0]
    if C < 1 or not SSIM_WINDOW <= H <= SSIM_MAX_H or not SSIM_WINDOW <= W <= SSIM_MAX_W or N >= 1 << 31 or R >= 1 << 31:
        raise L.JvaeHipError(f'ssim: C >= 1, {SSIM_WINDOW} <= H <= {SSIM_MAX_H}, {SSIM_WINDOW} <= W <= {SSIM_MAX_W} and N, R < 2^31 '
                             f'expected, got {tuple(y.shape)} (unsupported configuration)')
    L.ptr(x)
    dev = x.device
    if y.device != dev:
        raise L.JvaeHipError('ssim: x and x_reco on one device expected')
    out = torch.empty((2, R, N), dtype=torch.float32, device=dev)
    pix = torch.empty((R, N, H - 10, W - 10), dtype=torch.float32, device=dev) if maps else None
    if N and R:
        status = _status_word('ssim', dev, status, 'ssim', 'images')
        L.check(L.load().jvae_ssim_f32(L.ptr(x), L.ptr(y), N, R, C, H, W, L.ptr(out[0]), L.ptr(out[1]), L.ptr(pix), L.ptr(status),
                                       L.stream_ptr()), 'jvae_ssim_f32')
    return (out[0], out[1], pix) if maps else (out[0], out[1])


def ssim_check_status(status=None):
    """Read and clear what `ssim` flagged and raise ValueError for a non-finite pixel.  status: the word given to the op (a device
    tensor: read here - this is the synchronisation - and cleared), a host value, or None for the per-device default words."""
    seen = _read_status('ssim', status)
    if seen & SSIM_STATUS_X:
        raise ValueError('ssim: an image with a non-finite pixel was met (the scores of all its draws are NaN)')
    if seen & SSIM_STATUS_Y:
        raise ValueError('ssim: a reconstruction with a non-finite pixel was met (its scores are NaN)')
    return seen


# ------------------------------------------------------------ density of states: a KDE over a score bank (csrc/dose.hip)
DOSE_MAX_STATS = 8
DOSE_MAX_BANK = 1 << 24     # values of a bank row
DOSE_STATUS_QUERY = 1 << 16        # a query with a non-finite (or fp32-overflowing) element was met (-inf / NaN in its rows)
DOSE_FIT_KEYS = ('z', 'centre', 'sigma', 'h1', 'hS', 'lognorm', 'M', 'S', 'bandwidth')


def kde_status(device):
    """The per-device status word of `kde_logdensity` calls made without one of their own (created cleared)."""
    return _status_word('kde', device)


def kde_partition():
    """Bank values of a piece of the kernel's fixed bank partition (a property of the build)."""
    return int(L.load().jvae_kde_partition())


def kde_scott(M, d):
    """Scott's factor M^(-1 / (d + 4)) as `kde_fit` computes it (host fp64)."""
    return float(M) ** (-1. / (d + 4))


def kde_fit(bank, bandwidth=1.0):
    """bank (S, M) fp32 on the device, row s = statistic s of M samples -> the fit of `kde_logdensity`: {'z' (S, M) fp32, the bank
    centred and scaled in fp64, (B - centre) / h1, and rounded once; 'centre', 'sigma' (ddof = 1), 'h1' = bandwidth * sigma *
    M^(-1/5) (Scott's factor: scipy.stats.gaussian_kde's default), 'hS' = bandwidth * sigma * M^(-1/(S+4)) (S,) fp64; 'lognorm'
    (S + 1,) fp64, log(M h1_s sqrt(2 pi)) and, last, log M + sum_s log hS_s + (S / 2) log(2 pi); 'M', 'S', 'bandwidth'}.  The
    moments are fp64 sums on the device in a fixed order that hangs on M alone (csrc/dose.hip): a second call returns the same
    bits.  ValueError, naming the row, for a row without spread (sigma = 0), for a non-finite element and for M < 2: the device
    sets a status word that is read HERE - this call synchronises, scoring does not.  1 <= S <= DOSE_MAX_STATS,
    M <= DOSE_MAX_BANK, bandwidth > 0."""
    if not torch.is_tensor(bank) or bank.dim() != 2:
        raise L.JvaeHipError(f'kde_fit: bank (S, M) expected, got {tuple(bank.shape) if torch.is_tensor(bank) else type(bank)}')
    bank = _c(_f32(bank, 'kde_fit'))
    S, M = bank.shape
    bandwidth = float(bandwidth)
    if not 1 <= S <= DOSE_MAX_STATS or M > DOSE_MAX_BANK:
        raise L.JvaeHipError(f'kde_fit: 1 <= S <= {DOSE_MAX_STATS} and M <= 2^24 expected, got S={S}, M={M} (unsupported '
                             'configuration)')
    if M < 2:
        raise ValueError(f'kde_fit: a bank of at least two samples expected, got M={M}')
    if not 0 < bandwidth < math.inf:
        raise ValueError(f'kde_fit: a bandwidth > 0 expected, got {bandwidth}')
    L.ptr(bank)
    dev = bank.device

    def f64(n):
        return torch.empty(n, dtype=torch.float64, device=dev)
    fit = {'z': torch.empty((S, M), dtype=torch.float32, device=dev), 'centre': f64(S), 'sigma': f64(S), 'h1': f64(S), 'hS': f64(S),
           'lognorm': f64(S + 1)}
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = L.load()
    factors = (ctypes.c_double * 3)(bandwidth, kde_scott(M, 1), kde_scott(M, S))       # a host array, read by the call
    L.check(lib.jvae_kde_fit_f32(L.ptr(bank), M, S, factors, *(L.ptr(fit[k]) for k in fit), L.ptr(status),
                                 *_aligned_ws(lib.jvae_kde_fit_workspace_bytes(M, S), dev), L.stream_ptr()), 'jvae_kde_fit_f32')
    word = int(status[0])                                           # the synchronisation
    for s in range(S):
        if word >> s & 1:
            raise ValueError(f'kde_fit: row {s} of the bank holds a non-finite element')
    for s in range(S):
        if word >> (8 + s) & 1:
            raise ValueError(f'kde_fit: row {s} of the bank has no spread (sigma = 0): no bandwidth can be set for it')
    return dict(fit, M=M, S=S, bandwidth=bandwidth)


def kde_check_fit(fit, who='kde_logdensity'):
    """Keys, dtypes and shapes of a fit of `kde_fit` -> (S, M); ValueError otherwise."""
    def bad(why):
        return ValueError(f'{who}: not a fit of kde_fit ({why})')
    if not isinstance(fit, dict) or not set(DOSE_FIT_KEYS) <= set(fit):
        raise bad('keys ' + ', '.join(DOSE_FIT_KEYS) + ' expected')
    for k in ('M', 'S'):
        if not isinstance(fit[k], int) or isinstance(fit[k], bool):
            raise bad(f'{k}: an int expected')
    S, M = fit['S'], fit['M']
    if not 1 <= S <= DOSE_MAX_STATS or not 2 <= M <= DOSE_MAX_BANK:
        raise bad(f'1 <= S <= {DOSE_MAX_STATS} and 2 <= M <= 2^24 expected, got S={S}, M={M}')
    if not isinstance(fit['bandwidth'], float) or not 0 < fit['bandwidth'] < math.inf:
        raise bad('bandwidth: a float > 0 expected')
    shapes = {'z': (S, M), 'centre': (S,), 'sigma': (S,), 'h1': (S,), 'hS': (S,), 'lognorm': (S + 1,)}
    for k, shape in shapes.items():
        dt = torch.float32 if k == 'z' else torch.float64
        if not torch.is_tensor(fit[k]) or fit[k].dtype != dt:
            raise bad(f'{k}: a {dt} tensor expected')
        if tuple(fit[k].shape) != shape:
            raise bad(f'{k}: {shape} expected, got {tuple(fit[k].shape)}')
    return S, M


def kde_logdensity(stats, fit, status=None):
    """stats (S, N) fp32 on the device, raw (not standardised), against the fit of `kde_fit` -> (2 S + 2, N) fp32: rows 0 .. S - 1
    the marginal log-densities logq_s = logsumexp_m(-((T_s - B_sm) / h1_s)^2 / 2) - log(M h1_s sqrt(2 pi)); row S their sum over s
    ascending (`dose`); row S + 1 the log-density under the product kernel with the bandwidths hS (`dose-joint`); rows S + 2 ..
    2 S + 1 the typicality -|T_s - centre_s| / sigma_s.  Higher = more typical of the bank.  The query is centred and scaled in
    fp64 and rounded once; differences, squares and exponentials are fp32; every sum is shifted by its largest exponent, so a
    query far from every bank value gets a finite, correctly ordered score.  The bank is partitioned in pieces of
    `kde_partition()` values whatever N is: a sample's bits do not depend on its batch, and a second call returns the same bits
    (no floating-point atomics).  A +-inf element gives -inf in the rows that read it (its marginal and typicality row, `dose`,
    `dose-joint`; the typicality row by its own arithmetic), and so does a finite one more than about 2^63 bandwidths from the
    bank, whose square overflows fp32 (its typicality row stays finite); a NaN gives NaN; all set DOSE_STATUS_QUERY in `status` (default `kde_status(device)`; `kde_check_status`)
    and leave the other columns untouched.  N = 0 returns an empty result without a launch.  ONE scoring launch and one merge
    launch; nothing is read back (csrc/dose.hip)."""
    S, M = kde_check_fit(fit)
    if not torch.is_tensor(stats) or stats.dim() != 2 or stats.shape[0] != S:
        raise L.JvaeHipError(f'kde_logdensity: stats ({S}, N) expected, got {tuple(stats.shape) if torch.is_tensor(stats) else type(stats)}')
    if stats.dtype != torch.float32:
        raise L.JvaeHipError(f'kde_logdensity: fp32 stats expected, got {stats.dtype}')
    stats = _c(stats)
    N = stats.shape[1]
    if N >= 1 << 31:
        raise L.JvaeHipError(f'kde_logdensity: N < 2^31 expected, got {N} (unsupported configuration)')
    L.ptr(stats)
    dev = stats.device
    ops_ = [fit[k] for k in ('z', 'centre', 'sigma', 'h1', 'lognorm')]
    if any(t.device != dev for t in ops_):
        raise L.JvaeHipError('kde_logdensity: the fit on the device of the statistics expected')
    out = torch.empty((2 * S + 2, N), dtype=torch.float32, device=dev)
    if not N:
        return out
    status = _status_word('kde', dev, status, 'kde_logdensity', 'statistics')
    lib = L.load()
    nbytes = lib.jvae_kde_workspace_bytes(N, M, S)
    if not nbytes:
        raise L.JvaeHipError(f'kde_logdensity: sizes out of range (N={N}, M={M}, S={S})')
    ratio2 = ctypes.c_double((kde_scott(M, 1) / kde_scott(M, S)) ** 2)     # (h1 / hS)^2: the same for every row; read by the call
    L.check(lib.jvae_kde_logdensity_f32(L.ptr(stats), *(L.ptr(_c(t)) for t in ops_), L.ptr(out), N, M, S, ctypes.byref(ratio2), L.ptr(status),
                                        *_aligned_ws(nbytes, dev), L.stream_ptr()), 'jvae_kde_logdensity_f32')
    return out


def kde_check_status(status=None):
    """Raise JvaeHipError for what `kde_logdensity` flagged.  status: the word given to the op (a device tensor: read here - this
    is the synchronisation - and cleared), a host value, or None for the per-device default words."""
    if _read_status('kde', status) & DOSE_STATUS_QUERY:
        raise L.JvaeHipError('kde_logdensity: a query with a non-finite statistic, or one so far from the bank that its square '
                             'overflows fp32, was met (its rows hold -inf / NaN)')


# ------------------------------------------------------------ the aggregate posterior of a bank of posteriors (csrc/aggpost.hip)
AGGPOST_MAX_K = 1024
AGGPOST_MAX_BANK = 1 << 24         # rows of a bank
AGGPOST_MAX_PIECES = 1 << 14       # AGGPOST_MAX_BANK / aggpost_partition()
AGGPOST_STATUS_BANK = 1            # a non-finite stored operand (mu, exp(-log_var) or the sum of a row's log_var)
AGGPOST_STATUS_QUERY = 2           # a query with a non-finite element, or so far away that every exponent overflows fp32
AGGPOST_STATUS_EMPTY = 4           # a query whose group has no bank row (-inf)
AGGPOST_BANK_KEYS = ('mu', 'log_var', 'group', 'muT', 'wT', 'lvT', 'c')
AGGPOST_WS_BYTES = 1 << 28         # queries are scored in runs whose workspace stays below this (bits do not hang on the run)


def aggpost_status(device):
    """The per-device status word of `aggpost_logdensity` calls made without one of their own (created cleared)."""
    return _status_word('aggpost', device)


def aggpost_partition():
    """Bank rows of a piece of the kernel's fixed bank partition (a property of the build)."""
    return int(L.load().jvae_aggpost_partition())


def aggpost_bank(mu, log_var, group=None):
    """The stored operands of a bank of N diagonal Gaussian posteriors N(mu_n, diag exp(log_var_n)): mu, log_var (N, K) fp32 on the
    device, group (N,) int32 / int64 >= 0 or None (one group) -> {'mu', 'log_var' as given, 'group' (N,) int32, 'muT', 'wT', 'lvT'
    (K, Np) fp32: mu, fp32(exp(-log_var)) (formed in fp64) and log_var k-major with the rows padded to the kernel's tile, 'c' (Np,)
    fp32: the fp64 sum of a row's log_var, k ascending, rounded once}.  1 <= K <= AGGPOST_MAX_K, 1 <= N <= AGGPOST_MAX_BANK.  A
    negative group is a ValueError (read here: this call synchronises when groups are given); non-finite elements are flagged by
    the scoring call."""
    for name, t in (('mu', mu), ('log_var', log_var)):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise L.JvaeHipError(f'aggpost_bank: {name} (N, K) expected, got {tuple(t.shape) if torch.is_tensor(t) else type(t)}')
        _f32(t, f'aggpost_bank: {name}')
    if mu.shape != log_var.shape:
        raise L.JvaeHipError(f'aggpost_bank: mu and log_var of one shape expected, got {tuple(mu.shape)} and {tuple(log_var.shape)}')
    N, K = mu.shape
    if not 1 <= K <= AGGPOST_MAX_K or not 1 <= N <= AGGPOST_MAX_BANK:
        raise L.JvaeHipError(f'aggpost_bank: 1 <= K <= {AGGPOST_MAX_K} and 1 <= N <= 2^24 expected, got N={N}, K={K} (unsupported '
                             'configuration)')
    if group is not None:
        if not torch.is_tensor(group) or group.dtype not in (torch.int32, torch.int64) or tuple(group.shape) != (N,):
            raise L.JvaeHipError(f'aggpost_bank: group ({N},) int32 or int64 expected')
    dev = mu.device
    if log_var.device != dev or (group is not None and group.device != dev):
        raise L.JvaeHipError('aggpost_bank: mu, log_var and group on one device expected')
    mu, log_var = _c(mu), _c(log_var)
    L.ptr(mu)
    if group is None:
        group = torch.zeros(N, dtype=torch.int32, device=dev)
    else:
        if int(group.min()) < 0:
            raise ValueError('aggpost_bank: groups >= 0 expected')
        group = _c(group.to(torch.int32))
    lib = L.load()
    Np = int(lib.jvae_aggpost_padded_rows(N))
    muT, wT, lvT = (torch.empty((K, Np), dtype=torch.float32, device=dev) for _ in range(3))
    c = torch.empty(Np, dtype=torch.float32, device=dev)
    L.check(lib.jvae_aggpost_prepare_f32(L.ptr(mu), L.ptr(log_var), L.ptr(muT), L.ptr(wT), L.ptr(lvT), L.ptr(c), N, K, L.stream_ptr()),
            'jvae_aggpost_prepare_f32')
    return {'mu': mu, 'log_var': log_var, 'group': group, 'muT': muT, 'wT': wT, 'lvT': lvT, 'c': c}


def aggpost_check_bank(bank, who='aggpost_logdensity'):
    """Keys, dtypes, shapes and the one device of a bank of `aggpost_bank` -> (N, K); ValueError otherwise."""
    def bad(why):
        return ValueError(f'{who}: not a bank of aggpost_bank ({why})')
    if not isinstance(bank, dict) or not set(AGGPOST_BANK_KEYS) <= set(bank):
        raise bad('keys ' + ', '.join(AGGPOST_BANK_KEYS) + ' expected')
    mu = bank['mu']
    if not torch.is_tensor(mu) or mu.dtype != torch.float32 or mu.dim() != 2:
        raise bad('mu: a (N, K) fp32 tensor expected')
    N, K = mu.shape
    if not 1 <= K <= AGGPOST_MAX_K or not 1 <= N <= AGGPOST_MAX_BANK:
        raise bad(f'1 <= K <= {AGGPOST_MAX_K} and 1 <= N <= 2^24 expected, got N={N}, K={K}')
    Np = int(L.load().jvae_aggpost_padded_rows(N))           # host only: N rounded up to the kernel's row tile
    shapes = {'log_var': (N, K), 'group': (N,), 'muT': (K, Np), 'wT': (K, Np), 'lvT': (K, Np), 'c': (Np,)}
    for k, shape in shapes.items():
        dt = torch.int32 if k == 'group' else torch.float32
        if not torch.is_tensor(bank[k]) or bank[k].dtype != dt:
            raise bad(f'{k}: a {dt} tensor expected')
        if tuple(bank[k].shape) != shape:
            raise bad(f'{k}: {shape} expected, got {tuple(bank[k].shape)}')
        if bank[k].device != mu.device:
            raise bad(f'{k}: on the device of mu expected')
    return N, K


def aggpost_logdensity(z, bank, zgroup=None, conditional=False, dims=False, status=None):
    """z (M, K) fp32 on the device against a bank of `aggpost_bank` -> (logq (M,) fp32, logq_dims (M, K) fp32 or None): logq =
    log 1/|S_m| sum_{n in S_m} N(z_m; mu_n, diag exp(log_var_n)) with S_m the whole bank, or with `conditional` the rows whose
    group is zgroup[m] ((M,) int32 / int64); with `dims` the same for each coordinate alone.  A pair's exponent is the direct form
    -1/2 (sum_k log_var + sum_k (z - mu)^2 exp(-log_var)), an fp32 fmaf chain over k ascending; every sum is shifted by its
    largest exponent (the difference taken before the scaling), so a query far from every bank row gets a finite value.  The bank
    is partitioned in pieces of `aggpost_partition()` rows whatever M is: a query's bits do not depend on its batch, and a second
    call returns the same bits (no floating-point atomics).  No (M, N) array exists: the workspace is O(M pieces), times K with
    `dims`, and the queries are scored in runs that keep it below AGGPOST_WS_BYTES.  `status` (default `aggpost_status(device)`;
    `aggpost_check_status`) takes AGGPOST_STATUS_BANK for a non-finite stored operand, AGGPOST_STATUS_QUERY for a query with a
    non-finite element (NaN -> NaN, +-inf -> -inf) or one whose every exponent overflows fp32 (-inf), AGGPOST_STATUS_EMPTY for a
    query whose group has no bank row (-inf).  M = 0 returns empty results without a launch; nothing is read back."""
    N, K = aggpost_check_bank(bank)
    if not torch.is_tensor(z) or z.dim() != 2 or z.shape[1] != K:
        raise L.JvaeHipError(f'aggpost_logdensity: z (M, {K}) expected, got {tuple(z.shape) if torch.is_tensor(z) else type(z)}')
    _f32(z, 'aggpost_logdensity: z')
    M = z.shape[0]
    if M >= 1 << 31:
        raise L.JvaeHipError(f'aggpost_logdensity: M < 2^31 expected, got {M} (unsupported configuration)')
    conditional = bool(conditional)
    if conditional:
        if not torch.is_tensor(zgroup) or zgroup.dtype not in (torch.int32, torch.int64) or tuple(zgroup.shape) != (M,):
            raise L.JvaeHipError(f'aggpost_logdensity: the conditional form needs zgroup ({M},) int32 or int64')
        if zgroup.device != z.device:
            raise L.JvaeHipError('aggpost_logdensity: zgroup on the device of z expected')
    elif zgroup is not None:
        raise L.JvaeHipError('aggpost_logdensity: zgroup is read by the conditional form only (conditional=True)')
    dev = z.device
    if bank['mu'].device != dev:
        raise L.JvaeHipError('aggpost_logdensity: the bank on the device of z expected')
    z = _c(z)
    L.ptr(z)
    zg = _c(zgroup.to(torch.int32)) if conditional else None
    logq = torch.empty(M, dtype=torch.float32, device=dev)
    logq_dims = torch.empty((M, K), dtype=torch.float32, device=dev) if dims else None
    if not M:
        return logq, logq_dims
    status = _status_word('aggpost', dev, status, 'aggpost_logdensity', 'queries')
    lib = L.load()
    run = max(64, AGGPOST_WS_BYTES // lib.jvae_aggpost_workspace_bytes(1, N, K, int(bool(dims))) // 64 * 64)
    operands = [L.ptr(bank[k]) for k in ('muT', 'wT', 'lvT', 'c')]
    for a in range(0, M, run):
        b = min(M, a + run)
        nbytes = lib.jvae_aggpost_workspace_bytes(b - a, N, K, int(bool(dims)))
        L.check(lib.jvae_aggpost_logdensity_f32(L.ptr(z[a:b]), L.ptr(zg[a:b]) if conditional else None, *operands,
                                                L.ptr(bank['group']) if conditional else None, L.ptr(logq[a:b]),
                                                L.ptr(logq_dims[a:b]) if dims else None, b - a, N, K, int(conditional),
                                                L.ptr(status), *_aligned_ws(nbytes, dev, what='aggpost_logdensity'), L.stream_ptr()),
                'jvae_aggpost_logdensity_f32')
    return logq, logq_dims


def aggpost_check_status(status=None):
    """Raise JvaeHipError for what `aggpost_logdensity` flagged.  status: the word given to the op (a device tensor: read here -
    this is the synchronisation - and cleared), a host value, or None for the per-device default words."""
    word = _read_status('aggpost', status)
    if word & AGGPOST_STATUS_BANK:
        raise L.JvaeHipError('aggpost_logdensity: the bank holds a non-finite operand (mu, exp(-log_var) or a row\'s sum of log_var)')
    if word & AGGPOST_STATUS_QUERY:
        raise L.JvaeHipError('aggpost_logdensity: a query with a non-finite element, or one so far from the bank that every '
                             'exponent overflows fp32, was met (its outputs hold -inf / NaN)')
    if word & AGGPOST_STATUS_EMPTY:
        raise L.JvaeHipError('aggpost_logdensity: a query whose group has no bank row was met (its outputs hold -inf)')


# ------------------------------------------------------------ 2-D projections: exact t-SNE and PCA (csrc/embed.hip)
EMBED_MAX_N = 16384         # points of a t-SNE: a row of fp32 distances in LDS
EMBED_MAX_K = 1024          # dimensions of the points
EMBED_MAX_COMPONENTS = 16


def _embed_rows(x, what):
    x = _c(_f32(x, what))
    L.ptr(x)
    if x.dim() != 2 or x.shape[1] < 1:
        raise L.JvaeHipError(f'{what}: (N, K) expected, got {tuple(x.shape)}')
    return x


def pairwise_sqdist(x):
    """x (N, K) fp32 -> d (N, N) fp32, d_ij = fp32(sum_k (double(x_ik) - double(x_jk))^2) with k ascending: exactly symmetric,
    the diagonal exactly 0.  2 <= N <= EMBED_MAX_N, K <= EMBED_MAX_K.  One launch, nothing synchronised."""
    x = _embed_rows(x, 'pairwise_sqdist')
    N, K = x.shape
    d = torch.empty((N, N), dtype=torch.float32, device=x.device)
    L.check(L.load().jvae_pairwise_sqdist_f32(L.ptr(x), L.ptr(d), N, K, L.stream_ptr()), 'jvae_pairwise_sqdist_f32')
    return d


def tsne_affinities(d, perplexity):
    """d (N, N) fp32 squared distances -> (P (N, N) fp32, beta (N,) fp64, S (N,) fp64): scikit-learn's perplexity search per row
    in fp64 (beta_i, and the sum S_i of exp(-d_ij beta_i) over j != i) and the joint probabilities
    max((p_j|i + p_i|j) / sum, 2^-52) formed in fp64 and rounded once.  Three launches, nothing synchronised."""
    d = _embed_rows(d, 'tsne_affinities')
    N = d.shape[0]
    if d.shape[1] != N:
        raise L.JvaeHipError(f'tsne_affinities: a square (N, N) matrix expected, got {tuple(d.shape)}')
    lib = L.load()
    ws, nbytes = _aligned_ws(lib.jvae_tsne_affinities_workspace_bytes(N), d.device, what='tsne_affinities')
    P = torch.empty_like(d)
    beta = torch.empty(N, dtype=torch.float64, device=d.device)
    S = torch.empty(N, dtype=torch.float64, device=d.device)
    L.check(lib.jvae_tsne_affinities_f32(L.ptr(d), L.ptr(P), L.ptr(beta), L.ptr(S), float(perplexity), N, ws, nbytes,
                                         L.stream_ptr()), 'jvae_tsne_affinities_f32')
    return P, beta, S


def tsne_gradient(P, y, exaggeration=1., g=None, stats=None):
    """P (N, N) fp32, y (N, 2) fp32 -> g (N, 2) fp32, the gradient of KL(exaggeration P || Q) in y: pair arithmetic and sums in
    fp64, one rounding.  stats: a (2,) fp64 device tensor that receives the KL divergence and |g|_2 (a second pass), or None.
    Nothing is synchronised."""
    P, y = _embed_rows(P, 'tsne_gradient'), _embed_rows(y, 'tsne_gradient')
    N = P.shape[0]
    if P.shape[1] != N or tuple(y.shape) != (N, 2) or y.device != P.device:
        raise L.JvaeHipError(f'tsne_gradient: P (N, N) and y (N, 2) on one device expected, got {tuple(P.shape)} and {tuple(y.shape)}')
    if g is None:
        g = torch.empty_like(y)
    if g.dtype != torch.float32 or g.shape != y.shape or g.device != y.device or not g.is_contiguous():
        raise L.JvaeHipError('tsne_gradient: g (N, 2) fp32, dense, on the device of y expected')
    if stats is not None and (stats.dtype != torch.float64 or tuple(stats.shape) != (2,) or stats.device != y.device):
        raise L.JvaeHipError('tsne_gradient: stats (2,) fp64 on the device of y expected')
    lib = L.load()
    ws, nbytes = _aligned_ws(lib.jvae_tsne_gradient_workspace_bytes(N), P.device, what='tsne_gradient')
    L.check(lib.jvae_tsne_gradient_f32(L.ptr(P), L.ptr(y), L.ptr(g), float(exaggeration), N, L.ptr(stats), ws, nbytes,
                                       L.stream_ptr()), 'jvae_tsne_gradient_f32')
    return g


def tsne_update(y, update, gains, g, momentum, lr, norm=None):
    """One step of scikit-learn's gradient descent, in place on y, update, gains and g (all (N, 2) fp32), as numpy executes it in
    fp32: gains = max(gains + 0.2 where update * g < 0 else gains * 0.8, 0.01), g *= gains, update = momentum * update - lr * g,
    y += update.  norm: a (1,) fp64 device tensor that receives |g|_2 of the scaled g, or None.  Nothing is synchronised."""
    for t in (y, update, gains, g):
        _f32(t, 'tsne_update')
        L.ptr(t)
        if t.dim() != 2 or t.shape[1] != 2 or t.shape != y.shape or t.device != y.device:
            raise L.JvaeHipError('tsne_update: y, update, gains and g (N, 2) fp32 on one device expected')
    if norm is not None and (norm.dtype != torch.float64 or norm.numel() != 1 or norm.device != y.device):
        raise L.JvaeHipError('tsne_update: norm (1,) fp64 on the device of y expected')
    L.check(L.load().jvae_tsne_update_f32(L.ptr(y), L.ptr(update), L.ptr(gains), L.ptr(g), float(momentum), float(lr), y.shape[0],
                                          L.ptr(norm), L.stream_ptr()), 'jvae_tsne_update_f32')
    return y


def pca_moments(x):
    """x (N, K) fp32 -> (mean (K,) fp64, cov (K, K) fp64): the column means and the centred covariance / (N - 1), summed in fp64
    over slabs of rows folded in a fixed order.  N >= 2, K <= EMBED_MAX_K.  Four launches, nothing synchronised."""
    x = _embed_rows(x, 'pca_moments')
    N, K = x.shape
    lib = L.load()
    mean = torch.empty(K, dtype=torch.float64, device=x.device)
    cov = torch.empty((K, K), dtype=torch.float64, device=x.device)
    if N < 2:
        raise L.JvaeHipError('pca_moments: at least two rows expected')
    ws, nbytes = _aligned_ws(lib.jvae_pca_moments_workspace_bytes(N, K), x.device, what='pca_moments')
    L.check(lib.jvae_pca_moments_f32(L.ptr(x), L.ptr(mean), L.ptr(cov), N, K, ws, nbytes, L.stream_ptr()), 'jvae_pca_moments_f32')
    return mean, cov


def project(x, mean, V):
    """fp32((x - mean) V^T): x (N, K) fp32, mean (K,) fp64, V (n_components, K) fp64 -> (N, n_components) fp32, accumulated in
    fp64 with k ascending.  n_components <= EMBED_MAX_COMPONENTS.  One launch, nothing synchronised."""
    x = _embed_rows(x, 'project')
    N, K = x.shape
    L.ptr(mean), L.ptr(V)
    if mean.dtype != torch.float64 or V.dtype != torch.float64 or tuple(mean.shape) != (K,) or V.dim() != 2 or V.shape[1] != K \
            or V.shape[0] < 1 or mean.device != x.device or V.device != x.device:
        raise L.JvaeHipError('project: mean (K,) and V (n_components, K) fp64 on the device of x expected')
    out = torch.empty((N, V.shape[0]), dtype=torch.float32, device=x.device)
    if N:
        L.check(L.load().jvae_project_f32(L.ptr(x), L.ptr(_c(mean)), L.ptr(_c(V)), L.ptr(out), N, K, V.shape[0], L.stream_ptr()),
                'jvae_project_f32')
    return out


def misclass_split(scores, mask):
    """(M, N) fp32 score rows and an (N,) mask (non-zero / True = correctly classified) -> ins (M, n_correct), outs
    (M, N - n_correct), n_correct: both row sets compacted in their original order by ONE scan of the mask (two views of one
    M * N buffer).  n_correct (a Python int) is the single value read from the device."""
    lib = L.load()
    scores = _c(_f32(scores, 'misclass_split'))
    L.ptr(scores), L.ptr(_c(mask))
    if scores.dim() != 2 or scores.shape[0] < 1 or scores.shape[1] < 1:
        raise L.JvaeHipError(f'misclass_split: (M, N) score rows expected, got {tuple(scores.shape)}')
    M, N = scores.shape
    mask = _mask_u8(mask, N, 'misclass_split')
    nbytes = lib.jvae_misclass_split_workspace_bytes(N)
    if not nbytes or M > 65535:
        raise L.JvaeHipError(f'misclass_split: sizes out of range (M={M}, N={N})')
    ws = L.workspace(nbytes, scores.device)
    out = torch.empty(M * N, dtype=torch.float32, device=scores.device)
    count = torch.empty(1, dtype=torch.int32, device=scores.device)
    L.check(lib.jvae_misclass_split_f32(L.ptr(scores), L.ptr(mask), L.ptr(out), L.ptr(count), M, N, L.ptr(ws), ws.numel(),
                                        L.stream_ptr()), 'jvae_misclass_split_f32')
    nc = int(count.item())
    return out[:M * nc].view(M, nc), out[M * nc:].view(M, N - nc), nc


def misclass_confusion(scores, mask, thr):
    """tp / fp (M, K) int32 on the device: the correctly / wrongly classified samples whose score is >= thr[m, k] (cvae.py:2009-2015);
    thr: (M, K) fp64 (the 'low' thresholds of `roc_curve`), K <= 16.  Compared on exactly widened fp32 scores."""
    scores = _c(_f32(scores, 'misclass_confusion'))
    L.ptr(scores), L.ptr(_c(mask)), L.ptr(_c(thr))
    if scores.dim() != 2 or thr.dim() != 2 or thr.shape[0] != scores.shape[0] or thr.dtype != torch.float64 \
            or not 1 <= thr.shape[1] <= MISCLASS_MAX_KEPT:
        raise L.JvaeHipError(f'misclass_confusion: (M, N) fp32 scores and (M, K <= {MISCLASS_MAX_KEPT}) fp64 thresholds expected, '
                             f'got {tuple(scores.shape)} and {tuple(thr.shape)} {thr.dtype}')
    M, N = scores.shape
    K = thr.shape[1]
    mask, thr = _mask_u8(mask, N, 'misclass_confusion'), _c(thr)
    counts = torch.empty((2, M, K), dtype=torch.int32, device=scores.device)
    L.check(L.load().jvae_misclass_confusion_f32(L.ptr(scores), L.ptr(mask), L.ptr(thr), L.ptr(counts[0]), L.ptr(counts[1]),
                                                 M, N, K, L.stream_ptr()), 'jvae_misclass_confusion_f32')
    return counts[0], counts[1]


def misclass_rates(scores, correct_mask, kept_tpr, pr=False):
    """The device side of misclassification_detection_rates for M score rows of one prediction method: ONE split, ONE ROC
    (correct = in, missed = out, one-sided) and ONE confusion call.  -> dict of DEVICE tensors 'auc' (M,), 'fpr' / 'tpr' / 'low' /
    'up' (M, K) fp64, 'tp' / 'fp' (M, K) int32, 'status' (M,) int32 as `roc_curve` returns it, and 'n_correct' (Python int).
    With `pr`, also 'pr' (M, 5) fp64: the PR_FIGURES of ONE `pr_metrics` call on the same two row sets (correct = positive, then
    missed = positive with the score negated).
    ValueError when every sample - or none - is correct: there is no ROC of an empty set."""
    single = scores.dim() == 1
    scores = scores[None] if single else scores
    ins, outs, nc = misclass_split(scores, correct_mask)
    if nc == 0 or nc == scores.shape[1]:
        raise ValueError(f'misclass_rates: {nc} of {scores.shape[1]} samples are correct, no ROC of an empty set')
    res = roc_curve(ins, outs, kept_tpr, False)
    res['tp'], res['fp'] = misclass_confusion(scores, correct_mask, res['low'])
    if pr:
        figures = pr_metrics(ins, outs, False)
        res['pr'] = torch.stack([figures[k] for k in PR_FIGURES], 1)
    res ={k: v[0] for k, v in res.items()} if single else res
    res['n_correct'] = nc
    return res


# ------------------------------------------------------------------------------------------- ODIN (csrc/odin.hip)
def odin_head(logits, temps, want_grad=False, forwards_first=True):
    """Scores of F batched forwards: max softmax(mean over the draws l >= 1 of logits / T_f) -> (F, N) [, d(sum scores)/d(logits)].
    logits (F, L+1, N, C) - or (L+1, F, N, C) with forwards_first=False; temps: (F,) fp32 device tensor."""
    logits = _c(_f32(logits, 'odin_head'))
    if logits.dim() != 4:
        raise L.JvaeHipError(f'odin_head: 4-d logits expected, got {tuple(logits.shape)}')
    if forwards_first:
        F, L1, N, C = logits.shape
        sf, sl = L1 * N * C, N * C
    else:
        L1, F, N, C = logits.shape
        sf, sl = N * C, F * N * C
    temps = _c(_f32(temps, 'odin_head'))
    if temps.numel() != F or L1 < 2:
        raise L.JvaeHipError(f'odin_head: {temps.numel()} temperatures for {F} forwards of {L1 - 1} draws')
    scores = torch.empty((F, N), device=logits.device, dtype=torch.float32)
    dlogits = torch.empty_like(logits) if want_grad else None
    L.check(L.load().jvae_odin_head_f32(L.ptr(logits), L.ptr(temps), L.ptr(scores), L.ptr(dlogits), F, L1 - 1, N, C, sf, sl,
                                        L.stream_ptr()), 'jvae_odin_head_f32')
    return (scores, dlogits) if want_grad else scores


def odin_perturb(acc, g, x, eps):
    """acc += g (in place; g None: acc as it is), then -> (E * N, ...) = x + eps_e * sign(acc) for the E sizes of `eps`
    ((E,) fp32 device tensor), sign(0) = 0: the operand of the batched perturbed forward."""
    x = _c(_f32(x, 'odin_perturb'))
    eps = _c(_f32(eps, 'odin_perturb'))
    if not acc.is_contiguous() or acc.dtype != torch.float32 or acc.shape != x.shape or (g is not None and g.shape != x.shape):
        raise L.JvaeHipError('odin_perturb: acc (and g) must be dense fp32 tensors shaped like x')
    g = None if g is None else _c(_f32(g, 'odin_perturb'))
    E = eps.numel()
    out = torch.empty((E * x.shape[0], *x.shape[1:]), device=x.device, dtype=torch.float32)
    L.check(L.load().jvae_odin_perturb_f32(L.ptr(acc), L.ptr(g), L.ptr(x), L.ptr(eps), L.ptr(out), x.numel(), E,
                                           L.stream_ptr()), 'jvae_odin_perturb_f32')
    return out


# ------------------------------------------------------------------------------------------- input pipeline
def augment_batch(images_u8, flip=None, dy=None, dx=None, pad=0, nhwc=True):
    """uint8 batch (N,H,W,C) [or (N,C,H,W) with nhwc=False] -> float32 (N,C,H,W) in [0,1] with the reference's training
    augmentation (utils/torch_load.py:405-426): horizontal flip where flip[n], then edge padding by `pad` and a crop at
    (dy[n], dx[n]) in [0, 2*pad].  flip: uint8/bool (N,), dy/dx: int32 (N,), all on the device (None = identity)."""
    if images_u8.dtype != torch.uint8:
        raise L.JvaeHipError('augment_batch expects a uint8 batch')
    images_u8 = _c(images_u8)
    if nhwc:
        N, H, W, C = images_u8.shape
    else:
        N, C, H, W = images_u8.shape
    out = torch.empty((N, C, H, W), device=images_u8.device, dtype=torch.float32)
    f = None if flip is None else _c(flip.to(torch.uint8))
    a = None if dy is None else _c(dy.to(torch.int32))
    b = None if dx is None else _c(dx.to(torch.int32))
    rc = L.load().jvae_augment_u8_f32(L.ptr(images_u8), L.ptr(f), L.ptr(a), L.ptr(b), L.ptr(out), N, C, H, W, int(pad),
                                      int(nhwc), L.stream_ptr())
    L.check(rc, 'jvae_augment_u8_f32')
    return out


def draw_augmentation(N, pad, device, generator=None, flip=True, crop=True):
    """Random decisions of RandomHorizontalFlip(p=0.5) / RandomCrop(padding=pad) for N images, on the device."""
    f = (torch.rand(N, device=device, generator=generator) < 0.5) if flip else None
    dy = torch.randint(0, 2 * pad + 1, (N,), device=device, generator=generator, dtype=torch.int32) if crop else None
    dx = torch.randint(0, 2 * pad + 1, (N,), device=device, generator=generator, dtype=torch.int32) if crop else None
    return f, dy, dx



# ------------------------------------------------------------------------------------------- device-resident image sets
class ImagesetDesc:
    """Static transform chain of a device-resident image set (csrc/imageset.hip; the slots of include/jvae_hip.h), checked on
    the host ONCE so that no launch can read outside an image: extents through every stage, the resize tables against the
    extents they index.  `source` = (Hs, Ws, Cs); A, B = quarter-turn/flip elements k + 4 f; resize = None or (Hr, Wr, coef_h,
    bounds_h, coef_v, bounds_v) with the int32 CPU tables of jvae_compat.torch_load.pil_bilinear_tables; post = None | 'pad' |
    ('crop', th, tw).  `.shape` is the (C, H, W) of the batches; `.with_pa(pa)` is the same chain with the random crop's padding."""

    def __init__(self, source, nhwc, A=0, resize=None, p0=0, B=0, g2c=False, pa=0, post=None, device=None):
        Hs, Ws, Cs = (int(v) for v in source)
        if Cs not in (1, 3) or Hs < 1 or Ws < 1 or not 0 <= A < 8 or not 0 <= B < 8 or p0 < 0 or pa < 0 or (g2c and Cs != 1):
            raise ValueError(f'imageset chain: source {source}, A={A}, B={B}, p0={p0}, pa={pa}, g2c={g2c}')
        H, W = (Ws, Hs) if A & 1 else (Hs, Ws)
        self.tables = (None,) * 4
        rs = [0, 0, 0, 0, 0]
        if resize is not None:
            Hr, Wr, ch, bh, cv, bv = resize
            for name, coef, bnd, out, size in (('horizontal', ch, bh, Wr, W), ('vertical', cv, bv, Hr, H)):
                coef, bnd = torch.as_tensor(coef), torch.as_tensor(bnd)
                ok = (coef.dtype == bnd.dtype == torch.int32 and coef.dim() == 2 and tuple(bnd.shape) == (out, 2)
                      and coef.shape[0] == out and int(bnd.min()) >= 0 and int(bnd[:, 1].max()) <= coef.shape[1]
                      and int((bnd[:, 0] + bnd[:, 1]).max()) <= size and int(coef.min()) >= 0)
                if not ok:
                    raise ValueError(f'imageset chain: the {name} resize tables do not fit {size} -> {out}')
            rs = [1, int(Hr), int(Wr), int(ch.shape[1]), int(cv.shape[1])]
            self.tables = tuple(_c(torch.as_tensor(t).to(device)) for t in (ch, bh, cv, bv))
            H, W = int(Hr), int(Wr)
        H, W = H + 2 * p0, W + 2 * p0
        if B & 1:
            H, W = W, H
        oy = ox = 0
        if post == 'pad':
            kind, H, W = 1, H + 4, W + 4
        elif post:
            _, th, tw = post
            if th > H or tw > W:
                raise ValueError(f'imageset chain: centre crop to ({th}, {tw}) of a ({H}, {W}) image')
            kind, oy, ox, H, W = 2, int(round((H - th) / 2.)), int(round((W - tw) / 2.)), int(th), int(tw)
        else:
            kind = 0
        self.shape = (3 if g2c else Cs, H, W)
        self.source, self.nhwc, self.pa = (Hs, Ws, Cs), bool(nhwc), int(pa)
        self._args = dict(source=source, nhwc=nhwc, A=A, resize=resize, p0=p0, B=B, g2c=g2c, post=post, device=device)
        words = [int(bool(nhwc)), Hs, Ws, Cs, int(A)] + rs + [int(p0), int(B), int(bool(g2c)), int(pa), kind, oy, ox, *self.shape]
        assert len(words) == L.load().jvae_imageset_desc_words()
        self.words = (ctypes.c_int * len(words))(*words)
        self._pads = {self.pa: self}

    def with_pa(self, pa):
        d = self._pads.get(int(pa))
        if d is None:
            self._pads[int(pa)] = d = ImagesetDesc(pa=int(pa), **self._args)
            d._pads = self._pads
        return d


def imageset_batch(data, idx, desc, targets, lut=None, flip=None, dy=None, dx=None):
    """-> (x float32 (N, C, H, W), y int64 (N,)): images data[idx] of a device-resident uint8 set through the static chain
    `desc` (an ImagesetDesc) and, where given, the random flip / crop decisions of `draw_augmentation`; y = lut[targets[idx]]
    (lut None: identity).  `idx`: int64 on the device, every entry in [0, len(data)) - checked by the caller
    (DeviceImageSet.batch does it on the host before the upload), the kernel has no trap.  Does not synchronise."""
    if data.dtype != torch.uint8 or data.dim() != 4 or idx.dtype != torch.int64 or targets.dtype != torch.int64 or (
            lut is not None and lut.dtype != torch.int64):
        raise L.JvaeHipError('imageset_batch: data uint8 (n, ., ., .), idx / targets / lut int64')
    Hs, Ws, Cs = desc.source
    if tuple(data.shape[1:]) != ((Hs, Ws, Cs) if desc.nhwc else (Cs, Hs, Ws)) or targets.numel() != data.shape[0]:
        raise L.JvaeHipError(f'imageset_batch: data {tuple(data.shape)} / {targets.numel()} targets against the chain of {desc.source}')
    data, idx, targets = _c(data), _c(idx), _c(targets)
    N = idx.numel()
    x = torch.empty((N, *desc.shape), device=data.device, dtype=torch.float32)
    y = torch.empty((N,), device=data.device, dtype=torch.int64)
    f = None if flip is None else _c(flip.to(torch.uint8))
    a = None if dy is None else _c(dy.to(torch.int32))
    b = None if dx is None else _c(dx.to(torch.int32))
    for t in (f, a, b):
        if t is not None and t.numel() != N:
            raise L.JvaeHipError('imageset_batch: one flip / dy / dx decision per index')
    rc = L.load().jvae_imageset_batch_u8_f32(L.ptr(data), L.ptr(idx), L.ptr(targets), L.ptr(None if lut is None else _c(lut)),
                                             desc.words, *(L.ptr(t) for t in desc.tables), L.ptr(f), L.ptr(a), L.ptr(b),
                                             L.ptr(x), L.ptr(y), data.shape[0], N, L.stream_ptr())
    L.check(rc, 'jvae_imageset_batch_u8_f32')
    return x, y



class _MixLeaf(ctypes.Structure):
    """One leaf record of csrc/imageset.hip (struct MixLeaf)."""
    _fields_ = [('kind', ctypes.c_int), ('border', ctypes.c_int)] + [
        (n, ctypes.c_void_p) for n in ('data', 'targets', 'lut', 'coef_h', 'bounds_h', 'coef_v', 'bounds_v')] + [('desc', ctypes.c_int * 20)]


class ImagesetMixTable:
    """What one launch of `imageset_mixed_batch` needs of a resolved moving set (jvae_compat.ft_datasets: `resolve()`), built
    once and kept on `device`: a record per leaf - kind (image set / const / uniform), the pointers of the leaf's `data`,
    `targets`, `lut` and resize tables, its 20 descriptor words - and the per-item arrays `leaf`, `index`, `tag`.  A leaf is a
    device-resident image set (`.data`, `.targets`, `.lut`, `.desc`) or a synthetic one (`.data` None, `.kind` 'const' /
    'uniform', `.image_shape`, `.transformer`).  Everything a launch could read outside of is checked here, on the host:
    leaf numbers, every sample index against its leaf's length, tags; ValueError when the leaves' chains do not all end in the
    same (C, H, W), a leaf carries its own data_augmentation (a mixed batch has no random flip / crop) or holds a tensor that
    is not contiguous.  The table keeps every
    tensor whose pointer it stored; `matches()` tells whether it still describes the set (else: build another)."""

    KINDS = {'const': 1, 'uniform': 2}

    def __init__(self, leaves, leaf, index, tag, device):
        device = torch.device(device)
        leaves = list(leaves)
        if not leaves:
            raise ValueError('mixed image set: no leaf')
        shapes, kinds = [], []
        for l in leaves:
            if tuple(getattr(l, 'data_augmentation', ())):
                raise ValueError('mixed image set: {} carries its own data_augmentation {}; a mixed batch has no random flip / '
                                 'crop'.format(getattr(l, 'name', 'leaf'), list(l.data_augmentation)))
            if l.data is None:
                kind = self.KINDS.get(getattr(l, 'kind', None))
                if kind is None:
                    raise ValueError('mixed image set: {} is neither resident nor const / uniform'.format(getattr(l, 'name', 'leaf')))
                C, H, W = l.image_shape
                pad = 4 if l.transformer == 'pad' else 0
                shapes.append((C, H + pad, W + pad))
            else:
                kind = 0
                shapes.append(tuple(l.desc.shape))
            kinds.append(kind)
        if len(set(shapes)) != 1:
            raise ValueError('mixed image set: the leaves do not end in one shape: ' + ', '.join(
                '{} {}'.format(getattr(l, 'name', 'leaf'), s) for l, s in zip(leaves, shapes)))
        self.shape, self.kinds = shapes[0], tuple(kinds)
        self.u_dims = 4 if 2 in kinds else (2 if 1 in kinds else 0)
        leaf_np, index_np, tag_np = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (leaf, index, tag))
        n = len(leaf_np)
        if not (len(index_np) == len(tag_np) == n):
            raise ValueError('mixed image set: leaf, index and tag of one length')
        if n and (leaf_np.min() < 0 or leaf_np.max() >= len(leaves) or tag_np.min() < 0):
            raise IndexError('mixed image set: a leaf number outside the {} leaves, or a negative tag'.format(len(leaves)))
        lengths = np.asarray([len(l) for l in leaves], np.int64)
        if n and (index_np.min() < 0 or bool((index_np >= lengths[leaf_np]).any())):
            bad = int(np.flatnonzero((index_np < 0) | (index_np >= lengths[leaf_np]))[0])
            raise IndexError('mixed image set: item {} is sample {} of the {} of {}'.format(
                bad, int(index_np[bad]), int(lengths[leaf_np[bad]]), getattr(leaves[leaf_np[bad]], 'name', 'leaf')))
        self.n_items, self.device = n, device
        self._source = (leaves, leaf, index, tag)
        keep, records = [], (_MixLeaf * len(leaves))()
        for rec, l, kind in zip(records, leaves, kinds):
            rec.kind, rec.border = kind, int(kind != 0 and l.transformer == 'pad')
            words = [0] * 17 + list(self.shape)
            if kind == 0:
                desc = l.desc.with_pa(0)
                tensors = [l.data, l.targets, l.lut, *desc.tables]
                if not all(t is None or t.is_contiguous() for t in tensors):      # the table stores pointers, never a copy
                    raise ValueError('mixed image set: {} holds a tensor that is not contiguous'.format(getattr(l, 'name', 'leaf')))
                Hs, Ws, Cs = desc.source
                if (l.data.dtype != torch.uint8 or tuple(l.data.shape[1:]) != ((Hs, Ws, Cs) if desc.nhwc else (Cs, Hs, Ws))
                        or l.targets.dtype != torch.int64 or l.targets.numel() != l.data.shape[0]
                        or (l.lut is not None and l.lut.dtype != torch.int64)):
                    raise ValueError('mixed image set: {}: data {} / {} targets against the chain of {}'.format(
                        getattr(l, 'name', 'leaf'), tuple(l.data.shape), l.targets.numel(), desc.source))
                for t in tensors:
                    if t is not None and t.device != device:
                        raise ValueError('mixed image set: {} is on {}, the table on {}'.format(getattr(l, 'name', 'leaf'), t.device, device))
                for name, t in zip(('data', 'targets', 'lut', 'coef_h', 'bounds_h', 'coef_v', 'bounds_v'), tensors):
                    setattr(rec, name, L.ptr(t))
                keep += [t for t in tensors if t is not None]
                words = list(desc.words)
            rec.desc[:] = words
        assert ctypes.sizeof(_MixLeaf) == L.load().jvae_imageset_mix_leaf_bytes()
        self.records = records
        raw = np.frombuffer(bytes(records), np.uint8).copy()
        self.records_dev = torch.from_numpy(raw).to(device)
        self.leaf = torch.from_numpy(leaf_np.astype(np.int32)).to(device)
        self.index = torch.tensor(index_np).to(device)
        self.tag = torch.tensor(tag_np).to(device)
        self._keep = keep
        self._pointers = [t.data_ptr() for t in keep]

    def matches(self, leaves, leaf, index, tag):
        """Whether the table was built from these very arrays and every leaf's tensors are where they were."""
        mine = self._source
        if len(leaves) != len(mine[0]) or any(a is not b for a, b in zip(leaves, mine[0])):
            return False
        if leaf is not mine[1] or index is not mine[2] or tag is not mine[3]:
            return False
        now = []
        for l, kind in zip(leaves, self.kinds):
            if kind == 0:
                now += [t for t in (l.data, l.targets, l.lut, *l.desc.with_pa(0).tables) if t is not None]
        return len(now) == len(self._keep) and all(t.device == self.device and t.is_contiguous() and t.data_ptr() == p
                                                   for t, p in zip(now, self._pointers))


def imageset_mixed_batch(table, pos, u=None, vec=0):
    """-> (x float32 (N, C, H, W), tag int64 (N,), y int64 (N,)): the items `pos` (int64 on the device, every entry in
    [0, table.n_items) - checked by the caller on the host before the upload, the kernel has no trap) of a resolved moving set,
    each through the chain of its own leaf, in ONE launch.  `u`: what the synthetic leaves show, float32 drawn by the caller -
    (N, C) when only const leaves occur, (N, C, H, W) when a uniform leaf occurs, None without synthetic leaves.  `vec`:
    consecutive x per thread (1 | 4), 0 = the default.  Does not synchronise."""
    if pos.dtype != torch.int64 or pos.device != table.device:
        raise L.JvaeHipError('imageset_mixed_batch: pos int64 on the device of the table')
    pos = _c(pos.reshape(-1))
    N = pos.numel()
    C, H, W = table.shape
    if table.u_dims:
        want = (N, C) if table.u_dims == 2 else (N, C, H, W)
        if u is None or u.dtype != torch.float32 or tuple(u.shape) != want or u.device != table.device:
            raise L.JvaeHipError(f'imageset_mixed_batch: u float32 {want} on the device for the synthetic leaves')
        u = _c(u)
    elif u is not None:
        raise L.JvaeHipError('imageset_mixed_batch: u given, but the set has no synthetic leaf')
    x = torch.empty((N, C, H, W), device=table.device, dtype=torch.float32)
    tag = torch.empty((N,), device=table.device, dtype=torch.int64)
    y = torch.empty((N,), device=table.device, dtype=torch.int64)
    rc = L.load().jvae_imageset_mixed_u8_f32(ctypes.addressof(table.records), L.ptr(table.records_dev), len(table.kinds),
                                             L.ptr(table.leaf), L.ptr(table.index), L.ptr(table.tag), L.ptr(pos), L.ptr(u),
                                             table.u_dims, L.ptr(x), L.ptr(tag), L.ptr(y), N, int(vec), L.stream_ptr())
    L.check(rc, 'jvae_imageset_mixed_u8_f32')
    return x, tag, y


from . import ops_b8 as _b8  # noqa: E402  (the B8 layout; it builds on the fp32 wrappers above)
