"""Every swept case of tests/conv_cases.py on the device: the route is asserted first (no case passes on another kernel), then
forward (with its BatchNorm partial sums), dgrad and the weight gradient (fresh, and accumulated onto a non-zero gradient, with
the bias gradient) run through the raw ops and are compared with an fp64 PyTorch-CPU reference of the same operation - every
element against a derived rounding bound, every (image, channel) plane and every filter on its own scale at the project's bars
(conv_cases.elementwise_excess / plane_err), two runs bit for bit.  bf16-layout cases as tests/test_1_b8_gpu.py: operands
rounded to bf16 first, the reference on the rounded values."""
import ctypes

import pytest
import torch

import conv_cases as cc
from jvae_hip import lib, ops, ops_b8

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DIRS = ('fwd', 'dgrad', 'wgrad')


@pytest.fixture(autouse=True)
def _switches():
    L = lib.load()
    old = L.jvae_conv2d_set_split_bf16(1), L.jvae_conv2d_set_split_shape16(1)
    yield
    L.jvae_conv2d_set_split_bf16(old[0])
    L.jvae_conv2d_set_split_shape16(old[1])


def check(case, what, direction, kernel, y, ref, A, K, c=4, out_u=0.0):
    """Elementwise bound, then the per-plane (per-filter) bar of the kernel that ran."""
    ex = cc.elementwise_excess(y, ref, A, K, c, out_u)
    if ref.dim() == 4:
        worst, where = cc.worst_plane(y, ref, A)
    else:           # a bias gradient: every channel on its own scale
        e = (y.detach().double().cpu() - ref).abs() / A.clamp_min(1e-300)
        worst, where = float(e.max()), int(e.argmax())
    limit = cc.bar(case, direction, kernel)
    print(f'{case.name} [{what}] {kernel}: elementwise {ex:.3g} of the bound, worst plane {worst:.3g} at {where} (bar {limit:.3g})')
    assert ex <= 1, (case.name, what, kernel, ex)
    assert worst < limit, (case.name, what, kernel, worst, where, limit)


def check_stats(case, st, ns, cap, ref_nobias, b8):
    """BatchNorm partial sums of (y - bias) against the fp64 sums, per channel, relative to the channel's absolute sum."""
    cout = case.spec.cout
    assert 0 < ns <= cap, (case.name, ns, cap)
    part = st[:cout * ns * 2].view(cout, ns, 2).double().sum(1).cpu()
    d = ref_nobias
    s1, s2, a1 = d.sum((0, 2, 3)), (d * d).sum((0, 2, 3)), d.abs().sum((0, 2, 3))
    if b8:          # the bars of tests/test_1_b8_gpu.py
        assert torch.allclose(part[:, 0], s1, rtol=1e-4, atol=1e-3 * float(a1.max())), case.name
        assert torch.allclose(part[:, 1], s2, rtol=1e-4), case.name
        return
    e1 = float(((part[:, 0] - s1).abs() / a1.clamp_min(1e-300)).max())
    e2 = float(((part[:, 1] - s2).abs() / s2.clamp_min(1e-300)).max())
    print(f'{case.name} [BatchNorm sums] {ns} of {cap} partials: sum {e1:.3g}, sum of squares {e2:.3g} (bar 1e-5)')
    assert e1 < 1e-5 and e2 < 1e-5, (case.name, e1, e2)


def twice(f, cout=0):
    """Two launches, bit for bit (of a forward: y and the BatchNorm partials it wrote; the rest of that buffer is not its)."""
    a, b = f(), f()
    if isinstance(a, tuple) and len(a) == 3:
        assert a[2] == b[2] and torch.equal(a[0], b[0]), 'two runs differ'
        assert a[1] is None or torch.equal(a[1][:cout * a[2] * 2], b[1][:cout * a[2] * 2]), 'two runs differ (BatchNorm sums)'
        return a
    for s, t in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(s, t), 'two runs differ'
    return a


def run_f32(case, d, ref, A, K, routes):
    sp, N, H, W = case.spec, case.N, case.H, case.W
    x, w, gy, g0, b0 = (d[k].to(DEV) for k in ('x', 'w', 'gy', 'g0', 'b0'))
    b = d['b'].to(DEV) if case.bias else None
    aff = (d['sc'].to(DEV), d['sh'].to(DEV), case.aff) if case.aff else None
    ca = 2 if case.aff else 0
    if aff is not None:
        assert ops.conv_affine_ok(sp, N, H, W)
        y, st, ns = twice(lambda: ops.conv_fwd_aff_raw(x, w, b, sp, aff, case.stats), sp.cout)
    elif case.stats:
        y, st, ns = twice(lambda: ops.conv_fwd_stats_raw(x, w, b, sp), sp.cout)
    else:
        y, st, ns = twice(lambda: ops.conv_fwd_raw(x, w, b, sp)), None, 0
    check(case, 'forward', 'fwd', routes['fwd'].kernel, y, ref['fwd'], A['fwd'], K['fwd'], 4 + ca)
    assert (st is not None) == (case.stats and routes['fwd'].splits > 0), (case.name, ns, routes['fwd'].splits)
    if st is not None:
        check_stats(case, st, ns, routes['fwd'].splits, ref['nobias'], False)
    dx = twice(lambda: ops.conv_dgrad_raw(gy, w, sp, x.shape))
    check(case, 'dgrad', 'dgrad', routes['dgrad'].kernel, dx, ref['dgrad'], A['dgrad'], K['dgrad'])
    gw, gb = twice(lambda: ops.conv_wgrad_raw(x, gy, sp, case.wshape, True, aff=aff))
    kw = routes['wgrad'].kernel
    check(case, 'wgrad', 'wgrad', kw, gw, ref['wgrad'], A['wgrad'], K['wgrad'], 4 + ca)
    check(case, 'dbias', 'dbias', 'CK_GENERIC', gb, ref['dbias'], A['dbias'], K['dbias'])
    sw, sb = g0.clone(), b0.clone()
    ops.conv_wgrad_raw(x, gy, sp, case.wshape, True, sw, sb, aff=aff)          # accumulate = 1 onto a non-zero gradient
    g064, b064 = d['g0'].double(), d['b0'].double()
    check(case, 'wgrad, accumulated', 'wgrad', kw, sw, ref['wgrad'] + g064, A['wgrad'] + g064.abs(), K['wgrad'], 5 + ca)
    check(case, 'dbias, accumulated', 'dbias', 'CK_GENERIC', sb, ref['dbias'] + b064, A['dbias'] + b064.abs(), K['dbias'], 5)


def refused(f):
    """A direction without a bf16 kernel: the entry point returns JVAE_ENOTSUP (-2), which the wrappers raise."""
    with pytest.raises(lib.JvaeHipError, match='unsupported configuration'):
        f()


def run_b8(case, d, ref, A, K, routes):
    assert not case.aff, 'the sweep has no bf16 run with a deferred BatchNorm: such rows pin routes only (see conv_cases.py)'
    sp, N, H, W = case.spec, case.N, case.H, case.W
    x, w, gy, g0, b0 = (d[k].to(DEV) for k in ('x', 'w', 'gy', 'g0', 'b0'))
    b = d['b'].to(DEV) if case.bias else None
    xb, gyb = ops_b8.pack(x), ops_b8.pack(gy)
    mask = ops_b8.native_mask(sp, N, H, W)
    assert mask == sum(ops.ROUTE_DIR[k] for k in DIRS if ops.conv_route(sp, N, H, W, k, 'b8').kernel != 'CK_NONE')
    fwd = lambda: ops_b8.conv_fwd_raw(xb, w, b, sp, out_f32=case.y_f32, want_stats=case.stats)
    if routes['fwd'].kernel == 'CK_NONE':
        refused(fwd)
    else:
        y, st, ns = twice(fwd, sp.cout)
        if not case.y_f32:
            y = ops_b8.unpack(y, sp.cout)
        check(case, 'forward', 'fwd', routes['fwd'].kernel, y, ref['fwd'], A['fwd'], K['fwd'], 4, 0.0 if case.y_f32 else cc.UB)
        assert (st is not None) == case.stats, (case.name, ns)
        if st is not None:
            check_stats(case, st, ns, routes['fwd'].splits, ref['nobias'], True)
    dgrad = lambda: ops_b8.conv_dgrad_raw(gyb, w, sp, N, H, W)
    if routes['dgrad'].kernel == 'CK_NONE':
        refused(dgrad)
    else:
        dx = ops_b8.unpack(twice(dgrad), sp.cin)
        check(case, 'dgrad', 'dgrad', routes['dgrad'].kernel, dx, ref['dgrad'], A['dgrad'], K['dgrad'], 4, cc.UB)
    wgrad = lambda: ops_b8.conv_wgrad_raw(xb, gyb, sp, case.wshape, True)
    if routes['wgrad'].kernel == 'CK_NONE':
        refused(wgrad)
        return
    gw, gb = twice(wgrad)
    kw = routes['wgrad'].kernel
    check(case, 'wgrad', 'wgrad', kw, gw, ref['wgrad'], A['wgrad'], K['wgrad'])
    check(case, 'dbias', 'dbias', kw, gb, ref['dbias'], A['dbias'], K['dbias'])
    sw, sb = g0.clone(), b0.clone()
    ops_b8.conv_wgrad_raw(xb, gyb, sp, case.wshape, True, sw, sb)
    g064, b064 = d['g0'].double(), d['b0'].double()
    check(case, 'wgrad, accumulated', 'wgrad', kw, sw, ref['wgrad'] + g064, A['wgrad'] + g064.abs(), K['wgrad'], 5)
    check(case, 'dbias, accumulated', 'dbias', kw, sb, ref['dbias'] + b064, A['dbias'] + b064.abs(), K['dbias'], 5)


@pytest.mark.parametrize('case', cc.SWEEP, ids=lambda c: c.name.replace(' ', '_'))
def test_conv_sweep(case):
    """One case of the table, all directions.  (What it caught: the CK_GENERIC weight gradient on folded grids of more than 48
    positions added its per-image products onto dw with float atomics - two launches of a batch of three gave different bits.)"""
    L = lib.load()
    L.jvae_conv2d_set_split_bf16(case.split)
    L.jvae_conv2d_set_split_shape16(case.sh16)
    routes = {k: case.route(k) for k in DIRS}
    for k in DIRS:
        assert (routes[k].kernel, routes[k].swap) == case.expect[k], \
            f'{case.name} [{k}]: expected {case.expect[k][0]} swap={case.expect[k][1]}, routed to {routes[k].kernel} swap={routes[k].swap}'
    d = cc.make_data(case)
    ref, A, K = cc.references(case, d)
    (run_b8 if case.layout == 'b8' else run_f32)(case, d, ref, A, K, routes)


POISON = 12288.0          # exact in bf16


@pytest.mark.parametrize('name', ['conv32@32.2 N3', 'deconv32@out32.2 N3', 'conv32@32.4 N3', 'deconv32@out32.0 N3',
                                  'image tail aff', 'conv32+@64.2 N3 b8', '9x13 k3x5'])
@pytest.mark.parametrize('split', [1, 0])
def test_an_empty_batch_is_a_no_op(name, split):
    """N = 0 on every entry point of a geometry: 0 is returned, y / dx keep their poison, the weight gradient without
    `accumulate` zeroes dw and dbias and with it leaves them untouched."""
    L = lib.load()
    L.jvae_conv2d_set_split_bf16(split)
    c = cc.CASES[name]
    sp, st = c.spec, lib.stream_ptr()
    geom = sp.geom(0, c.H, c.W)
    oh, ow = sp.out_hw(c.H, c.W)
    b8 = c.layout == 'b8'
    P = lib.ptr
    f32 = lambda *shape: torch.full(shape, POISON, device=DEV)
    if b8:
        act = lambda C, h, w_: torch.full((1, (C + 7) // 8, h, w_, 8), POISON, device=DEV, dtype=torch.bfloat16)
        nb = max(L.jvae_conv2d_workspace_bytes_b8(*geom), 16)        # asked at the batch that runs, as ops does
    else:
        act = lambda C, h, w_: f32(1, C, h, w_)
        nb = max(L.jvae_conv2d_workspace_bytes(*geom), 16)
    x, y = act(sp.cin, c.H, c.W), act(sp.cout, oh, ow)                # one image of room; none is to be touched
    w, b, dw, db = f32(*c.wshape), f32(sp.cout), f32(*c.wshape), f32(sp.cout)
    sc, sh = torch.ones(max(sp.cin, 8), device=DEV).repeat(2), torch.zeros(2 * max(sp.cin, 8), device=DEV)
    stats, ns = f32(4096), ctypes.c_int(7)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    tail = (*geom, P(ws), nb, st)
    aff_ok = (L.jvae_conv2d_affine_ok_b8 if b8 else L.jvae_conv2d_affine_ok)(*geom)
    if b8:
        assert L.jvae_conv2d_fwd_b8(P(x), P(w), P(b), P(y), 0, P(stats), ctypes.byref(ns), *tail) == 0 and ns.value == 0
        assert L.jvae_conv2d_dgrad_b8(P(y), P(w), P(x), *tail) == 0
        if aff_ok:
            assert L.jvae_conv2d_fwd_aff_b8(P(x), P(w), P(b), P(y), 0, P(stats), ctypes.byref(ns), P(sc), P(sh), 1, *tail) == 0
        wgrads = [lambda acc: L.jvae_conv2d_wgrad_b8(P(x), P(y), P(dw), P(db), acc, *tail)]
        if aff_ok:
            wgrads.append(lambda acc: L.jvae_conv2d_wgrad_aff_b8(P(x), P(y), P(dw), P(db), acc, P(sc), P(sh), 1, *tail))
    else:
        assert L.jvae_conv2d_fwd_f32(P(x), P(w), P(b), P(y), *tail) == 0
        assert L.jvae_conv2d_fwd_stats_f32(P(x), P(w), P(b), P(y), P(stats), ctypes.byref(ns), *tail) == 0 and ns.value == 0
        assert L.jvae_conv2d_dgrad_f32(P(y), P(w), P(x), *tail) == 0
        if aff_ok:
            assert L.jvae_conv2d_fwd_aff_f32(P(x), P(w), P(b), P(y), P(stats), ctypes.byref(ns), P(sc), P(sh), 1, *tail) == 0
        wgrads = [lambda acc: L.jvae_conv2d_wgrad_f32(P(x), P(y), P(dw), P(db), acc, *tail)]
        if aff_ok:
            wgrads.append(lambda acc: L.jvae_conv2d_wgrad_aff_f32(P(x), P(y), P(dw), P(db), acc, P(sc), P(sh), 1, *tail))
    for wg in wgrads:
        dw.fill_(POISON)
        db.fill_(POISON)
        assert wg(1) == 0
        assert bool((dw == POISON).all()) and bool((db == POISON).all())          # accumulate: untouched
        assert wg(0) == 0
        assert bool((dw == 0).all()) and bool((db == 0).all())                    # fresh: zeroed
    torch.cuda.synchronize()
    for t in (x, y, w, b, stats):
        assert bool((t == POISON).all())
    # ... and through the wrappers, on empty tensors (their data pointers are NULL)
    e = lambda t: torch.empty((0, *t.shape[1:]), dtype=t.dtype, device=DEV)
    if b8:
        y0, st0, ns0 = ops_b8.conv_fwd_raw(e(x), w, b, sp, want_stats=True)
        assert y0.shape == (0, *y.shape[1:]) and ns0 == 0
        assert ops_b8.conv_dgrad_raw(e(y), w, sp, 0, c.H, c.W).shape == (0, *x.shape[1:])
        gw, gb = ops_b8.conv_wgrad_raw(e(x), e(y), sp, c.wshape, True)
    else:
        assert ops.conv_fwd_raw(e(x), w, b, sp).shape == (0, sp.cout, oh, ow)
        y0, st0, ns0 = ops.conv_fwd_stats_raw(e(x), w, b, sp)
        assert y0.shape == (0, sp.cout, oh, ow) and ns0 == 0
        assert ops.conv_dgrad_raw(e(y), w, sp, (0, sp.cin, c.H, c.W)).shape == (0, sp.cin, c.H, c.W)
        gw, gb = ops.conv_wgrad_raw(e(x), e(y), sp, c.wshape, True)
    assert bool((gw == 0).all()) and bool((gb == 0).all())


@pytest.mark.parametrize('plan', ['col-only', 'two-image chunks', 'queried'])
def test_generic_wgrad_chunk_plans(plan):
    """jvae_fold_wgrad on a grid of more than 48 positions takes as many images per chunk as its workspace holds of unfold buffer
    + per-image product, folds a chunk's products onto dw in image order and lets a chunk of one image accumulate straight onto
    it.  N = 5 through the raw entry point with: room for the unfold buffer of ONE image only (image by image), room for two
    images (chunks of 2, 2 and a tail of 1), the queried size (one chunk); each against fp64, bit for bit from run to run, and
    one byte less than one image's unfold buffer is refused with JVAE_EWORKSPACE."""
    L = lib.load()
    c = cc.Case('9x13 N5', 17, 33, 5, 1, 2, 0, 0, (9, 13), 5, 'GENERIC GENERIC~ GENERIC')
    assert c.route('wgrad').kernel == 'CK_GENERIC'
    d = cc.make_data(c)
    ref, A, K = cc.references(c, d)
    sp = c.spec
    geom = sp.geom(c.N, c.H, c.W)
    col = 4 * sp.cin * sp.k * sp.kw * c.H * c.W                    # unfold buffer of one image ('same' geometry: Hs x Ws = H x W)
    part = 4 * sp.cout * sp.cin * sp.k * sp.kw
    full = L.jvae_conv2d_workspace_bytes(*geom)
    assert full >= c.N * (col + part)
    nb = {'col-only': col, 'two-image chunks': 2 * (col + part) + part // 2, 'queried': full}[plan]
    x, gy = d['x'].to(DEV), d['gy'].to(DEV)
    ws = torch.empty(full, dtype=torch.uint8, device=DEV)          # full-size in every call: a wrong plan cannot write past it
    P, st = lib.ptr, lib.stream_ptr()

    def run(nbytes, acc, dw, db):
        return L.jvae_conv2d_wgrad_f32(P(x), P(gy), P(dw), P(db), acc, *geom, P(ws), nbytes, st)
    outs = []
    for _ in range(2):
        dw, db = torch.full(c.wshape, POISON, device=DEV), torch.full((sp.cout,), POISON, device=DEV)
        assert run(nb, 0, dw, db) == 0
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    check(c, f'wgrad, {plan}', 'wgrad', 'CK_GENERIC', outs[0][0], ref['wgrad'], A['wgrad'], K['wgrad'])
    sw, sb = d['g0'].to(DEV), d['b0'].to(DEV)
    assert run(nb, 1, sw, sb) == 0
    g064 = d['g0'].double()
    check(c, f'wgrad, {plan}, accumulated', 'wgrad', 'CK_GENERIC', sw, ref['wgrad'] + g064, A['wgrad'] + g064.abs(), K['wgrad'], 5)
    dw = torch.full(c.wshape, POISON, device=DEV)
    assert run(col - 1, 1, dw, None) == -3 and bool((dw == POISON).all())
