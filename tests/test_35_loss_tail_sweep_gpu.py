"""Every row of tests/tail_cases.py on the device, through jvae_hip.ops (the raw entry points where ops cannot reach a branch):
the kernels of csrc/latent.hip, csrc/loss.hip and csrc/adam.hip against the fp64 references and derived bounds of tail_cases,
element by element.  Common to every call: each fp32 tensor an op allocates for a result lies inside a poisoned buffer with a
guard band of 64 floats on either side (the allocations of jvae_hip.ops are routed through `Guarded` for the length of the call),
the guards must be intact and every element written; each call runs twice and must give the same bits (`twice`); an upstream
gradient left out must give the bits of an explicit zero tensor."""
import contextlib
import math

import pytest
import torch

import tail_cases as tc
from jvae_hip import lib, ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 64
P_ = lib.ptr
_cache = {}


def ref64(fam, c):
    key = (fam.name, c.name)
    if key not in _cache:
        d = fam.make(c)
        r = fam.ref(c, d, tc.F64)
        _cache[key] = (d, r, fam.bound(c, d, r))
    return _cache[key]


def dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


class Guarded:
    """Stands in for the `torch` of jvae_hip.ops: fp32 results are carved out of NaN-filled buffers with guard bands."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, k):
        return getattr(torch, k)

    def _alloc(self, shape, dtype, device, zero=False):
        shape = tuple(int(s) for s in shape)
        if dtype not in (None, torch.float32):
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), math.nan, device=device)
        self.bufs.append((buf, n))
        v = buf[GUARD:GUARD + n].view(shape)
        return v.zero_() if zero else v

    def empty(self, *size, device=None, dtype=None):
        return self._alloc(size[0] if len(size) == 1 and not isinstance(size[0], int) else size, dtype, device)

    def empty_like(self, t):
        return self._alloc(t.shape, t.dtype, t.device)

    def zeros_like(self, t):
        return self._alloc(t.shape, t.dtype, t.device, zero=True)

    def check(self):
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), 'a guard band was written'
            assert not bool(torch.isnan(buf[GUARD:GUARD + n]).any()), 'a result element was not written'
        return len(self.bufs)


@contextlib.contextmanager
def guarded():
    g = Guarded()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = torch
    g.check()


def own(t):
    """A caller-owned fp32 operand the kernel updates in place, inside guard bands -> (view, check)."""
    buf = torch.full((t.numel() + 2 * GUARD,), math.nan, device=DEV)
    v = buf[GUARD:GUARD + t.numel()].view(t.shape)
    v.copy_(t)

    def check():
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + t.numel():]).all()), 'a guard band was written'
    return v, check


def twice(f):
    """Two runs of f (-> dict of tensors), bit for bit; -> the first."""
    a, b = f(), f()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f'two runs differ in {k}'
    return a


def hold(fam, c, got, r=None, b=None):
    """Every output of the case against its fp64 reference under its bound; the figures are printed before they are held."""
    if r is None:
        _, r, b = ref64(fam, c)
    assert set(got) == set(r), (set(got), set(r))
    ex = {k: tc.excess(got[k], r[k], b[k]) for k in r}
    print(c.name, {k: round(v, 3) for k, v in ex.items()})
    assert all(v <= 1 for v in ex.values()), (c.name, ex)


# ============================================================================================ reconstruction
def run_recon(c, d, offset=False):
    """offset: x_reco and x are views one element into their buffers (not 16-byte aligned)."""
    def shifted(t):
        if not offset:
            return t.to(DEV)
        flat = torch.zeros(t.numel() + 1, device=DEV)
        flat[1:] = t.flatten().to(DEV)
        return flat[1:].view(t.shape)
    xr, x = shifted(d['xr']).requires_grad_(True), shifted(d['x'])
    sg = dev(d['sigma'], c.mode != tc.SIG_RMSE and not c.rows)
    with guarded():
        if c.rows:
            w = ops.mse_rows(xr, x)
        else:
            w = ops.recon_wmse(xr, x, sg, c.mode, snapshot=c.snapshot)
        if c.snapshot:
            sg.data.fill_(tc.SIGMA_NEW)           # the decay rule: in place, between forward and backward
        (w * d['gw'].to(DEV)).sum().backward()
    out = dict(wmse=w.detach(), gxr=xr.grad)
    if not c.rows and not c.snapshot and c.mode != tc.SIG_RMSE:
        out['gsigma'] = sg.grad
    return out


@pytest.mark.parametrize('c', tc.RECON_CASES, ids=tc.ids)
def test_recon(c):
    d, r, b = ref64(tc.RECON, c)
    got = twice(lambda: run_recon(c, d))
    hold(tc.RECON, c, got)
    if not c.rows:
        assert float(got['gxr'][0].abs().max()) == 0., 'row 0 of the x_reco gradient is not exactly zero'
    if c.mode == tc.SIG_RMSE and not c.rows:       # the rmse kind has no sigma gradient: the entry point refuses one
        L_, N, D = c.L, c.N, c.D
        z = torch.zeros(max(L_ * N, 4), device=DEV)
        rc = lib.load().jvae_recon_bwd_f32(P_(dev(d['xr'])), P_(dev(d['x'])), P_(z), 3, None, P_(z), P_(z), P_(torch.zeros_like(dev(d['xr']))),
                                           P_(z), 0, L_, N, D, P_(z), z.numel() * 4, lib.stream_ptr())
        assert rc == -1


@pytest.mark.parametrize('D', [4, 256, 1028])
def test_recon_refuses_and_ops_copies_a_row_that_is_not_16_byte_aligned(D):
    """The float4 path (D % 4 == 0) loads 16 bytes at a time: the raw entry points refuse an operand that is not aligned to
    them before any launch; ops.recon_wmse hands such a view over as a copy and gives the aligned call's bits."""
    c = next(c for c in tc.RECON_CASES if c.D == D and c.mode == tc.SIG_VALUE and not c.snapshot)
    d, _, _ = ref64(tc.RECON, c)
    L = lib.load()
    flat = torch.zeros(d['xr'].numel() + 1, device=DEV)
    odd, good = flat[1:].view(d['xr'].shape), dev(d['xr'])
    xflat = torch.zeros(d['x'].numel() + 1, device=DEV)
    xodd, xgood = xflat[1:].view(d['x'].shape), dev(d['x'])
    assert odd.data_ptr() % 16 == 4 and good.data_ptr() % 16 == 0
    sg, w, ws = dev(d['sigma']), torch.zeros(c.L, c.N, device=DEV), torch.zeros(c.L * c.N + 4, device=DEV)
    for a, x_ in ((odd, xgood), (good, xodd)):
        assert L.jvae_recon_fwd_f32(P_(a), P_(x_), P_(sg), 0, P_(w), c.L, c.N, c.D, lib.stream_ptr()) == -1
    gw = dev(d['gw'])
    for a, x_, o in ((odd, xgood, good), (good, xodd, good), (good, xgood, odd)):
        rc = L.jvae_recon_bwd_f32(P_(a), P_(x_), P_(sg), 0, None, P_(gw), P_(w), P_(o), None, 0, c.L, c.N, c.D, P_(ws), ws.numel() * 4,
                                  lib.stream_ptr())
        assert rc == -1
    assert float(w.abs().max()) == 0.
    a, o = run_recon(c, d), run_recon(c, d, offset=True)
    for k in a:
        assert torch.equal(a[k], o[k]), k


@pytest.mark.parametrize('D', [3, 7, 257])
def test_recon_scalar_path_takes_an_unaligned_row(D):
    c = next(c for c in tc.RECON_CASES if c.D == D and c.mode == tc.SIG_VALUE and not c.snapshot)
    d, _, _ = ref64(tc.RECON, c)
    flat = torch.zeros(d['xr'].numel() + 1, device=DEV)
    flat[1:] = dev(d['xr']).flatten()
    w = torch.zeros(c.L, c.N, device=DEV)
    odd, x, sg = flat[1:], dev(d['x']), dev(d['sigma'])          # named: the operands outlive the launch
    assert odd.data_ptr() % 16 == 4
    rc = lib.load().jvae_recon_fwd_f32(P_(odd), P_(x), P_(sg), 0, P_(w), c.L, c.N, c.D, lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    a, o = run_recon(c, d), run_recon(c, d, offset=True)
    assert torch.equal(w, a['wmse'])
    for k in a:
        assert torch.equal(a[k], o[k]), k
    hold(tc.RECON, c, o)


# ============================================================================================ ELBO
def run_elbo(c, d, cw=tc.CW, zeros=False):
    """zeros: the upstream gradients the case leaves out are handed over as explicit zero tensors."""
    w, kl, ce = dev(d['wmse_s'], True), dev(d['kl'], True), dev(d['ce'], True)
    sg = dev(d['sigma'], c.mode != tc.SIG_RMSE)
    with guarded():
        wm, cx, tot, mse = ops.elbo(w, kl, ce, sg, c.mode, c.D, tc.BETA, cw, with_mse=True)
        obj = 0.
        for k, o in (('w', wm), ('c', cx), ('t', tot)):
            g = d['g_' + k]
            if g is not None or zeros:
                obj = obj + (o * (torch.zeros(c.N, device=DEV) if g is None else g.to(DEV))).sum()
        obj.backward()
    out = dict(wmse=wm.detach(), cross_x=cx.detach(), total=tot.detach(), mse=mse.detach(), g_wmse_s=w.grad, g_kl=kl.grad)
    if ce is not None:
        out['g_ce'] = ce.grad
    if c.mode != tc.SIG_RMSE:
        out['gsigma'] = sg.grad
    return out


@pytest.mark.parametrize('c', tc.ELBO_CASES, ids=tc.ids)
def test_elbo(c):
    d, r, b = ref64(tc.ELBO, c)
    got = twice(lambda: run_elbo(c, d))
    hold(tc.ELBO, c, got)
    as_dev = run_elbo(c, d, cw=torch.tensor([tc.CW], device=DEV))
    explicit = run_elbo(c, d, zeros=True)
    for k in got:
        assert torch.equal(got[k], as_dev[k]), f'cw as a device scalar changes {k}'
        assert torch.equal(got[k], explicit[k]), f'an explicit zero upstream gradient changes {k}'
    assert len(ops.elbo(dev(d['wmse_s']), dev(d['kl']), dev(d['ce']), dev(d['sigma']), c.mode, c.D, tc.BETA, tc.CW)) == 3


@pytest.mark.parametrize('c', tc.CHAIN_CASES, ids=tc.ids)
def test_rmse_sigma_as_the_chain_recon_elbo(c):
    d, r, b = ref64(tc.CHAIN, c)

    def run():
        xr = dev(d['xr'], True)
        with guarded():
            ws = ops.recon_wmse(xr, dev(d['x']), dev(d['sigma']), tc.SIG_RMSE)
            wm, cx, tot, mse = ops.elbo(ws, dev(d['kl']), None, dev(d['sigma']), tc.SIG_RMSE, c.D, tc.BETA, 0., with_mse=True)
            ((cx * dev(d['g_c'])).sum() + (tot * dev(d['g_t'])).sum()).backward()
        return dict(wmse=wm.detach(), cross_x=cx.detach(), total=tot.detach(), mse=mse.detach(), gxr=xr.grad)
    hold(tc.CHAIN, c, twice(run))


# ============================================================================================ cross entropy
@pytest.mark.parametrize('c', tc.XENT_CASES, ids=tc.ids)
def test_cross_entropy_rows(c):
    d, r, b = ref64(tc.XENT, c)

    def run():
        lg = dev(d['logits'], True)
        with guarded():
            ce = ops.cross_entropy_rows(lg, dev(d['y']))
            (ce * dev(d['gw'])).sum().backward()
        return dict(ce=ce.detach(), glogits=lg.grad)
    got = twice(run)
    hold(tc.XENT, c, got)
    assert bool((got['glogits'].double().sum(-1).abs().cpu() <= b['glogits'].sum(-1)).all()), 'a backward row does not sum to zero'


# ============================================================================================ activations, dropout
@pytest.mark.parametrize('c', tc.ACT_CASES, ids=tc.ids)
def test_act(c):
    d, r, b = ref64(tc.ACT, c)

    def run():
        x = dev(d['x'], True)
        with guarded():
            y = ops.act(x, c.kind)
            y.backward(dev(d['g']))
        return dict(y=y.detach(), dx=x.grad)
    hold(tc.ACT, c, twice(run))


def test_dropout_at_the_grid_cap():
    n = 8192 * 256 + 5                         # the smallest size in the second trip of dropout_kernel's grid-stride loop
    x = torch.randn(n, device=DEV).abs() + 0.1
    for p in (0.1, 0.5):
        with guarded():
            y = ops.dropout(x, p, 12345)
        kept = y != 0
        assert abs(float(kept.float().mean()) - (1 - p)) < 0.01
        assert torch.equal(y, ops.dropout(x, p, 12345)) and not torch.equal(y, ops.dropout(x, p, 12346))
        assert float(((y[kept] - x[kept] / (1 - p)).abs() / (x[kept] / (1 - p))).max()) < 1e-6


# ============================================================================================ loss sums
@pytest.mark.parametrize('c', tc.LOSS_SUMS_CASES, ids=tc.ids)
def test_loss_sums(c):
    d, r, b = ref64(tc.LOSS_SUMS, c)
    rows = [t.to(DEV) for t in d['rows']]

    def run():
        acc, check = own(d['acc'])
        ops.loss_sums(rows, acc)
        check()
        return dict(acc=acc.clone())
    hold(tc.LOSS_SUMS, c, twice(run))


def test_loss_sums_takes_at_most_16_rows():
    rows = [torch.ones(3, device=DEV)] * 17
    with pytest.raises(lib.JvaeHipError):
        ops.loss_sums(rows, torch.zeros(17, device=DEV))


# ============================================================================================ optimiser
@pytest.mark.parametrize('c', tc.SQNORM_CASES, ids=tc.ids)
def test_sqnorm_accum(c):
    d, r, b = ref64(tc.SQNORM, c)
    g = dev(d['g'])

    def run():
        acc, check = own(d['acc'])
        ops.sqnorm_accum(g, acc, c.reset)
        check()
        return dict(acc=acc.clone())
    hold(tc.SQNORM, c, twice(run))


@pytest.mark.parametrize('c', tc.CLIP_CASES, ids=tc.ids)
def test_clip_scale(c):
    d = tc.clip_make(c)
    g0 = dev(d['g'])
    acc = torch.zeros(1, device=DEV)
    ops.sqnorm_accum(g0, acc, True)

    def run():
        g, check = own(d['g'])
        ops.clip_scale(g, acc, d['max_norm'])
        check()
        return dict(g=g.clone())
    got = twice(run)
    if not c.clips:
        assert torch.equal(got['g'], g0), 'a coefficient >= 1 must leave every bit alone'
    r = tc.clip_ref(c, d, acc.cpu(), tc.F64)
    hold(None, c, got, r, tc.clip_bound(c, d, r))


def _steps(c, d, form):
    """STEPS optimiser steps on guarded state; form: 'host' | 'dev' (Adam's device-resident hyper-parameters).  -> per step
    (state before, published sqnorm, state after), all on the CPU."""
    st = {k: own(v) for k, v in tc.opt_state0(c, d).items()}
    acc = torch.zeros(1, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    hyper = torch.tensor([tc.LR, tc.B1, tc.B2, c.step0 - 1, 0., 0.], device=DEV)
    out = []
    for i, g in enumerate(d['grads']):
        g = g.to(DEV)
        before = {k: v[0].clone().cpu() for k, v in st.items()}
        sq = None
        if c.max_norm > 0:
            ops.sqnorm_accum(g, acc, True)
            sq = acc
        T = {k: v[0] for k, v in st.items()}
        if c.kind == 'sgd':
            ops.sgd_step(T['p'], g, T['buf'] if c.mu else None, tc.LR, c.mu, c.nesterov, c.wd, i == 0, c.max_norm, sq, flag)
        elif form == 'host':
            ops.adam_step(T['p'], g, T['m'], T['v'], tc.LR, tc.B1, tc.B2, tc.AEPS, c.wd, c.step0 + i, c.max_norm, sq, flag)
        else:
            ops.adam_step_dev(T['p'], g, T['m'], T['v'], hyper, True, tc.AEPS, c.wd, c.max_norm, sq, flag)
            assert float(hyper[3]) == c.step0 + i
        for v in st.values():
            v[1]()
        out.append((before, None if sq is None else sq.clone().cpu(), {k: v[0].clone().cpu() for k, v in st.items()}))
    assert int(flag) == 0, 'the non-finite flag was raised on finite data'
    return out


@pytest.mark.parametrize('c', tc.OPT_CASES, ids=tc.ids)
def test_optimiser_steps(c):
    d = tc.opt_make(c)
    a, b2 = _steps(c, d, 'host'), _steps(c, d, 'host')
    for i, ((before, sq, after), (_, _, again)) in enumerate(zip(a, b2)):
        keys = [k for k in after if not (c.kind == 'sgd' and c.mu == 0 and k == 'buf')]
        for k in keys:
            assert torch.equal(after[k], again[k]), f'step {i}: two runs differ in {k}'
        r = tc.opt_step_ref(c, before, d['grads'][i], sq, i, tc.F64)
        hold(None, tc.Case(f'{c.name} step {i}'), {k: after[k] for k in r}, r, tc.opt_step_bound(c, before, d['grads'][i], sq, i, r))
    if c.kind == 'adam':
        for i, ((_, _, after), (_, _, as_dev)) in enumerate(zip(a, _steps(c, d, 'dev'))):
            for k in after:
                assert torch.equal(after[k], as_dev[k]), f'step {i}: the device-hyper form differs in {k}'


def test_adam_dev_without_advance_leaves_the_step_count():
    n = 37
    p, g, m, v = (torch.randn(n, device=DEV) for _ in range(4))
    v = v.abs()
    hyper = torch.tensor([tc.LR, tc.B1, tc.B2, 3., 0., 0.], device=DEV)
    ops.adam_step_dev(p, g, m, v, hyper, True, tc.AEPS, 0.)
    h = hyper.clone()
    assert float(h[3]) == 4.
    ops.adam_step_dev(p, g, m, v, hyper, False, tc.AEPS, 0.)
    assert torch.equal(h, hyper)


@pytest.mark.parametrize('n,where', [(1031, 'tail'), (1031, 'last vector'), (2048 * 1024 + 7, 'last vector'), (3, 'tail')])
@pytest.mark.parametrize('kind', ['adam', 'adam_dev', 'sgd'])
def test_nonfinite_flag(kind, n, where):
    """inf in an element of the n % 4 tail, nan in the last float4 of the strided region; untouched on finite data."""
    g = torch.randn(n, device=DEV)
    g[n - 1 if where == 'tail' else 4 * (n // 4) - 2] = math.inf if where == 'tail' else math.nan
    p, m, v = torch.randn(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    hyper = torch.tensor([tc.LR, tc.B1, tc.B2, 0., 0., 0.], device=DEV)
    if kind == 'adam':
        ops.adam_step(p, g, m, v, tc.LR, tc.B1, tc.B2, tc.AEPS, 0., 1, flag=flag)
    elif kind == 'adam_dev':
        ops.adam_step_dev(p, g, m, v, hyper, True, tc.AEPS, 0., flag=flag)
    else:
        ops.sgd_step(p, g, m, tc.LR, tc.MOMENTUM, False, 0., True, flag=flag)
    assert int(flag) == 1


def test_optimiser_refusals():
    L = lib.load()
    n = 64
    base = torch.zeros(4 * n + 8, device=DEV)
    good = [base[i * n:(i + 1) * n] for i in range(4)]
    odd = base[3 * n + 1:4 * n + 1]
    assert odd.data_ptr() % 16 == 4
    acc = torch.zeros(1, device=DEV)
    ws = torch.zeros(L.jvae_sqnorm_workspace_bytes(), dtype=torch.uint8, device=DEV)
    st = lib.stream_ptr()
    assert L.jvae_sqnorm_accum_f32(P_(odd), n, P_(acc), 1, P_(ws), ws.numel(), st) == -1
    assert L.jvae_sqnorm_accum_f32(P_(good[0]), n, P_(acc), 1, P_(ws), ws.numel() - 4, st) == -3
    hyper = torch.tensor([tc.LR, tc.B1, tc.B2, 0., 0., 0.], device=DEV)
    for j in range(4):
        t = list(good)
        t[j] = odd
        assert L.jvae_adam_step_f32(*(P_(x) for x in t), n, tc.LR, tc.B1, tc.B2, tc.AEPS, 0., 1, 0., None, None, st) == -1
        assert L.jvae_adam_step_dev_f32(*(P_(x) for x in t), n, P_(hyper), 0, tc.AEPS, 0., 0., None, None, st) == -1
    assert L.jvae_adam_step_f32(*(P_(x) for x in good), n, tc.LR, tc.B1, tc.B2, tc.AEPS, 0., 0, 0., None, None, st) == -1     # step < 1
    torch.cuda.synchronize()
    assert float(base.abs().max()) == 0. and float(acc) == 0., 'a refused call launched'


# ============================================================================================ importance-weighted bound
@pytest.mark.parametrize('c', tc.IWS_CASES, ids=tc.ids)
def test_iws(c):
    d, r, b = ref64(tc.IWS, c)

    def run():
        with guarded():
            out = ops.iws(dev(d['wmse_s']), dev(d['eps']), dev(d['log_var']), dev(d['log_pz']), dev(d['sigma']), c.mode, tc.IWS_D)
        return dict(iws=out.clone())
    got = twice(run)
    assert tuple(got['iws'].shape) == ((c.C, c.N) if c.C else (c.N,))
    hold(tc.IWS, c, got)


# ============================================================================================ measures
def run_measures(c, d, form):
    """The MEAS_BATCHES batches through the prev / batch form ('host') or the run / counter form ('dev') -> (batches, 16)."""
    scratch = torch.zeros(1, device=DEV)
    flag = None if c.flag is None else torch.tensor([c.flag], dtype=torch.int32, device=DEV)
    means, sigma = dev(d['means']), dev(d['sigma'])
    run, check = own(torch.full((16,), 7.5))                 # its content is ignored at batch 0
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    prev, outs = None, []
    for b, B in enumerate(d['batches']):
        args = (dev(B['x']), dev(B['wmse']), dev(B['zdist']), dev(B['var_kl']), sigma, c.kind, means, flag, scratch)
        if form == 'host':
            with guarded():
                prev = ops.measures(*args, prev=prev, batch=b)
            outs.append(prev.clone())
        else:
            out = ops.measures(*args, run=run, counter=counter)
            check()
            assert out is run and int(counter) == b + 1, 'the device counter did not advance'
            outs.append(run.clone())
    return dict(out=torch.stack(outs))


@pytest.mark.parametrize('c', tc.MEAS_CASES, ids=tc.ids)
def test_measures(c):
    d, r, b = ref64(tc.MEASURES, c)
    rest = [j for j in range(16) if j != 7]                   # slot 7 sums through LDS float atomics: any order
    a, a2, v = run_measures(c, d, 'host'), run_measures(c, d, 'host'), run_measures(c, d, 'dev')
    for other, what in ((a2, 'two runs differ'), (v, 'the prev / batch and run / counter forms differ')):
        assert torch.equal(a['out'][:, rest], other['out'][:, rest]), what
        assert bool(((a['out'][:, 7] - other['out'][:, 7]).abs().double().cpu() <= 2 * b['out'][:, 7]).all()), what + ' in slot 7'
    hold(tc.MEASURES, c, a)
    hold(tc.MEASURES, c, v)
    if c.special == 'twin':
        assert float(a['out'][:, 8].abs().max()) == 0.
    assert bool((a['out'][:, 9] == float(c.flag or 0)).all())


# ============================================================================================ latent
LAT_OUT = ('lv', 'z', 'kl', 'zdist', 'var_kl', 'dzdist')


def lat_args(c):
    prior, var = tc.KINDS[c.kind]
    tau = tc.TAU[prior]
    return dict(prior=prior, var_dim=var, tau=tau, alpha=tc.uniform_alpha(tau) if prior == 'uniform' else 0.)


def run_latent(c, d, w=None, up=('gz', 'gk', 'gd', 'gv'), zeros=False):
    """up: the upstream gradients that reach the op; zeros: the others are explicit zero tensors instead of absent."""
    mu, lr, means, T = (dev(d[k], True) for k in ('mu', 'lv_raw', 'means', 'T'))
    with guarded():
        res = ops.latent(mu, lr, dev(d['eps']), dev(d['y']), means, T, w=c.w if w is None else w, sampled=c.sampled,
                         forced_lv=c.forced, **lat_args(c))
        lv, z, kl, zd, vkl, dzd = res
        obj = 0.
        for k, o in (('gz', z), ('gk', kl), ('gd', zd), ('gv', vkl)):
            if k in up or zeros:
                obj = obj + (o * (dev(d[k]) if k in up else torch.zeros_like(o))).sum()
        obj.backward()
    out = dict(zip(LAT_OUT, (t.detach() for t in res)))
    out.update(gmu=mu.grad, glv=lr.grad, gmeans=means.grad)
    if tc.KINDS[c.kind][1] != 'scalar':
        out['gT'] = T.grad
    return out


@pytest.mark.parametrize('c', tc.LATENT_CASES, ids=tc.ids)
def test_latent(c):
    d, r, b = ref64(tc.LATENT, c)
    got = twice(lambda: run_latent(c, d))
    hold(tc.LATENT, c, got, {k: v for k, v in r.items() if k[0] != '_'}, b)
    assert torch.equal(got['lv'].cpu(), r['lv'].float()), 'the clipped log-variance is not exact'
    outside = (d['lv_raw'].abs() > 20) | (c.forced is not None)
    assert float(got['glv'].cpu()[outside].abs().max() if bool(outside.any()) else 0.) == 0., 'a gradient passed the clip'
    as_dev = run_latent(c, d, w=torch.tensor([c.w], device=DEV))
    for k in got:
        assert torch.equal(got[k], as_dev[k]), f'w as a device scalar changes {k}'
    part, explicit = run_latent(c, d, up=('gz', 'gd')), run_latent(c, d, up=('gz', 'gd'), zeros=True)
    for k in part:
        assert torch.equal(part[k], explicit[k]), f'an explicit zero upstream gradient changes {k}'


@pytest.mark.parametrize('ka,kb,K,N', [('gf', 'un', 64, 5), ('gd', 'ti', 65, 7), ('un', 'gf', 3, 7), ('gs', 'gf', 65, 5)])
@pytest.mark.parametrize('split', [0, 3, 'N'])
def test_latent_mixed_is_the_single_prior_kernel_sample_by_sample(ka, kb, K, N, split):
    split = N if split == 'N' else split
    mk = lambda kind: tc.Case(f'mixed {kind} K{K} N{N}', kind=kind, K=K, N=N, L=1, C=7, w=tc.f32(0.3), sampled=True, forced=None,
                              one_class=False)
    ca, cb = mk(ka), mk(kb)
    da, db = tc.latent_make(ca), tc.latent_make(cb)
    db = dict(da, means=db['means'], T=db['T'])                # one batch, two priors
    for d_ in (da, db):
        d_['means'], d_['T'] = d_['means'].clone(), d_['T'].clone()
    one = {0: run_latent(ca, da), 1: run_latent(cb, db)}

    def prior(c, d):
        return ops.latent_prior(dev(d['means']), dev(d['T']), **lat_args(c))
    mu, lr = dev(da['mu'], True), dev(da['lv_raw'], True)
    with guarded():
        res = ops.latent_mixed(mu, lr, dev(da['eps']), dev(da['y']), prior(ca, da), prior(cb, db), split, w=ca.w)
        lv, z, kl, zd, vkl, dzd = res
        ((z * dev(da['gz'])).sum() + (kl * dev(da['gk'])).sum() + (zd * dev(da['gd'])).sum() + (vkl * dev(da['gv'])).sum()).backward()
    got = dict(zip(LAT_OUT, res), gmu=mu.grad, glv=lr.grad)
    for k, v in got.items():
        if k == 'dzdist':
            assert torch.equal(v[:split], one[0][k][:split]) and float(v[split:].abs().max() if split < N else 0.) == 0.
            continue
        rows = (lambda t, s: t[:, s]) if k == 'z' else (lambda t, s: t[s])
        assert torch.equal(rows(v, slice(0, split)), rows(one[0][k], slice(0, split))), f'{k}: rows of prior A differ'
        assert torch.equal(rows(v, slice(split, N)), rows(one[1][k], slice(split, N))), f'{k}: rows of prior B differ'


@pytest.mark.parametrize('c', tc.DICT_CASES, ids=tc.ids)
def test_dict_stats(c):
    d, r, b = ref64(tc.DICT, c)
    means = dev(d['means'])

    def run():
        out, check = own(torch.zeros(c.K + 1))
        out.fill_(math.nan)
        lib.check(lib.load().jvae_dict_stats_f32(P_(means), P_(out), c.C, c.K, lib.stream_ptr()), 'dict_stats')
        check()
        return dict(dict=out.clone())
    hold(tc.DICT, c, twice(run))
