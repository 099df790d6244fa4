"""The case table of the loss tail - csrc/latent.hip, csrc/loss.hip, csrc/adam.hip - shared by tests/test_tail_cases_host.py (CPU: the references
against the oracle and torch, an fp32 restatement of every case inside its bound, and the planted mistakes those bounds must
catch) and tests/test_35_loss_tail_sweep_gpu.py (GPU: every case through jvae_hip.ops or the raw entry points against fp64).
A plain module without a GPU import, in the style of tests/bn_cases.py.

Every op is a Family: its cases, `make` (fp32 operands on the CPU, seeded from the case's name), `ref` (the operation restated
in torch, generic in the dtype: float64 is the reference, float32 the restatement the host test holds to the bounds; gradients
come from autograd of that forward, never from a second formula) and `bound` (per output element, from the fp64 reference).

A bound is k * U * A + TINY: U = 2^-24 the unit roundoff of fp32, A the magnitude of the element (the same formula with every
summed term replaced by its absolute value), k the roundings one element can pass through, counted from the kernel's arithmetic
in the comment beside it - for a reduction the serial length of one thread's share, the depth of the shuffle / LDS tree and the
elementwise roundings in front of and behind it.  TINY = 2^-126 (the smallest normal fp32) admits a result that underflows.
Where a result goes through more than one stage the bound is written as the propagated error of the stages, each of them
k * U * A of its own.  No bound is tuned against a kernel's output.

The fast intrinsics.  __expf and __logf have no documented maximum error in the HIP math documentation or the programming
guides that ship with the toolchain, so it is measured as the issue of this sweep prescribes: the worst deviation from fp64 of
torch's CPU fp32 exp / log over this module's own arguments (measure_intrinsics(), asserted by the host test), in ulps of the
result, times 4 (a hardware approximation of a few ulps against libm's one or less):
    exp: measured 0.552 ulp -> EXP_ULPS = 4 * 0.56 = 2.24 ulps     log: measured 0.511 ulp -> LOG_ULPS = 4 * 0.52 = 2.08 ulps
One ulp is 2 U.  On top of it the kernel's own arithmetic around the intrinsic is counted: __expf(x) is exp2(x * log2(e)), whose
product rounds once relative to |x| (|x| U on the result); __logf(x) is log2(x) * ln(2), one rounding of the result."""
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
F64, F32 = torch.float64, torch.float32
EXP_MEASURED, LOG_MEASURED = 0.56, 0.52          # ulps, torch CPU fp32 against fp64 over EXP_ARGS / LOG_ARGS of this module
EXP_ULPS, LOG_ULPS = 4 * EXP_MEASURED, 4 * LOG_MEASURED
SIG_VALUE, SIG_LOG, SIG_CODED, SIG_RMSE = 0, 1, 2, 3
LOG2PI = float(np.float32(1.8378770664093453))   # the kernels' constant, as fp32 holds it
SLOPE = float(np.float32(0.01))                  # JVAE_LEAKY_SLOPE
CLIP_EPS = float(np.float32(1e-6))


def f32(v):
    """A host value as the C ABI hands it to a kernel (float arguments are rounded to fp32)."""
    return float(np.float32(v))


def exp_k(arg):
    """Roundings (units of U, relative to the result) of __expf(arg): the intrinsic's allowance and its argument scaling."""
    return 2 * EXP_ULPS + torch.as_tensor(arg, dtype=F64).abs()


LOG_K = 2 * LOG_ULPS + 1          # ... of __logf: the allowance and the product with ln 2

EXP_ARGS, LOG_ARGS = [], []       # every argument a reference hands to exp / log at fp64 (measure_intrinsics reads them)


def _exp(t):
    if t.dtype == F64:
        EXP_ARGS.append(t.detach().flatten())
    return t.exp()


def _log(t):
    if t.dtype == F64:
        LOG_ARGS.append(t.detach().flatten())
    return t.log()


def measure_intrinsics():
    """-> (exp, log): worst |fp32 f(x) - fp64 f(x)| in ulps of the fp32 result, x the fp32 arguments the references above met."""
    out = []
    for args, f in ((EXP_ARGS, torch.exp), (LOG_ARGS, torch.log)):
        x = torch.cat(args).float()
        r32, r64 = f(x), f(x.double())
        ok = torch.isfinite(r32) & (r32.abs() >= TINY) & (r64.abs() > 0)
        r32, r64 = r32[ok], r64[ok]
        ulp = 2.0 ** (torch.floor(torch.log2(r32.double().abs())) - 23)
        out.append(float(((r32.double() - r64).abs() / ulp).max()))
    return tuple(out)


class Case:
    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)

    def gen(self):
        return torch.Generator().manual_seed(zlib.crc32(self.name.encode()))

    def __repr__(self):
        return self.name


class Family:
    def __init__(self, name, cases, make, ref, bound, plants=()):
        self.name, self.cases, self.make, self.ref, self.bound, self.plants = name, cases, make, ref, bound, tuple(plants)
        assert len({c.name for c in cases}) == len(cases)


def ids(c):
    return c.name.replace(' ', '_')


def excess(got, ref, bound):
    """max |got - ref| / bound over the elements (<= 1: inside); a non-finite result is outside."""
    got, ref, bound = (torch.as_tensor(t).detach().double().cpu() for t in (got, ref, bound))
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    bound = bound.expand_as(ref) if bound.shape != ref.shape else bound
    e = (got - ref).abs() / bound
    e = torch.where(torch.isfinite(got), e, torch.full_like(e, math.inf))
    return float(e.max())


def leaf(t, dt):
    """A fresh leaf of dtype dt (never the operand itself: .to() of the same dtype returns its argument)."""
    return t.detach().to(dt).clone().requires_grad_(True)


def _grad(t):
    return torch.zeros_like(t) if t.grad is None else t.grad


def cdiv(a, b):
    return -(-a // b)


TREE = 6 + 2      # block_sum: the xor butterfly of a wave (6 levels), then the four wave sums in a second butterfly (2)

# ============================================================================================ reconstruction
RECON_D = (1, 3, 4, 7, 255, 256, 257, 1028, 3072)
_LN = ((1, 1), (3, 5), (1, 5), (3, 1))
RECON_CASES = [Case(f'recon D{D} kind{m} L{L} N{N}', D=D, mode=m, L=L, N=N, rows=False, snapshot=False)
               for i, D in enumerate(RECON_D) for m in range(4) for (L, N) in [_LN[(i + m) % 4]]]
RECON_CASES += [Case(f'mse_rows D{D} L{L} N{N}', D=D, mode=SIG_RMSE, L=L, N=N, rows=True, snapshot=False)
                for i, D in enumerate(RECON_D) for (L, N) in [_LN[(i + 1) % 4]]]
RECON_CASES += [Case(f'recon snapshot D{D} L{L} N{N}', D=D, mode=SIG_VALUE, L=L, N=N, rows=False, snapshot=True)
                for D, L, N in ((7, 3, 5), (1028, 1, 5))]
SIGMA_NEW = 0.55      # the value a snapshot case writes into sigma between forward and backward


def sigma_of(mode, N, g):
    """sigma as the kind wants it: a value, a log value, N coded log values; the rmse kind reads none (a placeholder)."""
    return {SIG_VALUE: torch.tensor([0.7]), SIG_LOG: torch.tensor([0.3]), SIG_CODED: 0.4 * torch.randn(N, generator=g),
            SIG_RMSE: torch.ones(1)}[mode]


def recon_make(c):
    g = c.gen()
    return dict(xr=torch.randn(c.L + (0 if c.rows else 1), c.N, c.D, generator=g), x=torch.rand(c.N, c.D, generator=g),
                sigma=sigma_of(c.mode, c.N, g), gw=torch.randn(c.L, c.N, generator=g))


def _inv2(sg, mode, plant=None):
    if mode == SIG_RMSE:
        return 1.
    if mode == SIG_VALUE:
        return 1 / sg if plant == 'sigma1' else 1 / (sg * sg)
    return _exp(-sg) if plant == 'sigma1' else _exp(-2 * sg)


def recon_ref(c, d, dt=F64, plant=None):
    """wmse[l][n] = mean_D((x_reco[l+1][n] - x[n])^2) / sigma^2 and its gradients (losses.py:8-27, cvae.py:649-652)."""
    xr = leaf(d['xr'], dt)
    x, gw = d['x'].to(dt), d['gw'].to(dt)
    sg = leaf(d['sigma'], dt)
    diff = (xr if c.rows else xr[1:]) - x
    if plant == 'drop_last':
        diff = diff[..., :c.D - 1]
    if plant == 'drop_tail4':
        diff = diff[..., :4 * (c.D // 4)]
    Dd = c.D + {'D+1': 1, 'D-1': -1}.get(plant, 0)
    if c.snapshot:
        # the reference's decay rule rewrites sigma.data between forward and backward, and the division saved that very tensor
        old = float(sg.detach()[0])
        if plant in ('snap_collapse_new', 'snap_swap'):
            sg.data.fill_(SIGMA_NEW)
        wm = (diff / sg).square().sum(-1) / Dd
        if plant != 'snap_collapse_fwd':
            sg.data.fill_(old if plant == 'snap_swap' else SIGMA_NEW)
    else:
        wm = diff.square().sum(-1) / Dd * _inv2(sg, c.mode, plant)
    (wm * gw).sum().backward()
    out = dict(wmse=wm.detach(), gxr=xr.grad)
    if not c.rows and not c.snapshot and c.mode != SIG_RMSE:
        out['gsigma'] = _grad(sg)
    return out


def recon_seq(D):
    """Additions one thread of recon_fwd_kernel makes: four per float4 it meets (D % 4 == 0), else one per float."""
    return 4 * cdiv(D // 4, 256) if D % 4 == 0 else cdiv(D, 256)


def recon_kinv(c, d, backward=False):
    """Roundings of 1 / sigma^2: value: the square, the reciprocal (2; the snapshot's 1 / (sigma_fwd sigma) the same 2); log
    and coded: __expf(-2 sigma), its argument exact; the rmse kind and mse_rows: the constant 1."""
    if c.rows or c.mode == SIG_RMSE:
        return torch.zeros(1, dtype=F64)
    if c.mode == SIG_VALUE:
        return torch.full((1,), 2., dtype=F64)
    return exp_k(2 * d['sigma'].double())


def recon_kfwd(c, d):
    # a term: d = fl(a - b) enters squared (2), the product (1); the sum: seq + TREE; / D (1); 1 / sigma^2 and its product (1)
    return recon_seq(c.D) + TREE + 3 + 1 + recon_kinv(c, d) + 1


def recon_bound(c, d, r):
    kf = recon_kfwd(c, d)
    b = dict(wmse=kf * U * r['wmse'].abs() + TINY)
    # c = g * 2 (exact) * inv2 (1) / D (1); d = fl(a - b) (1); the product (1)
    b['gxr'] = (recon_kinv(c, d, True).reshape(-1, 1) + 4) * U * r['gxr'].abs() + TINY
    if 'gsigma' in r:
        # a part: the kernel's own wmse (kf), 2 * wmse exact, / sigma (1), * g (1); then vec_sum_kernel over L * N parts
        # (value, log) or rows_fold_kernel over the L parts of a sample in sequence (coded)
        sg = d['sigma'].double()
        part = (d['gw'].double() * 2 * r['wmse']).abs() / (sg if c.mode == SIG_VALUE else 1.)
        if c.mode == SIG_CODED:
            b['gsigma'] = (kf + 2 + c.L) * U * part.sum(0) + TINY
        else:
            b['gsigma'] = (kf + 2 + cdiv(c.L * c.N, 256) + TREE) * U * part.sum().reshape(1) + TINY
    return b


RECON = Family('recon', RECON_CASES, recon_make, recon_ref, recon_bound,
               ['D+1', 'D-1', 'drop_last', 'drop_tail4', 'sigma1', 'snap_collapse_new', 'snap_collapse_fwd', 'snap_swap'])

# ============================================================================================ ELBO assembly
BETA, CW = f32(0.8), f32(0.35)
_TOUCH = ('w', 'c', 't', 'wc', 'wt', 'ct', 'wct')
ELBO_CASES = [Case(f'elbo kind{m} L{(1, 3)[(m + j) % 2]} N{N} D{(3072, 7)[j % 2]} touch-{_TOUCH[(4 * m + j) % 7]}'
                   + (' ce' if (m + j) % 3 else ''), mode=m, L=(1, 3)[(m + j) % 2], N=N, D=(3072, 7)[j % 2],
                   touch=_TOUCH[(4 * m + j) % 7], ce=bool((m + j) % 3))
              for m in range(4) for j, N in enumerate((1, 255, 256, 257))]


def elbo_make(c):
    g = c.gen()
    d = dict(wmse_s=torch.rand(c.L, c.N, generator=g) + 0.1, kl=torch.randn(c.N, generator=g).square(),
             ce=3 * torch.rand(c.N, generator=g) if c.ce else None, sigma=sigma_of(c.mode, c.N, g))
    for k in 'wct':
        d['g_' + k] = torch.randn(c.N, generator=g) if k in c.touch else None
    return d


def elbo_terms(w, sg, mode, L, plant=None):
    """-> (wmse, log sigma, sigma^2) per sample from wmse_s (L, N): cvae.py:662-670."""
    s = w.sum(0) / L
    if mode == SIG_RMSE:
        m = s
        return (w / m).sum(0) / L, 0.5 * _log(m), m
    if mode == SIG_VALUE:
        return s, _log(sg), (sg if plant == 'sigma1' else sg * sg)
    return s, sg, _exp(sg if plant == 'sigma1' else 2 * sg)


def elbo_ref(c, d, dt=F64, plant=None):
    """cross_x = D/2 (2 log sigma + wmse + log 2pi); total = cross_x + cw ce + beta kl (cvae.py:773-791, 887-902)."""
    w = leaf(d['wmse_s'], dt)
    kl = leaf(d['kl'], dt)
    ce = None if d['ce'] is None else leaf(d['ce'], dt)
    sg = leaf(d['sigma'], dt)
    s, ls, sig2 = elbo_terms(w, sg, c.mode, c.L, plant)
    Dd = c.D + {'D+1': 1, 'D-1': -1}.get(plant, 0)
    cx = 0.5 * Dd * (2 * ls + s + LOG2PI)
    a, b = (BETA, CW) if plant == 'cw_beta_swapped' else (CW, BETA)
    tot = cx + (a * ce if ce is not None else 0.) + b * kl
    obj = sum((o * d['g_' + k].to(dt)).sum() for k, o in (('w', s), ('c', cx), ('t', tot)) if d['g_' + k] is not None)
    obj.backward()
    out = dict(wmse=s.detach(), cross_x=cx.detach(), total=tot.detach(), mse=(s * sig2).detach(), g_wmse_s=_grad(w), g_kl=_grad(kl))
    if ce is not None:
        out['g_ce'] = _grad(ce)
    if c.mode != SIG_RMSE:
        out['gsigma'] = _grad(sg).reshape(d['sigma'].shape)
    return out


def elbo_bound(c, d, r, kf=0):
    """kf: roundings already in wmse_s when it comes from the reconstruction kernel (the kind-3 chain)."""
    L, D, mode = c.L, c.D, c.mode
    w, sg = d['wmse_s'].double(), d['sigma'].double()
    z = lambda k: torch.zeros(c.N, dtype=F64) if d['g_' + k] is None else d['g_' + k].double().abs()
    gw, gc = z('w'), z('c') + z('t')
    m = w.sum(0) / L
    # s = sum_l w_l (L) / L (1); rmse: that is m, then w_l / m (1 + m's L + 1), their sum (L) and / L (1)
    ks = kf + L + 1 if mode != SIG_RMSE else 2 * (kf + L + 1) + L + 2
    b = dict(wmse=ks * U * r['wmse'].abs() + TINY)
    # log sigma: value: __logf(sigma); log / coded: sigma itself; rmse: 0.5 * __logf(m), m with L + 1 roundings of its own
    ls = {SIG_VALUE: sg.log(), SIG_LOG: sg, SIG_CODED: sg, SIG_RMSE: 0.5 * m.log()}[mode]
    e_ls = {SIG_VALUE: LOG_K * ls.abs(), SIG_LOG: 0 * ls, SIG_CODED: 0 * ls, SIG_RMSE: 0.5 * (kf + L + 1) + LOG_K * ls.abs()}[mode]
    # cx = (0.5 D) * ((2 ls + s) + c): two additions, the constant's own rounding, the product (4) on the whole magnitude
    A_cx = 0.5 * D * ((2 * ls).abs() + r['wmse'].abs() + LOG2PI)
    e_cx = U * ((ks + 4) * A_cx + D * e_ls)
    b['cross_x'] = e_cx + TINY
    # total = cx + cw ce + beta kl: two products, two additions (fused or not: at most 3 on the whole magnitude)
    A_t = A_cx + (CW * d['ce'].double().abs() if c.ce else 0.) + BETA * d['kl'].double().abs()
    b['total'] = e_cx + 3 * U * A_t + TINY
    # mse = s * sigma^2: the product (1); sigma^2: value: the square (1); log / coded: __expf(2 sigma); rmse: m
    k_s2 = {SIG_VALUE: 1., SIG_LOG: exp_k(2 * sg), SIG_CODED: exp_k(2 * sg), SIG_RMSE: float(kf + L + 1)}[mode]
    b['mse'] = (ks + 1 + k_s2) * U * r['mse'].abs() + TINY
    if mode == SIG_RMSE:
        # gw = gc * 0.5 (exact) * D (1) / (m * L) (m: L + 1, the product 1, the division 1), gc = g_cx + g_tot (1); the
        # derivative of wmse = mean_l(w_l / m) is zero, its two terms of magnitude |g_wmse| / (L m) each cancel
        A = (gc * 0.5 * D + 2 * gw) / (m * L)
        b['g_wmse_s'] = ((kf + L + 5) * U * A + TINY).expand(L, c.N)
    else:
        # gw = (g_wmse + gc * (0.5 D)) / L: gc (1), the product (1), the addition (1), the division (1)
        b['g_wmse_s'] = (4 * U * (gw + gc * 0.5 * D) / L + TINY).expand(L, c.N)
    b['g_kl'] = U * BETA * z('t') + TINY
    b['g_ce'] = U * CW * z('t') + TINY
    if mode != SIG_RMSE:
        # a part: gc (1) * D (1) [/ sigma (1)]; value / log: vec_sum_kernel over N parts; coded: one part per sample
        part = gc * D / (sg if mode == SIG_VALUE else 1.)
        b['gsigma'] = 3 * U * part + TINY if mode == SIG_CODED else (3 + cdiv(c.N, 256) + TREE) * U * part.sum().reshape(1) + TINY
    return b


ELBO = Family('elbo', ELBO_CASES, elbo_make, elbo_ref, elbo_bound, ['D+1', 'D-1', 'sigma1', 'cw_beta_swapped'])

# ------------------------------------------------------------------ kind 3 as the chain recon_wmse -> elbo (neither half alone)
CHAIN_CASES = [Case(f'chain3 D{D} L{L} N{N}', D=D, L=L, N=N, mode=SIG_RMSE, rows=False, snapshot=False, ce=False, touch='ct')
               for D, L, N in ((7, 3, 5), (256, 1, 5), (1028, 3, 1), (3, 3, 5))]


def chain_make(c):
    g = c.gen()
    d = recon_make(c)
    d.update(kl=torch.randn(c.N, generator=g).square(), ce=None, g_w=None, g_c=torch.randn(c.N, generator=g),
             g_t=torch.randn(c.N, generator=g))
    return d


def chain_ref(c, d, dt=F64, plant=None):
    """sigma_n^2 = the sample's own mse over its L draws: oracle.jvae_oracle.recon_terms, unchanged, on tensors of `dt`."""
    from oracle import jvae_oracle as O
    xr = leaf(d['xr'], dt)
    x = d['x'].to(dt)
    if plant == 'drop_last':
        xr_, x = xr[..., :c.D - 1], x[..., :c.D - 1]
    else:
        xr_ = xr
    _, wmse, mse, log_sigma, _ = O.recon_terms(dict(sigma=dict(is_rmse=True)), dict(sigma=torch.ones(1, dtype=dt)), None, x, xr_,
                                               c.L, c.N, False)
    Dd = c.D + {'D+1': 1, 'D-1': -1}.get(plant, 0)
    cx = 0.5 * Dd * (2 * log_sigma + wmse + LOG2PI)
    tot = cx + BETA * d['kl'].to(dt)
    ((cx * d['g_c'].to(dt)).sum() + (tot * d['g_t'].to(dt)).sum()).backward()
    return dict(wmse=wmse.detach(), cross_x=cx.detach(), total=tot.detach(), mse=mse.detach(), gxr=xr.grad)


def chain_bound(c, d, r):
    kf = recon_kfwd(c, d)
    raw = (d['xr'].double()[1:] - d['x'].double()).square().mean(-1)
    e = dict(d, wmse_s=raw)
    rb = elbo_bound(c, e, r, kf=int(kf))
    # gxr = gw * 2 (x_reco - x) / D: the elbo's gw at its own count, then recon_bwd_kernel's 4
    kg = int(kf) + c.L + 5 + 4
    return dict(wmse=rb['wmse'], cross_x=rb['cross_x'], total=rb['total'], mse=rb['mse'], gxr=kg * U * r['gxr'].abs() + TINY)


CHAIN = Family('chain3', CHAIN_CASES, chain_make, chain_ref, chain_bound, ['D+1', 'D-1', 'drop_last'])

# ============================================================================================ cross entropy
XENT_CASES = [Case(f'xent C{C} L{L} N{N} x{s}', C=C, L=L, N=N, scale=s)
              for C in (1, 2, 63, 64, 65, 200) for (L, N) in ((1, 1), (3, 5)) for s in (3, 80)]


def xent_make(c):
    g = c.gen()
    lg = torch.randn(c.L, c.N, c.C, generator=g)
    lg = lg * 3 if c.scale == 3 else lg / lg.abs().max() * 80         # +-80: the max subtraction carries the result
    y = torch.randint(0, c.C, (c.N,), generator=g)
    y[0] = c.C - 1                                                     # targets at both ends of the row
    if c.N > 1:
        y[-1] = 0
    return dict(logits=lg, y=y, gw=torch.randn(c.L, c.N, generator=g))


def xent_ref(c, d, dt=F64, plant=None):
    """ce[r] = -log softmax(logits[r])[y[r % N]], restated as the kernel computes it (losses.py:76-86)."""
    lg = leaf(d['logits'].reshape(-1, c.C), dt)
    R = lg.shape[0]
    r = torch.arange(R)
    t = d['y'][(r // c.N) % c.N if plant == 'y_div' else r % c.N]
    mx = lg.detach().max(-1, keepdim=True).values
    s = _exp(lg - mx).sum(-1)
    ce = _log(s) + mx[:, 0] - lg[r, t]
    (ce * d['gw'].to(dt).reshape(-1)).sum().backward()
    return dict(ce=ce.detach().reshape(c.L, c.N), glogits=lg.grad.reshape(c.L, c.N, c.C))


def xent_bound(c, d, r):
    lg = d['logits'].double().reshape(-1, c.C)
    R = lg.shape[0]
    t = d['y'][torch.arange(R) % c.N]
    mx = lg.max(-1, keepdim=True).values
    a = lg - mx
    p = torch.softmax(lg, -1)
    # a term e_c = __expf(a_c), a_c = fl(row - mx) (|a_c| U on the result) and exp_k; their sum: ceil(C / 64) per lane, the
    # butterfly (6); relative to s: S = sum_c p_c (exp_k(a_c) + |a_c|) + ceil(C / 64) + 6
    S = (p * (exp_k(a) + a.abs())).sum(-1) + cdiv(c.C, 64) + 6
    ls = torch.logsumexp(a, -1)
    # ce = (__logf(s) + mx) - row[t]: the logarithm's own error on |log s|, s's relative error as it stands, two additions
    A = ls.abs() + mx[:, 0].abs() + lg[torch.arange(R), t].abs()
    b = dict(ce=(U * (S + LOG_K * ls.abs() + 2 * A) + TINY).reshape(c.L, c.N))
    # g (p_c - [c == t]): p_c = e_c * (1 / s): e_c, s (S), the reciprocal (1), the product (1); the subtraction, the product (2)
    gv = d['gw'].double().reshape(-1, 1).abs()
    hot = torch.zeros_like(p)
    hot[torch.arange(R), t] = 1.
    # a term e_c below 2^-126 may be flushed to zero before it meets g / s (s >= 1): TINY once more, scaled by |g|
    b['glogits'] = (U * gv * (p * (exp_k(a) + a.abs() + S.unsqueeze(-1) + 2) + 2 * (p + hot)) + TINY * (1 + gv)).reshape(c.L, c.N, c.C)
    return b


XENT = Family('xent', XENT_CASES, xent_make, xent_ref, xent_bound, ['y_div'])

# ============================================================================================ activations
ACT_N = (1, 255, 257, 4096 * 256 + 3)     # the last: the smallest size in the second trip of the grid-stride loop (ew_grid)
ACT_CASES = [Case(f'act kind{k} n{n}', kind=k, n=n) for k in range(4) for n in ACT_N]
_SPECIAL = (-90., 0., -0., 90., 2.0 ** -130, -2.0 ** -130, 88., -88.)


def act_make(c):
    g = c.gen()
    x = 3 * torch.randn(c.n, generator=g)
    sp = torch.tensor(_SPECIAL)
    k = min(c.n, len(sp))
    x[:k] = sp[:k]
    x[c.n - k:] = sp[:k].flip(0)          # ... and in the loop's second trip
    return dict(x=x, g=torch.randn(c.n, generator=g))


def act_ref(c, d, dt=F64, plant=None):
    x = leaf(d['x'], dt)
    if c.kind == 0:
        y = x * 1
    elif c.kind == 1:
        y = torch.relu(x)
    elif c.kind == 2:
        _exp(-x.detach())                        # the argument the kernel hands to __expf
        y = torch.sigmoid(x)                     # its backward is g y (1 - y), the kernel's form (1 / (1 + inf) has no derivative)
    else:
        y = torch.where(x > 0, x, (1. if plant == 'no_slope' else SLOPE) * x)
    if plant == 'relu_as_identity' and c.kind == 1:
        y = x * 1
    y.backward(d['g'].to(dt))
    return dict(y=y.detach(), dx=x.grad)


def act_bound(c, d, r):
    x, g, y = d['x'].double(), d['g'].double().abs(), r['y']
    if c.kind in (0, 1):
        return dict(y=torch.full_like(y, TINY), dx=torch.full_like(y, TINY))          # copies and selects: exact
    if c.kind == 3:
        return dict(y=U * y.abs() + TINY, dx=U * r['dx'].abs() + TINY)                 # one product with the slope
    # y = 1 / (1 + e), e = __expf(-x): e's error reaches y scaled by e / (1 + e) = 1 - y; the addition, the reciprocal (2)
    ky = (1 - y) * exp_k(x) + 2
    # dx = g * y * (1 - y) from the kernel's own y: y's error moves y (1 - y) by |1 - 2y| <= 1 of it; 1 - y, two products (3)
    return dict(y=ky * U * y + TINY, dx=U * g * y * (ky + 3) + TINY)


ACT = Family('act', ACT_CASES, act_make, act_ref, act_bound, ['no_slope', 'relu_as_identity'])

# ============================================================================================ loss sums
LOSS_SUMS_CASES = [Case('loss_sums five lengths', lens=(1, 255, 256, 257, 100003)),
                   Case('loss_sums 16 rows', lens=tuple(3 + 17 * i for i in range(16))),
                   Case('loss_sums one row', lens=(258,))]


def loss_sums_make(c):
    g = c.gen()
    return dict(rows=[torch.randn(n, generator=g) + 0.25 for n in c.lens], acc=torch.randn(len(c.lens), generator=g) * 3)


def loss_sums_ref(c, d, dt=F64, plant=None):
    """acc[r] += mean(rows[r]); the kernel sums in fp64, so does the restatement, and rounds the mean once."""
    mean = torch.stack([(r.double()[:-1] if plant == 'drop_last' and r.numel() > 1 else r.double()).sum() / r.numel()
                        for r in d['rows']])
    return dict(acc=d['acc'].to(dt) + mean.to(dt))


def loss_sums_bound(c, d, r):
    mean = r['acc'] - d['acc'].double()
    return dict(acc=U * mean.abs() + U * r['acc'].abs() + TINY)      # one rounding of the mean, one of the addition


LOSS_SUMS = Family('loss_sums', LOSS_SUMS_CASES, loss_sums_make, loss_sums_ref, loss_sums_bound, ['drop_last'])

# ============================================================================================ optimiser
OPT_N = (0, 1, 3, 4, 5, 1023, 2048 * 1024 + 7)       # the last: grid_for's cap, second trip of the float4 loop, and a tail
#                                                      (sgd_kernel walks single floats: its second trip starts at 2048 * 256 + 1)
LR, B1, B2, AEPS, WD = f32(1e-3), f32(0.9), f32(0.999), f32(1e-8), f32(3e-5)
MOMENTUM = f32(0.9)


def grid_for(n4):
    return min(2048, max(1, cdiv(n4, 256)))


def sqnorm_k(n):
    """sqnorm_kernel + sqnorm_fold_kernel: a thread meets ceil(n4 / (blocks * 256)) float4s, each four products (1) added in
    sequence and onto s (4 additions: 5 with the product); block 0 adds one tail element (2); block_sum; the fold: a thread
    adds ceil(blocks / 256) partials, block_sum; the addition onto *acc (1)."""
    n4 = n // 4
    blocks = grid_for(n4)
    return 5 * cdiv(n4, blocks * 256) + 2 + TREE + cdiv(blocks, 256) + TREE + 1


SQNORM_CASES = [Case(f'sqnorm n{n} reset{r}', n=n, reset=r) for n in OPT_N for r in (1, 0)]


def sqnorm_make(c):
    g = c.gen()
    return dict(g=torch.randn(c.n, generator=g), acc=torch.tensor([3.5]))


def sqnorm_ref(c, d, dt=F64, plant=None):
    g = d['g'].to(dt)
    if plant == 'drop_tail4':
        g = g[:4 * (c.n // 4)]
    if plant == 'drop_last':
        g = g[:max(c.n - 1, 0)]
    return dict(acc=(0 if c.reset else d['acc'].to(dt)) + g.square().sum().reshape(1))


def sqnorm_bound(c, d, r):
    A = d['g'].double().square().sum() + (0 if c.reset else d['acc'].double().abs())
    return dict(acc=sqnorm_k(c.n) * U * A + TINY)


SQNORM = Family('sqnorm', SQNORM_CASES, sqnorm_make, sqnorm_ref, sqnorm_bound, ['drop_tail4', 'drop_last'])


def clip_coef(sq, max_norm, dt):
    """min(1, max_norm / (sqrt(sqnorm) + 1e-6)) from the PUBLISHED fp32 sqnorm: clip_grad_norm_'s coefficient."""
    return torch.clamp(max_norm / (sq.to(dt).sqrt() + CLIP_EPS), max=1.)


KCLIP = 4     # the square root, the addition of 1e-6 and that constant's own rounding, the division


class Opt(Case):
    """One optimiser step from the state the kernel itself left (p, m, v / buf as fp32): the reference is local to the step, so
    five steps are five comparisons at the bound of one, and a state the kernel did not store breaks the next."""


OPT_CASES = [Opt(f'adam n{n} wd{int(wd > 0)} clip{int(mn > 0)} step{s0}', kind='adam', n=n, wd=wd, max_norm=mn, step0=s0)
             for n in OPT_N for (wd, mn, s0) in ((WD, 1.0, 1), (0., 0., 1000))]
OPT_CASES += [Opt('adam n1023 wd1 clip0 step1', kind='adam', n=1023, wd=WD, max_norm=0., step0=1),
              Opt('adam n1023 wd0 clip1 step1000', kind='adam', n=1023, wd=0., max_norm=1.0, step0=1000)]
OPT_CASES += [Opt(f'sgd n{n} mu{mu} nesterov{int(nv)} wd{int(wd > 0)} clip{int(mn > 0)}', kind='sgd', n=n, mu=mu, nesterov=nv,
                  wd=wd, max_norm=mn, step0=1)
              for n in OPT_N + (2048 * 256 + 3,) for (mu, nv, wd, mn) in ((0., False, 0., 0.), (MOMENTUM, False, WD, 1.0),
                                                                              (MOMENTUM, True, f32(1e-4), 0.))]
STEPS = 5


def opt_make(c):
    g = c.gen()
    p = torch.randn(c.n, generator=g)
    gs = [torch.randn(c.n, generator=g) * (1. if c.n > 4 else 3.) for _ in range(STEPS)]    # |g| > max_norm = 1: every step clips
    return dict(p=p, grads=gs)


def opt_state0(c, d):
    z = torch.zeros(c.n)
    return dict(p=d['p'].clone(), m=z.clone(), v=z.clone()) if c.kind == 'adam' else dict(p=d['p'].clone(), buf=z.clone())


def opt_step_ref(c, st, g, sq, i, dt=F64, plant=None):
    """One step (i = 0 .. STEPS - 1) from the state st; sq: the published fp32 sum of squares of g (None without the clip)."""
    p, g = st['p'].to(dt), g.to(dt)
    coef = clip_coef(sq, c.max_norm, dt) if c.max_norm > 0 else torch.ones(1, dtype=dt)
    g1 = (g + c.wd * p) * coef if plant == 'wd_after_clip' else g * coef + c.wd * p
    if c.kind == 'sgd':
        if c.mu == 0:
            return dict(p=p - LR * g1)
        buf = g1 if i == 0 else c.mu * st['buf'].to(dt) + g1
        dd = g1 + c.mu * buf if (c.nesterov and plant != 'nesterov_no_extra') else buf
        return dict(p=p - LR * dd, buf=buf)
    step = c.step0 + i + {'step+1': 1, 'step-1': -1}.get(plant, 0)
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    lr1 = LR / bc1 if bc1 != 0 else math.inf
    m = B1 * st['m'].to(dt) + (1 - B1) * g1
    v = B2 * st['v'].to(dt) + (1 - B2) * g1 * g1
    denom = v.sqrt() / math.sqrt(bc2) + AEPS if bc2 > 0 else v.sqrt() * math.inf
    return dict(p=p - lr1 * (m / denom), m=m, v=v)


def opt_step_bound(c, st, g, sq, i, r):
    """The propagated error of adam1 / sgd_kernel, stage by stage (each stage: its roundings times U times its magnitude)."""
    p, g = st['p'].double(), g.double()
    kc = KCLIP if c.max_norm > 0 else 0
    coef = clip_coef(sq, c.max_norm, F64) if c.max_norm > 0 else torch.ones(1, dtype=F64)
    g1 = g * coef + c.wd * p
    # g' = fma(g, coef, wd * p): coef (kc), the product wd * p (1), the fused sum (1)
    e_g = (kc + 2) * U * ((g * coef).abs() + (c.wd * p).abs())
    if c.kind == 'sgd':
        if c.mu == 0:                                     # p - lr * d: the product (1), the subtraction (1)
            return dict(p=LR * e_g + U * (LR * g1).abs() + U * r['p'].abs() + TINY)
        first = i == 0
        # buf = mu * buf + g' and, under Nesterov, d = mu * buf + g': a product and a sum each (2; one when fused)
        e_b = e_g if first else e_g + 2 * U * ((c.mu * st['buf'].double()).abs() + g1.abs())
        dd = g1 + c.mu * r['buf'] if c.nesterov else r['buf']
        e_d = e_g + c.mu * e_b + 2 * U * ((c.mu * r['buf']).abs() + g1.abs()) if c.nesterov else e_b
        return dict(p=LR * e_d + U * (LR * dd).abs() + U * r['p'].abs() + TINY, buf=e_b + TINY)
    step = c.step0 + i
    bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
    lr1, isb = LR / bc1, 1 / math.sqrt(bc2)
    m0, v0 = st['m'].double(), st['v'].double()
    # m = b1 m + (1 - b1) g': 1 - b1 (1), two products, the sum: 3 on the magnitude; g' carries e_g
    e_m = 3 * U * ((B1 * m0).abs() + ((1 - B1) * g1).abs()) + (1 - B1) * e_g
    # v = b2 v + (1 - b2) g' g': 1 - b2, g' g', the two products, the sum: 4 on v (all terms >= 0); g' enters squared
    e_v = 4 * U * r['v'] + (1 - B2) * 2 * g1.abs() * e_g
    rv = r['v'].sqrt()
    e_sq = torch.where(rv > 0, e_v / (2 * rv).clamp_min(1e-300), e_v.sqrt()) + U * rv
    # denom = sqrt(v) * isb + eps: isb's own rounding, the product, the sum (3); eps's rounding (1)
    denom = rv * isb + AEPS
    e_den = e_sq * isb + 3 * U * rv * isb + 2 * U * AEPS
    # p - lr1 * (m / denom): lr1's rounding, the quotient, the product (3); the subtraction (1)
    upd = lr1 * r['m'] / denom
    e_u = lr1 * (e_m / denom + r['m'].abs() * e_den / (denom * denom)) + 3 * U * upd.abs()
    return dict(p=e_u + U * r['p'].abs() + TINY, m=e_m + TINY, v=e_v + TINY)


OPT_PLANTS = ['step+1', 'step-1', 'wd_after_clip', 'nesterov_no_extra']

CLIP_CASES = [Case(f'clip_scale n{n} {"clips" if cl else "passes"}', n=n, clips=cl) for n in OPT_N for cl in (1, 0)]


def clip_make(c):
    g = c.gen()
    gr = torch.randn(c.n, generator=g)
    sq = float(gr.double().square().sum())
    return dict(g=gr, max_norm=f32(0.5 * math.sqrt(sq) if c.clips and c.n else 2 * math.sqrt(sq) + 1.))


def clip_ref(c, d, sq, dt=F64, plant=None):
    coef = clip_coef(sq, d['max_norm'], dt)
    return dict(g=d['g'].to(dt) * (coef if plant != 'no_clip' else 1.))


def clip_bound(c, d, r):
    return dict(g=(KCLIP + 1) * U * r['g'].abs() + TINY)      # the coefficient and the product


# ============================================================================================ importance-weighted bound
IWS_D = 3072
_IWS_LNC = ((1, 1, 0), (3, 5, 3), (3, 90, 3), (3, 90, 0), (3, 5, 0), (1, 1, 3))
IWS_CASES = [Case(f'iws K{K} kind{m} L{L} N{N} C{C}', K=K, mode=m, L=L, N=N, C=C)
             for i, K in enumerate((1, 63, 64, 65, 130)) for m in range(4) for (L, N, C) in [_IWS_LNC[(i + m) % 6]]]
IWS_CASES += [Case(f'iws K{K} kind{m} L3 N90 C3', K=K, mode=m, L=3, N=90, C=3) for K, m in ((130, 3), (65, 2))]   # C N = 270: two blocks


def iws_make(c):
    g = c.gen()
    shape = (c.L, c.C, c.N) if c.C else (c.L, c.N)
    return dict(wmse_s=torch.rand(c.L, c.N, generator=g) + 0.1, eps=torch.randn(c.L, c.N, c.K, generator=g),
                log_var=torch.randn(c.N, c.K, generator=g), sigma=sigma_of(c.mode, c.N, g),
                log_pz=2 * torch.randn(*shape, generator=g) - 1000.)        # rows of order -5000: the max subtraction carries it


def iws_rows(c, d, dt):
    w, sg = d['wmse_s'].to(dt), d['sigma'].to(dt)
    s = (d['eps'].to(dt).square() + d['log_var'].to(dt)).sum(-1)
    if c.mode == SIG_RMSE:
        m = w.sum(0) / c.L
        w, ls = w / m, 0.5 * _log(m)
    else:
        ls = _log(sg) if c.mode == SIG_VALUE else sg
    return -0.5 * IWS_D * (w + 2 * ls + LOG2PI) + 0.5 * s + 0.5 * c.K * LOG2PI


def iws_ref(c, d, dt=F64, plant=None):
    """iws = mean_l exp(l_i - m) + m, l_i = log p(x | z_l) - log q(z_l | x) + log p(z_l), m = max_l l_i: the reference adds m to
    the mean, not to its logarithm (cvae.py:868, kept by iws_fold_kernel)."""
    rows = iws_rows(c, d, dt)
    lp = d['log_pz'].to(dt)
    li = rows.unsqueeze(1) + lp if c.C else rows + lp
    m = li.max(0).values
    t = _exp(li - m).sum(0) / c.L
    return dict(iws=_log(t) + m if plant == 'log_mean' else t + m)


def iws_bound(c, d, r):
    w, sg, L, D, K = d['wmse_s'].double(), d['sigma'].double(), c.L, IWS_D, c.K
    sa = (d['eps'].double().square() + d['log_var'].double().abs()).sum(-1)
    if c.mode == SIG_RMSE:
        m = w.sum(0) / L
        wn, ls = w / m, 0.5 * m.log()
        e_ls, kw = 0.5 * (L + 1) + LOG_K * ls.abs(), L + 2         # m: L + 1; w / m: one more
    else:
        wn, ls = w, (sg.log() if c.mode == SIG_VALUE else sg)
        e_ls, kw = (LOG_K * ls.abs() if c.mode == SIG_VALUE else 0 * ls), 0
    # s: a lane adds ceil(K / 64) terms fma(e, e, lv) (2), the butterfly (6); the row: five products / additions on the magnitude
    A_row = 0.5 * D * (wn.abs() + (2 * ls).abs() + LOG2PI) + 0.5 * sa + 0.5 * K * LOG2PI
    e_row = (cdiv(K, 64) + 6 + 2) * 0.5 * sa + 5 * A_row + D * e_ls + 0.5 * D * kw * wn            # units of U
    rows = iws_rows(c, d, F64)
    lp = d['log_pz'].double()
    if c.C:
        rows, e_row = rows.unsqueeze(1), e_row.unsqueeze(1)
    li = rows + lp
    e_li = e_row + li.abs()                                        # the addition of log_pz
    m = li.max(0).values
    e_m = e_li.max(0).values
    t = (li - m).exp()
    # exp(l_i - m): the argument's error (l_i, m, their difference) is the term's relative error, plus expf's own
    e_t = t * (e_li + e_m + (li - m).abs() + 2 * EXP_ULPS)
    # the sum over l (L), the division (1), the addition of m (1 on the result)
    return dict(iws=U * (e_m + e_t.sum(0) / L + (L + 1) * t.sum(0) / L + r['iws'].abs()) + TINY)


IWS = Family('iws', IWS_CASES, iws_make, iws_ref, iws_bound, ['log_mean'])

# ============================================================================================ measures
MEAS_BATCHES = 3
_DICTS = (None, (1, 1), (7, 3), (10, 64), (100, 130), (110, 128))    # (100, 130): 100 * 131 = 13100 <= 13312 floats, the last
#                                                                      size staged in LDS; (110, 128): 110 * 129 = 14190, global
MEAS_CASES = [Case(f'measures dict{"x".join(map(str, ck)) if ck else "-none"} kind{kind} N{N} flag{fl}', CK=ck, kind=kind, N=N,
                   Nz=(7 if N == 1 else 301), flag=fl, special=None)
              for i, ck in enumerate(_DICTS) for (kind, N, fl) in [((0, 1, 0), (1, 300, 1), (2, 300, 0))[i % 3]]]
MEAS_CASES += [Case('measures dict7x3 two identical rows', CK=(7, 3), kind=1, N=300, Nz=5, flag=None, special='twin'),
               # |a - b| <= |a| + |b| <= 2 max|m|: the cap is the minimum only where there is no pair at all, C = 1
               Case('measures dict1x3 the cap is the minimum', CK=(1, 3), kind=0, N=1, Nz=300, flag=1, special='cap'),
               Case('measures dict110x128 kind1', CK=(110, 128), kind=1, N=1, Nz=1, flag=None, special=None)]
MEAS_DX = 48


def meas_make(c):
    g = c.gen()
    means = None
    if c.CK:
        means = torch.randn(*c.CK, generator=g)
        if c.special == 'twin':
            means[4] = means[1]
    bs = []
    for _ in range(MEAS_BATCHES):
        bs.append(dict(x=torch.rand(c.N, MEAS_DX, generator=g), wmse=torch.rand(c.N, generator=g) + 0.05,
                       zdist=torch.randn(c.Nz, generator=g).square(), var_kl=torch.randn(c.Nz, generator=g)))
    return dict(batches=bs, means=means, sigma=torch.tensor([0.3 if c.kind == 1 else 0.7]))


def meas_ref(c, d, dt=F64, plant=None, sumsq=None):
    """The 16 packed measures of MEAS_BATCHES consecutive batches -> (batches, 16): cvae.py:619-624, 689-724, 747-762 and
    layers.py:323-348.  sumsq: the published fp32 sums of squares of x (the kernel reads them from jvae_sqnorm_accum_f32)."""
    sg = _exp(d['sigma'].to(dt))[0] if c.kind == 1 else d['sigma'].to(dt)[0]
    scale = 1. if c.kind >= 2 else sg * sg
    one = torch.ones((), dtype=dt)
    out, prev = [], None
    for b, B in enumerate(d['batches']):
        o = [one * 0] * 16
        o[0] = sg * one
        ss = B['x'].to(dt).square().sum() if sumsq is None else sumsq[b].to(dt)
        o[1] = ss / B['x'].numel()
        o[2] = B['wmse'].to(dt).sum() / c.N * scale
        o[3] = o[2].sqrt()
        o[4] = B['zdist'].to(dt).sum() / c.Nz
        o[5] = B['var_kl'].to(dt).sum() / c.Nz
        if d['means'] is not None:
            mm = d['means'].to(dt)
            C, K = mm.shape
            o[6] = mm.square().sum() / (C * K)
            d2 = (mm.unsqueeze(1) - mm.unsqueeze(0)).square().sum(-1)
            o[7] = math.log(C) - _log(_exp(-d2 / 4).sum(1)).sum() / C
            cap = 2 * mm.square().sum(-1).sqrt().max()
            dist = d2.sqrt() + torch.diag(torch.full((C,), math.inf, dtype=dt))
            o[8] = dist.min() if plant == 'no_cap' else torch.minimum(dist.min(), cap)
        o[9] = one * float(c.flag or 0)
        nb = float(b)
        wt, cnt = (max(nb - 1, 0.), max(nb, 1.)) if plant == 'batch_weight' else (nb, nb + 1)
        run = lambda j, cur: ((prev[j] if b else 0.) * wt + cur) / cnt
        o[10], o[11], o[14], o[15] = run(10, o[1]), run(11, o[2]), run(14, o[4]), run(15, o[5])
        o[12] = o[11].sqrt()
        o[13] = 10 * torch.log10(o[10] / o[11])
        prev = o
        out.append(torch.stack([v * one for v in o]))
    return dict(out=torch.stack(out))


def meas_bound(c, d, r):
    o = r['out']
    e = torch.zeros_like(o)                     # units of U
    ksg = exp_k(d['sigma'].double())[0] if c.kind == 1 else 0.
    red = lambda n: cdiv(n, 256) + TREE
    for b, B in enumerate(d['batches']):
        e[b, 0] = ksg * o[b, 0]
        e[b, 1] = (sqnorm_k(B['x'].numel()) + 1) * o[b, 1]                         # the sum of squares, the division
        k2 = red(c.N) + 1 + (0 if c.kind >= 2 else 2 * ksg + 2)                   # sum, / N, sigma^2 (its square: 1), the product
        e[b, 2] = k2 * B['wmse'].double().abs().sum() / c.N * (1. if c.kind >= 2 else o[b, 0] ** 2)
        e[b, 3] = e[b, 2] / (2 * o[b, 3]) + o[b, 3]
        e[b, 4] = (red(c.Nz) + 1) * B['zdist'].double().abs().sum() / c.Nz
        e[b, 5] = (red(c.Nz) + 1) * B['var_kl'].double().abs().sum() / c.Nz
        if d['means'] is not None:
            mm = d['means'].double()
            C, K = mm.shape
            e[b, 6] = (1 + red(C * K) + 1) * o[b, 6]
            d2 = (mm.unsqueeze(1) - mm.unsqueeze(0)).square().sum(-1)
            # d2: t = fl(a - b) squared (2), the product (1), K additions in sequence; / 4 exact; __expf; the LDS atomics add
            # the C terms of a row in any order (C); __logf; the block sum of the logarithms; / C; __logf(C); the subtraction
            p = torch.softmax(-d2 / 4, 1)
            rs = (-d2 / 4).exp().sum(1)
            e_rs = (p * ((K + 3) * d2 / 4 + exp_k(d2 / 4))).sum(1) + C
            e_log = e_rs + LOG_K * rs.log().abs()
            e[b, 7] = (e_log.sum() + (red(C) + 1) * rs.log().abs().sum()) / C + LOG_K * math.log(C) + math.log(C) + (rs.log().sum() / C).abs()
            # a distance: d2's K + 3, halved by the square root, its own rounding; min and max pass relative errors on; 2 * exact
            e[b, 8] = ((K + 3) / 2 + 1) * o[b, 8]
        nb = float(b)
        for j, cur in ((10, 1), (11, 2), (14, 4), (15, 5)):
            # (prev * nb + cur) * inv: the reciprocal, two products, the addition (4 on the magnitude)
            pe, pv = (e[b - 1, j], o[b - 1, j].abs()) if b else (0., 0.)
            e[b, j] = (pe * nb + e[b, cur]) / (nb + 1) + 4 * (pv * nb + o[b, cur].abs()) / (nb + 1)
        e[b, 12] = e[b, 11] / (2 * o[b, 12]) + o[b, 12]
        # 10 log10(rxp / rms): the quotient's relative error (its operands' and its own) lands on the logarithm as it stands
        e[b, 13] = 10 / math.log(10) * (e[b, 10] / o[b, 10].abs() + e[b, 11] / o[b, 11].abs() + 1) + (LOG_K + 1) * o[b, 13].abs()
    return dict(out=U * e + TINY)


MEASURES = Family('measures', MEAS_CASES, meas_make, meas_ref, meas_bound, ['batch_weight', 'no_cap'])

# ============================================================================================ latent
# clip + reparameterise + KL to the class-conditional prior (csrc/latent.hip).  One graph, lat_graph, is evaluated twice: as it
# stands (the reference: fp64, or the fp32 restatement) and as its MAGNITUDE graph - every signed quantity replaced by its
# absolute value, every subtraction by an addition, every derivative path kept positive - whose value is the A of a forward
# result and whose autograd gradient (with |upstream|) is the A of a gradient: the sum of the absolute values of all the path
# products, so a cancellation (b_ - a_ = span under the uniform prior, the rows of tril(T) . d) widens the bound where, and
# only where, the arithmetic is ill-conditioned.
KINDS = {'gs': ('gaussian', 'scalar'), 'gd': ('gaussian', 'diag'), 'gf': ('gaussian', 'full'), 'ti': ('tilted', 'scalar'),
         'un': ('uniform', 'scalar')}
TAU = {'tilted': f32(5.), 'uniform': f32(1.5), 'gaussian': 0.}
C12 = float(np.float32(1.2424533248940002))          # 0.5 log 12
SQ12 = float(np.float32(3.4641016151377544))         # 2 sqrt 3


def uniform_alpha(tau):
    return f32(math.log(2 * tau) - math.log(2 * (0.5 * (1 + math.erf(tau / math.sqrt(2)))) - 1))


_LAT_N, _LAT_L, _LAT_C, _LAT_W = (1, 5, 7, 18), (0, 1, 3), (1, 7), (1., f32(0.3))
LATENT_CASES = []
for _i, _kind in enumerate(KINDS):
    for _j, _K in enumerate((1, 3, 64, 65, 130)):
        if _kind == 'gf' and _K == 130:
            _K = 3                                       # the full variance goes up to K = 65; a second K = 3 at another N
        _q = _i + _j
        LATENT_CASES.append(Case(f'latent {_kind} K{_K} N{_LAT_N[_q % 4]} L{_LAT_L[_q % 3]} C{_LAT_C[(_q // 2) % 2]} '
                                 f'w{_LAT_W[_j % 2]:.1f} #{_j}', kind=_kind, K=_K, N=_LAT_N[_q % 4], L=_LAT_L[_q % 3],
                                 C=_LAT_C[(_q // 2) % 2], w=_LAT_W[_j % 2], sampled=True, forced=None, one_class=False))
LATENT_CASES += [Case(f'latent {k} K{K} N{N} L1 C7 not sampled', kind=k, K=K, N=N, L=1, C=7, w=1., sampled=False, forced=None,
                      one_class=False) for k, K, N in (('gs', 65, 7), ('un', 3, 5))]
LATENT_CASES += [Case(f'latent {k} K{K} N{N} L3 C7 forced', kind=k, K=K, N=N, L=3, C=7, w=f32(0.3), sampled=True, forced=-1.5,
                      one_class=False) for k, K, N in (('gf', 64, 5), ('gd', 130, 18), ('un', 65, 7))]
LATENT_CASES += [Case(f'latent {k} K{K} N18 L1 C7 one class', kind=k, K=K, N=18, L=1, C=7, w=1., sampled=True, forced=None,
                      one_class=True) for k, K in (('gf', 65), ('gd', 3), ('ti', 64))]


def latent_make(c):
    g = c.gen()
    N, K, C = c.N, c.K, c.C
    prior, var = KINDS[c.kind]
    mu = torch.randn(N, K, generator=g)
    lv = 2 * torch.randn(N, K, generator=g)
    edge = torch.tensor([20., -20., 30., -30.])          # on the clip's edge (the gradient passes) and well outside (zero)
    lv.view(-1)[:min(4, N * K)] = edge[:min(4, N * K)]
    lv = lv.clamp(-30, 30)
    eps = torch.randn(c.L + 1, N, K, generator=g)
    eps[0] = 0
    y = torch.randint(0, C, (N,), generator=g)
    if C == 7 and N >= 7:
        y[y == 5] = 4                                     # class 5 is absent from the batch
    if c.one_class:
        y[:] = 2
    means = torch.randn(C, K, generator=g)
    if prior == 'tilted' or K == 1:                       # away from dist = 0 (tau / sqrt(dist) in the tilted backward)
        means = means + 3. * torch.sign(means)
    if var == 'scalar':
        T = torch.rand(C, generator=g) + 0.5
    elif var == 'diag':
        T = (torch.rand(C, K, generator=g) + 0.5) * torch.sign(torch.randn(C, K, generator=g))
    else:                                                 # every entry filled: the upper triangle must not be read
        T = torch.randn(C, K, K, generator=g) * 0.3 / math.sqrt(K)
        dg = (torch.rand(C, K, generator=g) + 0.5) * torch.sign(torch.randn(C, K, generator=g))
        T = T + torch.diag_embed(dg)
    d = dict(mu=mu, lv_raw=lv, eps=eps, y=y, means=means, T=T, gz=torch.randn(c.L + 1, N, K, generator=g))
    for k in ('gk', 'gd', 'gv'):
        d[k] = torch.randn(N, generator=g)
    return d


class _LogMag(torch.autograd.Function):
    """|log t| with the derivative 1 / t (the magnitude graph's logarithm, t > 0)."""

    @staticmethod
    def forward(ctx, t):
        ctx.save_for_backward(t)
        return t.log().abs()

    @staticmethod
    def backward(ctx, g):
        return g / ctx.saved_tensors[0]


def _lk(t):
    return t - t.detach()             # zero, with the derivative 1


def lat_graph(c, t, mag=False, plant=None):
    """t: mu, lv_raw, means, T (leaves) and eps, y, gz, gk, gd, gv -> dict(lv, z, kl, zdist, var_kl, obj).  mag: the magnitude
    graph (values: the A of each forward result; obj: its gradient is the A of each gradient)."""
    prior, var = KINDS[c.kind]
    tau, w, K = TAU[prior], c.w, c.K
    mu, lr, y = t['mu'], t['lv_raw'], t['y']
    ab = (lambda v: v.abs()) if mag else (lambda v: v)
    if c.forced is not None:
        lv = torch.full_like(mu, f32(c.forced)).detach()
        lv_e, lv_a = lv, ab(lv)
    else:
        inside = ((lr >= -20) & (lr <= 20)).detach().to(mu.dtype)
        if plant == 'clip_grad_pass':
            inside = torch.ones_like(inside)
        clipped = lr.detach().clamp(-20, 20)
        lv = clipped + inside * _lk(lr)                  # clamp's sub-gradient: 1 on [-20, 20], edges included, 0 outside
        lv_e, lv_a = lv, (clipped.abs() + inside * _lk(lr) if mag else lv)
    sd = _exp(0.5 * lv_e)
    z = ab(mu).detach() + _lk(mu) + sd * ab(t['eps']) * (1. if c.sampled else 0.) if mag else mu + sd * t['eps'] * (1. if c.sampled else 0.)
    m = t['means'][y]
    d = (mu - m).detach().abs() + _lk(mu) + _lk(m) if mag else mu - m
    out = dict(lv=lv.detach(), z=z)
    if prior == 'uniform':
        alpha = uniform_alpha(tau)
        coef = alpha - 0.5 * LOG2PI
        span = SQ12 * sd
        dr = (mu - m).detach()
        lo, hi = ((dr - 0.5 * span.detach()) / tau), ((dr + 0.5 * span.detach()) / tau)
        ina, inb = ((lo > -1) & (lo < 1)).to(mu.dtype), ((hi > -1) & (hi < 1)).to(mu.dtype)
        if mag:
            a_ = (tau * lo.clamp(-1, 1)).abs() + ina * (_lk(d) + 0.5 * _lk(span))
            b_ = (tau * hi.clamp(-1, 1)).abs() + inb * (_lk(d) + 0.5 * _lk(span))
            isp = (1 / span).detach() + (1 / span ** 2).detach() * _lk(span)
        else:
            a_ = tau * torch.clamp((d - 0.5 * span) / tau, -1, 1)
            b_ = tau * torch.clamp((d + 0.5 * span) / tau, -1, 1)
            isp = 1 / span
        elogq = 0.5 * lv_a + C12 if mag else -0.5 * lv_a - C12
        nel = (LOG2PI + d * d + span * span / 12) * 0.5
        if mag:
            nel = nel + abs(coef) * (b_ + a_) * isp + (b_ ** 3 + a_ ** 3) * isp / 6
        else:
            nel = nel + coef * (b_ - a_) * isp - (b_ ** 3 - a_ ** 3) * isp / 6
        se, sn = elogq.sum(-1), nel.sum(-1)
        vk = se + ab(torch.tensor(K * alpha, dtype=mu.dtype))
        first = se + sn
        out['first'], out['vk'] = first, vk
        real = t.get('branch')
        take_first = (first >= vk).detach() if real is None else real
        out['branch'] = take_first
        kl = torch.where(take_first, first, vk)
        ww = 1. if plant == 'no_w' else w
        if ww != 1.:
            kl = kl + ab(torch.tensor(ww - 1., dtype=mu.dtype)) * vk
        vkl = vk if plant == 'uniform_vkl_no2' else 2 * vk
        dist = (d * d).sum(-1)
        out['lo'], out['hi'], out['span'] = lo, hi, span.detach()
    else:
        T = t['T']
        if var == 'full':
            Tl = (T.transpose(-1, -2) if plant == 'T_upper' else T).tril()[y]
            Tl = Tl.detach().abs() + _lk(Tl) if mag else Tl
            wd = (Tl @ d.unsqueeze(-1)).squeeze(-1)
            pd = Tl.square().sum(-2)
            dg = torch.diagonal(Tl, dim1=-2, dim2=-1)
            ldp = 2 * _LogMag.apply(dg).sum(-1) if mag else -2 * _log(dg.abs()).sum(-1)
        else:
            tt = T[y].unsqueeze(-1) if var == 'scalar' else T[y]
            tt = tt.detach().abs() + _lk(tt) if mag else tt
            wd, pd = d * tt, tt * tt
            if var == 'scalar':
                ldp = 2 * K * _LogMag.apply(tt[:, 0]) if mag else -2 * K * _log(tt[:, 0])
            else:
                ldp = 2 * _LogMag.apply(tt).sum(-1) if mag else -2 * _log(tt.abs()).sum(-1)
        dist = wd.square().sum(-1)
        if prior == 'tilted':
            kl = 0.5 * (dist.sqrt() + tau) ** 2 if mag else 0.5 * (dist.sqrt() - tau) ** 2
            vkl = torch.zeros_like(dist)
        else:
            trace = (_exp(lv_e) * pd).sum(-1)
            vkl = trace + lv_a.sum(-1) + ldp + K if mag else trace - lv_a.sum(-1) + ldp - K
            kl = 0.5 * (dist + (1. if plant == 'no_w' else w) * vkl)
    out.update(kl=kl, zdist=dist, var_kl=vkl)
    g = {k: ab(t[k]) for k in ('gz', 'gk', 'gd', 'gv')}
    out['obj'] = (z * g['gz']).sum() + (kl * g['gk']).sum() + (dist * g['gd']).sum() + (vkl * g['gv']).sum()
    return out


def _lat_leaves(c, d, dt):
    return {k: (leaf(v, dt) if k in ('mu', 'lv_raw', 'means', 'T') else (v if k == 'y' else v.to(dt))) for k, v in d.items()}


def latent_ref(c, d, dt=F64, plant=None, mag=False, branch=None):
    t = _lat_leaves(c, d, dt)
    if branch is not None:
        t['branch'] = branch
    o = lat_graph(c, t, mag, plant)
    o['obj'].backward()
    r = dict(lv=o['lv'], z=o['z'].detach(), kl=o['kl'].detach(), zdist=o['zdist'].detach(), var_kl=o['var_kl'].detach(),
             gmu=_grad(t['mu']), glv=_grad(t['lv_raw']), gmeans=_grad(t['means']))
    if KINDS[c.kind][1] != 'scalar':
        r['gT'] = _grad(t['T'])
    mm = d['means'].to(dt)
    dm = mm.sum(0) / c.C
    dmu = d['mu'].to(dt) - dm
    if mag:
        Am = mm.abs().sum(0) / c.C
        r['dzdist'] = (d['mu'].to(dt).abs() + Am).square().sum(1) + (mm.square().sum() / c.C + Am.square().sum())
    else:
        r['dzdist'] = dmu.square().sum(1) + (mm.square().sum(1).sum() / c.C - dm.square().sum())
    r['_aux'] = {k: o[k].detach() for k in ('first', 'vk', 'lo', 'hi', 'span', 'branch') if k in o}
    return r


def latent_counts(c, d):
    """The roundings k of each output, counted from latent_fwd_sample / latent_bwd_sample (ser: a lane's share of K; 6: the
    butterfly).  ke: __expf(lv) or __expf(lv / 2) at the largest |lv| of the case."""
    prior, var = KINDS[c.kind]
    K, ser = c.K, cdiv(c.K, 64)
    lvmax = 1.5 if c.forced is not None else float(d['lv_raw'].abs().clamp(max=20).max())
    ke = 2 * EXP_ULPS + lvmax
    k = dict(lv=0., z=ke + 3)                               # sd, sd * eps, (* sampled: exact), mu + .
    if prior == 'uniform':
        # span = c * sd (ke + 2); a_, b_: d (1), -+ span / 2 (1), / tau, * tau (2) -> ke + 6; their cubes (3 x, + 2), / span
        # (ke + 3), / 6 (1); the three parts of nel (3): 4 ke + 27 in all, generously; then the sum and the few steps behind it
        kel = 4 * ke + 27
        k.update(zdist=3 + ser + 6, var_kl=3 + ser + 6 + 2, kl=kel + ser + 6 + 4)
    else:
        kwd = 2 if var != 'full' else K + 2                 # d (1), * t (1) | the row of tril(T) . d: K products and sums
        kpd = 1 if var != 'full' else K + 2
        k['zdist'] = 2 * kwd + 1 + ser + 6
        k['var_kl'] = max(ke + kpd + 1, LOG_K + 2) + ser + 6 + 3
        k['kl'] = max(k['zdist'], k['var_kl'] + 1) + 2 if prior == 'gaussian' else k['zdist'] + 6
        if prior == 'tilted':
            k['var_kl'] = 0.
    kv = max(k['kl'], k['var_kl'], k['zdist'], k['z'])
    k['gmu'] = k['glv'] = kv + 8 + c.L + 1                  # the upstream sums (L + 1), the chain rule's few products
    fold = cdiv(c.N, 16) + 16                               # means_grad_kernel: a chunk in sample order, the 16 chunks
    k['gmeans'] = k['gmu'] + fold
    k['gT'] = k['gmu'] + (fold if var == 'diag' else c.N)   # gT_full_kernel walks the N samples
    groups = max(1, 1024 // K)
    # t = mu - dict[k] (1; dict[k]: dict_stats_kernel's mean, see dict_bound), t * t (2 x, + 1), the sum; + dict[K] (block sums)
    k['dzdist'] = 2 * (cdiv(c.C, groups) + groups + 1 + 1) + 1 + ser + 6 + TREE + cdiv(c.C, groups) * cdiv(K, 1024) + 4
    return k


def latent_bound(c, d, r):
    A = latent_ref(c, d, F64, mag=True, branch=r['_aux'].get('branch'))
    k = latent_counts(c, d)
    return {n: k[n] * U * A[n].abs() + TINY for n in r if n != '_aux'}


LATENT = Family('latent', LATENT_CASES, latent_make, latent_ref, latent_bound,
                ['T_upper', 'no_w', 'uniform_vkl_no2', 'clip_grad_pass'])

DICT_CASES = [Case(f'dict_stats C{C} K{K}', C=C, K=K) for C, K in ((1, 1), (7, 200), (3, 1030))]      # 1030: two trips of the K loop


def dict_make(c):
    return dict(means=torch.randn(c.C, c.K, generator=c.gen()) + 0.5)


def dict_ref(c, d, dt=F64, plant=None):
    """dict[0..K) = the mean of the dictionary's rows; dict[K] = mean_c |m_c|^2 - |mean|^2 (cvae.py:747-752)."""
    m = d['means'].to(dt)
    if plant == 'drop_last':
        m = torch.cat([m[:, :-1], 0 * m[:, -1:]], 1)
    dm = m.sum(0) / c.C
    return dict(dict=torch.cat([dm, (m.square().sum() / c.C - dm.square().sum()).reshape(1)]))


def dict_bound(c, d, r):
    m = d['means'].double()
    groups = max(1, 1024 // c.K)
    # a mean: a thread adds ceil(C / groups) rows, thread 0 of the column the groups' partial sums, / C
    kmean = cdiv(c.C, groups) + groups + 1
    Am = m.abs().sum(0) / c.C
    # dict[K]: v * v (1) over a thread's rows and K-trips, block_sum, / C; t * t of the means (2 kmean + 1), block_sum; the subtraction
    ksq = 1 + cdiv(c.C, groups) * cdiv(c.K, 1024 // groups if groups > 1 else 1024) + TREE + 1
    e = ksq * m.square().sum() / c.C + (2 * kmean + 1 + cdiv(c.K, 1024) + TREE) * Am.square().sum() + (m.square().sum() / c.C + Am.square().sum())
    return dict(dict=U * torch.cat([kmean * Am, e.reshape(1)]) + TINY)


DICT = Family('dict_stats', DICT_CASES, dict_make, dict_ref, dict_bound, ['drop_last'])

FAMILIES = [RECON, ELBO, CHAIN, XENT, ACT, LOSS_SUMS, SQNORM, IWS, MEASURES, LATENT, DICT]
