"""The class-marginal KL of csrc/semisup.hip restated in torch (fp64 by default), its hand-written gradients, the case table and the
per-output error bound B(case) that the GPU tests hold the kernels to: |error| <= 2^-24 B on every element.

Forward, for a row with y < 0 (a row with y >= 0 keeps its kl_in / zdist_in / var_kl_in and a one-hot row of r):

    d_c  = sum_k t_ck^2 (mu_k - m_ck)^2        v_c = sum_k e^lv_k t_ck^2 - sum_k lv_k - sum_k log t_ck^2 - K
    KL_c = 1/2 (d_c + w v_c)                    Q_c = KL_c - log pi_c,   a = min_c Q_c,   s = sum_c exp(-(Q_c - a))
    kl = U = a - log s      r_c = exp(-(Q_c - a)) / s      zdist = sum_c r_c d_c      var_kl = sum_c r_c v_c

Backward (g = d loss / d kl; unlabelled rows only, a labelled row hands g back to its kl_in):

    g_mu[n,k]    = g_n sum_c r_nc t_ck^2 (mu_nk - m_ck)            g_lv[n,k] = g_n w/2 (e^lv_nk sum_c r_nc t_ck^2 - 1)
    g_means[c,k] = -sum_n g_n r_nc t_ck^2 (mu_nk - m_ck)           g_T[c,k]  = sum_n g_n r_nc (t_ck ((mu_nk - m_ck)^2 + w e^lv_nk) - w / t_ck)

The bound B is DERIVED, nothing in it is fitted; u = 2^-24, and 2^-53 = 2^-29 u (U64 below).  The kernel is fp64 from its fp32
operands to the one rounding of each output (t^2 = t t and mu - m are exact in fp64), so:

  * every output is rounded once: + |output|.
  * KL_c: every addend of d_c, of the trace, of sum lv and of sum log t^2 is formed with at most 6 roundings (exp and log of the
    device library: 2 each at the most, the products) and then passes through at most K partial sums, the four-way merge of the
    logarithms and the last four operations: dKL_c <= U64 (K + 14) A_c, A_c = 1/2 (d_c + |w| (trace_c + sum |lv| + sum |log t^2| +
    K)); DQ = max_c dKL_c + 2 U64 |log pi_c| per row.
  * the shifted sum: the exponent -(Q_c - a) carries both Q (2 DQ) and its own rounding and exponential (U64 (3 + (Q_c - a))); the
    sum over a tile is a butterfly of 6 levels, the fold costs 3 per tile, the logarithm / the reciprocal and product 4: LEV = 10 +
    3 ceil(C / 64).  So ln r_c moves by RR_c = 2 DQ + U64 (LEV + 3 + (Q_c - a)), and U by sum_c r_c RR_c (a convex mix of the moves
    of its terms) + DQ.
  * zdist, var_kl: sum_c r_c x_c with both factors in error: sum_c r_c |x_c| (RR_c + U64 (K + 14 + LEV)) - for var_kl |x_c| is the
    sum of the magnitudes of the four parts of v_c.
  * an r_c so small that fp32 cannot hold it: TINY.
  * the backward reads the fp32 r the forward returned: |r32 - r| <= u B_r.  A sum of addends coef r x therefore carries sum |coef|
    B_r |x| and, for the fp64 chain and the formation of x, U64 (terms + 12) sum |coef| r |x| with the parts of x taken in
    magnitude; terms = C for a row sum, ceil(N / 16) + 16 for a class sum.
  * g_kl_in and every output of a labelled row are copies: B = 0, the GPU test asks for the same bits.

This is a closed bound for every output: the 4 x torch-fp32 margin the issue allows was not needed."""
import collections
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
U64 = 2.0 ** -29              # the unit roundoff of fp64 in units of u
TINY = 2.0 ** -100
CLASS_TILE = 64               # SS_CT of csrc/semisup.hip
ROW_CHUNKS = 16               # SS_CHUNKS

Case = collections.namedtuple('Case', 'name N C K var w pi stress')
PATTERNS = ('half', 'all_unlabelled', 'all_labelled', 'last')


def _c(name, N, C, K, var='scalar', w=1., pi=False, stress=None):
    return Case(name, N, C, K, var, w, pi, stress)


SHAPE_CASES = [
    _c('N1_C2_K1', 1, 2, 1),
    _c('N37_C3_K5_diag_w05_pi', 37, 3, 5, var='diag', w=0.5, pi=True),
    _c('N64_C10_K64', 64, 10, 64),
    _c('N65_C100_K65_diag', 65, 100, 65, var='diag'),          # crosses a class tile, a lane count and a K tile
    _c('N33_C7_K1024', 33, 7, 1024),
]
STRESS_CASES = [
    _c('spread_N9_C4_K8', 9, 4, 8, stress='spread'),           # the KL_c differ by more than 10^4: U finite, r exactly one-hot
    _c('equal_N9_C5_K8_diag', 9, 5, 8, var='diag', stress='equal'),      # equal classes, uniform pi: r = 1 / C, U = KL_c
    _c('tinypi_N9_C4_K8', 9, 4, 8, pi=True, stress='tinypi'),  # one pi_c of 1e-30: every output finite
    _c('empty_N9_C4_K8_diag', 9, 4, 8, var='diag', stress='empty'),      # class 2 is nobody's: its r column is exactly zero
]
ids = lambda c: c.name      # noqa: E731


def labels(c, pattern, gen):
    """y (N,) int64: a class in [0, C) for a labelled row, a negative number for an unlabelled one."""
    y = torch.randint(0, c.C, (c.N,), generator=gen, dtype=torch.int64)
    if c.stress == 'empty':
        y[y == 2] = 0
    hide = torch.zeros(c.N, dtype=torch.bool)
    if pattern == 'half':
        hide[torch.randperm(c.N, generator=gen)[:(c.N + 1) // 2]] = True
    elif pattern == 'all_unlabelled':
        hide[:] = True
    elif pattern == 'last':
        hide[-1] = True
    elif pattern != 'all_labelled':
        raise ValueError(pattern)
    y[hide] = -1
    y[hide & (torch.arange(c.N) % 3 == 1)] = -7               # any negative number means "no label"
    return y


def make(c, pattern='half', seed=0):
    """The operands of a case, on the CPU: mu, lv (N,K), y, means, T, log_pi (C,) fp64 | None, g (N,), the incoming kl_in, zd_in,
    vkl_in (N,) (any fp32 numbers: labelled rows must come back with their bits)."""
    gen = torch.Generator().manual_seed(3000 + seed + sum(map(ord, c.name + pattern)))

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float32)

    def ru(lo, hi, *s):
        return lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float32)
    N, C, K = c.N, c.C, c.K
    mu, lv = rn(N, K), ru(-3., 0.5, N, K)
    means = 1.5 * rn(C, K)
    T = ru(0.7, 1.4, C, K) if c.var == 'diag' else ru(0.7, 1.4, C)
    if c.var == 'diag':
        T[:, ::2] *= -1                                       # log t^2: the sign of a factor is free
    log_pi = None
    if c.pi:
        p = ru(0.2, 1., C).to(F64)
        if c.stress == 'tinypi':
            p[1] = 1e-30
        log_pi = (p / p.sum()).log()
    if c.stress == 'spread':
        means = 150. * rn(C, K)
        mu = means[torch.arange(N) % C] + rn(N, K)
    elif c.stress == 'equal':
        means = means[:1].expand(C, K).contiguous()
        T = T[:1].expand(C, K).contiguous()
    elif c.stress == 'empty':
        means[2] = 1e3
    return dict(mu=mu, lv=lv, y=labels(c, pattern, gen), means=means, T=T, log_pi=log_pi, g=ru(-1., 1., N),
                kl_in=ru(0., 50., N), zd_in=ru(0., 50., N), vkl_in=ru(-5., 50., N))


def _t(c, v):
    return v['T'] if c.var == 'diag' else v['T'].unsqueeze(-1).expand(c.C, c.K)


def classes(c, d, dt=F64, leaves=None):
    """-> dict of (N, C) tensors in `dt`: dist, trace, v, KL, Q and the (N,) / (C,) parts slv, slog, differentiable in the operands."""
    v = {k: d[k].to(dt) for k in ('mu', 'lv', 'means', 'T')}
    v.update(leaves or {})
    t = _t(c, v)
    t2 = t * t
    x = v['mu'].unsqueeze(1) - v['means'].unsqueeze(0)                              # (N, C, K)
    dist = (t2 * x * x).sum(-1)
    trace = (v['lv'].exp().unsqueeze(1) * t2).sum(-1)
    slv, slog = v['lv'].sum(-1), t2.log().sum(-1)
    var = trace - slv.unsqueeze(1) - slog.unsqueeze(0) - c.K
    KL = 0.5 * (dist + c.w * var)
    lpi = -math.log(c.C) if d['log_pi'] is None else d['log_pi'].to(dt).unsqueeze(0)
    return dict(dist=dist, trace=trace, v=var, KL=KL, Q=KL - lpi, slv=slv, slog=slog, t=t, x=x)


def marginal(cl):
    """-> U (N,), r (N, C), a (N,) of every row, as if none had a label."""
    Q = cl['Q']
    a = Q.min(1, keepdim=True).values
    e = (-(Q - a)).exp()
    s = e.sum(1, keepdim=True)
    return a.squeeze(1) - s.squeeze(1).log(), e / s, a.squeeze(1)


def ref(c, d, dt=F64):
    """Every output of forward and backward (the gradients written out by hand); everything in `dt`."""
    cl = classes(c, d, dt)
    U_, r_all, a = marginal(cl)
    unl = d['y'] < 0
    um = unl.to(dt)
    onehot = (d['y'].view(-1, 1) == torch.arange(c.C).view(1, -1)).to(dt)
    r = torch.where(unl.view(-1, 1), r_all, onehot)
    out = dict(kl=torch.where(unl, U_, d['kl_in'].to(dt)), zdist=torch.where(unl, (r_all * cl['dist']).sum(1), d['zd_in'].to(dt)),
               var_kl=torch.where(unl, (r_all * cl['v']).sum(1), d['vkl_in'].to(dt)), r=r)
    g = d['g'].to(dt)
    gu = (g * um).view(-1, 1, 1)
    t, x = cl['t'], cl['x']
    t2 = t * t
    e = d['lv'].to(dt).exp()
    rt2x = r_all.unsqueeze(-1) * t2 * x                                             # (N, C, K)
    out['g_kl_in'] = g * (1 - um)
    out['g_mu'] = (gu * rt2x).sum(1)
    out['g_lv'] = gu.squeeze(1) * 0.5 * c.w * (e * (r_all.unsqueeze(-1) * t2).sum(1) - 1)
    out['g_means'] = -(gu * rt2x).sum(0)
    if c.var == 'diag':
        out['g_T'] = (gu * r_all.unsqueeze(-1) * (t * (x * x + c.w * e.unsqueeze(1)) - c.w / t)).sum(0)
    out['parts'] = dict(cl, U=U_, r_all=r_all, a=a)
    return out


def autograd_ref(c, d):
    """The same gradients from torch.autograd in fp64 on the restatement's own forward: sum_n g_n kl_n."""
    names = ['mu', 'lv', 'means'] + (['T'] if c.var == 'diag' else [])
    leaves = {k: d[k].to(F64).clone().requires_grad_(True) for k in names}
    kl_in = d['kl_in'].to(F64).clone().requires_grad_(True)
    U_, _, _ = marginal(classes(c, d, F64, leaves))
    kl = torch.where(d['y'] < 0, U_, kl_in)
    grads = torch.autograd.grad((d['g'].to(F64) * kl).sum(), [leaves[k] for k in names] + [kl_in])
    return {'g_' + k: v for k, v in zip(names + ['kl_in'], grads)}


def torch_fp32(c, d, device=None):
    """The same objective as a plain torch fp32 expression under autograd (what a user would write; the (N, C, K) tensor exists)
    -> (kl, leaves): the comparison of tools/semi_bench.py and of the model-level gradient test."""
    dev = device or d['mu'].device
    names = ['mu', 'lv', 'means'] + (['T'] if c.var == 'diag' else [])
    v = {k: d[k].to(dev, torch.float32) for k in ('mu', 'lv', 'means', 'T')}
    leaves = {k: v[k].clone().requires_grad_(True) for k in names}
    dd = dict(d, log_pi=None if d['log_pi'] is None else d['log_pi'].to(dev))
    dd.update({k: d[k].to(dev) for k in ('mu', 'lv', 'means', 'T')})
    U_, _, _ = marginal(classes(c, dd, torch.float32, leaves))
    return torch.where(d['y'].to(dev) < 0, U_, d['kl_in'].to(dev)), leaves


def bounds(c, d, r):
    """B for every output of ref(c, d): |fp32 kernel - fp64 restatement| <= u B, element by element.  r = ref(c, d, F64)."""
    N, C, K = c.N, c.C, c.K
    w = abs(c.w)
    p = r['parts']
    unl = (d['y'] < 0)
    um = unl.to(F64)
    lv = d['lv'].to(F64)
    t, x = p['t'], p['x']
    t2 = t * t
    e = lv.exp()
    Av = p['trace'] + lv.abs().sum(-1, keepdim=True) + t2.log().abs().sum(-1).unsqueeze(0) + K           # (N, C)
    A = 0.5 * (p['dist'] + w * Av)
    lpi = torch.full((C,), math.log(C), dtype=F64) if d['log_pi'] is None else d['log_pi'].abs()
    DQ = (U64 * (K + 14) * A + 2 * U64 * lpi.unsqueeze(0)).max(1, keepdim=True).values                   # (N, 1)
    LEV = 10 + 3 * -(-C // CLASS_TILE)
    gap = (p['Q'] - p['a'].unsqueeze(1)).clamp(max=1e300)
    RR = 2 * DQ + U64 * (LEV + 3 + gap)                                                                  # (N, C)
    ra = p['r_all']
    rRR = torch.where(ra > 0, ra * RR, torch.zeros_like(ra))                  # an exponential that is exactly 0 stays 0
    Br_all = ra + rRR + TINY
    out = {}
    out['kl'] = um * (p['U'].abs() + rRR.sum(1) + DQ.squeeze(1))
    out['zdist'] = um * ((ra * p['dist']).sum(1).abs() + (rRR * p['dist']).sum(1) + U64 * (K + 14 + LEV) * (ra * p['dist']).sum(1))
    out['var_kl'] = um * ((ra * p['v']).sum(1).abs() + (rRR * Av).sum(1) + U64 * (K + 14 + LEV) * (ra * Av).sum(1))
    out['r'] = um.view(-1, 1) * Br_all
    g = (d['g'].to(F64).abs() * um).view(-1, 1, 1)
    Br, r3 = Br_all.unsqueeze(-1), ra.unsqueeze(-1)
    ax = (t2 * x).abs()                                                                                  # (N, C, K)
    out['g_kl_in'] = torch.zeros(N, dtype=F64)
    out['g_mu'] = r['g_mu'].abs() + (g * Br * ax).sum(1) + U64 * (C + 12) * (g * r3 * ax).sum(1)
    st2 = (r3 * t2).sum(1)
    out['g_lv'] = (r['g_lv'].abs() + g.squeeze(1) * 0.5 * w * e * (Br * t2).sum(1)
                   + U64 * (C + 12) * g.squeeze(1) * 0.5 * w * (e * st2 + 1))
    n_c = -(-N // ROW_CHUNKS) + ROW_CHUNKS + 12
    out['g_means'] = r['g_means'].abs() + (g * Br * ax).sum(0) + U64 * n_c * (g * r3 * ax).sum(0)
    if c.var == 'diag':
        hT = t * (x * x + c.w * e.unsqueeze(1)) - c.w / t
        aT = t.abs() * (x * x + w * e.unsqueeze(1)) + (w / t).abs()
        out['g_T'] = r['g_T'].abs() + (g * Br * hT.abs()).sum(0) + U64 * n_c * (g * r3 * aT).sum(0)
    return out


def excess(got, want, B):
    """max over the elements of |got - want| / (u B); 0 where the error vanishes; a non-finite result where a finite one is due, or
    an error where B is 0: inf."""
    got = got.detach().to('cpu', F64)
    if got.numel() == 0:
        return 0.
    if not bool(torch.isfinite(got).all()) or not bool(torch.isfinite(want).all()):
        return math.inf
    err = (got - want).abs()
    B = B.expand_as(want) if B.shape != want.shape else B
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * B))
    return float(ratio.max())


# ---- what SEMI_SUPERVISED refuses at the first training-mode evaluate: the rows of iwae_cases.refusal_table() that apply (a plain
# float kl_var_weighting IS supported: a device scalar takes that row's place), and the rows of its own
def refusal_table():
    import iwae_cases
    from oracle.cases import get_case
    base = get_case('c1_n16_mlp')['net']
    rows = [r for r in iwae_cases.refusal_table() if r[0] != 'kl_var_weighting']
    rows = [(n, kw, tw, ev, 'take a label on every row' if n == 'train_captured' else word) for n, kw, tw, ev, word in rows]
    rows += [
        ('device_weight', base, None, dict(kl_var_weighting=torch.tensor(0.5)), 'kl_var_weighting as a device scalar'),
        ('single_prior', dict(base, type='vae', prior=dict(distribution='gaussian', init_mean=0.)), None, {}, 'non-conditional'),
        ('iwae', base, lambda m: setattr(m, 'TRAIN_OBJECTIVE', 'iwae'), {}, "TRAIN_OBJECTIVE = 'iwae'"),
        ('tcvae', base, lambda m: setattr(m, 'TRAIN_OBJECTIVE', 'tcvae'), {}, "TRAIN_OBJECTIVE = 'tcvae'"),
    ]
    return rows


def refusal_model(kwargs, tweak, device=None):
    from cvae import ClassificationVariationalNetwork as Net
    m = Net(**kwargs)
    if device is not None:
        m.to(device)
    if tweak is not None:
        tweak(m)
    m.SEMI_SUPERVISED = True
    m.train()
    return m
