"""The beta-TCVAE split of csrc/tcvae.hip restated in torch (fp64 by default), its hand-written direct gradients, the case table
and the per-output error bound B(case) that the GPU tests hold the kernels to: |error| <= 2^-24 B on every element.

Forward, for sample i of class y_i, its draws l = 1..L (row 0 of z takes no part) and S_i = the rows j with y_j = y_i:

    l_ijk = -1/2 (lv_jk + (z_lik - mu_jk)^2 e^(-lv_jk) + log 2pi),      c_i = log |S_i| + log n_i      (n_i = |S_i| without log_n)
    A  = -1/2 sum_k (eps_lik^2 + lv_ik) - K/2 log 2pi          J = logsumexp_{j in S_i} sum_k l_ijk - c_i
    P  = sum_k [logsumexp_{j in S_i} l_ijk - c_i]               Bp = -K/2 log 2pi - 1/2 |T_y (z - m_y)|^2 + sum_k log|t_yk|
    mi = mean_l (A - J),  tc = mean_l (J - P),  dwkl = mean_l (P - Bp),  reg = alpha mi + beta_tc tc + gamma dwkl

Backward (direct partial derivatives, g = d loss / d reg): coefJ = g_i (beta_tc - alpha) / L, coefP = g_i (gamma - beta_tc) / L,
W = coefJ r_ij + coefP r_ijk with r the softmax over j of the joint / of coordinate k, d = z_lik - mu_jk, w = e^(-lv_jk):

    g_z[l,i,k] = -sum_j W d w + g_i gamma / L t^2 (z - m)        g_mu[j,k] = sum_{l,i} W d w
    g_lv[j,k]  = sum_{l,i} W (d^2 w - 1) / 2 - g_j alpha / 2     means, T: -gamma g / L times the gradients of Bp, summed per class

The bound B is DERIVED, nothing in it is fitted; u = 2^-24.  The two logsumexp are computed by the kernels of csrc/aggpost.hip, so
their part of B is the one tests/test_aggpost_restatement.py derives (restated here on whole tensors):

  * a pair's joint exponent Q_ij = c_j + sum_k t_k, t_k = d^2 w: EQ = |c_j| + 4 sum_k t_k + sum_k |c_j + sum_{k' <= k} t_k'|; a
    coordinate's q = lv + t: Eq = 4 t + |q|; each moves its logsumexp by its share p of the sum, halved; the shift costs 3 y, y =
    (Q - min Q) / 2; the sums cost LEVELS (test_aggpost_restatement.levels, which counts a piece of 1024 rows: an upper bound for
    the joint launch's pieces of 64; the pieces are merged in sequence here - an exponential, a product, a sum: 4 more per piece
    after the first).  BJ = sum_j p_j (EQ_j / 2 + 3 y_j) + LEVELS bounds J of one draw, Bk the same for a coordinate, and P carries
    sum_k Bk.
  * A, Bp, the differences, the mean over the draws and reg are fp64 inside the kernel: their roundings enter with 2^-53 = 2^-29 u
    (term F64 below: every addend of every sum, (K + 10) roundings each), and each output is rounded once: + |output|.  reg is
    alpha A + (beta_tc - alpha) J + (gamma - beta_tc) P - gamma Bp, so it carries |beta_tc - alpha| BJ + |gamma - beta_tc| sum_k Bk: with
    equal weights nothing of the mixture.
  * a weight of the backward: r = 2^(kk (Q - a)) * (1 / s) from the kept (a, s): ln r moves by EQ / 2 (its own Q) + (BJ - LEVELS)
    (the other Q of the sum, through s) + LEVELS (the sum's roundings) + 3 y + 2 (its exponent and exponential) + 2 (the
    reciprocal, the product): RJ = EQ / 2 + 3 y + BJ + 4, and RK likewise.  coefJ = fl(g fl((beta_tc - alpha) / L)) carries 2, the
    two products and the sum of W one each of their own size: |dW| <= u (|coefJ| rJ (RJ + 4) + |coefP| rK (RK + 4)) = u WB.
  * an addend W (d w): d w carries 3 (d, w, the product), the fp64 fma chain nothing to speak of:  a sum of addends is bounded by
    the sum of WB |d w| + 3 |W|abs |d w|; for g_lv the factor is h / 2, h = fmaf(d d, w, -1): 4 t + |h| for its own roundings.
    Every gradient is rounded once: + |gradient|.  The class sums are fp64 chains of fp32 operands: F64 and the final rounding.
  * an exponential so small that it is flushed to zero: TINY.

This is the closed bound for every output, the column gradients included (the 4 x torch-fp32 margin was not needed)."""
import collections
import math

import torch

from test_aggpost_restatement import levels, pieces_of

F64 = torch.float64
U = 2.0 ** -24
U64 = 2.0 ** -29              # the unit roundoff of fp64 in units of u
LOG2PI = math.log(2 * math.pi)
TINY = 2.0 ** -100
JOINT_PART = 64               # rows of a piece of the joint launch (TC_PART of csrc/tcvae.hip); the marginal launch: aggpost's 1024

Case = collections.namedtuple('Case', 'name K L N C classes var weights spread logn stress')


def _c(name, K, L, N, C=1, classes='rand', var='scalar', weights=(1., 6., 1.), spread='wide', logn=False, stress=None):
    return Case(name, K, L, N, C, classes, var, weights, spread, logn, stress)


# classes: 'rand' every class drawn; 'es' (C = 3): class 1 is empty, class 2 has one member (the last sample), the rest class 0;
# 'own' every sample its own class (C = N): singleton sets.  spread: 'wide' variances from 1e-4 to 1 and unit means (the rows of
# a set hardly overlap), 'near' variances from e^-1 to 1 and means within 0.3 (a real mixture).  logn: class counts are given.
SHAPE_CASES = [
    _c('K1_L1_N1_C1', 1, 1, 1),
    _c('K3_L3_N2_C1_diag_w523', 3, 3, 2, var='diag', weights=(0.5, 2., 3.), spread='near'),
    _c('K64_L1_N63_C3_es_logn', 64, 1, 63, C=3, classes='es', logn=True, spread='near'),
    _c('K65_L3_N64_C3_diag_w523', 65, 3, 64, C=3, var='diag', weights=(0.5, 2., 3.)),
    _c('K200_L1_N65_C1', 200, 1, 65, spread='near', logn=True),
    _c('K64_L1_N257_C3_es_diag', 64, 1, 257, C=3, classes='es', var='diag', spread='near'),
    _c('K3_L3_N257_C1_equal', 3, 3, 257, weights=(1., 1., 1.), spread='near'),
    _c('K65_L1_N65_C3_equal_diag', 65, 1, 65, C=3, var='diag', weights=(1., 1., 1.)),
    _c('K1_L3_N64_C3_w523', 1, 3, 64, C=3, weights=(0.5, 2., 3.), spread='near', logn=True),
    _c('K3_L1_N5_own', 3, 1, 5, C=5, classes='own', var='diag'),
]
# the other rows of a set sit 10^4 sigma away: the own row keeps every sum >= 1, every output is finite
STRESS_CASES = [_c('far_K16_L3_N65_C3', 16, 3, 65, C=3, stress='far')]
CASES = SHAPE_CASES + STRESS_CASES
ids = lambda c: c.name      # noqa: E731


def make(c, seed=0):
    """The fp32 operands of a case, on the CPU: z (L+1,N,K), mu, lv (N,K), eps (L,N,K), y, means, T, g (N,), log_n (C,) fp64 | None."""
    gen = torch.Generator().manual_seed(2000 + seed + sum(map(ord, c.name)))

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float32)

    def ru(lo, hi, *s):
        return lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float32)
    K, L, N, C = c.K, c.L, c.N, c.C
    if c.stress == 'far':
        mu, lv = 1e4 * torch.arange(N, dtype=torch.float32).view(N, 1) + rn(N, K), torch.zeros(N, K)
    elif c.spread == 'wide':
        mu, lv = rn(N, K), ru(math.log(1e-4), 0., N, K)
    else:
        mu, lv = 0.3 * rn(N, K), ru(-1., 0., N, K)
    eps = rn(L, N, K)
    z = torch.cat([mu.unsqueeze(0), mu + (0.5 * lv).exp() * eps])
    if c.classes == 'es':
        y = torch.zeros(N, dtype=torch.int64)
        y[-1] = 2
    elif c.classes == 'own':
        y = torch.arange(N, dtype=torch.int64)
    else:
        y = torch.randint(0, C, (N,), generator=gen, dtype=torch.int64)
    means = rn(C, K)
    T = ru(0.8, 1.2, C, K) if c.var == 'diag' else ru(0.8, 1.2, C)
    if c.var == 'diag':
        T[:, ::2] *= -1                                       # log|t|: the sign of a factor is free
    log_n = torch.tensor([1000. * (k + 1) for k in range(C)], dtype=F64).log() if c.logn else None
    return dict(z=z, mu=mu, lv=lv, eps=eps, y=y, means=means, T=T, g=ru(-1., 1., N), log_n=log_n)


def sets(c, d):
    """-> (mask (N, N) bool: j in S_i, ok (N,) bool: the label is in range, c_i (N,) fp64: log |S_i| + log n_i)."""
    y = d['y']
    ok = (y >= 0) & (y < c.C)
    mask = (y.view(-1, 1) == y.view(1, -1)) & ok.view(-1, 1) & ok.view(1, -1)
    B = mask.sum(1).to(F64)
    logB = B.clamp(min=1).log()
    logn = logB if d.get('log_n') is None else d['log_n'].to(F64)[y.clamp(0, c.C - 1)]
    return mask, ok, logB + logn


def _prior(c, v):
    y = v['y'].clamp(0, c.C - 1)
    m = v['means'][y]
    t = v['T'][y] if c.var == 'diag' else v['T'][y].unsqueeze(-1).expand(c.N, c.K)
    return m, t


def terms(c, d, dt=F64, leaves=None):
    """-> per-draw (L, N) A, J, P, Bp, differentiable in the operands.  dt: the precision of the mixture (the exponents, the two
    logsumexp); A and Bp are fp64 whatever dt is, as in the kernel.  leaves: operands already converted (autograd's own leaves)."""
    v = {k: (d[k] if k == 'y' or d[k] is None else d[k].to(F64)) for k in d}
    v.update(leaves or {})
    mask, ok, ci = sets(c, d)
    zq, mu, lv = v['z'][1:].to(dt), v['mu'].to(dt), v['lv'].to(dt)
    dd = (zq.unsqueeze(2) - mu.view(1, 1, c.N, c.K)) ** 2                          # (L, N, N, K)
    q = lv + dd * (-lv).exp()                                                       # coordinate exponents
    Q = q.sum(-1).masked_fill(~mask, math.inf)                                      # joint exponents
    q = q.masked_fill(~mask.view(1, c.N, c.N, 1), math.inf)
    J = (torch.logsumexp(-0.5 * Q, 2).to(F64) - 0.5 * c.K * LOG2PI) - ci
    P = (torch.logsumexp(-0.5 * q, 2).to(F64) - 0.5 * LOG2PI - ci.view(1, -1, 1)).sum(-1)
    A = -0.5 * (v['eps'] ** 2 + v['lv']).sum(-1) - 0.5 * c.K * LOG2PI
    m, t = _prior(c, v)
    Bp = -0.5 * c.K * LOG2PI - 0.5 * ((t * (v['z'][1:] - m)) ** 2).sum(-1) + t.abs().log().sum(-1)
    return A, J, P, Bp


def outputs(c, A, J, P, Bp, ok):
    a, b, g = c.weights
    mi, tc, dwkl = (A - J).mean(0), (J - P).mean(0), (P - Bp).mean(0)
    reg = a * mi + b * tc + g * dwkl
    nan = torch.full_like(reg, math.nan)
    return {k: torch.where(ok, v, nan) for k, v in dict(reg=reg, mi=mi, tc=tc, dwkl=dwkl).items()}


def ref(c, d, dt=F64):
    """Every output of forward and backward (the direct partial derivatives, written out by hand); the mixture in `dt`."""
    mask, ok, ci = sets(c, d)
    A, J, P, Bp = terms(c, d, dt)
    out = outputs(c, A, J, P, Bp, ok)
    a, b, gm = c.weights
    K, L, N = c.K, c.L, c.N
    v = {k: d[k].to(F64) for k in ('z', 'mu', 'lv', 'means', 'T', 'g')}
    v['y'] = d['y']
    g = torch.where(ok, v['g'], torch.zeros_like(v['g']))
    zq, mu, lv = v['z'][1:].to(dt), v['mu'].to(dt), v['lv'].to(dt)
    w = (-lv).exp()
    dl = zq.unsqueeze(2) - mu.view(1, 1, N, K)                                      # (L, N, N, K)
    t = dl * dl * w
    q = (lv + t).masked_fill(~mask.view(1, N, N, 1), math.inf)
    Q = (lv + t).sum(-1).masked_fill(~mask, math.inf)
    rJ = torch.softmax(-0.5 * Q, 2).nan_to_num(0.)                                  # a bad sample's row: no set, no weight
    rK = torch.softmax(-0.5 * q, 2).nan_to_num(0.)
    coefJ = (g * (b - a) / L).to(dt).view(1, N, 1, 1)
    coefP = (g * (gm - b) / L).to(dt).view(1, N, 1, 1)
    W = (coefJ * rJ.unsqueeze(-1) + coefP * rK).to(F64)                             # (L, N, N, K); every sum over it is fp64
    Wdw = W * (dl * w).to(F64)
    m, tt = _prior(c, v)
    dz = v['z'][1:] - m                                                             # (L, N, K)
    gg = (g * gm / L).view(1, N, 1)
    g_z = torch.zeros_like(v['z'])
    g_z[1:] = -Wdw.sum(2) + gg * tt * tt * dz
    g_mu = Wdw.sum((0, 1))
    g_lv = (W * 0.5 * (t - 1).to(F64)).sum((0, 1)) - (0.5 * a * g).view(N, 1)
    bad = ~ok
    g_z[1:, bad] = math.nan
    g_mu[bad] = math.nan
    g_lv[bad] = math.nan
    onehot = (v['y'].view(-1, 1) == torch.arange(c.C).view(1, -1)).to(F64)           # (N, C): a bad label adds to no class
    out.update(g_z=g_z, g_mu=g_mu, g_lv=g_lv, g_means=onehot.T @ (-gg[0] * (tt * tt * dz).sum(0)))
    if c.var == 'diag':
        out['g_T'] = onehot.T @ (-gg[0] * (1 / tt - tt * dz * dz).sum(0))
    out['per_draw'] = dict(A=A, J=J, P=P, Bp=Bp)
    return out


def autograd_ref(c, d):
    """The same gradients from torch.autograd in fp64 on the restatement's own forward: sum_i g_i reg_i."""
    names = ['z', 'mu', 'lv', 'means'] + (['T'] if c.var == 'diag' else [])
    leaves = {k: d[k].to(F64).clone().requires_grad_(True) for k in names}
    _, ok, _ = sets(c, d)
    reg = outputs(c, *terms(c, d, F64, leaves), ok)['reg']
    grads = torch.autograd.grad((d['g'].to(F64) * reg)[ok].sum(), [leaves[k] for k in names])
    return {'g_' + k: v for k, v in zip(names, grads)}


def bounds(c, d, r):
    """B for every output of ref(c, d): |fp32 kernel - fp64 restatement| <= u B, element by element.  r = ref(c, d, F64)."""
    K, L, N = c.K, c.L, c.N
    a, b, gm = c.weights
    mask, ok, ci = sets(c, d)
    v = {k: d[k].to(F64) for k in ('z', 'mu', 'lv', 'eps', 'means', 'T', 'g')}
    v['y'] = d['y']
    g = torch.where(ok, v['g'], torch.zeros_like(v['g'])).abs()
    zq, mu, lv = v['z'][1:], v['mu'], v['lv']
    w = (-lv).exp()
    dl = zq.unsqueeze(2) - mu.view(1, 1, N, K)
    t = dl * dl * w                                                                 # (L, N, N, K)
    cj = lv.sum(-1).view(1, 1, N)
    Q = (cj + t.sum(-1)).masked_fill(~mask, math.inf)
    EQ = cj.abs() + 4 * t.sum(-1) + (cj.unsqueeze(-1) + t.cumsum(-1)).abs().sum(-1)  # (L, N, N)
    yJ = (0.5 * (Q - Q.min(2, keepdim=True).values)).nan_to_num(0., posinf=0.)
    pJ = torch.softmax(-0.5 * Q, 2).nan_to_num(0.)
    lev_j = levels(N, False) + 4 * (-(-N // JOINT_PART) - 1)
    lev_k = levels(N, True) + 4 * (pieces_of(N) - 1)
    BJ = (pJ * (0.5 * EQ + 3 * yJ)).sum(2) + lev_j                                  # (L, N)
    q = (lv + t).masked_fill(~mask.view(1, N, N, 1), math.inf)
    Eq = 4 * t + (lv + t).abs()
    yK = (0.5 * (q - q.min(2, keepdim=True).values)).nan_to_num(0., posinf=0.)
    pK = torch.softmax(-0.5 * q, 2).nan_to_num(0.)
    Bk = (pK * (0.5 * Eq + 3 * yK)).sum(2) + lev_k                                  # (L, N, K)
    BP = Bk.sum(-1)
    # the fp64 part: every addend of A, Bp, the K marginals and the ends
    m, tt = _prior(c, v)
    dz = zq - m
    pd = r['per_draw']
    F = U64 * (K + 10) * ((0.5 * (v['eps'] ** 2 + lv.abs())).sum(-1) + 0.5 * ((tt * dz) ** 2).sum(-1) + tt.abs().log().abs().sum(-1)
                          + pd['J'].abs() + pd['P'].abs() + 2 * K * (LOG2PI + ci.abs()) + 1)
    out = {}
    fin = lambda x: x.nan_to_num(0.)                                                # noqa: E731  (a bad sample: NaN on both sides)
    out['mi'] = (BJ + F).mean(0) + fin(r['mi']).abs()
    out['tc'] = (BJ + BP + F).mean(0) + fin(r['tc']).abs()
    out['dwkl'] = (BP + F).mean(0) + fin(r['dwkl']).abs()
    out['reg'] = (abs(b - a) * BJ + abs(gm - b) * BP + (abs(a) + abs(b) + abs(gm)) * F).mean(0) + fin(r['reg']).abs()
    # ---- the weights of the backward ------------------------------------------------------------------------------------------
    RJ = 0.5 * EQ + 3 * yJ + BJ.unsqueeze(2) + 4                                    # (L, N, N)
    RK = 0.5 * Eq + 3 * yK + Bk.unsqueeze(2) + 4                                    # (L, N, N, K)
    cJ = (g * abs(b - a) / L).view(1, N, 1, 1)
    cP = (g * abs(gm - b) / L).view(1, N, 1, 1)
    WB = cJ * (pJ * (RJ + 4)).unsqueeze(-1) + cP * pK * (RK + 4) + (cJ + cP) * TINY
    Wabs = cJ * pJ.unsqueeze(-1) + cP * pK
    WB = WB * mask.view(1, N, N, 1)
    dw = (dl * w).abs()
    add = WB * dw + 3 * Wabs * dw                                                   # (L, N, N, K)
    gg = (g * abs(gm) / L).view(1, N, 1)
    prior_z = gg * (tt * tt * dz).abs()
    B_gz = torch.zeros_like(v['z'])
    B_gz[1:] = add.sum(2) + U64 * (N + 8) * (Wabs * dw).sum(2) + U64 * 8 * prior_z + fin(r['g_z'][1:]).abs()
    out['g_z'] = B_gz
    out['g_mu'] = add.sum((0, 1)) + U64 * (L * N + 8) * (Wabs * dw).sum((0, 1)) + fin(r['g_mu']).abs()
    h = (t - 1).abs()
    add_lv = 0.5 * (WB * h + Wabs * (4 * t + h))
    out['g_lv'] = (add_lv.sum((0, 1)) + U64 * (L * N + 8) * (Wabs * 0.5 * h).sum((0, 1)) + U64 * 4 * (0.5 * abs(a) * g).view(N, 1)
                   + fin(r['g_lv']).abs())
    onehot = (v['y'].view(-1, 1) == torch.arange(c.C).view(1, -1)).to(F64)
    n_c = L + 8 + (-(-N // 16) + 16)
    out['g_means'] = U64 * n_c * (onehot.T @ (gg[0] * (tt * tt * dz).abs().sum(0))) + r['g_means'].abs()
    if c.var == 'diag':
        out['g_T'] = U64 * n_c * (onehot.T @ (gg[0] * ((1 / tt).abs() + tt.abs() * dz * dz).sum(0))) + r['g_T'].abs()
    return out


def excess(got, want, B):
    """max over the elements of |got - want| / (u B); 0 where both the error and B vanish; NaN must meet NaN.  A non-finite
    result where a finite one is due: inf."""
    got = got.detach().to('cpu', F64)
    if got.numel() == 0:
        return 0.
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan) or not bool(torch.isfinite(got[~nan]).all()):
        return math.inf
    err = (got - want).abs()[~nan]
    B = (B.expand_as(want) if B.shape != want.shape else B)[~nan]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * B))
    return float(ratio.max()) if ratio.numel() else 0.


# ---- what TRAIN_OBJECTIVE = 'tcvae' refuses at the first training-mode evaluate: the rows of iwae_cases.refusal_table() (the same
# models, the same words) with this objective switched on
def refusal_table():
    import iwae_cases
    return iwae_cases.refusal_table()


def refusal_model(kwargs, tweak, device=None):
    from cvae import ClassificationVariationalNetwork as Net
    m = Net(**kwargs)
    if device is not None:
        m.to(device)
    if tweak is not None:
        tweak(m)
    m.TRAIN_OBJECTIVE = 'tcvae'
    m.train()
    return m
