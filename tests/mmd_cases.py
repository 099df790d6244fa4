"""The MMD objective of csrc/mmd.hip restated in torch fp64, its hand-written direct gradients, the case table and the per-output
error bound B(case) that the GPU tests hold the kernels to: |error| <= 2^-24 B on every element.

Forward, for sample i of class y_i, its draws l = 1..L (row 0 of z takes no part) and S_i = the rows j with y_j = y_i (joint off
or one class: every row):

    p_li = m_{y_i} + e'_li / t_{y_i}              formed in fp32, operation by operation, as ops.prior_sample forms it: the
                                                  restatement takes these fp32 values as given (d['p']) and works in fp64 from there
    m_i = mean_l [ 1/(N-1) sum_{j in S_i, j != i} k(z_li, z_lj) + 1/(N-1) sum_{j in S_i, j != i} k(p_li, p_lj)
                   - 2/N sum_{j in S_i} k(z_li, p_lj) ]                                 (N = 1: the two within sums are 0)
    'imq': k(a, b) = sum_s C_s / (C_s + |a - b|^2)        'rbf': k(a, b) = sum_s exp(-|a - b|^2 / (2 h_s))

Backward (direct partial derivatives, g = d loss / d m; k' = d k / d |a - b|^2, so grad_1 k(a, b) = 2 k' (a - b)):

    g_z[l,i] = 1/L [ sum_{j != i} (g_i + g_j)/(N-1) 2 k'(z_i, z_j) (z_i - z_j) - 2/N g_i sum_j 2 k'(z_i, p_j) (z_i - p_j) ]
    g_p[l,j] = 1/L [ sum_{i != j} (g_i + g_j)/(N-1) 2 k'(p_j, p_i) (p_j - p_i) - 2/N sum_i g_i 2 k'(z_i, p_j) (p_j - z_i) ]
    g_means[c] = sum over the class and the draws of g_p          g_T[c(, k)] = sum of -g_p e' / t^2

The bound B is DERIVED, nothing in it is fitted; u = 2^-24, every quantity below is an absolute error in units of u.

  * a squared distance is the fp32 chain acc = fmaf(d, d, acc), d = fl(a_k - b_k): the rounding of d moves d^2 by 2 d^2, each of
    the K accumulations rounds a partial sum that is at most the whole: E = (K + 2) |a - b|^2, whatever the order of the k.
  * an imq term q = fl(C / fl(C + d2)): the sum t carries E + t, the quotient one more: Rv = q (E / t + 2).
    an rbf term q = exp2(fl(c d2)), c = fl(-log2(e) / (2 h)): the exponent x = d2 / (2 h) carries 2 x + E / (2 h) in natural
    units, the hardware exponential (v_exp_f32, 1 ulp = 2 u) is given 3: Rv = q (2 x + E / (2 h) + 3) + TINY, TINY for a result
    so small that it is flushed to zero.
  * the S terms are added in fp32: RK = sum_s Rv_s + (S - 1) sum_s q_s.
  * the sums over the pairs of a row, the pieces and the draws are fp64 chains: 2^-29 u per addend (U64), (N + L + 40) addends
    and scalings counted for each; the output is rounded once: + |m_i|.
  * a derivative term: imq k' = -fl(q / t): R' = |k'| (2 E / t + 4); rbf k' = fl(q fl(-1 / (2 h))): R' = Rv / (2 h) + 2 |k'|;
    their fp32 sum: RK' = sum_s R'_s + (S - 1) sum_s |k'_s|.
  * a pair weight w = fl(coefficient x k'): the coefficient fl(fl(g_i + g_j) c) or fl(g_i c) with c a rounded constant carries
    at most 3, the product one more: dW = |coef| RK' + 4 |coef| |k'| + TINY.
  * a gradient is the fp64 chain acc = fma(w, a_k - b_k, acc) with the difference exact in fp64: sum_j dW |a_k - b_k|, U64 (2 N +
    L + 40) times the sum of |w| |a_k - b_k|, and - for g_z - the one rounding of the output.  g_p stays in fp64 up to the class
    sums, which are fp64 chains of fp64 operands rounded once: the sum of the g_p bounds (times |e' / t^2| for the factor) + U64
    n_c times the sum of the magnitudes + |output|.

This is the closed bound for every output (the 4 x torch-fp32 fallback was not needed at the level of the op)."""
import collections
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
U64 = 2.0 ** -29              # the unit roundoff of fp64 in units of u
TINY = 2.0 ** -100
WAE_SCALES = (.1, .2, .5, 1., 2., 5., 10.)

Case = collections.namedtuple('Case', 'name K L N C classes var kind scales joint stress')


def _c(name, K, L, N, C=1, classes='rand', var='scalar', kind='imq', scales=None, joint=True, stress=None):
    return Case(name, K, L, N, C, classes, var, kind, scales, joint, stress)


ONE = 'one'                    # one scale: 1.5 K
EIGHT = 'eight'                # eight scales: K s for s in (.05, .1, .2, .5, 1, 2, 5, 10)

# classes: 'rand' every class drawn; 'es' (C = 3): class 1 is empty, class 2 has one member (the last sample), the rest class 0;
# 'own' every sample its own class (C = N): all within sums are 0.
SHAPE_CASES = [
    _c('K1_L1_N1_C1', 1, 1, 1),
    _c('K3_L3_N2_C1_diag_rbf', 3, 3, 2, var='diag', kind='rbf'),
    _c('K64_L1_N63_C3_es', 64, 1, 63, C=3, classes='es'),
    _c('K65_L3_N64_C3_diag_rbf8', 65, 3, 64, C=3, var='diag', kind='rbf', scales=EIGHT),
    _c('K200_L1_N65_C1_one', 200, 1, 65, scales=ONE),
    _c('K64_L1_N257_C3_es_diag', 64, 1, 257, C=3, classes='es', var='diag'),
    _c('K3_L3_N257_C1_rbf_one', 3, 3, 257, kind='rbf', scales=ONE),
    _c('K65_L1_N65_C3_diag_mixtures', 65, 1, 65, C=3, var='diag', joint=False),
    _c('K1_L3_N64_C3_imq8', 1, 3, 64, C=3, scales=EIGHT),
    _c('K3_L1_N5_own', 3, 1, 5, C=5, classes='own', var='diag'),
    _c('K64_L3_N65_C3_rbf_mixtures', 64, 3, 65, C=3, kind='rbf', joint=False),
]
# far: codes 10^4 apart - every rbf term between two rows underflows to 0, everything stays finite; coincident: rows 0 and 1 of z
# are the same point (and carry the same label); p_eq_z: the draws of the prior ARE the codes, element by element
STRESS_CASES = [
    _c('far_K16_L3_N65_C3_rbf', 16, 3, 65, C=3, kind='rbf', stress='far'),
    _c('coincident_K16_L1_N33_C1', 16, 1, 33, stress='coincident'),
    _c('p_eq_z_K16_L3_N33_C3_diag', 16, 3, 33, C=3, var='diag', stress='p_eq_z'),
]
CASES = SHAPE_CASES + STRESS_CASES
ids = lambda c: c.name      # noqa: E731


def scales_of(c):
    """The absolute scales of a case, as ops.mmd_objective reads them (None: 2 K s for WAE's seven s)."""
    if c.scales is None:
        return tuple(2. * c.K * s for s in WAE_SCALES)
    if c.scales == ONE:
        return (1.5 * c.K,)
    if c.scales == EIGHT:
        return tuple(c.K * s for s in (.05, .1, .2, .5, 1., 2., 5., 10.))
    return tuple(float(s) for s in c.scales)


def kernel_of(c):
    """The `kernel` argument of ops.mmd_objective for a case."""
    return (c.kind, None if c.scales is None else scales_of(c))


def prior_draws32(y, means, T, eps_p, C):
    """p in fp32, operation by operation: means[y] + eps_p / T[y] (a bad label: the row of class 0, never read into a sum)."""
    yc = y.clamp(0, C - 1)
    t = T[yc]
    if t.dim() == 1:
        t = t.unsqueeze(-1)
    return means[yc] + eps_p / t


def make(c, seed=0):
    """The fp32 operands of a case, on the CPU: z (L+1,N,K), eps_p (L,N,K), y, means, T, g (N,) and p (L,N,K) = prior_draws32."""
    gen = torch.Generator().manual_seed(4100 + seed + sum(map(ord, c.name)))

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float32)

    def ru(lo, hi, *s):
        return lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float32)
    K, L, N, C = c.K, c.L, c.N, c.C
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
        T[:, ::2] *= -1                                       # the sign of a factor is free
    eps_p = rn(L, N, K)
    p = prior_draws32(y, means, T, eps_p, C)
    mu = means[y] + 0.5 * rn(N, K)
    z = torch.cat([mu.unsqueeze(0), mu + 0.8 * rn(L, N, K)])
    if c.stress == 'far':
        z = z + 1e4 * torch.arange(N, dtype=torch.float32).view(1, N, 1)
    elif c.stress == 'coincident':
        z[:, 1] = z[:, 0]
        y[1] = y[0]
    elif c.stress == 'p_eq_z':
        z[1:] = p
    return dict(z=z, eps_p=eps_p, y=y, means=means, T=T, g=ru(-1., 1., N), p=p)


def sets(c, d):
    """-> (mask (N, N) bool: j in S_i, ok (N,) bool: the label is in range)."""
    y = d['y']
    ok = (y >= 0) & (y < c.C)
    both = ok.view(-1, 1) & ok.view(1, -1)
    mask = both & (y.view(-1, 1) == y.view(1, -1)) if c.joint else both
    return mask, ok


def kernel_value(c, d2):
    """k as a function of the squared distance, any shape."""
    if c.kind == 'imq':
        return sum(s / (s + d2) for s in scales_of(c))
    return sum(torch.exp(-d2 / (2. * s)) for s in scales_of(c))


def kernel_slope(c, d2):
    """k' = d k / d d2."""
    if c.kind == 'imq':
        return sum(-s / (s + d2) ** 2 for s in scales_of(c))
    return sum(-torch.exp(-d2 / (2. * s)) / (2. * s) for s in scales_of(c))


def sqdist(a, b):
    """(L, N, K), (L, N, K) -> (L, N, N) direct squared distances."""
    return ((a.unsqueeze(2) - b.unsqueeze(1)) ** 2).sum(-1)


def draws64(c, d, leaves=None):
    """p in fp64: the fp32 values d['p'] as given; with autograd leaves (means, T) the SAME values, with the derivative of
    means[y] + eps_p / T[y] attached (the expression minus its own detached value adds exactly 0)."""
    p = d['p'].to(F64)
    if leaves is None or not ({'means', 'T'} & set(leaves)):
        return p
    means = leaves.get('means', d['means'].to(F64))
    T = leaves.get('T', d['T'].to(F64))
    expr = prior_draws32(d['y'], means, T, d['eps_p'].to(F64), c.C)
    return p + (expr - expr.detach())


def rows(c, d, leaves=None, within=None, diagonal=False, labels=True):
    """m (N,) in fp64 (in the precision and on the device of the leaves, where they are given), differentiable in the leaves; NaN
    for a label out of range.  within / diagonal / labels are the knobs of
    the WRONG references of tests/test_mmd_restatement.py: another divisor of the within sums, the diagonal pair kept, the label
    factor dropped."""
    leaves = leaves or {}
    z = leaves.get('z', d['z'].to(F64) if 'z' in d else None)[1:]
    p = leaves['p'] if 'p' in leaves else draws64(c, d, leaves)          # 'p': the draws themselves, in the caller's precision
    mask, ok = sets(c if labels else c._replace(joint=False), d)
    N = c.N
    off = mask if diagonal else mask & ~torch.eye(N, dtype=torch.bool, device=mask.device)
    div = (N - 1 if within is None else within)
    inv = 1. / div if div > 0 else 0.
    kzz, kpp, kzp = (kernel_value(c, sqdist(a, b)) for a, b in ((z, z), (p, p), (z, p)))
    m = ((kzz * off).sum(2) * inv + (kpp * off).sum(2) * inv - (2. / N) * (kzp * mask).sum(2)).mean(0)
    return torch.where(ok, m, torch.full_like(m, math.nan))


def _weighted(W, a, b):
    """sum_j W[l,i,j] (a[l,i] - b[l,j]) -> (L, N, K)."""
    return W.sum(2, keepdim=True) * a - torch.bmm(W, b)


def ref(c, d):
    """Every output of forward and backward (the direct partial derivatives, written out by hand) in fp64."""
    K, L, N = c.K, c.L, c.N
    mask, ok = sets(c, d)
    off = (mask & ~torch.eye(N, dtype=torch.bool)).to(F64)
    maskf = mask.to(F64)
    z = d['z'].to(F64)[1:]
    p = d['p'].to(F64)
    g = torch.where(ok, d['g'].to(F64), torch.zeros(N, dtype=F64))
    out = dict(m=rows(c, d))
    cw = ((g.view(-1, 1) + g.view(1, -1)) * (2. / ((N - 1) * L)) if N > 1 else torch.zeros(N, N, dtype=F64)) * off
    cc = (g * (-4. / (N * L))).view(-1, 1) * maskf                                    # [i, j]: the pair (z_i, p_j)
    szz, spp, szp = (kernel_slope(c, sqdist(a, b)) for a, b in ((z, z), (p, p), (z, p)))
    g_z = torch.zeros(L + 1, N, K, dtype=F64)
    g_z[1:] = _weighted(cw * szz, z, z) + _weighted(cc * szp, z, p)
    g_p = _weighted(cw * spp, p, p) + _weighted((cc * szp).transpose(1, 2), p, z)
    bad = ~ok
    g_z[1:, bad] = math.nan
    g_p[:, bad] = 0.
    onehot = (d['y'].view(-1, 1) == torch.arange(c.C).view(1, -1)).to(F64)              # (N, C): a bad label adds to no class
    t = d['T'].to(F64)[d['y'].clamp(0, c.C - 1)]
    t = t.unsqueeze(-1).expand(N, K) if c.var == 'scalar' else t
    gT = (-g_p * d['eps_p'].to(F64) / (t * t)).sum(0)                                   # (N, K)
    out.update(g_z=g_z, g_means=onehot.T @ g_p.sum(0), g_T=onehot.T @ (gT if c.var == 'diag' else gT.sum(-1)))
    out['g_p'] = g_p
    return out


def autograd_ref(c, d):
    """The same gradients from torch.autograd in fp64 on the restatement's own forward: sum_i g_i m_i."""
    names = ['z', 'means', 'T']
    leaves = {k: d[k].to(F64).clone().requires_grad_(True) for k in names}
    _, ok = sets(c, d)
    m = rows(c, d, leaves)
    if not bool(ok.any()) or not m.requires_grad:
        return {'g_' + k: torch.zeros_like(leaves[k]) for k in names}
    grads = torch.autograd.grad((d['g'].to(F64) * m)[ok].sum(), [leaves[k] for k in names], allow_unused=True)
    return {'g_' + k: (torch.zeros_like(leaves[k]) if v is None else v) for k, v in zip(names, grads)}


def _pair_bounds(c, d2):
    """d2 (L, N, N) exact -> (RK, |k'|, RK'): the error bounds of a pair's kernel value and slope, and the slope's magnitude."""
    E = (c.K + 2) * d2
    S = len(scales_of(c))
    rv = torch.zeros_like(d2)
    v = torch.zeros_like(d2)
    rs = torch.zeros_like(d2)
    sl = torch.zeros_like(d2)
    for s in scales_of(c):
        if c.kind == 'imq':
            t = s + d2
            q = s / t
            kp = q / t
            rv += q * (E / t + 2)
            rs += kp * (2 * E / t + 4)
        else:
            x = d2 / (2. * s)
            q = torch.exp(-x)
            kp = q / (2. * s)
            r = q * (2 * x + E / (2. * s) + 3) + TINY
            rv += r
            rs += r / (2. * s) + 2 * kp
        v += q
        sl += kp
    return rv + (S - 1) * v, sl, rs + (S - 1) * sl


def bounds(c, d, r):
    """B for every output of ref(c, d): |fp32 kernel - fp64 restatement| <= u B, element by element."""
    K, L, N = c.K, c.L, c.N
    mask, ok = sets(c, d)
    off = (mask & ~torch.eye(N, dtype=torch.bool)).to(F64)
    maskf = mask.to(F64)
    z = d['z'].to(F64)[1:]
    p = d['p'].to(F64)
    g = torch.where(ok, d['g'].to(F64), torch.zeros(N, dtype=F64)).abs()
    gpair = torch.where(ok, d['g'].to(F64), torch.zeros(N, dtype=F64))
    fin = lambda x: x.nan_to_num(0.)                                                # noqa: E731  (a bad sample: NaN on both sides)
    blocks = {'zz': (z, z), 'pp': (p, p), 'zp': (z, p)}
    pb = {k: _pair_bounds(c, sqdist(a, b)) for k, (a, b) in blocks.items()}
    kv = {k: kernel_value(c, sqdist(a, b)) for k, (a, b) in blocks.items()}
    inv = 1. / (N - 1) if N > 1 else 0.
    err = ((pb['zz'][0] * off).sum(2) * inv + (pb['pp'][0] * off).sum(2) * inv + (2. / N) * (pb['zp'][0] * maskf).sum(2)).mean(0)
    mag = ((kv['zz'] * off).sum(2) * inv + (kv['pp'] * off).sum(2) * inv + (2. / N) * (kv['zp'] * maskf).sum(2)).mean(0)
    out = {'m': err + U64 * (N + L + 40) * mag + fin(r['m']).abs()}
    # ---- the pair weights of the backward: (magnitude, error bound), each (L, N, N)
    cw = ((gpair.view(-1, 1) + gpair.view(1, -1)).abs() * (2. / ((N - 1) * L)) if N > 1 else torch.zeros(N, N, dtype=F64)) * off
    cc = (g * (4. / (N * L))).view(-1, 1) * maskf

    def weight(coef, key):
        _, sl, rs = pb[key]
        return coef * sl, coef * rs + 4 * coef * sl + TINY * (coef > 0)
    wzz, dzz = weight(cw, 'zz')
    wpp, dpp = weight(cw, 'pp')
    wzp, dzp = weight(cc, 'zp')

    def chain(Wm, Wd, a, b):
        """sum_j (Wd + U64 n Wm)[l,i,j] |a[l,i,k] - b[l,j,k]| -> (L, N, K), a draw at a time."""
        n = 2 * N + L + 40
        res = torch.zeros(L, N, K, dtype=F64)
        for l in range(L):
            diff = (a[l].unsqueeze(1) - b[l].unsqueeze(0)).abs()                   # (N, N, K)
            res[l] = torch.einsum('ij,ijk->ik', Wd[l] + U64 * n * Wm[l], diff)
        return res
    B_gz = torch.zeros(L + 1, N, K, dtype=F64)
    B_gz[1:] = chain(wzz, dzz, z, z) + chain(wzp, dzp, z, p) + fin(r['g_z'][1:]).abs()
    out['g_z'] = B_gz
    B_gp = chain(wpp, dpp, p, p) + chain(wzp.transpose(1, 2), dzp.transpose(1, 2), p, z)      # no rounding of its own: fp64
    B_gp[:, ~ok] = 0.
    onehot = (d['y'].view(-1, 1) == torch.arange(c.C).view(1, -1)).to(F64)
    n_c = L + 8 + (-(-N // 16) + 16) + K
    gp = r['g_p'].abs()
    out['g_means'] = onehot.T @ (B_gp + U64 * n_c * gp).sum(0) + r['g_means'].abs()
    t = d['T'].to(F64)[d['y'].clamp(0, c.C - 1)]
    t = t.unsqueeze(-1).expand(N, K) if c.var == 'scalar' else t
    fac = (d['eps_p'].to(F64) / (t * t)).abs()
    bT = ((B_gp + U64 * (n_c + 8) * gp) * fac).sum(0)
    out['g_T'] = onehot.T @ (bT if c.var == 'diag' else bT.sum(-1)) + r['g_T'].abs()
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


# ---- what TRAIN_OBJECTIVE = 'mmd' refuses at the first training-mode evaluate: the rows of iwae_cases.refusal_table() about the
# model and the step (the same models, the same words) - without the kl_var_weighting row, which this objective allows because
# the KL keeps its own path - and the semi-supervised switch
def refusal_table():
    import iwae_cases
    table = [row for row in iwae_cases.refusal_table() if row[0] != 'kl_var_weighting']
    base = table[-1][1]
    return table + [('semi_supervised', base, lambda m: setattr(m, 'SEMI_SUPERVISED', True), {}, 'SEMI_SUPERVISED')]


def refusal_model(kwargs, tweak, device=None):
    from cvae import ClassificationVariationalNetwork as Net
    m = Net(**kwargs)
    if device is not None:
        m.to(device)
    if tweak is not None:
        tweak(m)
    m.TRAIN_OBJECTIVE = 'mmd'
    m.train()
    return m
