"""The importance-weighted bound of csrc/iwae.hip restated in torch (fp64 by default), its hand-written direct gradients, the
case table and the per-output error bound B(case) that the GPU tests hold the kernels to: |error| <= 2^-24 B on every element.

Forward, for sample n of class y and the draws l = 1..L (row 0 of z takes no part):

    log w_l = -D/2 (wmse_s[l,n] + 2 log sigma + log 2pi) + beta (1/2 (q_l - dist_l) + slog)
    dist_l = sum_k (t_k (z_lk - m_k))^2,   q_l = sum_k (eps_lk^2 + lv_k),   slog = sum_k log|t_k|   (the K/2 log 2pi of log p(z|y)
    and of log q(z|x) cancel)
    bound = logsumexp_l(log w_l) - log L,   wt = softmax_l(log w_l),   ess = 1 / sum_l wt_l^2

The bound B is DERIVED, nothing in it is fitted: every sum contributes (sum of the absolute values of its addends) x (number of
roundings an addend can meet on its way: the additions of the kernel's summation tree plus the roundings of forming the addend),
and the logsumexp contributes its own terms.  `bounds()` spells each count out.  u = 2^-24 is the unit roundoff of fp32; the
device's expf is taken as good to 2 u (its documented error is 1 ulp).  The kernel forms log w in fp64 (unit roundoff 2^-53 =
2^-29 u: its roundings enter B with that weight) and parks fp32(log w - max); the fold of the parked values, the weights and
every result are fp32.  The backward's product chains and class sums run in fp64 and are rounded once; their part of B counts
them as if each step were an fp32 rounding - an upper bound of what the fp64 chains can do, with the weight's own error in it.
"""
import collections
import math

import torch

F64 = torch.float64
U = 2.0 ** -24
LOG2PI = math.log(2 * math.pi)
SIG_VALUE, SIG_LOG, SIG_CODED, SIG_RMSE = 0, 1, 2, 3
TINY = 2.0 ** -100            # u * TINY is above the smallest normal fp32: covers results flushed to zero below it

Case = collections.namedtuple('Case', 'name K L N C classes var sig beta D stress')


def _c(name, K, L, N, C=3, classes='rand', var='scalar', sig=SIG_VALUE, beta=1., D=3072, stress=None):
    return Case(name, K, L, N, C, classes, var, sig, beta, D, stress)


# classes: 'rand' every class drawn; 'empty1' class 1 of C = 3 has no sample; 'one' all samples in class C - 1
SHAPE_CASES = [
    _c('K1_L1_N1_C1', 1, 1, 1, C=1),                                                 # the non-conditional layout, smallest of all
    _c('K3_L2_N3_diag_empty1', 3, 2, 3, classes='empty1', var='diag', sig=SIG_LOG),
    _c('K63_L5_N3_coded_b025', 63, 5, 3, sig=SIG_CODED, beta=0.25),
    _c('K64_L64_N3_diag_D1', 64, 64, 3, var='diag', D=1),
    _c('K65_L65_N1_one', 65, 65, 1, classes='one', sig=SIG_LOG),
    _c('K200_L5_N257_diag_coded', 200, 5, 257, var='diag', sig=SIG_CODED),          # 5 sample chunks of 17 and 15 short ones
    _c('K16_L257_N3_b025', 16, 257, 3, beta=0.25),                                   # a thread folds more than one draw
    _c('K64_L1_N257_C1_diag', 64, 1, 257, C=1, var='diag', D=1),
    _c('K3_L64_N257_one_log', 3, 64, 257, classes='one', sig=SIG_LOG),
    _c('K65_L2_N3_empty1_D1_b025', 65, 2, 3, classes='empty1', D=1, beta=0.25),
    _c('K1_L65_N3_diag', 1, 65, 3, var='diag'),
    _c('K200_L64_N1_C1_coded', 200, 64, 1, C=1, sig=SIG_CODED),
]
# stress rows: 'lead' one draw ahead of the others by 10^4; 'equal' all draws of a sample equal; 'deep' log w near -10^5;
# 'huge' a wmse_s of 10^30 (sample 0: one draw; sample 1: every draw)
STRESS_CASES = [
    _c('lead_K16_L5_N3', 16, 5, 3, stress='lead'),
    _c('equal_K16_L5_N3_diag', 16, 5, 3, var='diag', stress='equal'),
    _c('deep_K64_L64_N3', 64, 64, 3, stress='deep'),
    _c('huge_K16_L5_N3', 16, 5, 3, stress='huge'),
]
CASES = SHAPE_CASES + STRESS_CASES
ids = lambda c: c.name      # noqa: E731


def make(c, seed=0):
    """The fp32 operands of a case, on the CPU: wmse_s (L,N), z (L+1,N,K), lv (N,K), eps (L,N,K), y, means, T, sigma, g (N,)."""
    gen = torch.Generator().manual_seed(1000 + seed + sum(map(ord, c.name)))

    def rn(*s):
        return torch.randn(*s, generator=gen, dtype=torch.float32)

    def ru(lo, hi, *s):
        return lo + (hi - lo) * torch.rand(*s, generator=gen, dtype=torch.float32)
    K, L, N, C = c.K, c.L, c.N, c.C
    mu, lv, eps = rn(N, K), ru(-2., 1., N, K), rn(L, N, K)
    if c.stress == 'equal':
        eps = eps[:1].expand(L, N, K).contiguous()
    z = torch.cat([mu.unsqueeze(0), mu + (0.5 * lv).exp() * eps])
    if c.classes == 'one':
        y = torch.full((N,), C - 1, dtype=torch.int64)
    elif c.classes == 'empty1':
        y = 2 * torch.randint(0, 2, (N,), generator=gen, dtype=torch.int64)
    else:
        y = torch.randint(0, C, (N,), generator=gen, dtype=torch.int64)
    means = rn(C, K)
    T = ru(0.8, 1.2, C, K) if c.var == 'diag' else ru(0.8, 1.2, C)
    if c.var == 'diag':
        T[:, ::2] *= -1                                       # log|t|: the sign of a factor is free, diagonal ...
    else:
        T[::2] *= -1                                          # ... or scalar
    wmse_s = ru(0.5, 1.5, L, N)
    if c.stress == 'equal':
        wmse_s = wmse_s[:1].expand(L, N).contiguous()
    elif c.stress == 'lead':                                  # D/2 x 7 = 10752 > 10^4 ahead of the others
        wmse_s = ru(8., 8.1, L, N)
        wmse_s[L // 2] = 1.
    elif c.stress == 'deep':                                  # -D/2 (60 + 1.8) = -9.5 x 10^4
        wmse_s = ru(60., 61., L, N)
    elif c.stress == 'huge':
        wmse_s[1, 0] = 1e30
        wmse_s[:, 1] = 1e30
    sigma = {SIG_VALUE: torch.tensor([0.7]), SIG_LOG: torch.tensor([math.log(0.7)]), SIG_CODED: ru(-0.5, 0.3, N)}[c.sig]
    return dict(wmse_s=wmse_s, z=z, lv=lv, eps=eps, y=y, means=means, T=T, sigma=sigma, g=ru(-1., 1., N))


def log_w(c, d, dt=F64, leaves=None):
    """(L, N) log w, differentiable in the operands; leaves: operands already converted (the autograd check's own leaves)."""
    v = {k: (d[k] if k == 'y' else d[k].to(dt)) for k in d}
    v.update(leaves or {})
    y = v['y']
    m = v['means'][y]
    t = v['T'][y] if c.var == 'diag' else v['T'][y].unsqueeze(-1)
    dist = (t * (v['z'][1:] - m)).pow(2).sum(-1)
    slog = t.abs().log().sum(-1) if c.var == 'diag' else c.K * t.squeeze(-1).abs().log()
    q = (v['eps'].pow(2) + v['lv']).sum(-1)
    ls = v['sigma'].log() if c.sig == SIG_VALUE else v['sigma']
    a = -0.5 * c.D * (v['wmse_s'] + 2 * ls + LOG2PI)
    return a + c.beta * (0.5 * (q - dist) + slog)


def fold(lw):
    """log w (L, N) -> bound, wt, ess."""
    L = lw.shape[0]
    # the shifted sum written out: torch.logsumexp's backward is exp(x - result), which loses log L where |x| is so large that
    # x + log L rounds to x (the 10^30 rows); the gradient of this form is the softmax itself
    top = lw.detach().max(0).values
    bound = top + (lw - top).exp().sum(0).log() - math.log(L)
    wt = torch.softmax(lw, 0)
    return bound, wt, 1 / wt.pow(2).sum(0)


def ref(c, d, dt=F64):
    """Every output of forward and backward (the direct partial derivatives, written out by hand) in `dt`."""
    lw = log_w(c, d, dt)
    bound, wt, ess = fold(lw)
    g, y = d['g'].to(dt), d['y']
    z, means, T, sigma = d['z'].to(dt), d['means'].to(dt), d['T'].to(dt), d['sigma'].to(dt)
    t = T[y] if c.var == 'diag' else T[y].unsqueeze(-1).expand(c.N, c.K)
    dz = z[1:] - means[y]                                                        # (L, N, K)
    gw = g * c.beta
    g_z = torch.zeros_like(z)
    g_z[1:] = -(gw.view(1, -1, 1) * wt.unsqueeze(-1)) * (t * t * dz)
    out = dict(bound=bound, wt=wt, ess=ess, g_wmse_s=-g * wt * (0.5 * c.D), g_z=g_z,
               g_lv=(0.5 * gw).view(-1, 1).expand(c.N, c.K).clone())
    onehot = torch.nn.functional.one_hot(y, c.C).to(dt)                          # (N, C)
    out['g_means'] = onehot.T @ (gw.view(-1, 1) * (wt.unsqueeze(-1) * (t * t * dz)).sum(0))
    if c.var == 'diag':
        out['g_T'] = onehot.T @ (gw.view(-1, 1) * (wt.unsqueeze(-1) * (1 / t - t * dz * dz)).sum(0))
    if c.sig == SIG_VALUE:
        out['g_sigma'] = (-g * c.D / sigma).sum().reshape(1)
    elif c.sig == SIG_LOG:
        out['g_sigma'] = (-g * c.D).sum().reshape(1)
    else:
        out['g_sigma'] = -g * c.D
    out['log_w'] = lw
    return out


def autograd_ref(c, d):
    """The same gradients from torch.autograd in fp64 on the restatement's own forward: sum_n g_n bound_n."""
    names = ['wmse_s', 'z', 'lv', 'means', 'sigma'] + (['T'] if c.var == 'diag' else [])
    leaves = {k: d[k].to(F64).clone().requires_grad_(True) for k in names}
    bound, _, _ = fold(log_w(c, d, F64, leaves))
    grads = torch.autograd.grad((d['g'].to(F64) * bound).sum(), [leaves[k] for k in names])
    return {'g_' + k: v for k, v in zip(names, grads)}


def _tree(n, width):
    """Roundings a partial sum meets when n addends are dealt to `width` lanes in turn, each lane adding its own in sequence,
    and the lanes are joined by a butterfly of log2(width) steps."""
    return -(-n // width) + int(math.log2(width))


def n_S(L):
    """Additions a term of S (or Q) meets in the fold: thread t adds its draws t, t + 256, ... in sequence (ceil(L / 256)), the
    wave's butterfly (6), the butterfly over the four wave sums in block_sum (6), and 2 for the zero start and the hand-over."""
    return -(-L // 256) + 6 + 6 + 2


def bounds(c, d, r):
    """B for every output of ref(c, d): |fp32 kernel - fp64 restatement| <= u B, element by element.  r = ref(c, d, F64)."""
    K, L, N, D, beta = c.K, c.L, c.N, c.D, c.beta
    y = d['y']
    v = {k: d[k].to(F64) for k in d if k != 'y'}
    t = v['T'][y] if c.var == 'diag' else v['T'][y].unsqueeze(-1).expand(N, K)
    dz = v['z'][1:] - v['means'][y]
    tk = _tree(K, 64)                                          # a lane's K / 64 addends in sequence, six butterfly steps
    # ---- log w -------------------------------------------------------------------------------------------------------------
    # formed in fp64: every addend meets the roundings of its sum (a lane's K / 64 in sequence, six butterfly steps), at most 4
    # of forming it (the subtraction, the product with t, the square; log 2 u) and 4 more behind the sums (q - dist, + slog,
    # x beta, + a): each of 2^-53 = U64 u.  The addends: a's three, (t (z - m))^2, eps^2 + lv, log|t|.
    U64 = 2.0 ** -29
    ls = v['sigma'].log().abs() if c.sig == SIG_VALUE else v['sigma'].abs()
    A_a = 0.5 * D * (v['wmse_s'].abs() + 2 * ls + LOG2PI)
    A_dist = (t * dz).pow(2).sum(-1)
    A_q = (v['eps'].pow(2) + v['lv'].abs()).sum(-1)
    A_s = (t.abs().log().abs().sum(-1) if c.var == 'diag' else K * t[:, 0].abs().log().abs())
    B_lw = U64 * (tk + 4 + 4) * (A_a + beta * (0.5 * A_dist + 0.5 * A_q + A_s))
    # ---- the fold over the draws -------------------------------------------------------------------------------------------
    lw = r['log_w']
    M, im = lw.max(0)
    B_M = B_lw.gather(0, im.unsqueeze(0))[0]
    # a draw is LIVE when its exponent log w - max can come within 100 of the top under the errors of both: a dead draw's e is
    # below e^-100 = 4e-44 on both sides, whatever its own error, and vanishes in TINY
    live = (lw - M + U * (B_lw + B_M)) >= -100.
    mb = torch.where(live, B_lw, torch.zeros_like(B_lw)).max(0).values           # the largest error bound of a live log w
    nS = n_S(L)
    # e_l = expf(fp32(log w - max)): the parked difference is rounded once (<= 100 u for a live draw), expf 2 u; then the sum
    rel_S = 102 + nS
    S = (lw - M).exp().sum(0)
    out = {}
    # bound = max + logf(S) - log(count): the live draws' errors move the logsumexp by at most their largest (it is a convex
    # mixture); S's relative error is the absolute error of its logarithm; logf twice (2 u each) and two additions
    out['bound'] = mb + rel_S + 2 * (S.log().abs() + math.log(L)) + 2 * (M.abs() + S.log().abs() + math.log(L)) + 1
    # wt_l = e_l / S: e_l moves by its own and the maximum's error, S by twice the largest live error, then e's and S's roundings
    # and the division
    out['wt'] = r['wt'] * (B_lw + B_M + 2 * mb + 102 + rel_S + 1) * live + TINY
    # ess = S^2 / Q: unchanged by a common shift, the draws differ by at most 2 mb -> S by 2 mb, Q by 4 mb; S twice, Q's addends
    # are squares (2 x 102 + 1) and summed like S, one product, one division
    out['ess'] = r['ess'] * (8 * mb + 2 * rel_S + (2 * 102 + 1 + nS) + 2)
    # ---- backward: the kernel reads ITS wt, in error by u out['wt'] ----------------------------------------------------------
    g = v['g'].abs()
    B_wt, wt = out['wt'], r['wt']
    out['g_wmse_s'] = g * 0.5 * D * (B_wt + 3 * wt)
    # g_z = -(g beta) (wt (t^2 (z - m))): subtraction, t^2, three products, g beta: 6
    tt = (t * t * dz).abs()                                                      # (L, N, K)
    gb = (g * beta).view(1, N, 1)
    B_gz = torch.zeros_like(v['z'])
    B_gz[1:] = gb * tt * (B_wt.unsqueeze(-1) + 6 * wt.unsqueeze(-1))
    out['g_z'] = B_gz
    out['g_lv'] = (2 * 0.5 * g * beta).view(N, 1).expand(N, K).clone()
    # class sums: a sample's contribution is a fused sum over its L draws in sequence (addend: 4 roundings + the weight's error),
    # then g beta (2); the samples of a class are summed in sample order inside 16 chunks of ceil(N / 16), the chunks in turn
    n_c = -(-N // 16) + 16
    onehot = torch.nn.functional.one_hot(y, c.C).to(F64)
    per = (gb * tt * (B_wt.unsqueeze(-1) + (L + 4 + 2 + n_c) * wt.unsqueeze(-1))).sum(0)          # (N, K)
    out['g_means'] = onehot.T @ per
    if c.var == 'diag':
        # addend wt (1/t - t d^2): the division, d (1), d^2, t d^2, the difference: 5, + the weight's error
        ad = (1 / t).abs() + t.abs() * dz * dz
        per = (gb * ad * (B_wt.unsqueeze(-1) + (L + 5 + 2 + n_c) * wt.unsqueeze(-1))).sum(0)
        out['g_T'] = onehot.T @ per
    # sigma: -g D [/ sigma] (2 roundings); value / log: block_sum64 - a thread's ceil(N / 256) in sequence, the butterfly (6), the
    # four waves in sequence (3) - and the rounding of the result
    if c.sig == SIG_CODED:
        out['g_sigma'] = 2 * g * D
    else:
        s = v['sigma'].abs() if c.sig == SIG_VALUE else torch.ones(1, dtype=F64)
        out['g_sigma'] = ((g * D / s).sum() * (-(-N // 256) + 6 + 3 + 2 + 1)).reshape(1)
    return out


def excess(got, want, B):
    """max over the elements of |got - want| / (u B); 0 where both the error and B vanish.  Non-finite results: inf."""
    got = got.detach().to('cpu', F64)
    if got.numel() == 0:
        return 0.
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - want).abs()
    B = B.expand_as(err) if B.shape != err.shape else B
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * B))
    return float(ratio.max())


# ---- what TRAIN_OBJECTIVE = 'iwae' refuses at the first training-mode evaluate: (name, how to build the model, evaluate
# keywords, a word of the message).  Every model is the MLP case c1_n16_mlp with one thing changed (the categorical decoder
# needs a conv imager: its own case).
def refusal_table():
    from oracle.cases import get_case
    base = get_case('c1_n16_mlp')['net']
    prior = dict(base['prior'])

    def net(**kw):
        return dict(base, **kw)
    other = dict(distribution='gaussian', init_mean=0., mean_shift=1.5, var_dim='scalar')
    return [
        ('jvae', net(type='jvae', y_is_coded=True, gamma=2., classifier=[20], prior=dict(distribution='gaussian', init_mean=0.)),
         None, {}, "not 'jvae'"),
        ('vib', net(type='vib', gamma=2., classifier=[20], prior=dict(distribution='gaussian', init_mean=0.)), None, {}, "not 'vib'"),
        ('coded_labels', net(y_is_coded=True), None, {}, 'coded labels'),
        ('categorical', get_case('g2_n4_categorical')['net'], None, {}, 'categorical'),
        ('rmse_sigma', net(sigma={'is_rmse': True}), None, {}, 'rmse'),
        ('tilted', net(prior=dict(prior, distribution='tilted', tau=5.)), None, {}, 'tilted'),
        ('uniform', net(prior=dict(prior, distribution='uniform', tau=3.)), None, {}, 'uniform'),
        ('full_variance', net(prior=dict(prior, var_dim='full')), None, {}, 'full'),
        ('mixed_encode', net(), lambda m: setattr(m.encoder, 'mixed_prior', (_build_prior(other, m.latent_dim), 4)), {}, 'mixed'),
        ('bf16', net(), lambda m: m.set_compute_dtype('bf16'), {}, 'bf16'),
        ('kl_var_weighting', net(), None, dict(kl_var_weighting=0.5), 'kl_var_weighting'),
        ('world', net(), lambda m: setattr(m.optimizer, '_world', 2), {}, '_world'),
        ('train_captured', net(), lambda m: setattr(m, 'TRAIN_CAPTURED', True), {}, 'TRAIN_CAPTURED'),
    ]


def _build_prior(params, dim):
    from module.priors import build_prior
    return build_prior(dim=dim, **params)


def refusal_model(kwargs, tweak, device=None):
    """The model of one row of refusal_table() in training mode with the importance-weighted objective switched on."""
    from cvae import ClassificationVariationalNetwork as Net
    m = Net(**kwargs)
    if device is not None:
        m.to(device)
    if tweak is not None:
        tweak(m)
    m.TRAIN_OBJECTIVE = 'iwae'
    m.train()
    return m
