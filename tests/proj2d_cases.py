"""Inputs and the numpy fp64 restatement shared by tests/test_proj2d_restatement.py (CPU), tests/test_25_proj2d_gpu.py and
tools/gen_proj2d_golden.py: what csrc/embed.hip computes, written the way scikit-learn 1.7 computes it (manifold/_utils.pyx
::_binary_search_perplexity, manifold/_t_sne.py::_joint_probabilities, _kl_divergence, _gradient_descent;
decomposition.PCA), without importing scikit-learn."""
import os

import numpy as np

EPS = 2.220446049250313e-16               # MACHINE_EPSILON of _t_sne.py
TOL = float(np.float32(1e-5))             # PERPLEXITY_TOLERANCE of _utils.pyx is a C float
S_FLOOR = float(np.float32(1e-8))         # EPSILON_DBL of _utils.pyx is a C float as well
KNIFE_EDGE = 1e-9                         # a search step whose |H - log perplexity| is this close to TOL could stop either way

# (N, K, perplexity) of the fixtures in tests/golden/proj2d, and the seed of each
CASES = {(5, 3, 2): 1, (64, 16, 10): 1, (65, 1, 10): 1, (130, 37, 30): 1, (300, 16, 30): 1}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'proj2d')


def case_file(N, K, perplexity):
    return os.path.join(GOLDEN, f'case_{N}_{K}_{perplexity}.npz')


def blobs(N, K, seed):
    """Three Gaussian blobs: centres 6 N(0, I), unit noise, from default_rng(seed) -> (x (N, K) fp32, the blob of each row)."""
    rng = np.random.default_rng(seed)
    centres = 6. * rng.standard_normal((3, K))
    label = np.arange(N) * 3 // N
    return (centres[label] + rng.standard_normal((N, K))).astype(np.float32), label


def sqdist(x):
    """d_ij = fp32(sum_k (double(x_ik) - double(x_jk))^2), k ascending, every operation rounded on its own."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    acc = np.zeros((len(x), len(x)))
    for k in range(x.shape[1]):
        t = x[:, None, k] - x[None, :, k]
        acc = acc + t * t
    return acc.astype(np.float32)


def search(d, perplexity):
    """_binary_search_perplexity on a square fp32 matrix -> (conditional P (N, N) fp64, beta (N,), S (N,), margin): margin is the
    smallest ||H - log perplexity| - TOL| over every step of every row."""
    d = np.asarray(d, dtype=np.float32)
    N = len(d)
    want = np.log(float(np.float32(perplexity)))
    P, betas, sums, margin = np.zeros((N, N)), np.zeros(N), np.zeros(N), np.inf
    for i in range(N):
        keep = np.arange(N) != i
        di = d[i, keep]
        dd = di.astype(np.float64)
        beta, bmin, bmax = 1., -np.inf, np.inf
        for _ in range(100):
            p = np.exp((-di).astype(np.float64) * beta)
            S = p.sum()
            if S == 0.:
                S = S_FLOOR
            p = p / S
            diff = np.log(S) + beta * (dd * p).sum() - want
            margin = min(margin, abs(abs(diff) - TOL))
            used = beta
            if abs(diff) <= TOL:
                break
            if diff > 0.:
                bmin = beta
                beta = beta * 2. if bmax == np.inf else (beta + bmax) / 2.
            else:
                bmax = beta
                beta = beta / 2. if bmin == -np.inf else (beta + bmin) / 2.
        P[i, keep], betas[i], sums[i] = p, used, S
    return P, betas, sums, margin


def entropies(d, betas):
    """H_i = log S_i + beta_i sum_j d_ij p_j / S_i of the conditional distributions at the given precisions."""
    d = np.asarray(d, dtype=np.float64)
    out = np.zeros(len(d))
    for i in range(len(d)):
        di = np.delete(d[i], i)
        p = np.exp(-di * betas[i])
        S = p.sum()
        out[i] = np.log(S) + betas[i] * (di * p).sum() / S
    return out


def joint(cond):
    """_joint_probabilities' last three lines on the full matrix (the diagonal, which the condensed form leaves out, is floored
    like every entry)."""
    P = cond + cond.T
    return np.maximum(P / np.maximum(P.sum(), EPS), EPS)


def condensed(full):
    """The upper triangle in scipy's squareform order."""
    return full[np.triu_indices(len(full), 1)]


def expand(cond_form, N):
    """squareform of a condensed vector (zero diagonal)."""
    full = np.zeros((N, N), dtype=cond_form.dtype)
    iu = np.triu_indices(N, 1)
    full[iu] = cond_form
    return full + full.T


def kl_and_gradient(P, y, f=1.):
    """_kl_divergence(y, f P) for a full symmetric P (its diagonal is not read) and y (N, 2) fp32 -> (kl, grad (N, 2) fp32,
    abs-sum (N, 2) of the terms of the gradient's sum, |grad|_2): fp64 arithmetic on the widened values, one rounding; the
    factor y_i - y_j of the gradient is the fp32 difference, as there."""
    y32 = np.asarray(y, dtype=np.float32)
    y = y32.astype(np.float64)
    N = len(y)
    off = ~np.eye(N, dtype=bool)
    fP = f * np.asarray(P, dtype=np.float64)
    diff = y[:, None, :] - y[None, :, :]
    qn = 1. / (1. + (diff ** 2).sum(-1))
    diff = (y32[:, None, :] - y32[None, :, :]).astype(np.float64)      # `X_embedded[i] - X_embedded`: an fp32 difference
    Q = np.maximum(qn / qn[off].sum(), EPS)
    kl = float((fP[off] * np.log(np.maximum(fP[off], EPS) / Q[off])).sum())
    w = np.where(off, (fP - Q) * qn, 0.)
    grad = (4. * (w[:, :, None] * diff).sum(1)).astype(np.float32)
    terms = np.where(off, (np.abs(fP) + Q) * qn, 0.)[:, :, None] * np.abs(diff)
    return kl, grad, terms.sum(1), float(np.linalg.norm(grad.astype(np.float64)))


def update(y, upd, gains, g, momentum, lr):
    """One step of _gradient_descent on fp32 arrays, as numpy executes it -> the new (y, update, gains, g)."""
    y, upd, gains, g = (np.array(a, dtype=np.float32) for a in (y, upd, gains, g))
    inc = upd * g < 0.0
    dec = np.invert(inc)
    gains[inc] += 0.2
    gains[dec] *= 0.8
    np.clip(gains, 0.01, np.inf, out=gains)
    g *= gains
    upd = momentum * upd - lr * g
    y += upd
    assert all(a.dtype == np.float32 for a in (y, upd, gains, g))
    return y, upd, gains, g


def covariance(x):
    """fp64 means and centred covariance / (N - 1), and sum |terms| / (N - 1) for the error bar."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    mean = x.mean(0)
    c = x - mean
    return mean, c.T @ c / (len(x) - 1), np.abs(c).T @ np.abs(c) / (len(x) - 1)


def nearest_neighbour_purity(emb, label):
    """The fraction of points whose nearest embedded neighbour has their label."""
    e = np.asarray(emb, dtype=np.float64)
    d = ((e[:, None, :] - e[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((label[d.argmin(1)] == label).mean())


def case257(K=16, perplexity=30.):
    """The N = 257 input of the GPU tests: the first seed whose search keeps KNIFE_EDGE away from its stopping rule ->
    (x, d, conditional P, beta, S)."""
    for seed in range(1, 20):
        x, _ = blobs(257, K, seed)
        d = sqdist(x)
        cond, beta, S, margin = search(d, perplexity)
        if margin > KNIFE_EDGE:
            return x, d, cond, beta, S
    raise AssertionError('no seed without a knife edge')
