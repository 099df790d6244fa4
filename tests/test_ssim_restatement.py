"""The SSIM of csrc/ssim.hip restated in fp64 numpy, held to an independent anchor - scipy's
gaussian_filter, which is what scikit-image's structural_similarity(gaussian_weights=True) calls - to a window worked by hand and
to its identities; and the kernel's error bound as a function, which tests/test_32_ssim_gpu.py asserts.  No GPU."""
import numpy as np
import pytest

from test_ic_restatement import checkerboard, constant, smooth_noise, uniform_noise

WIN, HALO, SIGMA = 11, 10, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
U = 2. ** -24                      # the unit roundoff of fp32
# the rounded operations of the kernel, in its own order, per map pixel - 327.6 in first order, and 1 %
# on B^2 for the fp32 rounding of the centring constant
BOUND_C = 340.


def taps():
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-k * k / (2. * SIGMA * SIGMA))
    return g / g.sum()


def valid_filter(p):
    """g applied separably over the valid region of the last two axes: (..., H, W) -> (..., H - 10, W - 10), fp64."""
    g = taps()
    H, W = p.shape[-2:]
    rows = sum(g[k] * p[..., :, k:k + W - HALO] for k in range(WIN))
    return sum(g[k] * rows[..., k:k + H - HALO, :] for k in range(WIN))


def ssim_planes(x, y, a=None):
    """x (..., H, W), y of the same shape -> (map, cs map, B) per plane, fp64.  a: the centring constant per plane (default: the
    plane mean of x); B (...): max(|x - a|, |y - a|) over the plane."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    a = x.mean((-2, -1), keepdims=True) if a is None else np.asarray(a, dtype=np.float64)
    xc, yc = x - a, y - a
    mx, my = valid_filter(xc), valid_filter(yc)
    vx, vy, cxy = valid_filter(xc * xc) - mx * mx, valid_filter(yc * yc) - my * my, valid_filter(xc * yc) - mx * my
    cs = (2. * cxy + C2) / (vx + vy + C2)
    fx, fy = mx + a, my + a
    lum = (2. * fx * fy + C1) / (fx * fx + fy * fy + C1)
    return lum * cs, cs, np.maximum(np.abs(xc).max((-2, -1)), np.abs(yc).max((-2, -1)))


def ssim_batch(x, y):
    """x (N, C, H, W), y (R, N, C, H, W) -> {'ssim' (R, N), 'cs' (R, N), 'map' (R, N, H - 10, W - 10), 'B' (R, N, C)} in fp64: what
    ops.ssim computes, and the largest centred magnitude of every plane pair."""
    m, cs, B = ssim_planes(np.asarray(x)[None], y)
    return {'ssim': m.mean((-3, -2, -1)), 'cs': cs.mean((-3, -2, -1)), 'map': m.mean(-3), 'B': B}


def pixel_bound(B):
    """|map - map64| of ONE plane pair whose largest centred magnitude is B: c 2^-24 (1 + B^2 / C2)."""
    return BOUND_C * U * (1. + np.asarray(B, dtype=np.float64) ** 2 / C2)


def map_bound(B):
    """B (..., C) -> the bound on the channel-mean map: the mean of the planes' bounds, and C - 1 fp32 additions of values of
    at most C in magnitude and one division, (C + 1) 2^-24 after the division."""
    B = np.asarray(B, dtype=np.float64)
    return pixel_bound(B).mean(-1) + (B.shape[-1] + 1) * U


def score_bound(B):
    """B (..., C) -> the bound on ssim[r, n] and cs[r, n]: the mean of the planes' bounds (the sums are fp64 in a fixed order,
    whose error is below 2^-40) and the one rounding to fp32 of a value of at most 1 in magnitude."""
    return pixel_bound(np.asarray(B, dtype=np.float64)).mean(-1) + U


# ----------------------------------------------------------------------------------------------- images
def near_constant(C, H, W, seed, level=0.99, spread=1e-3):
    rng = np.random.default_rng(seed)
    return (level + spread * rng.uniform(-1, 1, (C, H, W))).astype(np.float32)


KINDS = ('constant', 'noise', 'smooth', 'checkerboard', 'near-constant')


def image(kind, C, H, W, seed):
    if kind == 'constant':
        return constant(C, H, W, (37 * seed + 11) % 256)
    if kind == 'noise':
        return uniform_noise(C, H, W, seed)
    if kind == 'smooth':
        return smooth_noise(C, H, W, 4., seed)
    if kind == 'checkerboard':
        return checkerboard(C, H, W).copy()
    return near_constant(C, H, W, seed)


def batch(N, R, C, H, W, seed=0):
    """x (N, C, H, W) cycling through KINDS and y (R, N, C, H, W) fp32: draw 0 = x plus noise of the image's own spread (10^-3
    on the near-constant planes), draw 1 = x itself, draw 2 = a blur-like mix with values outside [0, 1], the others noisy
    copies of other noise levels."""
    rng = np.random.default_rng(1000 + seed)
    x = np.stack([image(KINDS[(i + seed) % len(KINDS)], C, H, W, 100 * seed + i) for i in range(N)]).astype(np.float32)
    near = np.array([KINDS[(i + seed) % len(KINDS)] == 'near-constant' for i in range(N)]).reshape(N, 1, 1, 1)
    y = np.empty((R,) + x.shape, dtype=np.float32)
    for r in range(R):
        if r == 1:
            y[r] = x
        elif r == 2:
            y[r] = 1.4 * x - 0.3 + 0.05 * rng.standard_normal(x.shape)
        else:
            y[r] = x + np.where(near, 1e-3, 0.02 * (1 + r % 7)) * rng.standard_normal(x.shape)
    return x, y


# ----------------------------------------------------------------------------------------------- the anchor
def scipy_ssim_maps(x, y):
    """scikit-image's structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=1) per plane, written
    out on scipy's gaussian_filter (its implementation), cropped to the interior."""
    from scipy.ndimage import gaussian_filter
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def f(p):
        return gaussian_filter(p, sigma=SIGMA, truncate=3.5, mode='reflect')
    ux, uy = f(x), f(y)
    vx, vy, vxy = f(x * x) - ux * ux, f(y * y) - uy * uy, f(x * y) - ux * uy
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    return s[5:-5, 5:-5]


@pytest.mark.parametrize('kind', KINDS)
def test_against_scipys_gaussian_filter(kind):
    x = image(kind, 2, 32, 32, 3).astype(np.float64)
    rng = np.random.default_rng(5)
    y = x + (1e-3 if kind == 'near-constant' else 0.05) * rng.standard_normal(x.shape)
    worst = 0.
    for c in range(2):
        want = scipy_ssim_maps(x[c], y[c])
        got = ssim_planes(x[c], y[c], a=0.)[0]                 # uncentred, as the anchor
        centred = ssim_planes(x[c], y[c])[0]
        assert got.shape == want.shape == (22, 22)
        worst = max(worst, np.abs(got / want - 1).max(), np.abs(centred / want - 1).max())
    print(kind, 'largest relative difference to the anchor', worst)
    assert worst <= 1e-11


def test_taps():
    g = taps()
    assert g.shape == (11,) and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1 / 4.5)) < 1e-15 and abs(g[0] / g[5] - np.exp(-25 / 4.5)) < 1e-15


def test_a_single_window_by_hand():
    rng = np.random.default_rng(2)
    x, y = rng.uniform(0, 1, (11, 11)), rng.uniform(-.2, 1.2, (11, 11))
    w = np.outer(taps(), taps())                                # the 2-D window: one output pixel
    mx, my = (w * x).sum(), (w * y).sum()
    vx, vy, cxy = (w * x * x).sum() - mx * mx, (w * y * y).sum() - my * my, (w * x * y).sum() - mx * my
    want_cs = (2 * cxy + C2) / (vx + vy + C2)
    want = (2 * mx * my + C1) / (mx * mx + my * my + C1) * want_cs
    m, cs, B = ssim_planes(x, y, a=0.)
    assert m.shape == (1, 1) and abs(m[0, 0] - want) <= 1e-14 and abs(cs[0, 0] - want_cs) <= 1e-14
    assert B == max(np.abs(x).max(), np.abs(y).max())
    got = ssim_batch(x[None, None], y[None, None, None])
    assert got['ssim'].shape == (1, 1) and abs(got['ssim'][0, 0] - want) <= 1e-13 and got['map'].shape == (1, 1, 1, 1)


def test_identities():
    x, y = batch(5, 4, 3, 16, 19, seed=1)
    got = ssim_batch(x, y)
    assert got['ssim'].shape == (4, 5) and got['map'].shape == (4, 5, 6, 9) and got['B'].shape == (4, 5, 3)
    assert np.abs(got['ssim'][1] - 1).max() <= 1e-12 and np.abs(got['cs'][1] - 1).max() <= 1e-12      # draw 1 is x
    assert (got['ssim'][[0, 2, 3]] < 1).all()
    for a in (0., 0.5, -3.):                                   # the centring constant changes nothing but rounding
        m, cs, _ = ssim_planes(x[None], y, a=a)
        assert np.abs(m.mean(-3) - got['map']).max() <= 1e-9 and np.abs(cs.mean((-3, -2, -1)) - got['cs']).max() <= 1e-9
    # symmetric in its arguments (the centring constant apart)
    m_xy, m_yx = ssim_planes(x, y[0], a=0.)[0], ssim_planes(y[0], x, a=0.)[0]
    assert np.abs(m_xy - m_yx).max() <= 1e-12


def test_the_bound_function():
    assert pixel_bound(0.) == BOUND_C * U
    b = pixel_bound(np.array([1e-3, 0.03, 0.5]))
    assert np.allclose(b / (BOUND_C * U), [1 + 1e-6 / C2, 2., 1 + .25 / C2], rtol=1e-12)
    # what the centring buys: on the near-constant planes the bound stays within 1 % of its floor, c units of 2^-24
    x, y = near_constant(1, 32, 32, 0), near_constant(1, 32, 32, 1)
    B = ssim_planes(x, y)[2]
    assert B.max() < 2.1e-3 and pixel_bound(B).max() < 1.01 * BOUND_C * U
    B3 = np.array([[0., 0.03, 0.03]])
    assert np.allclose(score_bound(B3), BOUND_C * U * 5 / 3 + U) and np.allclose(map_bound(B3), BOUND_C * U * 5 / 3 + 4 * U)
