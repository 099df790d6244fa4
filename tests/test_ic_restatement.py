"""The lossless image code length of csrc/ic.hip restated in numpy, with its closed forms and properties.
No GPU.  tests/test_30_ic_gpu.py holds the kernel to `code_length`, bit for bit: the histograms are integers, and the one
floating-point sum of a histogram runs over the symbols ascending in fp64, here as there, over the same table (ops.ic_table).

The coder: q = clamp(rint(255 x), 0, 255) in fp32; planes = the channels, at C == 3 also the space (G, (R - G) mod 256,
(B - G) mod 256); per plane the residual (v - pred) mod 256 of six predictors over a = left, b = up, c = up-left (0 outside) -
0, a, b, (a + b) >> 1, PNG's Paeth, the LOCO-I median edge detector - and a stored mode at 8 n bits; a residual plane with
histogram n_s over k used symbols costs 8 + log2 C(256, k) + log2[(n + k - 1)! / ((k - 1)! prod n_s!)] bits, every term from
T[m] = log2(m!); the image costs min over the spaces of sum over the planes of (3 + min over the modes), + 1 at C == 3; ties go
to the lower index."""
import math

import numpy as np
import pytest

MODES = 7
STORED = 6
STATUS_INEXACT, STATUS_NONFINITE = 1, 2
_TABLES = {}


def table(n):
    """T[m] = log2(m!), m = 0 .. n + 256, as a list of Python floats: the op's own host table."""
    from jvae_hip import ops
    if n not in _TABLES:
        _TABLES[n] = ops.ic_table(n).tolist()
    return _TABLES[n]


def quantise(x):
    """x (C, H, W) fp32 -> (q int32, status bits); the product and the difference are fp32 operations."""
    x = np.asarray(x, dtype=np.float32)
    t = np.float32(255.) * x
    finite = np.isfinite(t)
    status = 0 if finite.all() else STATUS_NONFINITE
    t = np.where(finite, t, np.float32(0.))                    # a non-finite pixel sets its own bit alone
    q = np.clip(np.rint(t), np.float32(0.), np.float32(255.)).astype(np.float32)
    if (np.abs(t - q) > np.float32(0.015625)).any():
        status |= STATUS_INEXACT
    return q.astype(np.int32), status


def residuals(plane):
    """plane (H, W) int32 in 0 .. 255 -> the six residual planes, (6, H, W) in 0 .. 255."""
    v = plane.astype(np.int32)
    a, b, c = np.zeros_like(v), np.zeros_like(v), np.zeros_like(v)
    a[:, 1:] = v[:, :-1]
    b[1:, :] = v[:-1, :]
    c[1:, 1:] = v[:-1, :-1]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    med = np.where(c >= hi, lo, np.where(c <= lo, hi, p))
    preds = (np.zeros_like(v), a, b, (a + b) >> 1, paeth, med)
    return np.stack([(v - q) & 255 for q in preds])


def histogram_bits(h, n, T):
    """The length of a residual plane with histogram h (256 counts that add up to n), in the kernel's order of operations."""
    k = int((h > 0).sum())
    s = 0.
    for count in h.tolist():                                   # ascending from symbol 0, fp64
        s += T[count]
    bits = 8. + ((T[256] - T[k]) - T[256 - k])
    bits += T[n + k - 1]
    bits -= T[k - 1]
    bits -= s
    return bits


def plane_mode_bits(plane, T):
    """The seven lengths of a plane: the six predictors', then the stored mode's 8 n."""
    n = plane.size
    res = residuals(plane)
    return [histogram_bits(np.bincount(r.ravel(), minlength=256), n, T) for r in res] + [8. * n]


def first_min(values):
    best = 0
    for i, v in enumerate(values):
        if v < values[best]:
            best = i
    return best


def choice_word(space, modes):
    word = space
    for p, m in enumerate(modes):
        word |= (m + 1) << (4 + 3 * p)
    return word


def code_length(x):
    """x (C, H, W) fp32 -> (bits, choice word, status); NaN and -1 for an image with a non-finite pixel."""
    q, status = quantise(x)
    if status & STATUS_NONFINITE:
        return float('nan'), -1, status
    C, H, W = q.shape
    T = table(H * W)
    planes = [q[c] for c in range(C)]
    spaces = [list(range(C))]
    if C == 3:
        planes += [(q[0] - q[1]) & 255, (q[2] - q[1]) & 255]
        spaces.append([1, 3, 4])
    per_plane = [plane_mode_bits(p, T) for p in planes]
    mode = [first_min(b) for b in per_plane]
    totals = []
    for sp in spaces:
        total = 0.
        for p in sp:
            total += 3. + per_plane[p][mode[p]]
        if C == 3:
            total += 1.
        totals.append(total)
    s = first_min(totals)
    return totals[s], choice_word(s, [mode[p] for p in spaces[s]]), status


def batch_code_length(x):
    """x (N, C, H, W) -> (bits (N,) fp64, choice (N,) int32, the OR of the status bits)."""
    got = [code_length(img) for img in x]
    status = 0
    for g in got:
        status |= g[2]
    return np.array([g[0] for g in got], dtype=np.float64), np.array([g[1] for g in got], dtype=np.int32), status


# ----------------------------------------------------------------------------------------------- images
def levels(q):
    """8-bit levels -> fp32 in [0, 1] as a /255 produces them."""
    return (np.asarray(q, dtype=np.float32) / np.float32(255.)).astype(np.float32)


def smooth_noise(C, H, W, sigma, seed):
    """Natural-like: a smooth field per channel (low-frequency waves on a shared base) plus Gaussian noise of `sigma` levels."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 128 + 60 * np.sin(2 * np.pi * (xx / max(W, 2) * rng.uniform(.5, 1.5) + rng.uniform())) * np.cos(
        2 * np.pi * (yy / max(H, 2) * rng.uniform(.5, 1.5) + rng.uniform()))
    img = np.stack([base + 25 * np.sin(2 * np.pi * (xx + yy) / (max(H + W, 2)) + rng.uniform(0, 6)) + rng.uniform(-20, 20)
                    for _ in range(C)])
    img = img + sigma * rng.standard_normal(img.shape)
    return levels(np.clip(np.rint(img), 0, 255))


def uniform_noise(C, H, W, seed):
    return levels(np.random.default_rng(seed).integers(0, 256, (C, H, W)))


def constant(C, H, W, level):
    return levels(np.full((C, H, W), level))


def checkerboard(C, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return levels(np.broadcast_to(((yy + xx) & 1) * 255, (C, H, W)))


def grey(C, H, W, seed):
    return np.ascontiguousarray(np.broadcast_to(smooth_noise(1, H, W, 6., seed), (C, H, W)))


KINDS = ('const0', 'const77', 'const255', 'uniform', 'smooth0', 'smooth4', 'smooth16', 'checker', 'grey')


def image(kind, C, H, W, seed=0):
    if kind.startswith('const'):
        return constant(C, H, W, int(kind[5:]))
    if kind.startswith('smooth'):
        return smooth_noise(C, H, W, float(kind[6:]), seed)
    return {'uniform': lambda: uniform_noise(C, H, W, seed), 'checker': lambda: checkerboard(C, H, W),
            'grey': lambda: grey(C, H, W, seed)}[kind]()


def batch(N, C, H, W, seed=0):
    """N images that cycle through KINDS, starting at a kind that hangs on the seed -> (N, C, H, W) fp32."""
    return np.stack([image(KINDS[(i + seed) % len(KINDS)], C, H, W, seed=100 * seed + i) for i in range(N)])


# ----------------------------------------------------------------------------------------------- closed forms
def log2_factorial(m):
    return math.lgamma(m + 1) / math.log(2)


def test_the_table_is_log2_factorial():
    T = table(1024)
    assert len(T) == 1024 + 257 and T[0] == 0. and T[1] == 0. and abs(T[2] - 1.) < 1e-15
    assert all(T[m] == math.lgamma(m + 1) / math.log(2) for m in (3, 255, 256, 1024, 1280))
    assert table(1024) is T                                    # kept per n


def test_a_constant_image_costs_58_bits():
    for level in (0, 77, 255):
        bits, word, status = code_length(constant(3, 32, 32, level))
        # per plane: 8 for k = 1, log2 C(256, 1) = 8 for the symbol, 0 for the 1024 pixels, 3 for the mode; 1 for the space
        print('constant', level, 'bits', repr(bits))
        assert abs(bits - 58.) <= 1e-9 and status == 0
        assert word == choice_word(0, [0, 0, 0])               # ties: the first space, the first mode


def test_a_single_pixel_is_stored():
    for level in (0, 9, 255):
        bits, word, status = code_length(constant(1, 1, 1, level))
        assert bits == 11. and word == choice_word(0, [STORED]) and status == 0    # 8 + 3: every predictor costs 16


def ramp_sub_bits(H, W):
    """The `sub` predictor on v[y][x] = x: the first column leaves 0, every other pixel 1 -> k = 2, n_0 = H, n_1 = H (W - 1)."""
    n = H * W
    return (8 + math.log2(256 * 255 / 2)
            + log2_factorial(n + 1) - log2_factorial(1) - log2_factorial(H) - log2_factorial(H * (W - 1)))


def test_a_horizontal_ramp_costs_the_sub_predictors_length():
    for H, W in ((1, 40), (5, 17), (3, 256)):
        x = levels(np.broadcast_to(np.arange(W), (1, H, W)))
        per_mode = plane_mode_bits(quantise(x)[0][0], table(H * W))
        want = ramp_sub_bits(H, W)
        print('ramp', (H, W), 'sub', per_mode[1], 'by hand', want)
        assert abs(per_mode[1] - want) <= 1e-9 * want
        bits, word, _ = code_length(x)
        assert bits == 3. + min(per_mode) and bits <= 3. + per_mode[1]
        if H == 1:                     # one row: up-left and up are 0, Paeth and the median fall back to `left` and tie with it
            assert per_mode[4] == per_mode[1] == per_mode[5] and bits == 3. + per_mode[1] and word == choice_word(0, [1])


SHAPES = ((1, 1, 1), (1, 2, 3), (3, 7, 5), (3, 32, 32), (4, 9, 9), (2, 8, 8), (1, 28, 28))


@pytest.mark.parametrize('C,H,W', SHAPES)
def test_bounds_hold_for_every_kind_of_image(C, H, W):
    n = H * W
    T = table(n)
    for kind in KINDS:
        x = image(kind, C, H, W, seed=3)
        bits, word, status = code_length(x)
        assert status == 0 and 0 < bits <= C * (8 * n + 3) + (C == 3), (kind, bits)
        q = quantise(x)[0]
        for plane in q:
            for r, got in zip(residuals(plane), plane_mode_bits(plane, T)):
                h = np.bincount(r.ravel(), minlength=256)
                p = h[h > 0] / n
                assert got >= n * float(-(p * np.log2(p)).sum()) - 1e-9, kind      # an adaptive code is no shorter than n H
        from jvae_hip import ops
        space, modes = ops.ic_choice(word)
        assert space in ((0, 1) if C == 3 else (0,)) and len(modes) == C and all(0 <= m < MODES for m in modes)
        assert ops.ic_choice_word(space, modes) == word


def test_uniform_noise_is_stored_and_noise_costs_bits():
    bits, word, _ = code_length(uniform_noise(3, 32, 32, 1))
    assert bits == 3 * (8 * 1024 + 3) + 1 and word == choice_word(0, [STORED] * 3)
    ladder = [code_length(smooth_noise(3, 32, 32, s, 4))[0] for s in (0., 4., 16.)]
    print('smooth + noise, sigma 0 / 4 / 16:', ladder)
    assert ladder[0] < ladder[1] < ladder[2] < bits


def test_the_difference_space_wins_on_a_grey_image():
    x = grey(3, 32, 32, 5)
    bits, word, _ = code_length(x)
    one = code_length(x[:1])[0]
    from jvae_hip import ops
    space, modes = ops.ic_choice(word)
    print('grey x 3:', bits, 'one plane:', one)
    assert space == 1 and modes[1:] == [0, 0]                  # R - G and B - G are constant planes: 16 + 3 bits each
    assert abs(bits - (one + 2 * 19 + 1)) <= 1e-9


def test_ties_go_to_the_lower_index():
    assert first_min([3., 2., 2., 5.]) == 1 and first_min([1., 1.]) == 0
    # a one-row image: `up` predicts 0 like `none`, Paeth and the median predict `left` like `sub`
    x = smooth_noise(1, 1, 60, 3., 2)
    per_mode = plane_mode_bits(quantise(x)[0][0], table(60))
    assert per_mode[0] == per_mode[2] and per_mode[1] == per_mode[4] == per_mode[5]
    assert first_min(per_mode) in (0, 1, 3, STORED)
    # the two colour spaces of a constant image cost the same: space 0
    assert code_length(constant(3, 4, 4, 200))[1] & 15 == 0


def test_choice_words_round_trip():
    from jvae_hip import ops
    assert ops.IC_MODES == ('none', 'sub', 'up', 'average', 'paeth', 'med', 'stored') and len(ops.IC_MODES) == MODES
    for space, modes in ((0, [0]), (0, [6, 0, 3]), (1, [5, 6, 6]), (0, [1, 2, 3, 4]), (0, [6, 6, 6, 6])):
        word = ops.ic_choice_word(space, modes)
        assert word == choice_word(space, modes) and ops.ic_choice(word) == (space, modes)
    assert ops.ic_choice(-1) == (-1, [])
    import torch
    assert ops.ic_choice(torch.tensor(choice_word(1, [2, 0, 4]), dtype=torch.int32)) == (1, [2, 0, 4])


def test_quantisation_flags():
    x = constant(1, 4, 4, 100)
    assert quantise(x + np.float32(0.3 / 255))[1] == STATUS_INEXACT
    assert np.array_equal(quantise(x + np.float32(0.3 / 255))[0], quantise(x)[0])
    assert quantise(x + np.float32(0.01 / 255))[1] == 0
    assert quantise(x * 3)[1] == STATUS_INEXACT and quantise(x * 3)[0].max() == 255       # clamped: far from its level
    y = x.copy()
    y[0, 1, 2] = np.nan
    assert code_length(y)[1:] == (-1, STATUS_NONFINITE) and math.isnan(code_length(y)[0])
    y[0, 1, 2] = np.inf
    assert quantise(y)[1] & STATUS_NONFINITE
    every = levels(np.arange(256).reshape(1, 16, 16))          # /255 and back: every level is recovered exactly
    assert np.array_equal(quantise(every)[0].ravel(), np.arange(256)) and quantise(every)[1] == 0
