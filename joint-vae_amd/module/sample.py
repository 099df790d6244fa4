"""Use a network to generate new images: grids of prior draws and of reconstructions (reference: module/sample.py).

`sample()` keeps the reference's contract (module/sample.py:36-173): the same N / L / name-width rules, `%j` in `root`
replaced by the job number (six digits for an int), `params.tex`, the returned `list_of_images` ([{'name', 'tensor'[, 'tex']}],
the grid first, then the cells row by row) and one `.png` (+ `.tex`) per entry.

What differs underneath: the grid is not concatenated cell by cell.  ONE launch of the grid kernel (csrc/sample.hip,
ops.image_grid) writes the whole fp32 grid and its 8-bit, channel-last form from the decoded rows; every `tensor` of the list
is a VIEW into that one fp32 grid, every PNG a slice of the 8-bit grid (torchvision's save_image arithmetic,
floor(clamp(255 v + 0.5, 0, 255))), written with the standard library alone (zlib, struct; filter type 0, 8-bit grey or RGB:
neither torchvision nor PIL is needed).  The prior branch draws and decodes through `net.generate()`, the `x` branch runs the
label-free `net.evaluate(x[:N], None, z_output=True)` once.  `save=False` returns the list without touching the disk.

`zsample()` writes the per-dimension statistics of the posterior (`hist_var_z.dat`, `mu_z_var_z.dat`, and one pair per class)
through the encode-only pass `net.latent_posterior()` - no image is decoded - and ONE `ops.latent_moments` launch pair per batch
into fp64 device accumulators grouped by label; the only read-back is at the end.  Unlike the reference, whose per-class
files repeat the all-sample statistics (it builds the class mask and never applies it), the per-class files hold the
statistics of that class's samples.  `comparison()` returns the reference's (div, y_pred) dictionaries; every pair's mean
squared difference of the mean reconstructions comes from one `ops.cascade_mse` call.

Not rebuilt here, it stays in the reference: the command-line block.
"""
import logging
import os
import struct
import zlib

import numpy as np
import torch

from jvae_hip import ops

DEFAULT_RESULTS_DIR = 'jobs/results'            # utils/parameters.py:14


class DefaultClasses(object):

    def __getitem__(self, k):
        return k


def job_to_str(number, string, formats={int: '{:06d}'}):
    """utils/save_load/misc.py:16-18"""
    return string.replace('%j', formats.get(type(number), '{}').format(number))


def _texdef(f, **kw):
    for k, v in kw.items():
        f.write(r'\def\model{}{{{}}}'.format(k, v))


def png_bytes(image):
    """(H, W, D) uint8 array, D = 1 (grey) or 3 (RGB) -> the bytes of a PNG file (one IDAT chunk, filter type 0 on every row)."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w, d = image.shape
    if d not in (1, 3):
        raise ValueError('PNG output is built for 1 (grey) or 3 (RGB) channels, got {}'.format(d))
    rows = np.zeros((h, 1 + w * d), dtype=np.uint8)
    rows[:, 1:] = image.reshape(h, w * d)

    def chunk(tag, data):
        return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)
    header = struct.pack('>IIBBBBB', w, h, 8, 0 if d == 1 else 2, 0, 0, 0)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', header) + chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)) + chunk(b'IEND', b'')


def sample(net, x=None, y=None, root=os.path.join(DEFAULT_RESULTS_DIR, '%j', 'samples'), directory='test',
           in_classes=DefaultClasses(), out_classes=DefaultClasses(),
           N=20, L=10, save=True):
    r"""Creates a grid of output images. If x is None the output images are the ones created when the decoder is fed with
    prior z: one row per class (N = num_labels for a cvae), one column per draw.  With x: one row per input, holding the
    input, its mean reconstruction, the average over ALL latent_sampling draws (when there is more than one) and the first
    L draws."""
    if x is not None:
        N = min(N, len(x))
    elif net.is_cvae:
        N = net.num_labels

    wN = int(np.log10(N - 1)) + 1
    L = min(L, net.latent_sampling)
    with_average = net.latent_sampling > 1
    wL = 1 if L <= 1 else int(np.log10(L - 1)) + 1

    dir_path = os.path.join(job_to_str(net.job_number, root), directory)
    if save:
        if not os.path.exists(dir_path):
            os.makedirs(dir_path)
        elif not os.path.isdir(dir_path):
            raise FileExistsError
        with open(os.path.join(dir_path, 'params.tex'), 'w') as f:
            _texdef(f, sigma=net.sigma, latentdim=net.latent_dim, dset=net.training_parameters['set'])

    defy = r'\def\y{{{}}}'
    (D, H, W) = net.input_shape[-3:]

    if x is not None:
        with torch.no_grad():
            x_, logits, batch_losses, measures, mu, log_var, z = net.evaluate(x[:N], None, z_output=True)
            if net.predict_methods:
                y_ = net.predict_after_evaluate(logits, batch_losses)
            else:
                y_ = torch.zeros_like(y)
            # columns of a row: in, out_mean, [out_average over every draw], out_0 .. out_{L-1}
            columns = [('input',), ('draw', 0)] + ([('average', 1, x_.shape[0] - 1)] if with_average else []) \
                + [('draw', 1 + l_) for l_ in range(L)]
            grid, grid_u8 = ops.image_grid(x[:N].reshape(N, D, H, W), x_.reshape(-1, N, D, H, W), columns, u8=save)
        y_in, y_out = y[:N].cpu(), y_[:N].cpu()          # indices into the class names, as the reference passes them
        names = [('in', in_classes, y_in), ('out_mean', out_classes, y_out)] \
            + ([('out_average', out_classes, y_out)] if with_average else []) \
            + [(f'out_{l_:0{wL}}', out_classes, y_out) for l_ in range(L)]
        list_of_images = [{'name': f'grid-{N}x{L}', 'tensor': grid}]
        for row in range(N):
            for col, (tail, classes, labels) in enumerate(names):
                list_of_images.append({'name': f'x_{row:0{wN}}_{tail}',
                                       'tensor': grid[:, row * H:(row + 1) * H, col * W:(col + 1) * W],
                                       'tex': defy.format(classes[labels[row]]),
                                       'cell': (row, col)})

    elif net.is_cvae or net.is_jvae or net.is_vae:
        x_ = net.generate(y=torch.arange(N, device=net.device), L=L)
        with torch.no_grad():
            grid, grid_u8 = ops.image_grid(None, x_.reshape(L, N, D, H, W), [('draw', l_) for l_ in range(L)], u8=save)
        list_of_images = [{'name': f'grid-{N}x{L}', 'tensor': grid}]
        for row in range(N):
            for l_ in range(L):
                list_of_images.append({'name': f'x{row:0{wN}}_out_{l_:0{wL}}',
                                       'tensor': grid[:, row * H:(row + 1) * H, l_ * W:(l_ + 1) * W],
                                       'cell': (row, l_)})

    else:
        raise ValueError('You try to generate images with a net'
                         f'which is {net.type}')

    if save:
        pixels = grid_u8.cpu().numpy()                   # ONE copy to the host: (N H, Ncol W, D) uint8, cells are slices of it
    for image in list_of_images:
        cell = image.pop('cell', None)
        if not save:
            continue
        path = os.path.join(dir_path, image['name'] + '.png')
        logging.debug('Saving image in %s', path)
        tile = pixels if cell is None else pixels[cell[0] * H:(cell[0] + 1) * H, cell[1] * W:(cell[1] + 1) * W]
        with open(path, 'wb') as f:
            f.write(png_bytes(tile))
        if 'tex' in image:
            path = os.path.join(dir_path, image['name'] + '.tex')
            with open(path, 'w') as f:
                f.write(image['tex'])

    return list_of_images


def zsample(x, net, y=None, batch_size=128, root=os.path.join(DEFAULT_RESULTS_DIR, '%j', 'samples'), bins=10, directory='test'):
    r"""Statistics of the posterior q(z|x) over a set (reference module/sample.py:176-233): per latent dimension the mean of
    mu^2, the mean variance, their sum, the mean of mu and the unbiased std of the variance (`mu_z_var_z.dat`, rows sorted by the
    first column, descending) and the histogram of the K mean variances over (0, max) (`hist_var_z.dat`); with `y`, the same
    two files per class c (`hist_var_z<c>.dat`, `mu_z_var_z<c>.dat`) over that class's samples - no file for a class
    without samples, `nan` in std_var_z for a class with one.  N is cut to a multiple of `batch_size`.

    Per batch: `net.latent_posterior` (features and the two encoder heads: nothing is decoded), then `ops.latent_moments`
    with group = y into (C + 1, 4, K) fp64 accumulators on the device (the last group takes labels outside [0, C)); they are
    read once, at the end, and the all-sample statistics are the sum of the groups.  -> {'dir', 'sums' (C + 1, 4, K),
    'counts' (C + 1,)} (the reference returns None)."""
    from jvae_compat import inspection
    N = len(x)
    N -= N % batch_size
    assert net.type != 'cvae' or y is not None
    device = net.device
    K = net.latent_dim
    C = net.num_labels if y is not None else 0
    sums = torch.zeros((C + 1, 4, K), dtype=torch.float64, device=device)
    counts = torch.zeros(C + 1, dtype=torch.int64, device=device)
    logging.debug('Computes mu_z var_z for {} samples'.format(N))
    for start in range(0, N, batch_size):
        xb = x[start:start + batch_size].to(device)
        yb = None if y is None else y[start:start + batch_size].to(device)
        mu, log_var = net.latent_posterior(xb, yb if net.y_is_coded else None)
        group = None
        if yb is not None:
            group = torch.where((yb >= 0) & (yb < C), yb, torch.full_like(yb, C)).to(torch.int32)
        ops.latent_moments(mu.reshape(-1, K), log_var.reshape(-1, K), group, sums, counts)
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()              # the only read-back

    dir_path = os.path.join(job_to_str(net.job_number, root), directory)
    os.makedirs(dir_path, exist_ok=True)

    def write(tag, s, n):
        stats = inspection.per_dim_statistics(s, n)
        with open(os.path.join(dir_path, f'hist_var_z{tag}.dat'), 'w') as f:
            f.write(inspection.hist_text(*inspection.per_dim_hist(stats['mu_var_z'], bins=bins)))
        with open(os.path.join(dir_path, f'mu_z_var_z{tag}.dat'), 'w') as f:
            f.write(inspection.scatter_text(stats))

    if counts.sum():
        write('', sums.sum(0), counts.sum())
    for c in range(C):
        if counts[c]:
            write(c, sums[c], counts[c])
    return {'dir': dir_path, 'sums': sums, 'counts': counts}


def comparison(x, *nets, batch_size=128, root=os.path.join(DEFAULT_RESULTS_DIR, '%j', 'samples'), directory='ood'):
    r"""Comparison of different nets on the same inputs (reference module/sample.py:236-274) -> (div, y_pred):
    div[j][jj], for the job numbers jj > j, is the (N,) mean squared difference between the mean reconstructions of the two
    nets, y_pred[j] (N,) the classes net j predicts; N = len(x) cut to a multiple of the batch size, which is bounded by
    every net's max_batch_sizes['test'].  All pairs come from ONE `ops.cascade_mse` call with the mean reconstructions as
    one-draw stages (its rows against x itself are ignored).  Both dictionaries hold host tensors, as in the reference."""
    root = root.replace('%j', '-'.join(str(n.job_number) for n in nets))
    for n in nets:
        batch_size = min(n.max_batch_sizes['test'], batch_size)
    logging.info('Batch size for comparison: %s', batch_size)
    N = x.shape[0] // batch_size * batch_size
    jobs = [n.job_number for n in nets]
    x_, y_pred = {}, {}
    for n in nets:
        reco, pred = [], []
        for start in range(0, N, batch_size):
            with torch.no_grad():
                x__, logits, losses, _ = n.evaluate(x[start:start + batch_size].to(n.device))
                pred.append(n.predict_after_evaluate(logits, losses))
                reco.append(x__[0])
        x_[n.job_number] = torch.cat(reco).unsqueeze(0).contiguous() if reco else None
        y_pred[n.job_number] = torch.cat(pred).cpu() if pred else torch.zeros(0, dtype=torch.int64)
    div = {j: {jj: torch.zeros(0) for jj in jobs if jj > j} for j in jobs}
    if N:
        x0 = x[:N].to(nets[0].device).contiguous()
        mse = ops.cascade_mse(x0, [x_[j].to(x0.device) for j in jobs]).cpu()
        for a, j in enumerate(jobs):
            for b, jj in enumerate(jobs):
                if jj > j:
                    hi, lo = max(a, b) + 1, min(a, b) + 1          # stages of the two nets; stage 0 is x
                    div[j][jj] = mse[hi * (hi - 1) // 2 + lo]
    return div, y_pred
