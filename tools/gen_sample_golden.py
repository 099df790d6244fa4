#!/usr/bin/env python3
"""Write tests/golden/sample/*.npz: what the REFERENCE's module/sample.py::sample() returns and writes, on deterministic models.

    python tools/gen_sample_golden.py --reference <checkout of moxime/joint-vae>

The reference's `module.sample` is imported under the placeholder modules of oracle/gen_golden.py::import_reference();
its `save_image` is replaced by a capture (name of the file -> the tensor it was handed), `job_number` and
`training_parameters['set']` are set, the model is put in eval mode with the deterministic weights of oracle/det_init.py
and the noise is injected with oracle/gen_golden.py::inject_eps.  Per model two files:

  <case>_prior.npz   sample(net, N=20, L=10): the prior branch - one row per class, one column per draw (L is cut to the
                     model's latent_sampling); `eps` (L, N, K) is the noise the reference's torch.randn(L, N, K) returned
  <case>_x.npz       sample(net, x[:N], y[:N], N=N, L=L): the inputs of oracle/det_init.py::det_inputs beside their mean
                     reconstruction, the average over the draws (latent_sampling > 1) and the single draws; `eps`
                     (latent_sampling + 1, N, K) is the noise of the evaluation

Cases: `e2_n8_L3` (conv model, 3 x 32 x 32, latent_sampling 3: x branch at N = 8, L = 2, class names given) and `c1_n16_mlp`
(dense decoder, 1 x 28 x 28, sigmoid output, latent_sampling 1 - no average column; default class names).
Every file holds: `eps`, `names` (list_of_images in order), `grid` (the first entry's tensor, fp32), `cell_names` / `tex`
(the entries with a .tex string and the strings), `params_tex`, `saved` (the names save_image was called with, in order),
`job_number`, `dset`, `N`, `L`; the x branch also `y_` (the predicted classes).  The cells are not stored: the reference
builds the grid by concatenating them, so they are slices of it (asserted here).  Only data is written.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'sample')
sys.path.insert(0, REPO)

JOB_NUMBER = 4217
DSET = 'cifar10'
CLASS_NAMES = ['class-%d' % c for c in range(10)]
X_BRANCH = {'e2_n8_L3': dict(N=8, L=2, named=True), 'c1_n16_mlp': dict(N=16, L=10, named=False)}


def run(Net, ref_sample, name, branch):
    from oracle import gen_golden
    from oracle.cases import get_case
    from oracle.det_init import det_inputs, load_det_state
    case = get_case(name)
    kw = case['net']
    torch.manual_seed(0)
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.eval()
    net.job_number = JOB_NUMBER
    net.training_parameters['set'] = DSET
    K, C, Ls = kw['latent_dim'], kw['num_labels'], net.latent_sampling
    saved = []
    ref_sample.save_image = lambda tensor, path, **k: saved.append((os.path.basename(path), tensor.detach().clone()))
    extra = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, '%j', 'samples')
        if branch == 'prior':
            N, L = C, min(10, Ls)
            eps = torch.randn(L, N, K, generator=torch.Generator().manual_seed(4321))
            with gen_golden.inject_eps(eps):
                images = ref_sample.sample(net, root=root, directory='generate', N=20, L=10)
            directory = 'generate'
        else:
            N, L = X_BRANCH[name]['N'], min(X_BRANCH[name]['L'], Ls)
            x, y, eps = det_inputs(N, kw['input_shape'], C, Ls, K)
            classes = dict(in_classes=CLASS_NAMES, out_classes=CLASS_NAMES) if X_BRANCH[name]['named'] else {}
            with torch.no_grad(), gen_golden.inject_eps(eps):
                images = ref_sample.sample(net, x, y, root=root, directory='test', N=N, L=X_BRANCH[name]['L'], **classes)
                x_, logits, losses, _ = net.evaluate(x[:N], None)          # the prediction sample() printed into the .tex
                extra['y_'] = net.predict_after_evaluate(logits, losses).numpy()
            directory = 'test'
        dir_path = os.path.join(tmp, '%06d' % JOB_NUMBER, 'samples', directory)
        params_tex = open(os.path.join(dir_path, 'params.tex')).read()
        for im in images:
            assert os.path.exists(os.path.join(dir_path, im['name'] + '.tex')) == ('tex' in im), im['name']
            if 'tex' in im:
                assert open(os.path.join(dir_path, im['name'] + '.tex')).read() == im['tex']
    names = [im['name'] for im in images]
    assert [n for n, _ in saved] == [n + '.png' for n in names]
    grid = images[0]['tensor'].detach()
    D, H, W = kw['input_shape']
    per_row = (len(images) - 1) // N
    assert tuple(grid.shape) == (D, N * H, per_row * W) and names[0] == f'grid-{N}x{L}'
    for i, im in enumerate(images[1:]):                    # every cell is the slice of the grid at its place
        r, c = divmod(i, per_row)
        assert torch.equal(im['tensor'].detach(), grid[:, r * H:(r + 1) * H, c * W:(c + 1) * W]), im['name']
    with_tex = [im for im in images if 'tex' in im]
    data = dict(eps=eps.numpy(), names=np.array(names), grid=grid.numpy(), cell_names=np.array([im['name'] for im in with_tex]),
                tex=np.array([im['tex'] for im in with_tex]), params_tex=np.array(params_tex),
                saved=np.array([n for n, _ in saved]), job_number=np.int64(JOB_NUMBER), dset=np.array(DSET), N=np.int64(N),
                L=np.int64(L), **extra)
    assert data['grid'].dtype == np.float32
    path = os.path.join(OUT, f'{name}_{branch}.npz')
    np.savez_compressed(path, **data)
    print(f'{name}_{branch}: {names[0]} grid {tuple(grid.shape)} in [{float(grid.min()):.3f}, {float(grid.max()):.3f}], '
          f'{len(names)} images, row: {names[1:1 + per_row]}, params.tex {params_tex!r}, {os.path.getsize(path)} bytes')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds cvae.py)')
    a = ap.parse_args()
    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(a.reference)
    Net = gen_golden.import_reference()
    import module.sample as ref_sample
    assert os.path.abspath(ref_sample.__file__).startswith(gen_golden.REF), ref_sample.__file__
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    for name in X_BRANCH:
        for branch in ('prior', 'x'):
            run(Net, ref_sample, name, branch)


if __name__ == '__main__':
    main()
