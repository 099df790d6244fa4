#!/usr/bin/env python3
"""Write tests/golden/cascad/*.npz: what the REFERENCE's module/cascad.py returns on chains of deterministic models.

    python tools/gen_cascad_golden.py --reference <checkout of moxime/joint-vae>

The reference is imported under the placeholder modules of oracle/gen_golden.py::import_reference(); the models get the
deterministic weights of oracle/det_init.py and are put in eval mode (each one: the cascade's own eval() raises in the
reference); their reparameterisation noise is injected, one noise per stage, in order
(tools/gen_aggregation_golden.py::inject_eps_queue).  The reference's constructor copies the last model through save() /
load(): every model is given `trained = 1` and a training set name, and the copy goes to a temporary directory.  Only data is
written.

Chains (tests/test_cascad_restatement.py::CHAINS; x = det_inputs(8, ..., seed CHAIN_X_SEED), stage i: load_det_state(seed i),
noise det_inputs(..., seed CHAIN_X_SEED + 1 + i)), evaluate(x, z_output=True, temps=[1, 5]):
  <chain>.npz   eps<i> (L + 1, N, K) per stage, stage_in (M, N, D): what every stage read (x, then the first draw of the stage
                before), y_ (M, N, C), loss.<k>: every stacked loss, mse (M (M + 1) / 2, N), Im-1 and Im-5 (M (M - 1) / 2, N),
                measure.<k> (M,); mse_err: the reference's own error against the fp64 restatement (mse64) on ITS fp32
                reconstructions, which are not stored
  iterate.npz   posterior (M, C, N) = iterate_with_prior(iter_inputs(*ITER_GOLDEN)) and its error against fp64 (err)
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, 'tests', 'golden', 'cascad')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))


def build(Net, name, seed, job_dir):
    from oracle.cases import get_case
    from oracle.det_init import load_det_state
    kw = get_case(name)['net']
    torch.manual_seed(0)
    net = Net(**kw)
    load_det_state(net, seed=seed)
    net.eval()
    net.trained = 1
    net.training_parameters['set'] = 'cifar10'
    net.job_number = 100 + seed
    net.saved_dir = os.path.join(job_dir, str(net.job_number))
    return net, kw


def run_chain(Net, ref_cascad, chain, job_dir):
    import test_cascad_restatement as R
    from gen_aggregation_golden import inject_eps_queue
    from oracle.det_init import det_inputs
    name, seeds = R.CHAINS[chain]
    nets, kws = zip(*[build(Net, name, s, job_dir) for s in seeds])
    kw, N, M = kws[0], R.CHAIN_N, len(seeds)
    C, K, L = kw['num_labels'], kw['latent_dim'], nets[0].latent_sampling
    x = det_inputs(N, kw['input_shape'], C, 1, K, seed=R.CHAIN_X_SEED)[0]
    eps = [det_inputs(N, kw['input_shape'], C, L, K, seed=R.CHAIN_X_SEED + 1 + i)[2] for i in range(M)]
    model = ref_cascad.CascadModels(*nets)
    assert len(model) == M and all(not n.training for n in nets)
    with torch.no_grad(), inject_eps_queue(eps) as left:
        x_, y_, losses, measures = model.evaluate(x, z_output=True, temps=R.CHAIN_TEMPS)
    assert not left
    D = x[0].numel()
    assert tuple(x_.shape) == (M, L + 1, N) + tuple(kw['input_shape']) and x_.dtype == torch.float32
    data = {f'eps{i}': e.numpy() for i, e in enumerate(eps)}
    data['stage_in'] = torch.stack([x] + [x_[k][1] for k in range(M - 1)]).reshape(M, N, D).numpy()
    data['y_'] = y_.numpy()
    for k, v in losses.items():
        data[k if k == 'mse' or k.startswith('Im-') else 'loss.' + k] = v.numpy()
    for k, v in measures.items():
        data['measure.' + k] = v.double().numpy()
    stages = [x_[k][1:].reshape(L, N, D).numpy() for k in range(M)]
    exact = R.mse64(x.reshape(N, D).numpy(), stages)
    assert data['mse'].shape == exact.shape and data['mse'].dtype == np.float32
    data['mse_err'] = np.float64(np.abs(exact - data['mse']).max())
    path = os.path.join(OUT, chain + '.npz')
    np.savez_compressed(path, **data)
    top = float(np.abs(exact).max())
    print(f'{chain}: M={M} L={L} C={C} {os.path.getsize(path)} bytes; mse err {data["mse_err"] / top:.2e} of max {top:.3e}; '
          f'losses {sorted(losses)}; measures {sorted(measures)}')


def run_iterate(ref_cascad):
    import test_cascad_restatement as R
    p = R.iter_inputs(*R.ITER_GOLDEN)
    post = ref_cascad.iterate_with_prior(torch.from_numpy(p)).numpy()
    err = np.abs(post - R.iter64(p)).max()
    path = os.path.join(OUT, 'iterate.npz')
    np.savez_compressed(path, posterior=post, err=np.float64(err))
    print(f'iterate: {os.path.getsize(path)} bytes; err {err:.2e}')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds cvae.py)')
    a = ap.parse_args()
    from oracle import gen_golden
    gen_golden.REF = os.path.abspath(a.reference)
    Net = gen_golden.import_reference()
    import module.cascad as ref_cascad
    assert os.path.abspath(ref_cascad.__file__).startswith(gen_golden.REF), ref_cascad.__file__
    import test_cascad_restatement as R
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(8)
    with tempfile.TemporaryDirectory() as job_dir:
        for chain in R.CHAINS:
            run_chain(Net, ref_cascad, chain, job_dir)
    run_iterate(ref_cascad)


if __name__ == '__main__':
    main()
