#!/usr/bin/env python3
"""Write tests/golden/regret/*.npz: the likelihood-regret loop of small models, by the plain-torch restatement.

    python tools/gen_regret_golden.py [case ...]

The reference has no likelihood regret, so there is nothing of it to run: the goldens come from
tests/test_regret_restatement.py::regret_restatement - the functional model of oracle/jvae_oracle.py, torch.autograd and
torch.optim.Adam on the deterministic weights of oracle/det_init.py - once in fp64 and once in fp32, on the CPU.  Only data is
written:

    x (N, ...), y (N,), eps (steps + 1, L, N, K), steps, lr, seed
    mu64, lv64 (steps + 1, N, K), J64 (steps + 1, N), regret64 (N,)     the fp64 trajectory (J_steps under the last noise)
    d_ref_mu, d_ref_lv, d_ref_J, d_ref_regret                           the fp32 run's max-norm distance to fp64, relative to
                                                                        the largest fp64 value, over the samples not left out
    preact_min64, preact_err32 (steps, N)       per iteration and sample: the smallest |pre-activation| of any hidden unit of the
                                                decoder in the fp64 gradient pass, and the largest fp32-vs-fp64 difference of one

A sample is LEFT OUT when, in some iteration, preact_min64 < preact_err32: a ReLU unit of its decoder sits closer to zero than
the fp32 forward error, fp32 takes the other side's gradient and the two trajectories part (the rule of
tests/test_6_odin_gpu.py, extended over the iterations).  The seed of a case is the first one from 1234 on with at most 1 of
the N samples left out; tests/test_27_regret_gpu.py relies on that cap, so it is asserted here."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd'), os.path.join(REPO, 'tests')):
    sys.path.insert(0, p)
OUT = os.path.join(REPO, 'tests', 'golden', 'regret')

import test_regret_restatement as R                              # noqa: E402


def per_sample(t, N, how):
    """Dense (L+1, N, d) or conv ((L+1) * N, C, H, W) pre-activations -> (N,) reduction over everything but the sample axis."""
    rows = t.shape[0] if t.dim() == 4 else t.shape[0] * t.shape[1]
    return how(t.reshape(rows // N, N, -1).transpose(0, 1).reshape(N, -1), 1)[0]


def run_case(name, kw, N):
    L, K = kw['test_latent_sampling'], kw['latent_dim']
    for seed in range(1234, 1334):
        g = torch.Generator().manual_seed(seed)
        x = torch.rand((N, *kw['input_shape']), generator=g)
        y = torch.randint(0, kw['num_labels'], (N,), generator=g)
        eps = torch.randn((R.STEPS + 1, L, N, K), generator=g)
        out = {}
        for dtype, tag in ((torch.float64, '64'), (torch.float32, '32')):
            seen = []
            reg, traj = R.regret_restatement(kw, R.regret_state(kw, dtype), x.to(dtype), y, eps.to(dtype), R.STEPS, R.LR, seen)
            out['regret' + tag] = reg.double()
            for i, key in enumerate(('mu', 'lv', 'J')):
                out[key + tag] = torch.stack([t[i] for t in traj]).double()
            out['pre' + tag] = seen
        pmin = torch.stack([torch.stack([per_sample(p.abs(), N, torch.min) for p in it]).min(0)[0] for it in out['pre64']])
        perr = torch.stack([torch.stack([per_sample((a.double() - b).abs(), N, torch.max) for a, b in zip(i32, i64)]).max(0)[0]
                            for i32, i64 in zip(out['pre32'], out['pre64'])])
        gone = (pmin < perr).any(0)
        print(f'{name}: seed {seed}: samples left out {int(gone.sum())}')
        if int(gone.sum()) <= 1:
            break
    else:
        raise SystemExit(f'{name}: no seed found')
    assert int(gone.sum()) <= 1                                   # the cap tests/test_27_regret_gpu.py relies on
    keep = ~gone
    data = dict(x=x.numpy(), y=y.numpy(), eps=eps.numpy(), steps=np.int64(R.STEPS), lr=np.float64(R.LR), seed=np.int64(seed),
                preact_min64=pmin.numpy(), preact_err32=perr.numpy())
    for key in ('mu', 'lv', 'J', 'regret'):
        a64, a32 = out[key + '64'], out[key + '32']
        data[key + '64'] = a64.numpy()
        sel = (lambda t: t[keep]) if key == 'regret' else (lambda t: t[:, keep])
        data['d_ref_' + key] = np.float64(float((sel(a32) - sel(a64)).abs().max() / sel(a64).abs().max()))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **data)
    print(f'{name}: regret {out["regret64"].tolist()}\n  d_ref ' + ', '.join(f'{k} {float(data["d_ref_" + k]):.2e}' for k in
          ('mu', 'lv', 'J', 'regret')) + f' -> {path} ({os.path.getsize(path) / 1024:.0f} KiB)')


def main():
    torch.set_num_threads(8)
    for name, (kw, N) in R.regret_cases().items():
        if len(sys.argv) < 2 or name in sys.argv[1:]:
            run_case(name, kw, N)


if __name__ == '__main__':
    main()
