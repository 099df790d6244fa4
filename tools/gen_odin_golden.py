#!/usr/bin/env python3
"""Write tests/golden/odin/*.npz: what the REFERENCE's ODIN loop (cvae.py:1645-1663) computes for small vib models.

    python tools/gen_odin_golden.py --reference <checkout of moxime/joint-vae> [--timing]

The reference model class is imported from the checkout with the placeholder modules oracle/gen_golden.py uses, gets the
deterministic weights of oracle/det_init.py (running means / variances away from 0 / 1, so the BatchNorm factor counts) and
runs, in eval mode, the loop exactly as cvae.py:1645-1663 has it - x.grad never zeroed between the temperatures, a fresh
epsilon per forward (torch.randn is patched to serve a seeded tensor per forward), no clamping - with
ODIN_TEMPS = [1, 10, 1000] and ODIN_EPS = [0, 0.0014, 0.004] on the instance, once in fp32 and once with model and input in
fp64.  Only data is written:

    x (N, ...), eps_noise (T, 1+E, L+1, N, K)      slot [t, 0]: gradient pass of temperature t, [t, 1+e]: perturbed forward e
    acc32 / acc64 (T, N, ...)                       the ACCUMULATED input gradient after temperature t; sign (int8) of acc32
    scores32 / scores64 (T, E, N), names (T*E)      the odin-T-eps score vectors
    logits (T, L+1, N, C)                           of the gradient passes (fp32)
    grad_err (T)                                    max|acc32 - acc64| / max|acc64|: the reference's own fp32 error
    preact_min64 / preact_err32 (N)                 per sample: the smallest |pre-activation| of any ReLU unit in the fp64 forward
                                                    of the first gradient pass, and the largest fp32-vs-fp64 difference of one
    flips32                                         share of sign(acc32) != sign(acc64) elements (per case, over all T)

The seed of a case is the first one (from 1234 on) for which the reference's own fp32 run has no sample with
preact_min64 < preact_err32 and at most 0.5 % sign flips against its fp64 run (tests/test_6_odin_gpu.py allows the product
as much).  --timing also times the reference on one batch of 100 CIFAR-shaped images (conv32, K = 64, C = 10, L = 16) through
the full 10 x 21 grid on this CPU -> tests/golden/odin/timing.json (the yardstick of tools/odin_bench.py).
"""
import argparse
import json
import os
import platform
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, 'tests', 'golden', 'odin')

from oracle import gen_golden                                    # noqa: E402
from oracle.cases import get_case                                # noqa: E402
from oracle.det_init import load_det_state                       # noqa: E402

TEMPS, SIZES = [1, 10, 1000], [0, 0.0014, 0.004]


def cases():
    base = dict(get_case('eb2_n8_vib_L2')['net'])
    mlp = dict(base, input_shape=(1, 28, 28), features=None, encoder=[64], batch_norm=False, latent_dim=16)
    return {'eb2_n8_vib_L2': dict(net=base, N=8),
            'eb2_n8_vib_L2_leaky': dict(net=dict(base, activation='leaky'), N=8),
            'mb2_n8_vib_L2_mlp': dict(net=mlp, N=8)}


class Noise:
    """torch.randn stand-in: forward number i of the loop gets slot i of the (T * (1 + E), L+1, N, K) noise."""

    def __init__(self, noise, dtype):
        self.slots, self.i, self.dtype = noise.reshape(-1, *noise.shape[2:]), 0, dtype

    def __call__(self, *size, **kw):
        size = size[0] if len(size) == 1 and not isinstance(size[0], int) else size
        e = self.slots[self.i]
        assert tuple(size) == tuple(e.shape), (size, e.shape)
        self.i += 1
        return e.clone().to(self.dtype)


def odin_loop(net, x, noise, temps, sizes, watch=None):
    """cvae.py:1645-1663 -> (accumulated gradients (T, N, ...), scores (T, E, N), gradient-pass logits (T, L+1, N, C))."""
    real = torch.randn
    torch.randn = Noise(noise, x.dtype)
    try:
        x = x.clone().requires_grad_(True)
        accs, scores, logits = [], [], []
        for t, T in enumerate(temps):
            if watch is not None and t == 0:
                watch['on'] = True
            with torch.enable_grad():
                _, no_temp_logits = net.forward(x, z_output=False)
                X = (no_temp_logits[1:].mean(0) / T).softmax(-1).max(-1)[0].sum()
            if watch is not None:
                watch['on'] = False
            X.backward()
            logits.append(no_temp_logits.detach().clone())
            accs.append(x.grad.detach().clone())
            dx = x.grad.sign()
            row = []
            for eps in sizes:
                with torch.no_grad():
                    _, odin_logits = net.forward(x + eps * dx, z_output=False)
                    row.append((odin_logits[1:].mean(0) / T).softmax(-1).max(-1)[0])
            scores.append(torch.stack(row))
        return torch.stack(accs), torch.stack(scores), torch.stack(logits)
    finally:
        torch.randn = real


def watch_preactivations(net):
    """Record the input of every activation module call while watch['on'] -> list of (N-leading or (L+1, N)-leading) tensors."""
    watch = {'on': False, 'seen': []}

    def hook(mod, args):
        if watch['on']:
            watch['seen'].append(args[0].detach().clone())
    for m in net.modules():
        if isinstance(m, (torch.nn.ReLU, torch.nn.LeakyReLU)):
            m.register_forward_pre_hook(hook)
    return watch


def per_sample(t, N, how):
    """(N, ...) or (L+1, N, ...) -> (N,) reduction `how` over everything but the sample axis."""
    t = t if t.shape[0] == N else t.transpose(0, 1)
    return how(t.reshape(N, -1), 1)[0]


def build(Net, kw, dtype):
    torch.manual_seed(0)
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.eval()
    return net.double() if dtype == torch.float64 else net


def run_case(Net, name, case):
    kw, N = case['net'], case['N']
    L, K = kw['test_latent_sampling'], kw['latent_dim']
    for seed in range(1234, 1334):
        g = torch.Generator().manual_seed(seed)
        x = torch.rand((N, *kw['input_shape']), generator=g)
        noise = torch.randn((len(TEMPS), 1 + len(SIZES), L + 1, N, K), generator=g)
        noise[:, :, 0] = 0
        out = {}
        for dtype, tag in ((torch.float32, '32'), (torch.float64, '64')):
            net = build(Net, kw, dtype)
            net.ODIN_TEMPS, net.ODIN_EPS = list(TEMPS), list(SIZES)
            watch = watch_preactivations(net)
            acc, sc, lg = odin_loop(net, x.to(dtype), noise, TEMPS, SIZES, watch)
            out['acc' + tag], out['scores' + tag], out['pre' + tag] = acc, sc, watch['seen']
            if tag == '32':
                out['logits'] = lg
        pmin = torch.stack([per_sample(p.abs(), N, torch.min) for p in out['pre64']]).min(0)[0]
        perr = torch.stack([per_sample((a.double() - b).abs(), N, torch.max)
                            for a, b in zip(out['pre32'], out['pre64'])]).max(0)[0]
        a32, a64 = out['acc32'].double(), out['acc64']
        flips = float((a32.sign() != a64.sign()).double().mean())
        left_out = int((pmin < perr).sum())
        print(f'{name}: seed {seed}: samples left out {left_out}, sign flips {flips:.5f}')
        if left_out == 0 and flips <= 0.005:
            break
    else:
        raise SystemExit(f'{name}: no seed found')
    T = len(TEMPS)
    err = (a32 - a64).reshape(T, -1).abs().max(1)[0] / a64.reshape(T, -1).abs().max(1)[0]
    names = ['odin-{:.0f}-{:.4f}'.format(t, e) for t in TEMPS for e in SIZES]
    data = dict(x=x.numpy(), eps_noise=noise.numpy(), seed=np.int64(seed), temps=np.asarray(TEMPS, np.float64),
                sizes=np.asarray(SIZES, np.float64), names=np.array(names),
                acc32=out['acc32'].numpy(), acc64=out['acc64'].numpy(), sign=out['acc32'].sign().numpy().astype(np.int8),
                scores32=out['scores32'].numpy(), scores64=out['scores64'].numpy(), logits=out['logits'].numpy(),
                grad_err=err.numpy(), preact_min64=pmin.numpy(), preact_err32=perr.numpy(), flips32=np.float64(flips))
    path = os.path.join(OUT, name + '.npz')
    np.savez_compressed(path, **data)
    print(f'{name}: grad_err {err.tolist()} scores[0] {out["scores32"][0, :, 0].tolist()} -> {path} '
          f'({os.path.getsize(path) / 1024:.0f} KiB)')


def timing(Net):
    kw = dict(get_case('eb2_n8_vib_L2')['net'], classifier=[], test_latent_sampling=16)
    net = build(Net, kw, torch.float32)
    N, L, K = 100, 16, kw['latent_dim']
    temps, sizes = list(Net.ODIN_TEMPS), list(Net.ODIN_EPS)
    g = torch.Generator().manual_seed(7)
    x = torch.rand((N, *kw['input_shape']), generator=g)
    real = torch.randn
    t0 = time.perf_counter()
    x = x.requires_grad_(True)
    for T in temps:                                  # the loop of odin_loop with the generator's own draws
        _, lg = net.forward(x, z_output=False)
        (lg[1:].mean(0) / T).softmax(-1).max(-1)[0].sum().backward()
        dx = x.grad.sign()
        for eps in sizes:
            with torch.no_grad():
                net.forward(x + eps * dx, z_output=False)
    dt = time.perf_counter() - t0
    assert torch.randn is real
    json.dump({'what': 'reference ODIN loop (cvae.py:1645-1663), one batch, full 10 x 21 grid, PyTorch CPU',
               'model': 'vib conv32 K=64 C=10 L=16 batch_norm', 'N': N, 'image_forwards': 220 * N, 'seconds': dt,
               'threads': torch.get_num_threads(), 'machine': platform.machine(), 'python': platform.python_version(),
               'torch': torch.__version__}, open(os.path.join(OUT, 'timing.json'), 'w'), indent=1)
    print(f'reference, one batch of {N}: {dt:.2f} s')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='checkout of the reference (the directory that holds cvae.py)')
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('cases', nargs='*')
    a = ap.parse_args()
    gen_golden.REF = os.path.abspath(a.reference)
    Net = gen_golden.import_reference()
    torch.set_num_threads(8)
    os.makedirs(OUT, exist_ok=True)
    for name, case in cases().items():
        if not a.cases or name in a.cases:
            run_case(Net, name, case)
    if a.timing:
        timing(Net)


if __name__ == '__main__':
    main()
