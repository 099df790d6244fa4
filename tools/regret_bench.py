#!/usr/bin/env python3
"""Time cvae.likelihood_regret on config 2 of BASELINE.json (CIFAR-10 conv CVAE, conv32 / deconv32, K = 64, BatchNorm) at
N = 512 for every (steps, lr) pair of REGRET_PARAMS, one GPU, and in the same process, interleaved call by call, the same loop
with the step between two decoder passes COMPOSED from the ops that existed before the fused launch: ops.latent under autograd
(its backward gives d J / d (mu, lv_raw)), ops.adam_step on mu and on lv_raw, ops.latent for the next draw.

    python tools/regret_bench.py [--calls 15] [--warmup 3] [--n 512] [--out profiles/regret_bench.json]

HIP events around every call on the launch stream; medians after the warm-up.  Per pair: ms per batch and per iteration, fused
and composed; the share of a batch that is decoder forward plus input gradient (`_regret_objective` with gradient, timed alone,
times the steps); and the step alone - 100 back-to-back steps between two events - in microseconds, fused and composed.
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def event_ms(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def composed_refine(ops):
    """ops.latent_refine's interface on the ops of the parent commit (lv is not refreshed: the timed loop does not read it)."""
    def refine(mu, raw, lv, y, means, T, *, eps_cur=None, dz=None, state=None, step=0, lr=0., eps_next=None, **kw):
        means, T = means.detach(), T.detach()
        if dz is not None:
            with torch.enable_grad():
                a = mu.detach().requires_grad_(True)
                b = (mu if raw is None else raw).detach().requires_grad_(raw is not None)
                _, z, kl, _, _, _ = ops.latent(a, b, eps_cur, y, means, T, **kw)
                grads = torch.autograd.grad([z, kl], [a] + ([b] if raw is not None else []), [dz, torch.ones_like(kl)])
            ops.adam_step(mu, grads[0], state[0], state[1], lr, 0.9, 0.999, 1e-8, 0., step)
            if raw is not None:
                ops.adam_step(raw, grads[1], state[2], state[3], lr, 0.9, 0.999, 1e-8, 0., step)
        if eps_next is None:
            return None
        out = ops.latent(mu, mu if raw is None else raw, eps_next, y, means, T, **kw)
        return out[1], out[2], out[3], out[4]
    return refine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from cvae import ClassificationVariationalNetwork as Net
    from jvae_hip import ops
    from oracle.cases import full_config
    from oracle.det_init import load_det_state
    dev = 'cuda:0'
    kw = full_config(2, a.n)['net']
    net = Net(**kw)
    load_det_state(net, seed=0)
    net.to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(a.n, *kw['input_shape'], device=dev, generator=g)
    y = torch.randint(0, kw['num_labels'], (a.n,), device=dev, generator=g)
    fused, composed = ops.latent_refine, composed_refine(ops)
    K, L = kw['latent_dim'], net.latent_sampling

    def loop(step_fn, steps, lr):
        ops.latent_refine = step_fn
        try:
            return net.likelihood_regret(x, y, steps=steps, lr=lr)
        finally:
            ops.latent_refine = fused

    # the decoder's part of one iteration and the step alone, on tensors of the loop's shapes
    pr = net.encoder.prior
    mu, raw = torch.randn(a.n, K, device=dev, generator=g), torch.randn(a.n, K, device=dev, generator=g)
    eps = torch.randn(2, L + 1, a.n, K, device=dev, generator=g)
    eps[:, 0] = 0
    lab, means, T = pr._kernel_operands(y, a.n, dev)
    pk = dict(prior=pr.distribution, var_dim=pr.var_dim, tau=pr._tau, alpha=pr._alpha_k, sampled=True, forced_lv=None)
    lv = torch.empty_like(mu)
    z, kl = fused(mu, raw, lv, lab, means, T, eps_next=eps[0], **pk)[:2]
    sg = net.sigma.detach()
    kind = ops.SIGMA_LOG if net.sigma.is_log else ops.SIGMA_VALUE
    frozen = [p for p in net.parameters() if p.requires_grad]
    from jvae_hip import lib as _lib

    def objective():
        return net._regret_objective(z, kl, x, sg, kind, True)
    # as inside the loop: weights frozen, ONE span of constant weights around all the passes
    for p in frozen:
        p.requires_grad_(False)
    _lib.span_hold += 1
    try:
        with torch.no_grad(), net._constant_weights(x):
            dz = objective()[1]
            obj_ms = [event_ms(objective) for _ in range(a.warmup + a.calls)][a.warmup:]
    finally:
        _lib.span_hold -= 1
        for p in frozen:
            p.requires_grad_(True)

    def steps_alone(step_fn, reps=100):
        state = ops.latent_refine_state(mu)
        m, r = mu.clone(), raw.clone()

        def run():
            with torch.no_grad():
                for i in range(reps):
                    step_fn(m, r, lv, lab, means, T, eps_cur=eps[0], dz=dz, state=state, step=i + 1, lr=1e-4, eps_next=eps[1], **pk)
        return 1e3 * float(np.median([event_ms(run) for _ in range(a.warmup + 5)][a.warmup:])) / reps
    step_us = {'fused': steps_alone(fused), 'composed': steps_alone(composed)}

    out = {'metric': 'likelihood_regret_ms', 'model': 'cvae conv32/deconv32 K=64 C=10 L=%d batch_norm (BASELINE config 2)' % L,
           'N': a.n, 'calls': a.calls, 'warmup': a.warmup, 'timing': 'HIP events around each call on the launch stream; medians',
           'decoder_forward_plus_gradient_ms': float(np.median(obj_ms)), 'step_alone_us': step_us,
           'step_alone_fused_over_composed': step_us['fused'] / step_us['composed'], 'pairs': []}
    for steps, lr in net.REGRET_PARAMS:
        ms = {'fused': [], 'composed': []}
        for i in range(a.warmup + a.calls):                     # interleaved: fused, composed, fused, ...
            for name, fn in (('fused', fused), ('composed', composed)):
                t = event_ms(lambda: loop(fn, steps, lr))
                if i >= a.warmup:
                    ms[name].append(t)
        f, c = float(np.median(ms['fused'])), float(np.median(ms['composed']))
        out['pairs'].append({'steps': steps, 'lr': lr, 'ms_per_batch': f, 'ms_per_iteration': f / steps,
                             'ms_per_batch_min_max': [float(np.min(ms['fused'])), float(np.max(ms['fused']))],
                             'composed_ms_per_batch': c, 'composed_ms_per_iteration': c / steps, 'fused_over_composed': f / c,
                             'decoder_share': steps * float(np.median(obj_ms)) / f})
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
