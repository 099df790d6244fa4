#!/usr/bin/env python3
"""Benchmark of the per-batch joint-CVAE training step on MI355X (BASELINE.json metric: training images/s).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = cvae.py:2429-2461 of the reference on one synthetic batch already resident in HBM:
zero_grad -> evaluate(x, y, with_beta=True) -> total.mean().backward() -> clip_grad_norm_(100) -> Adam, with the
reparameterisation noise drawn on the device.  Workload = BASELINE.json configs[1] (CIFAR-10 conv CVAE, bs=512
per GPU, fp32).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the headline figures.  --full adds what takes runs of its own:
the roofline probes of the dominant kernels and the CPU baseline of the reference's step.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (REPO, os.path.join(REPO, 'joint-vae_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

FLOP_PER_IMAGE = 923.2e6          # conv/linear MACs*2, fwd + bwd, L=1 (decoder runs on 2N latents)
MFMA_F32_PEAK = 157.3e12          # MI355X dense fp32 MFMA, MI355X_MICROARCH.md
MFMA_BF16_PEAK = 2.5e15           # dense bf16 MFMA (same guide)
X3_PRODUCTS = 6                   # bf16 MFMA products per fp32 product in conv_x3.hip (3-way exact operand split)
BATCH_PER_GPU = 512


WORKLOADS = {   # id -> (description, FLOP per image fwd+bwd)   (BASELINE.json configs; the metric is quoted on 2)
    2: ('BASELINE configs[1]: CIFAR-10 3x32x32 conv CVAE (conv32/deconv32, latent_dim=64, C=10, batch_norm=both, '
        'learned sigma, L=1), bs=512 per GPU, fp32, fwd+bwd+clip+Adam', 923.2e6),
    3: ('BASELINE configs[2]: CIFAR-100 3x32x32 conv CVAE, class-conditional gaussian prior C=100, bs=512 per GPU, fp32',
        923.2e6),
    5: ('BASELINE configs[4]: ImageNet-20-shaped 3x64x64 conv CVAE (conv32+/deconv32+, latent_dim=200, C=20), '
        'bs=256 per GPU; --dtype bf16 = bf16 activations + bf16 MFMA from fp32 master weights, f32 = same geometry in fp32',
        5105e6),
}


_ADAM = dict(optim_type='adam', lr=1e-3, weight_decay=3e-5, grad_clipping=100)


def model_kwargs(workload):
    """Constructor arguments of the BASELINE.json configurations (reference `config.ini:137-169`)."""
    C, K, shape, feat, ups = {2: (10, 64, (3, 32, 32), 'conv32', 'deconv32'),
                              3: (100, 64, (3, 32, 32), 'conv32', 'deconv32'),
                              5: (20, 200, (3, 64, 64), 'conv32+', 'deconv32+')}[workload]
    return dict(input_shape=shape, num_labels=C, type='cvae', features=feat, upsampler=ups, encoder=[], decoder=[],
                classifier=[], batch_norm='both', latent_dim=K, latent_sampling=1, test_latent_sampling=1,
                sigma={'value': 1.0, 'learned': True}, gamma=0, beta=1., output_activation='linear',
                prior=dict(distribution='gaussian', init_mean=0., learned_means=True, var_dim='scalar', freeze_means=0),
                optimizer=dict(_ADAM))


def build_model(device, workload=2, test_latent_sampling=1):
    from cvae import ClassificationVariationalNetwork as Net
    torch.manual_seed(0)
    net = Net(**dict(model_kwargs(workload), test_latent_sampling=test_latent_sampling))
    net.to(device)
    net.train()
    return net


def dominant_kernel_roofline(device, reps=20, in_step_ms=None, where='the timed steps'):
    """Largest layer of the step (imager.15: ConvTranspose2d 32->32 5x5 on 1024x32x32x32, 53.69 GFLOP fwd).

    `achieved` = algorithmic FLOPs of one launch / its average duration INSIDE the timed steps (`in_step_ms`: one HIP-event
    pair per step around that launch on its launch stream, recorded by jvae_hip.ops.LaunchProbe; the step launches it with
    the deferred BatchNorm+ReLU of its input applied while staging and the BatchNorm partial sums of its output in the
    epilogue; its weights come packed from the step's pack cache).  `standalone` repeats the same launch `reps` times back
    to back outside the step (its own pack kernel in front of every launch, no neighbours): under 20 consecutive launches of
    the heaviest kernel the chip holds a lower clock than in the step's mix, so that figure is the pessimistic one.

    The layer runs on conv5_x3_kernel (conv_x3.hip): fp32 in / fp32 out, every operand split exactly into three bf16
    terms and each fp32 product accumulated from 6 bf16 MFMA products.  `achieved` counts the ALGORITHMIC fp32 FLOPs;
    `peak` is what the matrix pipes allow for that arithmetic: dense bf16 MFMA peak / 6.  `vs_f32_mfma_peak` relates the
    same rate to the fp32-MFMA peak the north-star target is phrased in (the native fp32 MFMA kernel conv5_fwd_kernel
    reaches 0.69-0.81 of it on this layer; JVAE_X3=0 selects it)."""
    from jvae_hip import ops
    N, C, H = 2 * BATCH_PER_GPU, 32, 32
    spec = ops.ConvSpec(C, C, 5, 1, 2, 0, transposed=True)
    x = torch.randn(N, C, H, H, device=device)
    w = torch.randn(C, C, 5, 5, device=device) * 0.03
    b = torch.zeros(C, device=device)
    aff = (torch.rand(C, device=device) + 0.5, torch.randn(C, device=device) * 0.1, True)
    for _ in range(3):
        ops.conv_fwd_aff_raw(x, w, b, spec, aff, True)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.conv_fwd_aff_raw(x, w, b, spec, aff, True)
    e1.record()
    torch.cuda.synchronize()
    alone = e0.elapsed_time(e1) * 1e-3 / reps
    flops = 2.0 * N * H * H * C * C * 25
    x3 = os.environ.get('JVAE_X3', '1') != '0'
    sec, measured = alone, 'standalone: %d back-to-back launches outside the step' % reps
    if in_step_ms:
        sec = sum(in_step_ms) / len(in_step_ms) * 1e-3
        measured = 'inside %s: %d HIP-event pairs (one per step) around the launch, on its launch stream' % (where, len(in_step_ms))
    traffic, traffic_source = None, None
    for name in (('r05_x3_fwd_pmc.json', 'r04_x3_fwd_pmc.json') if x3 else ('r01_dominant_kernel_pmc.json',)):
        pmc = os.path.join(REPO, 'profiles', name)
        if os.path.exists(pmc):       # HBM bytes per launch from separate rocprofv3 --pmc passes of THIS kernel (not of this run)
            d = json.load(open(pmc))
            traffic = d.get('hbm_bytes_per_launch') or ((d.get('hbm_read_bytes') or 0) + (d.get('hbm_write_bytes') or 0)) or None
            traffic_source = f'profiles/{name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same launch (committed file, not this run)'
            break
    peak = MFMA_BF16_PEAK / X3_PRODUCTS if x3 else MFMA_F32_PEAK
    out = {'bound': 'mfma',
           'kernel': ('conv5_x3_kernel<1,32,2,aff,%s>: imager.15 forward (ConvT 32->32 5x5 s1, 1024x32x32x32), fp32 operands split exactly '
                      'into 3 bf16 terms, 6 %s per fp32 product tile' % ('16x16x32', 'v_mfma_f32_16x16x32_bf16 (K = 2 taps x 16 channels)') if x3 else
                      'conv5_fwd_kernel<1,32,4,1,8,aff>: imager.15 forward (ConvT 32->32 5x5 s1, 1024x32x32x32)'),
           'achieved': flops / sec / 1e12, 'peak': peak / 1e12, 'unit': 'TFLOP/s', 'frac': flops / sec / peak,
           'traffic': traffic, 'traffic_source': traffic_source, 'launch_ms': sec * 1e3, 'measured': measured,
           'algorithmic_flops_per_launch': flops,
           'standalone': {'launch_ms': alone * 1e3, 'achieved': flops / alone / 1e12, 'frac': flops / alone / peak,
                          'note': 'the same launch repeated back to back outside the step, its pack kernel included'}}
    if in_step_ms:
        t = sorted(in_step_ms)
        out['launch_ms_min'], out['launch_ms_max'] = t[0], t[-1]
    if x3:
        out.update({'peak_definition': 'dense bf16 MFMA 2500 TFLOP/s / 6 bf16 products per fp32 product',
                    'bf16_mfma_achieved': X3_PRODUCTS * flops / sec / 1e12, 'vs_f32_mfma_peak': flops / sec / MFMA_F32_PEAK})
    return out


def wgrad_kernel_roofline(device, reps=20):
    """The second MFMA-bound family of the step: the weight gradient of the same layer (imager.15, 53.69 GFLOP) on
    conv5_wgrad_x3_kernel + its slab fold, launched through the C ABI as the step launches it (deferred BatchNorm on the layer
    input, accumulation into an existing gradient), timed with HIP events on the launch stream.  Same peak definition as
    `roofline`; HBM traffic from profiles/r05_wgrad_x3_pmc.json (committed rocprofv3 --pmc passes, not this run)."""
    from jvae_hip import ops
    N, C, H = 2 * BATCH_PER_GPU, 32, 32
    spec = ops.ConvSpec(C, C, 5, 1, 2, 0, transposed=True)
    x = torch.randn(N, C, H, H, device=device)
    gy = torch.randn(N, C, H, H, device=device)
    gw = torch.zeros(C, C, 5, 5, device=device)
    aff = (torch.rand(C, device=device) + 0.5, torch.randn(C, device=device) * 0.1, True)
    for _ in range(3):
        ops.conv_wgrad_raw(x, gy, spec, gw.shape, False, gw, None, aff)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.conv_wgrad_raw(x, gy, spec, gw.shape, False, gw, None, aff)
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) * 1e-3 / reps
    flops = 2.0 * N * H * H * C * C * 25
    peak = MFMA_BF16_PEAK / X3_PRODUCTS
    traffic, src = None, None
    for name in ('r05_wgrad_x3_pmc.json', 'r04_wgrad_x3_pmc.json'):
        pmc = os.path.join(REPO, 'profiles', name)
        if os.path.exists(pmc):
            d = json.load(open(pmc))
            traffic = ((d.get('hbm_read_bytes') or 0) + (d.get('hbm_write_bytes') or 0)) or None
            src = 'profiles/%s (committed file, not this run)' % name
            break
    return {'bound': 'mfma', 'kernel': 'conv5_wgrad_x3_kernel<1,32,0,aff,16x16x32> + wgrad_reduce4_kernel: imager.15 weight gradient '
                                       '(1024x32x32x32 activations), both operands split exactly into 3 bf16 terms',
            'achieved': flops / sec / 1e12, 'peak': peak / 1e12, 'unit': 'TFLOP/s', 'frac': flops / sec / peak,
            'traffic': traffic, 'traffic_source': src, 'launch_ms': sec * 1e3}


HBM_PEAK = 8.0e12                  # MI355X HBM3E spec (6.3e12 measured achievable), MI355X_MICROARCH.md


def bn_backward_hbm(device, reps=20):
    """The HBM-bound side of the step (north_star asks for achieved-HBM evidence): BatchNorm(+ReLU) backward of the largest
    activation (imager.16: 1024 x 32 x 32 x 32 fp32), launched ALONE, timed with HIP events on the launch stream.
    Algorithmic bytes: the reduction reads dy and x (8 B/element), the apply pass reads dy and x and writes dx (12 B)."""
    from jvae_hip import lib as L
    lib = L.load()
    N, C, H = 2 * BATCH_PER_GPU, 32, 32
    x = torch.randn(N, C, H, H, device=device)
    dy = torch.randn_like(x)
    dx = torch.empty_like(x)
    gamma, beta = torch.rand(C, device=device) + 0.5, torch.randn(C, device=device) * 0.1
    mean, invstd = torch.zeros(C, device=device), torch.ones(C, device=device)
    gg, gb = torch.empty(C, device=device), torch.empty(C, device=device)
    ws = L.workspace(lib.jvae_bn_workspace_bytes(C), device)

    def launch():
        L.check(lib.jvae_bn_bwd_f32(L.ptr(dy), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(mean), L.ptr(invstd), L.ptr(dx),
                                    L.ptr(gg), L.ptr(gb), 0, N, C, H * H, 1, L.ptr(ws), ws.numel(), L.stream_ptr()), 'jvae_bn_bwd_f32')
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    sec = e0.elapsed_time(e1) * 1e-3 / reps
    nbytes = 20.0 * x.numel()
    out = {'bound': 'hbm', 'kernel': 'bn_bwd_reduce_kernel + bn_bwd_apply_kernel: BatchNorm+ReLU backward of imager.16 (1024x32x32x32 fp32), alone',
           'achieved': nbytes / sec / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': nbytes / sec / HBM_PEAK,
           'launch_ms': sec * 1e3, 'algorithmic_bytes': nbytes}
    for name in ('r05_bench_kernel_stats.json', 'r04_bench_kernel_stats.json'):
        prof = os.path.join(REPO, 'profiles', name)
        if not os.path.exists(prof):
            continue                  # the same family inside the step (two streams share the CUs): committed rocprofv3 summary
        d = json.load(open(prof))
        if d.get('bn_bwd_ms_per_step'):
            out['in_step'] = {'ms_per_step': d['bn_bwd_ms_per_step'], 'achieved': 20.0 * 135.7e6 * 4 / 4 / (d['bn_bwd_ms_per_step'] * 1e-3) / 1e9,
                              'unit': 'GB/s', 'source': 'profiles/%s (rocprofv3 --kernel-trace of bench.py)' % name}
        break
    return out


def cpu_baseline(max_seconds=60.0):
    """The CPU oracle (PyTorch-CPU restatement of the reference step, pinned to the reference's goldens) on the host
    cores, bounded samples of the same workload.  bs=512 (the metric's batch) is timed at several intra-op thread counts -
    1 warm-up + 2 steps each, about a minute in all - and the BEST is reported with its thread count as `cores` (VERDICT r3:
    PyTorch's default of one thread per logical CPU, 128-256 on the GPU boxes, oversubscribes MKL-DNN and ran the same code
    2.6x slower than 8 threads do); the whole sweep stays in the JSON.  bs=32 (what the reference's unmodified train.py would
    run: its max_batch_sizes is hard-wired to 32) is timed at the best count of the sweep and at 8 threads."""
    import platform
    import statistics
    from oracle import jvae_oracle as O
    from oracle.cases import full_config
    from oracle.det_init import det_inputs
    model = platform.processor() or ''
    try:
        for line in open('/proc/cpuinfo'):
            if line.startswith('model name'):
                model = line.split(':', 1)[1].strip()
                break
    except OSError:
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        usable = os.cpu_count() or 1
    default_threads = torch.get_num_threads()

    def run(bs, steps, budget, warm):
        kw = full_config(2, bs)['net']
        sp = O.make_spec(**kw)
        P = O.init_state(sp, seed=0)
        opt = O.AdamState(sp)
        x, y, eps = det_inputs(bs, kw['input_shape'], 10, 1, 64, seed=1234)
        for _ in range(warm):
            O.train_step(sp, P, opt, x, y, eps)               # warm-up
        times, t_start = [], time.time()
        while len(times) < steps and (not times or time.time() - t_start < budget):
            t0 = time.time()
            O.train_step(sp, P, opt, x, y, eps)
            times.append(time.time() - t0)
        med = statistics.median(times)
        return {'batch': bs, 'threads': torch.get_num_threads(), 'steps': len(times), 'median_s_per_step': med,
                'min_s_per_step': min(times), 'images_per_s': bs / med}
    t_sweep = time.time()
    sweep = []
    try:
        for nt in (8, 16, 32, 64, 128):
            if nt > max(usable, 8) or (sweep and time.time() - t_sweep > max_seconds):
                break
            torch.set_num_threads(nt)
            sweep.append(run(BATCH_PER_GPU, 2, max_seconds / 4, 1))
        best = max(sweep, key=lambda r: r['images_per_s'])
        torch.set_num_threads(best['threads'])
        small = [run(32, 10, 4.0, 3)]
        if best['threads'] != 8:
            torch.set_num_threads(8)
            small.append(run(32, 10, 4.0, 3))
    finally:
        torch.set_num_threads(default_threads)
    small_best = max(small, key=lambda r: r['images_per_s'])
    return {'value': best['images_per_s'], 'unit': 'images/s', 'cores': best['threads'], 'kind': 'port',
            'sample': f'bs={BATCH_PER_GPU} train steps of config 2 with the PyTorch-CPU oracle, 2 timed steps after 1 warm-up at each of '
                      f'{[r["threads"] for r in sweep]} intra-op threads, best median reported (cores = its thread count); '
                      f'{os.cpu_count()} logical CPUs visible, {usable} usable by this process, CPU: {model}',
            'cpu_model': model, 'logical_cpus': os.cpu_count(), 'usable_cpus': usable, 'torch_default_threads': default_threads,
            'thread_sweep_bs512': sweep, 'bs512': best, 'bs32': small_best, 'bs32_runs': small}


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, net, losses, meas):
    """--dump-outputs: what a caller of the timed step holds after its last call, one float32 / float64 .npy file per array -
    the losses it returned (`loss.<key>`), its measures (`measure.<key>`) and the model state it updated in place
    (`state.<key>`: parameters, BatchNorm running statistics; integer counters as float64)."""
    import numpy as np
    arrays = {}
    for k, v in losses.items():
        arrays['loss.' + k] = v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float64)
    for k, v in (meas.items() if meas is not None else ()):
        arrays['measure.' + k] = np.asarray(v, dtype=np.float64)
    for k, v in net.state_dict().items():
        v = v.detach()
        arrays['state.' + k] = (v.float() if v.is_floating_point() else v.double()).cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        raise SystemExit('--dump-outputs: %d bytes exceed the %d-byte budget' % (total, DUMP_MAX_BYTES))
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + '.npy'), a)


def _watchdog(seconds):
    """Abort (exit code 3, stacks dumped) instead of hanging the box if the process makes no progress for `seconds`."""
    import faulthandler
    faulthandler.dump_traceback_later(seconds, exit=True)
    return faulthandler


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--full', action='store_true',
                    help='also the roofline probes of the dominant kernels and the CPU baseline (runs of their own beside the timed steps)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the losses, measures and model state of the last timed step as DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: leave the CPU baseline out')
    ap.add_argument('--batch', type=int, default=None, help='diagnostics only: per-GPU batch (the metric is defined at 512)')
    ap.add_argument('--sync-bn', action='store_true', help='BatchNorm statistics over all ranks (default: per rank)')
    ap.add_argument('--graph', action='store_true',
                    help='(default since round 5) replay the step as a captured HIP graph - ClassificationVariationalNetwork.graph_train_step: '
                         'one host call per step, three when data parallel; the same kernels as the eager loop')
    ap.add_argument('--eager', action='store_true',
                    help='time the eager loop (train_step: ~180 launches per step enqueued from Python, ~3 ms of host time per step) '
                         'instead of the graph replay')
    ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'], help='bf16: the mixed-precision mode of BASELINE configs[4]')
    ap.add_argument('--workload', default='2', choices=[str(k) for k in sorted(WORKLOADS)] + ['eval'],
                    help="diagnostics: other BASELINE configs; 'eval' = the label-free evaluation pass (SURVEY.md §8f-1): config 2, "
                         "N=512 images, L=128 latent draws (decoder batch 66 048) per step")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error('--steps must be at least 1')
    eval_mode = a.workload == 'eval'
    a.workload = 2 if eval_mode else int(a.workload)
    # What is timed (round 5): the captured step.  The eager loop needs ~3.0 ms of host time per 3.6 ms step and may run at most one
    # step ahead of the GPU (the NaN flag of the previous update is read before every backward, as the reference does), so any
    # host hiccup of a few ms lands in the wall clock: the driver's r04 line read mean 3.87 / median 3.67 ms for that reason.
    # The replay needs 0.4 ms of host time per step.  --eager times the loop of train_step() calls instead.
    a.graph = not a.eager and not eval_mode
    fh = _watchdog(900)
    if a.batch is None:
        a.batch = 256 if a.workload == 5 else BATCH_PER_GPU
    side, ncls = (64, 20) if a.workload == 5 else (32, 100 if a.workload == 3 else 10)

    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        ndev = torch.cuda.device_count()
        backend = os.environ.get('JVAE_BENCH_BACKEND', 'nccl')       # 'gloo': rehearsal of the DP path on one GPU
        local = local % max(ndev, 1)
        torch.cuda.set_device(local)
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        else:
            dist.init_process_group(backend)
    device = torch.device('cuda', local)
    torch.cuda.set_device(device)

    net = build_model(device, a.workload, test_latent_sampling=128 if eval_mode else 1)
    if a.dtype == 'bf16':
        net.set_compute_dtype('bf16')
    if world > 1:
        net.set_distributed(world)          # broadcasts rank 0's state, offsets the epsilon generator per rank
        if a.sync_bn:
            net.set_sync_batchnorm(world)
    g = torch.Generator(device=device).manual_seed(1234 + rank)
    x = torch.rand(a.batch, 3, side, side, device=device, generator=g)
    y = torch.randint(0, ncls, (a.batch,), device=device, generator=g)

    def sync():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    meas = None
    if eval_mode:
        net.eval()

        def one_step(i, meas):
            with torch.no_grad():
                _, _, losses, meas = net.evaluate(x, batch=i, current_measures=meas)
            return losses, meas
    elif a.graph:
        replay = net.graph_train_step(x, y)

        def one_step(i, meas):
            return replay(x, y)
    else:
        def one_step(i, meas):
            return net.train_step(x, y, batch=i, current_measures=meas)
    for i in range(a.warmup):
        _, meas = one_step(i, meas)
    probe = None
    want_probe = (a.full and a.workload == 2 and a.dtype == 'f32' and not eval_mode
                  and os.environ.get('JVAE_BENCH_NO_PROBES') != '1')
    if want_probe:
        # the dominant kernel (imager.15 forward: ConvT 32->32 5x5 s1 on the 2N x 32 x 32 x 32 decoder activation) timed INSIDE
        # running steps: one HIP-event pair per step around that launch, on the stream it is launched on.  Eager timing: inside the
        # timed steps; graph replay (no events inside a captured graph): inside eager steps run right after the timed region.
        from jvae_hip import ops as _ops
        probe = _ops.FWD_AFF_PROBE = _ops.LaunchProbe(lambda sp, N, H: sp.transposed and sp.s == 1 and sp.cin == 32 and sp.cout == 32
                                                      and H == 32 and N == 2 * a.batch)
    sync()
    if probe is not None and not a.graph:
        probe.armed = True
    # per-step HIP events on the launch stream (median / min are reported beside the contract's mean over the K steps)
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
    host_marks = [0.0] * (a.steps + 1)
    t0 = time.time()
    marks[0].record()
    host_marks[0] = t0
    for i in range(a.steps):
        losses, meas = one_step(i, meas)
        marks[i + 1].record()
        host_marks[i + 1] = time.time()
    sync()
    dt = time.time() - t0
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, net, losses, meas)
    probe_steps = 0
    if probe is not None and a.graph:
        # the instrumented EAGER steps behind the timed replay (same model, same batch, same kernels in the same order)
        losses = meas = None
        m2 = None
        for i in range(3):
            _, m2 = net.train_step(x, y, batch=i, current_measures=m2)
        torch.cuda.synchronize()
        probe.armed = True
        probe_steps = max(10, min(a.steps, 40))
        for i in range(probe_steps):
            losses, m2 = net.train_step(x, y, batch=3 + i, current_measures=m2)
        torch.cuda.synchronize()
    if probe is not None:
        probe.armed = False
    # in launch order (which step is the slow one must stay visible); sorted only for the median / min below
    per_step_order = [marks[i].elapsed_time(marks[i + 1]) for i in range(a.steps)]
    per_step_host = [(host_marks[i + 1] - host_marks[i]) * 1e3 for i in range(a.steps)]
    per_step = sorted(per_step_order)
    if dist is not None:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t)
    value = world * a.batch * a.steps / dt
    final_loss = float(losses['total'].detach().mean())
    replicas = None
    if dist is not None and not eval_mode:
        # data-parallel replicas must hold bit-identical parameters after the timed steps: exact integer checksum of the
        # parameters' bit patterns, gathered over the ranks (BatchNorm running statistics are per-rank by design)
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()]).contiguous()
        chk = flat.view(torch.int32).to(torch.int64).sum().reshape(1)
        if os.environ.get('JVAE_BENCH_BACKEND', 'nccl') != 'nccl':
            chk = chk.cpu()                       # gloo gathers host tensors
        got = [torch.zeros_like(chk) for _ in range(world)]
        dist.all_gather(got, chk)
        replicas = [int(t) for t in got]

    if rank == 0:
        out = {'metric': 'evaluation_images_per_sec (diagnostic)' if eval_mode else 'training_images_per_sec', 'value': value,
               'unit': 'images/s', 'n_gpus': world,
               'steps': a.steps, 'warmup': a.warmup, 'ms_per_step': dt / a.steps * 1e3,
               'ms_per_step_median': per_step[len(per_step) // 2], 'ms_per_step_min': per_step[0],
               'ms_per_step_max': per_step[-1],
               'per_step_ms': [round(t, 4) for t in per_step_order],
               'per_step_host_enqueue_ms': [round(t, 4) for t in per_step_host],
               'drain_ms_after_last_enqueue': round((t0 + dt - host_marks[-1]) * 1e3, 4),
               'timing': 'value / ms_per_step: wall clock over the K steps between barrier+synchronize (max over ranks); '
                         'median / min: HIP events around every step on the launch stream of rank 0',
               'higher_is_better': True,
               'scaling': 'weak', 'vs_baseline': None, 'dtype': a.dtype, 'data': 'synthetic',
               'config': {'workload': ('label-free evaluation pass of BASELINE configs[1] (all-class losses + importance-weighted bound), '
                                       'N=512 images x L=128 latent draws per step, eval-mode BatchNorm, fp32'
                                       if eval_mode else WORKLOADS[a.workload][0]),
                          'global_batch': world * a.batch, 'parallelism': f'dp{world}',
                          'launch': ('HIP graph replay (ClassificationVariationalNetwork.graph_train_step: the whole step captured once, '
                                     'one host call per step' + (', two graphs with the gradient all-reduce between them' if world > 1 else '') +
                                     '; --eager times the loop of train_step() calls)') if (a.graph and not eval_mode) else 'eager',
                          'bn_statistics': 'synchronised over ranks' if (a.sync_bn and world > 1) else 'per-rank (local)',
                          'arithmetic': ('fp32 operands, products and accumulation everywhere; the stride-1 and 4-phase 5x5 layers '
                                         'accumulate each fp32 product from 6 bf16 MFMA products of exactly 3-way split operands (dropped terms < 2^-24 of '
                                         'the product: below fp32 rounding) '
                                         '(csrc/conv_x3.hip; JVAE_X3=0: fp32 MFMA in every layer)'
                                         if (a.dtype == 'f32' and os.environ.get('JVAE_X3', '1') != '0') else
                                         ('fp32 MFMA in every layer' if a.dtype == 'f32' else
                                          'bf16 activations / MFMA operands, fp32 accumulation, statistics, losses, optimiser'))},
               'final_loss': final_loss}
        if replicas is not None:
            out['replicas_identical'] = len(set(replicas)) == 1
            out['replica_param_checksums'] = replicas
            out['config']['backend'] = os.environ.get('JVAE_BENCH_BACKEND', 'nccl')
        if not eval_mode:
            # NOT a utilisation figure: algorithmic conv/linear FLOPs per second divided by the fp32-MFMA peak the north-star
            # target (>= 0.5) is phrased in; most of those FLOPs run on the bf16 pipes (6 bf16 products per fp32 product)
            out['step_throughput_vs_f32_mfma_peak'] = value / world * WORKLOADS[a.workload][1] / (MFMA_F32_PEAK if a.dtype == 'f32' else MFMA_BF16_PEAK)
        # the roofline probes and the CPU baseline belong to the headline config (JVAE_BENCH_NO_PROBES=1: kernel traces of the step alone)
        if want_probe:
            out['roofline'] = dominant_kernel_roofline(device, in_step_ms=probe.times_ms() if probe is not None else None,
                                                       where=('%d eager train_step() calls run right after the timed graph-replay region (events cannot be '
                                                              'recorded inside a captured graph)' % probe_steps) if a.graph else 'the timed steps')
            out['roofline_wgrad'] = wgrad_kernel_roofline(device)
            out['roofline_hbm'] = bn_backward_hbm(device)
        if a.full and world == 1 and not a.no_cpu_baseline and a.workload == 2 and a.dtype == 'f32' and not eval_mode:
            out['cpu_baseline'] = cpu_baseline()
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    fh.cancel_dump_traceback_later()


if __name__ == '__main__':
    main()
