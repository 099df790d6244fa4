"""GPU box: the 3x3 padding-1 layers of vgg11 features (3x64x64), ivgg (64x64 output), conv32- (3x32x32) and deconv32- in the
bf16 mode, direction by direction, two ways: on the native B8 kernel, and on the path the mode took before it had one (B8 ->
fp32 conversion, fp32 unfold + GEMM, conversion back to B8).  TF/s = the layer's FLOPs over the native kernel time.

    python tools/conv_bench_b8_3x3.py                 per-layer table (B=256 images, env B)
    python tools/conv_bench_b8_3x3.py --step [REPO]   ms per train_step of a vgg11 + ivgg cvae (bs B, 3x64x64) in bf16 and fp32,
                                                      importing the package from REPO (default: this tree; a build of another
                                                      revision gives the before / after pair on one box)
"""
import os, sys, json, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = int(os.environ.get('B', 256))
LAYERS = [  # name, N, cin, cout, s, op, transposed, H
    ('vgg.0', B, 3, 64, 1, 0, False, 64), ('vgg.1', B, 64, 128, 1, 0, False, 32), ('vgg.2', B, 128, 256, 1, 0, False, 16),
    ('vgg.3', B, 256, 256, 1, 0, False, 16), ('vgg.4', B, 256, 512, 1, 0, False, 8), ('vgg.5', B, 512, 512, 1, 0, False, 8),
    ('vgg.6', B, 512, 512, 1, 0, False, 4),
    ('ivgg.0', 2 * B, 64, 128, 1, 0, False, 8), ('ivgg.1', 2 * B, 128, 64, 1, 0, False, 16),
    ('ivgg.2', 2 * B, 64, 32, 1, 0, False, 32), ('ivgg.3', 2 * B, 32, 3, 1, 0, False, 64),
    ('c32-.0', B, 3, 32, 1, 0, False, 32), ('c32-.1', B, 32, 32, 1, 0, False, 32), ('c32-.3', B, 32, 32, 2, 0, False, 32),
    ('c32-.4', B, 32, 64, 1, 0, False, 16), ('c32-.7', B, 64, 64, 2, 0, False, 16),
    ('d32-.1', 2 * B, 64, 64, 1, 0, True, 8), ('d32-.4', 2 * B, 64, 64, 2, 1, True, 8), ('d32-.5', 2 * B, 64, 32, 1, 0, True, 16),
    ('d32-.8', 2 * B, 32, 32, 2, 1, True, 16), ('d32-.9', 2 * B, 32, 32, 1, 0, True, 32)]


def timeit(f, reps=10):
    import torch
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def layers():
    sys.path[:0] = [REPO, os.path.join(REPO, 'joint-vae_amd')]
    import torch
    from jvae_hip import ops, ops_b8
    rows, tot = [], {'native': 0., 'fallback': 0.}
    for name, N, cin, cout, s, op, tr, H in LAYERS:
        spec = ops.ConvSpec(cin, cout, 3, s, 1, op, tr)
        oh, ow = spec.out_hw(H, H)
        xf = torch.randn(N, cin, H, H, device='cuda')
        gyf = torch.randn(N, cout, oh, ow, device='cuda')
        x, gy = ops_b8.pack(xf), ops_b8.pack(gyf)
        wshape = (cin, cout, 3, 3) if tr else (cout, cin, 3, 3)
        w = torch.randn(wshape, device='cuda') * 0.05
        b = torch.zeros(cout, device='cuda')
        flops = 2.0 * N * (H * H if tr else oh * ow) * cin * cout * 9
        mask = ops_b8.native_mask(spec, N, H, H)
        native = {1: lambda: ops_b8.conv_fwd_raw(x, w, b, spec, want_stats=True),
                  2: lambda: ops_b8.conv_dgrad_raw(gy, w, spec, N, H, H),
                  4: lambda: ops_b8.conv_wgrad_raw(x, gy, spec, wshape, False)}
        # the bf16 mode without a 3x3 kernel: convert, run the fp32 unfold + GEMM path, convert back
        fallback = {1: lambda: ops_b8.pack(ops.conv_fwd_raw(ops_b8.unpack(x, cin), w, b, spec)),
                    2: lambda: ops_b8.pack(ops.conv_dgrad_raw(ops_b8.unpack(gy, cout), w, spec, (N, cin, H, H))),
                    4: lambda: ops.conv_wgrad_raw(ops_b8.unpack(x, cin), ops_b8.unpack(gy, cout), spec, wshape, False)}
        row = {'layer': name, 'N': N, 'cin': cin, 'cout': cout, 'stride': s, 'transposed': tr, 'H': H, 'GFLOP': flops / 1e9}
        for bit, d in ((1, 'fwd'), (2, 'dgrad'), (4, 'wgrad')):
            tf = timeit(fallback[bit])
            row[d + '_fallback_us'] = round(tf, 1)
            tot['fallback'] += tf
            if mask & bit:
                tn = timeit(native[bit])
                tot['native'] += tn
                row[d + '_native_us'] = round(tn, 1)
                row[d + '_native_TFs'] = round(flops / tn / 1e6, 1)
                row[d + '_speedup'] = round(tf / tn, 2)
            else:
                tot['native'] += tf
                row[d + '_native_us'] = None
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({'sum_native_or_fallback_ms': tot['native'] / 1e3, 'sum_fallback_ms': tot['fallback'] / 1e3}), flush=True)


def step(repo, steps=20, warmup=5):
    """ms per train_step of the vgg11 + ivgg model, bf16 and fp32 (the package imported from `repo`)."""
    sys.path[:0] = [repo, os.path.join(repo, 'joint-vae_amd')]
    import torch
    from oracle.cases import get_case
    from oracle.det_init import load_det_state
    from cvae import ClassificationVariationalNetwork as Net
    kw = get_case('c5_n4')['net']
    kw.update(features='vgg11', upsampler='ivgg', latent_dim=256)
    torch.manual_seed(0)
    x = torch.rand(B, *kw['input_shape'], device='cuda')
    y = torch.randint(0, kw['num_labels'], (B,), device='cuda')
    out = {'repo': repo, 'B': B}
    for dtype in ('bf16', 'fp32', 'bf16'):
        net = Net(**kw)
        load_det_state(net, seed=0)
        net.to('cuda').train()
        net.set_compute_dtype(dtype)
        for _ in range(warmup):
            net.train_step(x, y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            net.train_step(x, y)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out.setdefault(dtype + '_ms_per_step', []).append(round(ms, 2))
        del net
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--step':
        step(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else REPO)
    else:
        layers()
