"""bench.py at one GPU as it is run for every change: a plain run carries the headline figures only (the roofline probes and the
CPU baseline are --full's), and --dump-outputs writes the last timed step's losses, measures and model state - the same
arrays bit for bit from run to run, float32 / float64, within the 64 MB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    res = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1'] + list(args), cwd=REPO,
                         capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(600)
def test_plain_bench_dumps_the_last_timed_step_reproducibly(tmp_path):
    dirs = [tmp_path / 'a', tmp_path / 'b']
    runs = [_bench('--steps', '3', '--warmup', '1', '--dump-outputs', str(d)) for d in dirs]
    for d in runs:
        assert d['metric'] == 'training_images_per_sec' and d['unit'] == 'images/s' and d['higher_is_better'] is True
        assert d['dtype'] == 'f32' and d['steps'] == 3 and d['warmup'] == 1
        assert d['value'] > 0 and abs(d['value'] - 512 * 3 / (d['ms_per_step'] * 3e-3)) < 1e-6 * d['value']
        assert not {'roofline', 'roofline_wgrad', 'roofline_hbm', 'cpu_baseline'} & set(d)
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert 'loss.total.npy' in names and 'measure.rmse.npy' in names and 'state.features.0.weight.npy' in names
    total = 0
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert a.dtype == b.dtype and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    # the dumped losses are those of the last timed step: the result line's final_loss is their mean
    tot = np.load(dirs[0] / 'loss.total.npy')
    assert tot.shape == (512,) and abs(float(tot.mean(dtype=np.float64)) - runs[0]['final_loss']) <= 1e-5 * abs(runs[0]['final_loss'])
