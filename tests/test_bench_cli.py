"""bench.py's command line: --dump-outputs (what the last timed step computed, on disk, bounded in size, reproducible) and the
plain run, which reports the headline and nothing that needs a leg of its own (those are behind --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_budget_and_fixed_sample(tmp_path, monkeypatch):
    """Arrays within their share are written whole; a larger one is replaced by a sample of its flattened elements that is
    the same on every call; float64 stays float64, everything else becomes float32; the files stay within the budget."""
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 3 * 4096)
    g = torch.Generator().manual_seed(5)
    arrays = {'big': torch.randn(64, 100, generator=g), 'small': torch.randn(7, 3, generator=g, dtype=torch.float64),
              'half': torch.randn(16, generator=g).half(), 'scalar': torch.tensor(2.5)}
    w1 = bench._dump_outputs(str(tmp_path / 'a'), arrays)
    w2 = bench._dump_outputs(str(tmp_path / 'b'), arrays)
    assert w1 == w2 and sorted(w1) == ['big', 'half', 'scalar', 'small']
    assert w1['big']['sampled'] and w1['big']['shape'] == [64, 100] and w1['small']['sampled'] is None
    total = 0
    for name in w1:
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert np.array_equal(a, b)
        total += os.path.getsize(tmp_path / 'a' / f'{name}.npy')
    assert total <= bench.DUMP_BYTES
    big = np.load(tmp_path / 'a' / 'big.npy')
    assert big.ndim == 1 and big.size == w1['big']['sampled'] and np.isin(big, arrays['big'].numpy().reshape(-1)).all()
    assert np.load(tmp_path / 'a' / 'small.npy').dtype == np.float64
    assert np.array_equal(np.load(tmp_path / 'a' / 'half.npy'), arrays['half'].float().numpy())
    assert np.load(tmp_path / 'a' / 'scalar.npy').shape == ()


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    """Two plain runs of the default C2 workload with --dump-outputs: the line carries the headline fields and `steps` as
    asked, none of the --full legs, and both runs write the same outputs bit for bit (the gradients of 4096 x 512 points
    are larger than their share: a fixed sample of them), within 64 MB."""
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'LOCAL_WORLD_SIZE', 'BENCH_SELF_LAUNCH'):
        env.pop(k, None)
    dumps = []
    for i in range(2):
        out = tmp_path / f'run{i}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1',
                            '--dump-outputs', str(out)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
        assert line['steps'] == 4 and line['warmup'] == 1 and line['unit'] == 'instances/s' and line['higher_is_better'] is True
        assert line['dtype'] == 'f32' and line['ms_per_step'] > 0
        assert abs(line['value'] - 4096 / (line['ms_per_step'] * 1e-3)) <= 0.01 * line['value']
        assert not {'roofline', 'kernel_ms', 'cpu_baseline', 'hipgraph_replay', 'with_stage_events_in_region'} & set(line)
        files = sorted(os.listdir(out))
        assert sum(os.path.getsize(out / f) for f in files) <= 64 * 2 ** 20
        dumps.append({f[:-4]: np.load(out / f) for f in files})
    a, b = dumps
    assert sorted(a) == ['cost_init', 'grad_w2d', 'grad_x2d', 'grad_x3d', 'logw', 'loss', 'pose_opt']
    assert a['pose_opt'].shape == (4096, 7) and a['cost_init'].shape == (4096,)
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
