"""GPU (-m gpu): bench.py's plain line -- one timed region of exactly --steps steps, the headline fields and none of the
records --full adds -- and --dump-outputs: the disparity map of the last timed step, identical over two runs with the same
arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(extra):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + extra
    out = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    lines = [l for l in out.stdout.decode(errors='replace').splitlines() if l.startswith('{')]
    assert out.returncode == 0 and len(lines) == 1, out.stderr.decode(errors='replace')[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(hip_library, tmp_path):
    maps = []
    for run in range(2):
        folder = tmp_path / str(run)
        line = run_bench(['--steps', '6', '--warmup', '2', '--dump-outputs', str(folder)])
        assert line['metric'].startswith('stereo pairs/sec') and line['unit'] == 'pairs/s', line
        assert line['higher_is_better'] is True and line['dtype'] == 'f32' and line['steps'] == 6, line
        assert line['value'] > 0 and abs(line['value'] * line['ms_per_step'] - 1e3) < 1e-6, line
        for key in ('windows', 'ms_per_frame', 'sequential', 'roofline', 'path_roofline', 'cpu_baseline', 'gpu_baseline',
                    'full_forward_ms', 'time_per_image', 'sustained', 'exact_fp32', 'config4', 'train'):
            assert key not in line, key
        assert sorted(os.listdir(folder)) == ['disparity.npy']
        disparity = np.load(folder / 'disparity.npy')
        assert disparity.dtype == np.float32 and disparity.shape == (1, 576, 960)
        assert np.isfinite(disparity).all() and disparity.max() > 0
        maps.append(disparity)
    assert np.array_equal(maps[0], maps[1])
