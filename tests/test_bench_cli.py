"""bench.py's command line: a plain run times only the SECOND steps behind `value`; --full adds the other legs and tables;
--dump-outputs writes what the last timed step handed its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    import bench
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '1', '--steps', '7', '--warmup', '2'])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--full', '--dump-outputs', 'out'])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == 'out'


def test_dump_outputs_writes_the_step_as_float32(tmp_path):
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    m.train()
    loss = m(torch.randn(8, 4)).square().mean()
    loss.backward()
    n, total = bench.dump_outputs(str(tmp_path), m, loss.detach(), {'part': 2 * loss.detach(), 'count': 3, 'name': 'skipped'})
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(['loss.npy', 'tb.part.npy', 'tb.count.npy',
                            'param.0.weight.npy', 'param.0.bias.npy', 'param.1.weight.npy', 'param.1.bias.npy',
                            'grad.0.weight.npy', 'grad.0.bias.npy', 'grad.1.weight.npy', 'grad.1.bias.npy',
                            'buffer.1.running_mean.npy', 'buffer.1.running_var.npy'])
    assert n == len(files)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in files}
    assert all(a.dtype == np.float32 for a in got.values())
    assert total == sum(a.nbytes for a in got.values())
    assert got['loss'] == np.float32(loss.item()) and got['tb.count'] == 3
    np.testing.assert_array_equal(got['grad.0.weight'], m[0].weight.grad.numpy())
    np.testing.assert_array_equal(got['buffer.1.running_var'], m[1].running_var.numpy())


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 1000)
    m = torch.nn.Linear(300, 1)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / 'out'), m, torch.zeros(()), {})
    assert not os.path.exists(tmp_path / 'out')


@pytest.mark.gpu
def test_plain_bench_runs_print_the_contract_line_and_dump_the_same_bits(tmp_path):
    """two plain runs with the same arguments: the contract line without the --full legs, and dumped outputs that are bit-equal"""
    dumps, lines = [], []
    for run in range(2):
        out = tmp_path / ('outputs%d' % run)
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        found = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        assert len(found) == 1, r.stdout[-2000:]
        lines.append(json.loads(found[0]))
        dumps.append({f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)})
    d = lines[0]
    assert d['steps'] == 3 and d['warmup'] == 1 and d['full'] is False
    assert d['unit'] == 'frames/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    assert abs(d['value'] - 16 * 3 / (d['ms_per_step'] * 3 / 1e3)) < 1e-2 * d['value']
    for leg in ('roofline', 'kernel_table', 'fwd_bwd_only', 'miopen_convs', 'pvrcnn', 'crb_scoring', 'cpu_baseline'):
        assert leg not in d
    got = dumps[0]
    assert d['dumped_outputs']['files'] == len(got) and d['dumped_outputs']['bytes'] <= 64 << 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert float(got['loss']) == np.float32(d['dumped_outputs']['loss'])
    assert {'tb.rpn_loss_cls', 'tb.rpn_loss_loc', 'tb.rpn_loss_dir'} <= set(got)
    grads = [k for k in got if k.startswith('grad.')]
    assert 0 < len(grads) <= len([k for k in got if k.startswith('param.')])
    assert any(float(np.abs(got[k]).sum()) > 0 for k in grads)
    assert sorted(dumps[1]) == sorted(got)
    differ = [k for k in got if not np.array_equal(got[k], dumps[1][k])]
    assert not differ, differ
