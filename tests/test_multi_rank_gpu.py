"""`-m gpu`: the N > 1 path of bench.py exactly as the driver launches it (`python -m torch.distributed.run --nnodes=1
--nproc-per-node 2 ... bench.py --gpus 2`), on a ONE-GPU box: both ranks are pinned to device 0 (NR_DIST_DEVICE) and
rendezvous over gloo (RCCL refuses two ranks on one device).  Proves that the sharded scene construction, the barrier /
max-over-ranks timing, the `--gather` all-gather of the rendered shards and the one-JSON-line contract execute; it is not a
scaling measurement.  The log is kept under gpurun_out/ (copied to profiles/ by the round script)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize('gather', [False, True], ids=['no_collective', 'all_gather'])
def test_bench_two_ranks_on_one_gpu(gather):
    env = dict(os.environ, NR_DIST_DEVICE='0', NR_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1',
           '--cpu-sample-views', '0', '--stage-iters', '2', '--light']
    if gather:
        cmd.append('--gather')
    out_dir = os.path.join(ROOT, 'gpurun_out')
    try:
        res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired as ex:  # a rank waiting in a collective the other never enters
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, 'two_ranks_one_gpu_TIMEOUT.log'), 'w') as f:
                f.write(' '.join(cmd) + '\n' + str(ex.stdout)[-4000:] + '\n--- stderr ---\n' + str(ex.stderr)[-4000:])
        raise
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, 'two_ranks_one_gpu%s.log' % ('_gather' if gather else '')), 'w') as f:
            f.write('$ NR_DIST_DEVICE=0 NR_DIST_BACKEND=gloo ' + ' '.join(cmd) + '\n' + res.stdout + '\n--- stderr ---\n' +
                    res.stderr[-4000:])
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout
    d = json.loads(lines[0])
    # the 64-view batch is SPLIT (BASELINE.md "Multi-GPU rows": B / R views per rank); 64 per GPU is the weak_scaling object
    assert d['n_gpus'] == 2 and d['value'] > 0 and d['steps'] == 2 and d['scaling'] == 'strong'
    assert d['config']['views_total'] == 64 and d['config']['views_per_gpu'] == 64 // 2
    assert abs(d['value'] - 64 * 256 * 256 / (d['ms_per_step'] * 1e-3) / 1e6) <= 1e-6 * d['value']
    w = d['weak_scaling']
    assert w['scaling'] == 'weak' and w['views_per_gpu'] == 64 and w['views_total'] == 128 and w['value'] > 0
    assert ('all_gather' in d['config']['parallelism']) == gather
    assert d['cpu_baseline'] is None  # (--cpu-sample-views 0 in this test; an N > 1 run otherwise carries rank 0's CPU rows)


def _launch(n_ranks, extra, log_name, timeout=420):
    env = dict(os.environ, NR_DIST_DEVICE='0', NR_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n_ranks), '--master-addr',
           '127.0.0.1', '--master-port', str(_free_port()), os.path.join(ROOT, 'bench.py'), '--gpus', str(n_ranks), '--steps', '2',
           '--warmup', '1', '--cpu-sample-views', '0', '--stage-iters', '2', '--light', '--prewarm-ms', '0'] + extra
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    out_dir = os.path.join(ROOT, 'gpurun_out')
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, log_name), 'w') as f:
            f.write('$ NR_DIST_DEVICE=0 NR_DIST_BACKEND=gloo ' + ' '.join(cmd) + '\n' + res.stdout + '\n--- stderr ---\n' +
                    res.stderr[-4000:])
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize('views', [64, 62], ids=['even_16_views_each', 'uneven_62_views'])
def test_bench_four_ranks_on_one_gpu(views):
    """The control path of a multi-GPU run beyond two ranks (VERDICT r04 missing #3): 4 ranks, gloo rendezvous, all on the one
    GPU of the test box -- rank -> shard bounds (an uneven split of 62 views: two ranks of 16, two of 15), pin_to_l3_group
    (local_rank) for four local ranks, the reference-face broadcast, barrier / max-over-ranks timing, the weak-scaling leg, the
    padded all-gather of uneven shards.  Not a measurement.  (Four ranks, not eight: with the test process itself no more than
    six processes may hold one GPU at a time.)"""
    d = _launch(4, ['--batch', str(views), '--gather'], 'four_ranks_one_gpu_%d.log' % views)
    assert d['n_gpus'] == 4 and d['scaling'] == 'strong' and d['value'] > 0
    assert d['config']['views_total'] == views and d['config']['views_per_gpu'] == -(-views // 4)  # rank 0 holds a larger shard
    assert abs(d['value'] - views * 256 * 256 / (d['ms_per_step'] * 1e-3) / 1e6) <= 1e-6 * d['value']
    assert d['weak_scaling']['views_total'] == 4 * views and 'all_gather' in d['config']['parallelism']
    assert d['grad_check']['face_index_mismatch'] == 0


@pytest.mark.parametrize('gather', [False, True], ids=['no_collective', 'all_gather'])
def test_bench_config4_two_ranks_on_one_gpu(gather):
    """BASELINE.json configs[3] in its stated form (VERDICT r04 missing #2): `bench.py --workload c4` shards the 512 seeded meshes
    over the ranks (here 8 meshes over 2 ranks: the job's size is an argument), RGB forward + backward, `--gather` all-gathers
    the rendered [meshes / R, 256, 256, 3] shards; the line names the workload and keeps roofline + grad_check."""
    d = _launch(2, ['--workload', 'c4', '--batch', '8'] + (['--gather'] if gather else []),
                'c4_two_ranks_one_gpu%s.log' % ('_gather' if gather else ''))
    assert d['n_gpus'] == 2 and d['scaling'] == 'strong' and 'configs[3]' in d['metric'] and 'configs[3]' in d['config']['workload']
    assert d['config']['views_total'] == 8 and d['config']['views_per_gpu'] == 4 and d['config']['num_faces'] == 10240
    assert d['config']['texture_size'] == 4
    assert abs(d['value'] - 8 * 256 * 256 / (d['ms_per_step'] * 1e-3) / 1e6) <= 1e-6 * d['value']
    assert ('all_gather' in d['config']['workload']) == gather
    g = d['grad_check']
    assert g['face_index_mismatch'] == 0 and g['grad_faces']['max_rel_err_floor_1e-3_of_max'] <= 1e-4
    assert g['grad_textures']['max_abs_err'] <= 1e-4 * g['grad_textures']['max_abs']
    w = d['roofline']['whole_step']  # rgb only: SURVEY 8d's 76 B per pixel
    assert w['algorithmic_bytes'] == 76 * 8 * 256 * 256 + (108 + 24 * 64) * 8 * 10240
