"""The drop-in CLI surface: tools/train.py and tools/test.py accept the reference's flags
(tools/train.py:22-89, tools/test.py:24-130) and tools/dist_train.sh exists with the reference's calling convention."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(f'oadg_tools_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


def test_train_cli_accepts_the_reference_flags(monkeypatch):
    train = _load('train')
    monkeypatch.setattr(sys, 'argv', ['train.py', 'cfg.py', '--work-dir', 'w', '--resume-from', 'r.pth', '--auto-resume',
                                      '--no-validate', '--gpu-ids', '0', '1', '--seed', '3', '--deterministic',
                                      '--cfg-options', 'a.b=1', 'c=x', '--launcher', 'pytorch', '--local_rank', '2',
                                      '--debug_mode'])
    a = train.parse_args()
    assert (a.config, a.work_dir, a.resume_from, a.auto_resume, a.no_validate) == ('cfg.py', 'w', 'r.pth', True, True)
    assert a.gpu_ids == [0, 1] and a.seed == 3 and a.deterministic and a.launcher == 'pytorch' and a.local_rank == 2
    assert a.cfg_options == {'a.b': '1', 'c': 'x'} and os.environ['LOCAL_RANK'] in ('2', os.environ['LOCAL_RANK'])
    monkeypatch.setattr(sys, 'argv', ['train.py', 'cfg.py', '--gpus', '1', '--gpu-ids', '0'])
    with pytest.raises(SystemExit):              # mutually exclusive, as in the reference
        train.parse_args()
    monkeypatch.setattr(sys, 'argv', ['train.py', 'cfg.py', '--options', 'a=1', '--cfg-options', 'b=2'])
    with pytest.raises(ValueError):
        train.parse_args()


def test_test_cli_and_eval_map(monkeypatch):
    import numpy as np
    test = _load('test')
    monkeypatch.setattr(sys, 'argv', ['test.py', 'cfg.py', 'ck.pth', '--out', 'r.pkl', '--eval', 'bbox', '--cfg-options',
                                      'a=1', '--launcher', 'none', '--local_rank', '0'])
    a = test.parse_args()
    assert (a.config, a.checkpoint, a.out, a.eval) == ('cfg.py', 'ck.pth', 'r.pkl', ['bbox'])
    # mean_ap.py semantics on a hand-checked case: class 0: 2 gts, detections (tp 0.9, fp 0.8, tp 0.7) -> AP = 0.5 + 0.5 * 2/3
    res = [[np.array([[0, 0, 10, 10, 0.9], [50, 50, 60, 60, 0.8], [100, 100, 120, 120, 0.7]], np.float32),
            np.zeros((0, 5), np.float32)]]
    ann = [(np.array([[0, 0, 10, 10], [100, 100, 120, 120]], np.float32), np.array([0, 0]))]
    m, aps = test.eval_map(res, ann, 2)
    assert abs(aps[0] - (0.5 + 0.5 * 2 / 3)) < 1e-6 and len(aps) == 1 and abs(m - aps[0]) < 1e-12
    # a duplicate detection of an already matched gt is a false positive
    res = [[np.array([[0, 0, 10, 10, 0.9], [0, 0, 10, 10, 0.8]], np.float32), np.zeros((0, 5), np.float32)]]
    ann = [(np.array([[0, 0, 10, 10]], np.float32), np.array([0]))]
    assert abs(test.eval_map(res, ann, 2)[1][0] - 1.0) < 1e-6


def test_dist_train_script_follows_the_reference_convention():
    sh = open(os.path.join(ROOT, 'tools', 'dist_train.sh')).read()
    assert 'CONFIG=$1' in sh and 'GPUS=$2' in sh and 'PORT' in sh and '--launcher pytorch' in sh


def test_bench_self_launches_n_ranks_when_no_launcher_is_present(monkeypatch):
    """``python bench.py --gpus N`` with no WORLD_SIZE in the environment re-launches itself as N ranks under
    torch.distributed.run on 127.0.0.1 (VERDICT r1 missing #1; tools/dist_train.sh:7-9)."""
    import subprocess
    spec = importlib.util.spec_from_file_location('oadg_bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_call(cmd, env=None):
        seen['cmd'], seen['env'] = cmd, env
        return 7
    monkeypatch.setattr(subprocess, 'call', fake_call)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '3', '--warmup', '1'])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 7
    cmd = seen['cmd']
    assert cmd[1:4] == ['-m', 'torch.distributed.run', '--nnodes=1'] and '--nproc-per-node=8' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1' and int(cmd[cmd.index('--master-port') + 1]) > 0
    assert cmd[-6:] == ['--gpus', '8', '--steps', '3', '--warmup', '1'] and cmd[-7].endswith('bench.py')
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'


@pytest.mark.gpu
def test_train_cli_shuffles_checkpoints_and_resumes_epoch_and_iter(tmp_path):
    """tools/train.py end to end on synthetic samples: per-epoch shuffled order (GroupSampler), epoch checkpoints with
    meta epoch / iter, and --resume-from continuing with the NEXT epoch at the saved iteration (EpochBasedRunner.resume)
    instead of starting over."""
    import subprocess
    import torch
    cfg = tmp_path / 'tiny.py'
    cfg.write_text(
        f"_base_ = ['{ROOT}/configs/oadg/faster_rcnn_r50_fpn_1x_cityscapes_oadg.py']\n"
        "data = dict(samples_per_gpu=2, train=dict(img_shape=(256, 512), num_boxes=6, box_size=(16, 120), length=8))\n"
        "runner = dict(type='EpochBasedRunner', max_epochs=3)\n"
        "checkpoint_config = dict(interval=1)\n"
        "log_config = dict(interval=1, hooks=[dict(type='TextLoggerHook')])\n"
        "lr_config = dict(policy='step', warmup=None, step=[1])\n")
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    w1 = tmp_path / 'w1'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg), '--work-dir', str(w1), '--seed', '0'],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('Epoch [')]
    assert len(lines) == 12 and lines[0].startswith('Epoch [1][1/4]') and lines[-1].startswith('Epoch [3][4/4]')
    assert 'lr: 1.000e-02' in lines[0] and 'lr: 1.000e-03' in lines[4]           # step decay at epoch index 1
    ck = torch.load(str(w1 / 'epoch_2.pth'), map_location='cpu', weights_only=False)
    assert ck['meta']['epoch'] == 2 and ck['meta']['iter'] == 8
    w2 = tmp_path / 'w2'
    r2 = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg), '--work-dir', str(w2), '--seed', '0',
                         '--resume-from', str(w1 / 'epoch_2.pth')], capture_output=True, text=True, env=env, timeout=900)
    assert r2.returncode == 0, r2.stdout[-2000:] + r2.stderr[-2000:]
    assert 'resumed epoch 2, iter 8' in r2.stdout
    lines2 = [l for l in r2.stdout.splitlines() if l.startswith('Epoch [')]
    assert len(lines2) == 4 and lines2[0].startswith('Epoch [3][1/4]') and 'lr: 1.000e-03' in lines2[0]
    ck2 = torch.load(str(w2 / 'epoch_3.pth'), map_location='cpu', weights_only=False)
    assert ck2['meta']['epoch'] == 3 and ck2['meta']['iter'] == 12
    assert not (w2 / 'epoch_1.pth').exists()                                          # earlier epochs are not redone
    # a run cut short INSIDE an epoch (--max-iters 6 = 2 batches into epoch 2): latest.pth records the unfinished epoch and
    # the batches done, --auto-resume finishes that epoch's (seeded) order from batch 3 instead of skipping it
    w3 = tmp_path / 'w3'
    r3 = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg), '--work-dir', str(w3), '--seed', '0',
                         '--max-iters', '6'], capture_output=True, text=True, env=env, timeout=900)
    assert r3.returncode == 0, r3.stdout[-2000:] + r3.stderr[-2000:]
    ck3 = torch.load(str(w3 / 'latest.pth'), map_location='cpu', weights_only=False)
    assert ck3['meta']['epoch'] == 1 and ck3['meta']['iter'] == 6 and ck3['meta']['inner_iter'] == 2
    assert (w3 / 'epoch_1.pth').exists() and not (w3 / 'epoch_2.pth').exists()
    r4 = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg), '--work-dir', str(w3), '--seed', '0',
                         '--auto-resume'], capture_output=True, text=True, env=env, timeout=900)
    assert r4.returncode == 0, r4.stdout[-2000:] + r4.stderr[-2000:]
    lines4 = [l for l in r4.stdout.splitlines() if l.startswith('Epoch [')]
    assert len(lines4) == 6 and lines4[0].startswith('Epoch [2][3/4]') and lines4[-1].startswith('Epoch [3][4/4]')
    ck4 = torch.load(str(w3 / 'epoch_3.pth'), map_location='cpu', weights_only=False)
    assert ck4['meta']['epoch'] == 3 and ck4['meta']['iter'] == 12


@pytest.mark.gpu
def test_test_cli_coco_style_eval_and_robustness_loop(tmp_path):
    """tools/test.py --eval bbox mAP (COCO-style numbers + VOC AP50) and tools/analysis_tools/test_robustness.py
    (corruption x severity loop, severity 0 once, P / mPC / rPC aggregation) on the synthetic test split."""
    import json
    import pickle
    import subprocess
    cfg = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes_oadg.py')
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    wd = tmp_path / 'eval'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), cfg, 'none', '--eval', 'bbox', 'mAP',
                        '--max-samples', '2', '--work-dir', str(wd), '--out', str(tmp_path / 'r.pkl')],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    ev = json.load(open(wd / 'eval.json'))
    # CocoDataset.evaluate's numbers and names: maxDets (100, 300, 1000), mAP at 1000 detections (coco.py:468-480)
    assert list(ev['bbox']) == ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l', 'AR@100', 'AR@300', 'AR@1000', 'AR_s@1000',
                                'AR_m@1000', 'AR_l@1000']
    assert -1.0 <= ev['bbox']['mAP'] <= 1.0 and 'mAP' in ev['mAP']
    assert len(pickle.load(open(tmp_path / 'r.pkl', 'rb'))) == 2
    out = tmp_path / 'rob.pkl'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'analysis_tools', 'test_robustness.py'), cfg, 'none',
                        '--corruptions', 'fog', 'snow', '--severities', '0', '1', '--max-samples', '2', '--out', str(out),
                        '--final-prints', 'P', 'mPC', 'rPC', '--final-prints-aggregate', 'all'],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count('Testing ') == 3                       # fog 0, fog 1, snow 1 (snow 0 reuses fog 0)
    agg = pickle.load(open(tmp_path / 'rob_results.pkl', 'rb'))
    assert set(agg) == {'fog', 'snow'} and set(agg['snow']) == {0, 1} and agg['snow'][0] is agg['fog'][0] or \
        agg['snow'][0] == agg['fog'][0]
    summ = json.load(open(tmp_path / 'rob_summary.json'))
    assert set(summ) == {'P', 'mPC', 'rPC'} and 'Mean Performance under Corruption [mPC] (bbox)' in r.stdout
    # --load-dataset original: the Corrupt transform is inserted after the loading step and corrupts on the fly
    # (test_robustness.py:269-277); a corruption that needs the absent third-party pieces stops with its name
    out2 = tmp_path / 'rob2.pkl'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'analysis_tools', 'test_robustness.py'), cfg, 'none',
                        '--corruptions', 'contrast', 'gaussian_noise', '--severities', '0', '3', '--max-samples', '2',
                        '--load-dataset', 'original', '--out', str(out2), '--seed', '0'],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    agg2 = pickle.load(open(tmp_path / 'rob2_results.pkl', 'rb'))
    assert set(agg2) == {'contrast', 'gaussian_noise'} and set(agg2['contrast']) == {0, 3}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'analysis_tools', 'test_robustness.py'), cfg, 'none',
                        '--corruptions', 'frost', '--severities', '1', '--max-samples', '1', '--load-dataset', 'original'],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode != 0 and "corruption 'frost'" in r.stderr


@pytest.mark.timeout(900)
def test_bench_two_ranks_through_its_own_launch_path_on_gloo():
    """``python bench.py --gpus 2`` end to end - self-launch under torch.distributed.run on 127.0.0.1, env:// rendezvous,
    warm-up, barrier-bracketed timed region, MAX over ranks, ONE JSON line from rank 0 - with the whole detector step of
    tests/ddp_bench_factory.py on CPU ranks over gloo (no multi-GPU node exists for the RCCL path):
    world plumbing as reported, parameters identical on both ranks after 2 steps of different data per rank."""
    import json
    import subprocess
    env = dict(os.environ)
    env['OADG_BENCH_STEP_FACTORY'] = 'ddp_bench_factory:make'
    env['PYTHONPATH'] = os.path.join(ROOT, 'tests') + os.pathsep + env.get('PYTHONPATH', '')
    env.pop('WORLD_SIZE', None)
    env['OMP_NUM_THREADS'] = '3'
    env['OADG_AFFINITY_PROBE'] = '0'     # the first cores of each slice, not the quietest ones of the moment (host load)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '0',
                        '--batch', '1', '--height', '128', '--width', '192', '--no-cpu-baseline'],
                       env=env, capture_output=True, text=True, timeout=850)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]           # rank 0 only
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['world_size'] == 2 and d['dist_backend'] == 'gloo' and d['steps'] == 2
    assert d['scaling'] == 'weak' and d['config']['global_batch'] == 2 and d['config']['parallelism'] == 'dp2'
    assert d['rccl_ranks'] == 0 and 'PLUMBING' in d['config']['workload']
    assert d['config']['params_equal_across_ranks'] is True
    # every rank pinned to a compact set of physical cores inside its own slice of the host (oadg_amd.apis.pin_rank_to_cores)
    from oadg_amd.apis import physical_cores
    phys = physical_cores(os.sched_getaffinity(0))
    mine = phys[:len(phys) // 2][:8]
    assert d['config']['cpu_affinity'].startswith(f'{len(mine)} of {len(phys)} physical cores ')
    assert d['config']['cpu_affinity'].endswith(f'slices of {len(phys) // 2} (rank 0: CPUs {mine[0]}-{mine[-1]})')
    assert d['config']['param_tensors_changed'] == d['config']['param_tensors'] > 100
    assert np.isfinite(d['config']['final_loss']) and d['value'] > 0


def test_bench_workloads_and_clock_sampler_without_a_gpu(monkeypatch):
    """bench.py's --config / --workload table names BASELINE configs 2, 4 and 5 with their per-GPU sizes, and the clock
    sampler degrades to {'available': False} (never an exception) where amdsmi cannot reach a device"""
    spec = importlib.util.spec_from_file_location('oadg_bench2', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert set(bench.CONFIGS) == {'r50_fpn', 'r101_dc5'}
    for k, c in bench.CONFIGS.items():
        assert os.path.exists(os.path.join(ROOT, 'configs', 'oadg', c['cfg'])), k
    assert (bench.CONFIGS['r50_fpn']['batch'], bench.CONFIGS['r50_fpn']['height'], bench.CONFIGS['r50_fpn']['width']) == (4, 1024, 2048)
    assert (bench.CONFIGS['r101_dc5']['batch'], bench.CONFIGS['r101_dc5']['height'], bench.CONFIGS['r101_dc5']['width']) == (2, 736, 1280)
    assert bench.CONFIGS['r101_dc5']['roi_strides'] == [16] and bench.CONFIGS['r101_dc5']['roi_channels'] == 2048
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--workload', 'oamix_stress'])
    a = bench.parse()
    assert (a.batch, a.height, a.width) == (8, 1024, 2048)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--config', 'r101_dc5'])
    a = bench.parse()
    assert (a.batch, a.height, a.width, a.workload) == (2, 736, 1280, 'train')
    # (per-family table, CPU baseline): only with --full, only on one GPU, and --no-families / --no-cpu-baseline drop either
    for argv, want in (([], (False, False)), (['--no-cpu-baseline'], (False, False)), (['--full'], (True, True)),
                       (['--full', '--no-cpu-baseline'], (True, False)), (['--full', '--no-families'], (False, True)),
                       (['--full', '--workload', 'oamix_stress'], (True, True)), (['--full', '--gpus', '2'], (False, False))):
        monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '20', '--warmup', '5'] + argv)
        a = bench.parse()
        assert a.full == ('--full' in argv) and bench.full_extras(a) == want, argv
    s = bench.ClockSampler(0).start().stop()
    assert s['available'] in (True, False) and ('sclk_mhz' in s or 'note' in s)
    # a single rank is pinned too (a compact set of physical cores: the run-to-run spread of the host time), the CPU-baseline
    # leg gets every CPU back, and OADG_BENCH_NO_AFFINITY=1 switches it off
    before = os.sched_getaffinity(0)
    try:
        monkeypatch.setenv('OADG_BENCH_NO_AFFINITY', '1')
        assert bench.pin_rank_to_cores(0, 1) is None and os.sched_getaffinity(0) == before
        monkeypatch.delenv('OADG_BENCH_NO_AFFINITY')
        desc = bench.pin_rank_to_cores(0, 1)
        assert 'physical cores' in desc and len(os.sched_getaffinity(0)) <= 8 and os.sched_getaffinity(0) <= before
        assert bench.baseline_cores() == len(before) and os.sched_getaffinity(0) == before
        # LOCAL_RANK without LOCAL_WORLD_SIZE (local_rank >= world): wraps around instead of an empty CPU set
        from oadg_amd.apis import pin_rank_to_cores
        os.sched_setaffinity(0, before)
        assert pin_rank_to_cores(3, 1) is not None and len(os.sched_getaffinity(0)) >= 1
    finally:
        os.sched_setaffinity(0, before)
        torch.set_num_threads(max(1, min(len(before), 16)))


@pytest.mark.timeout(900)
def test_bench_dump_outputs_are_the_last_timed_step_and_repeat(tmp_path):
    """``bench.py --dump-outputs DIR`` (plumbing run on one CPU rank): DIR/<name>.npy in float32 / float64 holds what the last
    of the --steps timed steps returned (its loss is the line's final_loss), and a second run with the same arguments
    writes the same arrays"""
    import json
    import subprocess
    env = dict(os.environ)
    env['OADG_BENCH_STEP_FACTORY'] = 'ddp_bench_factory:make'
    env['PYTHONPATH'] = os.path.join(ROOT, 'tests') + os.pathsep + env.get('PYTHONPATH', '')
    env.pop('WORLD_SIZE', None)
    env['OMP_NUM_THREADS'] = '3'
    dumps = []
    for run in range(2):
        d = tmp_path / f'run{run}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                            '--batch', '1', '--height', '128', '--width', '192', '--no-cpu-baseline', '--dump-outputs', str(d)],
                           env=env, capture_output=True, text=True, timeout=850)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')][-1])
        assert line['steps'] == 2 and line['ms_per_step'] > 0
        arrays = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
        assert {'loss', 'log_vars.loss_cls', 'log_vars.loss_cont'} <= set(arrays)
        assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
        assert round(float(arrays['loss']), 4) == line['config']['final_loss']
        dumps.append(arrays)
    assert set(dumps[0]) == set(dumps[1])
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k


def test_bench_dump_samples_are_fixed_and_bounded(tmp_path):
    """the parameter / gradient samples of --dump-outputs: the same seeded indices for the same size on every call,
    taken in named-parameter order (no gradient = zeros), and the 64 MB limit enforced"""
    spec = importlib.util.spec_from_file_location('oadg_bench3', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = bench.DUMP_SAMPLE + 12345
    i0, i1 = bench.sample_index(n), bench.sample_index(n)
    assert np.array_equal(i0, i1) and len(i0) == bench.DUMP_SAMPLE and (np.diff(i0) > 0).all() and i0[-1] < n
    assert bench.sample_index(100) is None
    torch.manual_seed(0)
    m = torch.nn.ModuleList([torch.nn.Linear(2048, 2049), torch.nn.Linear(4, 4)])
    m[0](torch.ones(2, 2048)).sum().backward()                   # the second layer receives no gradient
    out = bench.train_step_outputs({'loss': torch.tensor(1.5), 'log_vars': {'acc': 50.0, 'note': 'x'}}, m)
    assert set(out) == {'loss', 'log_vars.acc', 'params_sample', 'grads_sample'}
    flat = torch.cat([p.detach().flatten() for p in m.parameters()]).numpy()
    idx = bench.sample_index(flat.size)
    assert np.array_equal(out['params_sample'], flat[idx])
    n0 = sum(p.numel() for p in m[0].parameters())
    assert (out['grads_sample'][idx >= n0] == 0).all() and np.count_nonzero(out['grads_sample'][idx < n0]) > 0
    bench.dump_outputs(str(tmp_path / 'd'), out)
    assert np.load(tmp_path / 'd' / 'log_vars.acc.npy').dtype == np.float64
    assert np.load(tmp_path / 'd' / 'params_sample.npy').dtype == np.float32
    with pytest.raises(AssertionError, match='--dump-outputs'):
        bench.dump_outputs(str(tmp_path / 'big'), {'x': np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
