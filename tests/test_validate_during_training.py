"""GPU: validation during training (EvalHook) sees exactly the weights of the epoch it follows - also the SECOND time, when
anything prepared for the first test-mode forward pass is an epoch old - and leaves the training run as it found it:
same log lines, same parameters and momentum as a run that never validated; no random stream moved; two ranks sharding
the val set return what one process returns.  The tiny configuration of tests/test_cli.py (R50-FPN OA-DG Cityscapes,
256 x 512 synthetic samples, 2 per batch, 8 train images) plus a 4-image val split of the same shape.
Reference: mmcv/runner/hooks/evaluation.py, mmdet/apis/test.py."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes_oadg.py')
VAL_PIPELINE = """[
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=(512, 256), flip=False,
         transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                     dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                     dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                     dict(type='Collect', keys=['img'])])]"""
TINY = (f"_base_ = ['{BASE}']\n"
        f"val_pipeline = {VAL_PIPELINE}\n"
        "data = dict(samples_per_gpu=2,\n"
        "            train=dict(img_shape=(256, 512), num_boxes=6, box_size=(16, 120), length=8),\n"
        "            val=dict(img_shape=(256, 512), num_boxes=6, box_size=(16, 120), length=4, pipeline=val_pipeline))\n"
        "runner = dict(type='EpochBasedRunner', max_epochs=2)\n"
        "checkpoint_config = dict(interval=1)\n"
        "log_config = dict(interval=1, hooks=[dict(type='TextLoggerHook')])\n"
        "lr_config = dict(policy='step', warmup=None, step=[1])\n")
EVALUATION = "evaluation = dict(interval=1, metric='bbox', save_best='auto')\n"


def _train(cfg, work_dir, *flags, dump=False):
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    if dump:
        env['OADG_EVAL_DUMP'] = '1'
    return subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg), '--work-dir', str(work_dir),
                           '--seed', '0', *flags], capture_output=True, text=True, env=env, timeout=600)


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    """A = the tiny config with validation after both epochs, B = the same with --no-validate, B2 = B again (the control:
    is tools/train.py as a whole repeatable?).  One process after the other; nothing more is started after a failure."""
    d = tmp_path_factory.mktemp('validate')
    cfg = d / 'tiny_val.py'
    cfg.write_text(TINY + EVALUATION)            # (ONE config for all three: --no-validate alone switches validation off)
    out = dict(dir=d, cfg=cfg)
    for name, flags, dump in (('A', (), True), ('B', ('--no-validate',), False), ('B2', ('--no-validate',), False)):
        r = _train(cfg, d / name, *flags, dump=dump)
        out[name] = r
        if r.returncode != 0:
            break
    return out


def _ok(runs, *names):
    for n in names:
        assert n in runs, f'run {n} was not started: an earlier run failed'
        r = runs[n]
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]


def _val_lines(stdout):
    out = []
    for ln in stdout.splitlines():
        m = re.match(r'Epoch\(val\) \[(\d+)\]\[(\d+)\] (.*)$', ln)
        if m:
            out.append((int(m.group(1)), int(m.group(2)), dict(kv.split(': ', 1) for kv in m.group(3).split(', '))))
    return out


def _fresh_evaluation(cfg_path, checkpoint, dev):
    """a model built from the config, the checkpoint loaded, tested as tools/test.py tests: (results, evaluate's dict)"""
    from oadg_amd import Config, build_detector, hip_conv
    from oadg_amd.apis import single_gpu_test
    from oadg_amd.checkpoint import load_checkpoint
    from oadg_amd.datasets import build_dataset
    from oadg_amd.pipelines import DevicePipeline
    cfg = Config.fromfile(str(cfg_path))
    cfg.model.pop('pretrained', None)
    model = build_detector(cfg.model, test_cfg=cfg.get('test_cfg'))
    rep = load_checkpoint(model, str(checkpoint), map_location='cpu', strict=False, logger=None)
    assert not rep['missing'] and not rep['mismatched']
    model = model.to(dev).to(memory_format=torch.channels_last).eval()
    val = dict(cfg.data.val.to_dict() if hasattr(cfg.data.val, 'to_dict') else cfg.data.val)
    ds = build_dataset(val, default_args=dict(seed=12345, device=dev, test_mode=True), synthetic_fallback=True)
    pipe = DevicePipeline(val['pipeline'], dtype=torch.bfloat16)
    hip_conv.enable()
    try:
        results = single_gpu_test(model, ds, pipe, torch.bfloat16, 1)
        torch.cuda.synchronize()
    finally:
        hip_conv.enable(False)
    return results, ds.evaluate(results, metric='bbox')


def _same_results(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(x, y))
                                    for x, y in zip(a, b))


@pytest.mark.gpu
def test_validation_sees_the_checkpoint_weights_both_times(runs, dev):
    """what the hook logged and detected after epoch 1 and after epoch 2 == a fresh model loaded from epoch_1.pth /
    epoch_2.pth, tested in this process: every logged number (as printed, 3 decimals) and every detection array, bit for
    bit.  Epoch 2 is the one a stale prepared weight (BN fold, bf16 layout, the RPN head's padded 1x1 maps) would fail."""
    _ok(runs, 'A')
    d = runs['dir'] / 'A'
    lines = _val_lines(runs['A'].stdout)
    assert [(e, n) for e, n, _ in lines] == [(1, 4), (2, 4)], runs['A'].stdout[-3000:]
    fresh = {}
    for epoch, _, logged in lines:
        results, ev = _fresh_evaluation(runs['cfg'], d / f'epoch_{epoch}.pth', dev)
        fresh[epoch] = results
        assert list(logged) == list(ev) == ['bbox_mAP', 'bbox_mAP_50', 'bbox_mAP_75', 'bbox_mAP_s', 'bbox_mAP_m',
                                            'bbox_mAP_l', 'bbox_mAP_copypaste']
        for k, v in ev.items():
            print(f'epoch {epoch} {k}: logged {logged[k]} fresh {v}')
            want = f'{v:.3f}' if isinstance(v, float) else v
            got = f'{float(logged[k]):.3f}' if isinstance(v, float) else logged[k]
            assert got == want, (epoch, k, logged[k], v)
        with open(d / f'val_results_epoch_{epoch}.pkl', 'rb') as f:
            hooked = pickle.load(f)
        n_det = sum(len(c) for r in results for c in r)
        print(f'epoch {epoch}: {n_det} detections in {len(results)} images')
        assert len(results) == 4 and n_det > 0               # (an empty list would be equal to anything empty)
        assert _same_results(hooked, results), f'epoch {epoch}: the detections of the hook differ from the checkpoint\'s'
    assert not _same_results(fresh[1], fresh[2])             # the two epochs really have different weights to show
    best = sorted(f for f in os.listdir(d) if f.startswith('best_bbox_mAP_epoch_'))
    assert len(best) == 1, os.listdir(d)
    ck = torch.load(str(d / best[0]), map_location='cpu', weights_only=False)
    e = ck['meta']['epoch']
    same = torch.load(str(d / f'epoch_{e}.pth'), map_location='cpu', weights_only=False)
    assert all(torch.equal(v, same['state_dict'][k]) for k, v in ck['state_dict'].items())
    assert ck['meta']['hook_msgs']['best_ckpt'].endswith(best[0])
    assert ck['meta']['hook_msgs']['best_score'] == float(dict((ep, lg) for ep, _, lg in lines)[e]['bbox_mAP'])


def _epoch_lines(stdout):
    return [re.sub(r' time: [0-9.]+ ', ' time: - ', ln) for ln in stdout.splitlines() if ln.startswith('Epoch [')]


def _first_difference(a, b):
    """the first tensor of two checkpoints' state_dict / optimizer momentum that differs, or None"""
    for k, v in a['state_dict'].items():
        if not torch.equal(v, b['state_dict'][k]):
            return f'state_dict[{k}]'
    sa, sb = a['optimizer']['state'], b['optimizer']['state']
    assert set(sa) == set(sb)
    for i in sorted(sa):
        if not torch.equal(sa[i]['momentum_buffer'], sb[i]['momentum_buffer']):
            return f'optimizer.state[{i}].momentum_buffer'
    return None


@pytest.mark.gpu
def test_validation_does_not_perturb_the_training_run(runs):
    """A (validated after both epochs) against B (--no-validate): the same ``Epoch [`` lines but for ``time:``, and
    bit-equal parameters and momentum buffers in epoch_2.pth.  The control comes first: B2 = B once more must reproduce
    B in exactly these terms (two runs of tools/train.py with one seed - loader threads, pipeline worker and all - are
    bit-identical), otherwise A == B would test nothing this feature controls."""
    _ok(runs, 'A', 'B', 'B2')
    d = runs['dir']
    la, lb, lb2 = (_epoch_lines(runs[n].stdout) for n in ('A', 'B', 'B2'))
    assert len(lb) == 8 and lb[0].startswith('Epoch [1][1/4]') and lb[-1].startswith('Epoch [2][4/4]')
    assert not _val_lines(runs['B'].stdout) and not [f for f in os.listdir(d / 'B') if f.startswith('best_')]
    ck = {n: torch.load(str(d / n / 'epoch_2.pth'), map_location='cpu', weights_only=False) for n in ('A', 'B', 'B2')}
    # the control
    diff = [i for i, (x, y) in enumerate(zip(lb, lb2)) if x != y]
    assert not diff, f'tools/train.py does not repeat itself: line {diff[0]}\n{lb[diff[0]]}\n{lb2[diff[0]]}'
    assert _first_difference(ck['B'], ck['B2']) is None, _first_difference(ck['B'], ck['B2'])
    # the feature
    diff = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    assert len(la) == len(lb) and not diff, f'first differing line {diff[0]}\n{la[diff[0]]}\n{lb[diff[0]]}'
    assert _first_difference(ck['A'], ck['B']) is None, _first_difference(ck['A'], ck['B'])
    assert ck['A']['meta']['iter'] == ck['B']['meta']['iter'] == 8
    # epoch_2.pth is written BEFORE the second validation (CheckpointHook first): it carries the best of epoch 1 only
    assert 'hook_msgs' not in ck['B']['meta'] and ck['A']['meta']['hook_msgs']['best_ckpt'].endswith('_epoch_1.pth')


VAL_CFG = dict(type='SyntheticCityscapes', img_shape=(256, 512), num_boxes=6, box_size=(16, 120), length=4, num_classes=8,
               pipeline=eval(VAL_PIPELINE))


@pytest.mark.gpu
def test_hook_between_steps_leaves_losses_parameters_and_random_streams_alone(dev):
    """in one process: two steps, a validation, two steps (and a second validation) against a twin that never validates
    - bit-equal losses and parameters; numpy's global stream, torch's CPU generator and the device generator are where
    they were across each hook call; the model is back in train mode with its BatchNorms in eval (norm_eval) and
    ``log_vars_on_host`` as set.  The second validation equals a fresh model carrying the same state."""
    import copy
    from torch.nn.modules.batchnorm import _BatchNorm
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from oadg_amd import Config, hip_conv
    from oadg_amd.apis import EvalHook, TrainEngine, build_optimizer, set_random_seed, single_gpu_test
    from oadg_amd.pipelines import DevicePipeline, SyntheticCityscapes
    from test_model_parity import CFG, build_and_load
    cfg = Config.fromfile(CFG)
    set_random_seed(0)
    det = build_and_load(dev).to(memory_format=torch.channels_last).train()
    det.log_vars_on_host = False
    ds = SyntheticCityscapes(img_shape=(256, 512), num_boxes=6, num_classes=8, box_size=(16, 120), seed=3, device=dev)
    pipe = DevicePipeline(cfg.data.train.pipeline, dtype=torch.bfloat16)
    set_random_seed(5)
    batches = [pipe(*ds.batch([2 * i, 2 * i + 1])) for i in range(4)]
    state0 = copy.deepcopy(det.state_dict())
    lines = []
    hook = EvalHook(interval=1, metric='bbox', logger=lines.append).build(VAL_CFG, dev, torch.bfloat16)
    last = {}

    def rng():
        return np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state(dev)

    def same_rng(a, b):
        return a[0][0] == b[0][0] and np.array_equal(a[0][1], b[0][1]) and a[0][2:] == b[0][2:] and \
            torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])

    def run(validate):
        det.load_state_dict(state0)
        det.train()
        eng = TrainEngine(det, build_optimizer(det, cfg.optimizer), amp_dtype=torch.bfloat16)
        hip_conv.refresh_prepared()
        set_random_seed(11)
        logs = []
        for i in range(4):
            out = eng.step({k: (list(v) if isinstance(v, list) else v) for k, v in batches[i].items()})
            torch.cuda.synchronize()
            logs.append({k: float(v) for k, v in out['log_vars'].items()})
            if validate and i in (1, 3):
                before = rng()
                if i == 1:
                    ev = hook.after_train_epoch(0, det)
                    assert ev is not None and 'bbox_mAP' in ev
                else:
                    last['results'] = hook.run_test(det)
                torch.cuda.synchronize()
                assert same_rng(before, rng()), 'a random stream moved during validation'
                assert det.training and det.log_vars_on_host is False
                assert not any(m.training for m in det.backbone.modules() if isinstance(m, _BatchNorm))
        return logs, {n: p.detach().clone() for n, p in det.named_parameters() if p.requires_grad}

    try:
        logs_v, params_v = run(True)
        logs_t, params_t = run(False)
        assert hook.validations == 1 and len([ln for ln in lines if ln.startswith('Epoch(val) [1][4] ')]) == 1
        assert all(np.isfinite(list(lg.values())).all() for lg in logs_t)
        for i, (a, b) in enumerate(zip(logs_v, logs_t)):
            assert a == b, (i, a, b)
        worst = [n for n in params_t if not torch.equal(params_v[n], params_t[n])]
        assert not worst, worst[:5]
        assert any(not torch.equal(params_t[n], state0[n].to(dev)) for n in params_t)          # (the steps did train)
        # the second validation ran with the weights of step 4: those of run(True), which run(False) has just reproduced
        fresh = build_and_load(dev).to(memory_format=torch.channels_last)
        fresh.load_state_dict(det.state_dict())
        results = single_gpu_test(fresh.eval(), hook.dataset, hook.pipe, torch.bfloat16, 1)
        assert sum(len(c) for r in results for c in r) > 0
        assert _same_results(last['results'], results)
    finally:
        hip_conv.enable(False)


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dev = torch.device('cuda:0')
    dist.init_process_group('gloo', rank=rank, world_size=world)
    import oadg_amd  # noqa: F401
    from oadg_amd import hip_conv
    from oadg_amd.apis import EvalHook, collect_results, set_random_seed, single_gpu_test
    from test_model_parity import build_and_load
    try:
        set_random_seed(0)
        det = build_and_load(dev).to(memory_format=torch.channels_last).train()
        hip_conv.enable()
        hook = EvalHook(interval=1, metric='bbox', logger=None).build(VAL_CFG, dev, torch.bfloat16)
        part = hook.run_test(det)
        merged = collect_results(part, len(hook.dataset))
        res = dict(rank=rank, n_part=len(part), merged=merged is not None, training=det.training)
        if rank == 0:
            alone = single_gpu_test(det.eval(), hook.dataset, hook.pipe, torch.bfloat16, 1)
            res.update(n=len(merged), same=_same_results(merged, alone), dets=sum(len(c) for r in alone for c in r),
                       ev=hook.dataset.evaluate(merged, metric='bbox') == hook.dataset.evaluate(alone, metric='bbox'))
        torch.cuda.synchronize()
        q.put(res)
        dist.barrier()
    finally:
        hip_conv.enable(False)
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_ranks_shard_the_val_set_and_rank_0_gets_the_single_process_results():
    """two gloo ranks on the one device (the pattern of tests/test_two_ranks_one_gpu.py): rank r tests images r, r + 2 of
    the 4-image val set, one ``all_gather_object``, rank 0's merged list == ``single_gpu_test`` alone, bit for bit"""
    import queue
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 28500 + os.getpid() % 2000
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out, t0 = [], time.time()
    try:
        while len(out) < len(procs):
            try:
                out.append(q.get(timeout=2))
            except queue.Empty:          # fail fast when a worker died instead of waiting out the timeout
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f'worker exited with {dead}'
                assert time.time() - t0 < 400, 'timed out waiting for the workers'
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    r0, r1 = sorted(out, key=lambda r: r['rank'])
    assert (r0['n_part'], r1['n_part']) == (2, 2) and r0['merged'] and not r1['merged']
    assert r0['training'] and r1['training']
    assert r0['n'] == 4 and r0['dets'] > 0 and r0['same'] and r0['ev'], r0
