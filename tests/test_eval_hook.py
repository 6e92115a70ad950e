"""Validation during training without a GPU: ``parse_evaluation`` (what an ``evaluation`` config key turns into, and what
it rejects by name before any training work), the schedule of ``EvalHook`` against mmcv's ``_should_evaluate`` written
out here, ``save_best`` with a scripted evaluator, ``dataset.evaluate`` against the evaluators it is built on, and the
reordering of sharded results in a real world of two gloo ranks.  Reference: mmcv/runner/hooks/evaluation.py,
mmdet/core/evaluation/eval_hooks.py, mmdet/apis/test.py:126-169, mmdet/datasets/{coco,voc}.py."""
import os
import queue
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oadg_amd  # noqa: F401
from oadg_amd import Config, evaluation as E
from oadg_amd.apis import EvalHook, merge_sharded_results, parse_evaluation, shard_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_PIPELINE = [dict(type='LoadImageFromFile'),
                 dict(type='MultiScaleFlipAug', img_scale=(512, 256), flip=False,
                      transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                                  dict(type='Normalize', mean=[0, 0, 0], std=[1, 1, 1], to_rgb=True),
                                  dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                                  dict(type='Collect', keys=['img'])])]


def _cfg(evaluation=None, val_type='SyntheticCityscapes'):
    d = dict(data=dict(val=dict(type=val_type, pipeline=TEST_PIPELINE)))
    if evaluation is not None:
        d['evaluation'] = evaluation
    return Config(d)


# ------------------------------------------------------------------------------------------------ parsing and rejection
def test_parse_evaluation_none_without_the_key_or_with_no_validate():
    assert parse_evaluation(_cfg(), False) is None
    assert parse_evaluation(_cfg(dict(interval=1, metric='bbox')), True) is None
    kw = parse_evaluation(_cfg(dict(interval=1, metric='bbox')), False)
    assert kw == dict(interval=1, start=None, metric='bbox', save_best=None, rule=None, eval_kwargs={})
    kw = parse_evaluation(_cfg(dict(interval=2, start=3, metric=['bbox'], save_best='auto', rule='greater',
                                    metric_items=['mAP', 'mAP_50'], proposal_nums=(1, 10, 100), classwise=None)), False)
    assert kw == dict(interval=2, start=3, metric=['bbox'], save_best='auto', rule='greater',
                      eval_kwargs=dict(metric_items=['mAP', 'mAP_50'], proposal_nums=(1, 10, 100)))
    assert EvalHook(**kw).eval_kwargs == kw['eval_kwargs']
    # the VOC-style datasets take 'mAP' (and default to it, as voc.py does)
    kw = parse_evaluation(_cfg(dict(interval=1, iou_thr=0.5), val_type='SdgodDataset'), False)
    assert kw['metric'] == 'mAP' and kw['eval_kwargs'] == dict(iou_thr=0.5)


@pytest.mark.parametrize('evaluation, val_type, exc, names', [
    (dict(metric='segm'), 'CityscapesDataset', NotImplementedError, ("'segm'", 'CityscapesDataset')),
    (dict(metric=['bbox', 'proposal']), 'CocoDataset', NotImplementedError, ("'proposal'", 'CocoDataset')),
    (dict(metric='proposal_fast'), 'SyntheticCityscapes', NotImplementedError, ("'proposal_fast'", 'SyntheticCityscapes')),
    (dict(metric='recall'), 'SdgodDataset', NotImplementedError, ("'recall'", 'SdgodDataset')),
    (dict(metric='bbox'), 'XMLDataset', KeyError, ('bbox', 'XMLDataset')),
    (dict(metric='nonsense'), 'CocoDataset', KeyError, ('nonsense',)),
    (dict(metric='bbox', classwise=True), 'CityscapesDataset', NotImplementedError, ("'classwise'", 'CityscapesDataset')),
    (dict(metric='bbox', iou_thrs=[0.5]), 'CocoDataset', NotImplementedError, ("'iou_thrs'",)),
    (dict(metric='bbox', jsonfile_prefix='x'), 'CocoDataset', NotImplementedError, ("'jsonfile_prefix'",)),
    (dict(metric='mAP', scale_ranges=[(0, 32)]), 'SdgodDataset', NotImplementedError, ("'scale_ranges'",)),
    (dict(metric='bbox', iou_thr=0.5), 'CocoDataset', TypeError, ("'iou_thr'",)),          # a keyword of the OTHER protocol
    (dict(metric='bbox', no_such_argument=1), 'CocoDataset', TypeError, ("'no_such_argument'",)),
    (dict(metric='bbox', dynamic_intervals=[(2, 1)]), 'CocoDataset', TypeError, ("'dynamic_intervals'",)),
    (dict(metric='bbox', by_epoch=False), 'CocoDataset', NotImplementedError, ('by_epoch=False',)),
    (dict(metric='bbox', rule='bigger'), 'CocoDataset', KeyError, ('bigger',)),
    (dict(metric='bbox', save_best='speed'), 'CocoDataset', ValueError, ('speed',)),
    (dict(metric='bbox', interval=0), 'CocoDataset', ValueError, ('interval',)),
])
def test_parse_evaluation_rejects_by_name_before_any_work(evaluation, val_type, exc, names):
    with pytest.raises(exc) as e:
        parse_evaluation(_cfg(evaluation, val_type), False)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_train_cli_help_no_longer_calls_evaluation_out_of_scope():
    src = open(os.path.join(ROOT, 'tools', 'train.py')).read()
    assert 'evaluation is out of scope' not in src and 'parse_evaluation(cfg, a.no_validate)' in src


# ------------------------------------------------------------------------------------------------ schedule
def _mmcv_should_evaluate(epoch, interval, start):
    """mmcv EvalHook._should_evaluate, by_epoch: ``epoch`` = runner.epoch inside after_train_epoch"""
    if start is None:
        if (epoch + 1) % interval != 0:          # every_n_epochs(runner, interval)
            return False
    elif (epoch + 1) < start:
        return False
    else:
        if (epoch + 1 - start) % interval:
            return False
    return True


def _mmcv_run(first_epoch, max_epochs, interval, start):
    """the epochs (1-based, as logged) after which an mmcv run validates; 'before' = before_train_epoch's initial_flag"""
    out, initial = [], True
    for epoch in range(first_epoch, max_epochs):
        if initial:
            if start is not None and epoch >= start and _mmcv_should_evaluate(epoch, interval, start):
                out.append(('before', epoch + 1))
            initial = False
        if _mmcv_should_evaluate(epoch, interval, start):
            out.append(('after', epoch + 1))
    return out


@pytest.mark.parametrize('first_epoch, interval, start, expect', [
    (0, 1, None, [('after', e) for e in range(1, 9)]),
    (0, 2, None, [('after', e) for e in (2, 4, 6, 8)]),
    (0, 2, 3, [('after', e) for e in (3, 5, 7)]),
    (0, 1, 0, [('before', 1)] + [('after', e) for e in range(1, 9)]),
    (4, 2, 3, [('before', 5), ('after', 5), ('after', 7)]),   # resumed past start, on the interval's phase: once before training
    (5, 2, 3, [('after', 7)]),                                # resumed past start, off phase: before_run's check says no
    (5, 1, 3, [('before', 6), ('after', 6), ('after', 7), ('after', 8)]),
    (5, 1, None, [('after', e) for e in (6, 7, 8)]),   # resumed without start: nothing before training
])
def test_schedule_follows_mmcv_should_evaluate(first_epoch, interval, start, expect):
    assert _mmcv_run(first_epoch, 8, interval, start) == expect          # (the table is what the written-out rule gives)
    seen = []
    hook = EvalHook(interval=interval, start=start, logger=None)
    hook.validate = lambda epoch, model, state_fn=None: seen.append((phase[0], epoch + 1))
    phase = ['before']
    for epoch in range(first_epoch, 8):
        phase[0] = 'before'
        hook.before_train_epoch(epoch, None)
        phase[0] = 'after'
        hook.after_train_epoch(epoch, None)
    assert seen == expect
    for epoch in range(12):
        assert hook.should_evaluate(epoch) == _mmcv_should_evaluate(epoch, interval, start)


# ------------------------------------------------------------------------------------------------ save_best
class _Scripted:
    """a val set of three images whose evaluate() returns the next scripted dict"""

    def __init__(self, script):
        self.script, self.calls = list(script), 0

    def __len__(self):
        return 3

    def evaluate(self, results, metric='bbox', logger=None, **kw):
        self.calls += 1
        return dict(self.script.pop(0))


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.log_vars_on_host = False


def _scripted_hook(tmp_path, scores, key='bbox_mAP', lines=None, **kw):
    hook = EvalHook(work_dir=str(tmp_path), logger=(lines.append if lines is not None else None),
                    test_fn=lambda model: [None] * 3, **kw)
    hook.dataset = _Scripted([{key: s, 'bbox_mAP_50': 0.5, 'bbox_mAP_copypaste': 'x'} for s in scores])
    return hook


def _best_files(tmp_path):
    return sorted(f for f in os.listdir(tmp_path) if f.startswith('best_'))


def test_save_best_rotates_keeps_ties_and_logs_one_val_line(tmp_path):
    lines, model = [], _Model().train()
    hook = _scripted_hook(tmp_path, [0.10, 0.30, 0.30, 0.20, 0.31], lines=lines, save_best='auto')
    seen = []
    for epoch in range(5):
        with torch.no_grad():
            model.w.fill_(float(epoch))
        hook.after_train_epoch(epoch, model, lambda: dict(state_dict={k: v.clone() for k, v in model.state_dict().items()},
                                                          meta=dict(epoch=epoch + 1)))
        seen.append((_best_files(tmp_path), hook.best_score))
        assert model.training and model.log_vars_on_host is False          # the mode switch is undone
    assert seen == [(['best_bbox_mAP_epoch_1.pth'], 0.10), (['best_bbox_mAP_epoch_2.pth'], 0.30),
                    (['best_bbox_mAP_epoch_2.pth'], 0.30),                 # a tie does not replace: the rule is strict
                    (['best_bbox_mAP_epoch_2.pth'], 0.30), (['best_bbox_mAP_epoch_5.pth'], 0.31)]
    assert hook.key_indicator == 'bbox_mAP' and hook.rule == 'greater'     # 'auto': first key, rule from its name
    ck = torch.load(tmp_path / 'best_bbox_mAP_epoch_5.pth', weights_only=False)
    assert float(ck['state_dict']['w']) == 4.0 and ck['meta']['epoch'] == 5
    assert ck['meta']['hook_msgs'] == dict(best_score=0.31, best_ckpt=str(tmp_path / 'best_bbox_mAP_epoch_5.pth'))
    val = [ln for ln in lines if ln.startswith('Epoch(val) ')]
    assert len(val) == 5 and not any(ln.startswith('Epoch [') for ln in lines)
    assert val[1] == 'Epoch(val) [2][3] bbox_mAP: 0.3000, bbox_mAP_50: 0.5000, bbox_mAP_copypaste: x'


def test_save_best_rule_less_named_key_and_inferred_rules(tmp_path):
    hook = _scripted_hook(tmp_path, [0.5, 0.7, 0.4, 0.4], key='loss_val', save_best='loss_val')
    assert hook.rule == 'less'
    for epoch in range(4):
        hook.after_train_epoch(epoch, _Model(), lambda: dict(meta={}))
    assert _best_files(tmp_path) == ['best_loss_val_epoch_3.pth'] and hook.best_score == 0.4
    # an explicit rule wins over the key's name; a named key that evaluate does not return is an error, not a silent skip
    hook = _scripted_hook(tmp_path / 'x', [0.5, 0.4], save_best='bbox_mAP', rule='less')
    os.makedirs(tmp_path / 'x')
    for epoch in range(2):
        hook.after_train_epoch(epoch, _Model(), lambda: dict(meta={}))
    assert _best_files(tmp_path / 'x') == ['best_bbox_mAP_epoch_2.pth']
    hook = _scripted_hook(tmp_path, [0.5], save_best='AR@100')
    with pytest.raises(KeyError, match='AR@100'):
        hook.after_train_epoch(0, _Model(), lambda: dict(meta={}))
    for key, rule in (('bbox_mAP', 'greater'), ('AP50', 'greater'), ('AR@100', 'greater'), ('acc', 'greater'),
                      ('loss', 'less'), ('loss_bbox', 'less')):
        assert EvalHook.infer_rule(key) == rule
    with pytest.raises(ValueError, match='speed'):
        EvalHook.infer_rule('speed')
    assert EvalHook(save_best=None).hook_msgs() is None


def test_hook_msgs_survive_a_resume(tmp_path):
    """the best score travels in meta.hook_msgs: a resumed run does not start from minus infinity"""
    first = _scripted_hook(tmp_path, [0.2, 0.6], save_best='auto')
    for epoch in range(2):
        first.after_train_epoch(epoch, _Model(), lambda: dict(meta={}))
    msgs = first.hook_msgs()
    assert msgs == dict(best_score=0.6, best_ckpt=str(tmp_path / 'best_bbox_mAP_epoch_2.pth'))
    later = dict(state_dict={}, meta=dict(epoch=2, hook_msgs=msgs))          # what every later checkpoint carries
    torch.save(later, tmp_path / 'epoch_2.pth')
    resumed = _scripted_hook(tmp_path, [0.5, 0.61], save_best='auto')
    resumed.restore(torch.load(tmp_path / 'epoch_2.pth', weights_only=False)['meta'].get('hook_msgs'))
    resumed.after_train_epoch(2, _Model(), lambda: dict(meta={}))
    assert _best_files(tmp_path) == ['best_bbox_mAP_epoch_2.pth'] and resumed.best_score == 0.6      # 0.5 is no new best
    resumed.after_train_epoch(3, _Model(), lambda: dict(meta={}))
    assert _best_files(tmp_path) == ['best_bbox_mAP_epoch_4.pth'] and resumed.best_score == 0.61     # the old file is removed
    fresh = _scripted_hook(tmp_path / 'y', [0.5], save_best='auto')
    os.makedirs(tmp_path / 'y')
    fresh.restore(None)
    fresh.after_train_epoch(2, _Model(), lambda: dict(meta={}))
    assert fresh.best_score == 0.5                                           # without hook_msgs: from minus infinity


# ------------------------------------------------------------------------------------------------ dataset.evaluate
def _three_image_set_and_results():
    from oadg_amd.pipelines import SyntheticCityscapes
    ds = SyntheticCityscapes(img_shape=(256, 512), num_boxes=5, num_classes=3, length=3, box_size=(16, 200), seed=7,
                             device='cpu', test_mode=True)
    rs = np.random.RandomState(0)
    results = []
    for i in range(len(ds)):
        b, l = ds.boxes(i)
        per_class = []
        for c in range(3):
            g = b[l == c]
            hit = g + rs.uniform(-6, 6, g.shape).astype(np.float32)          # jittered ground truth: IoU varies with the size
            miss = np.array([[10., 10., 60., 40.], [300., 100., 420., 230.]], np.float32)[:rs.randint(0, 3)]
            boxes = np.concatenate([hit, miss])
            per_class.append(np.concatenate([boxes, rs.uniform(0.05, 1, (len(boxes), 1)).astype(np.float32)], 1))
        results.append(per_class)
    return ds, results


def test_dataset_evaluate_bbox_is_the_mmdet_style_coco_numbers_rounded():
    ds, results = _three_image_set_and_results()
    want = E.coco_eval_bbox(E.dataset_gt_anns(ds), results, 3, max_dets=E.MMDET_MAX_DETS, names=E.MMDET_METRICS)
    assert 0 < want['mAP'] < 1 and want['mAP'] < want['mAP_50']                       # a case where the numbers say something
    got = ds.evaluate(results, metric='bbox')
    assert list(got) == ['bbox_mAP', 'bbox_mAP_50', 'bbox_mAP_75', 'bbox_mAP_s', 'bbox_mAP_m', 'bbox_mAP_l',
                         'bbox_mAP_copypaste']
    for k in E.MMDET_METRICS[:6]:
        assert isinstance(got[f'bbox_{k}'], float) and got[f'bbox_{k}'] == float(f'{want[k]:.3f}'), k
    assert got['bbox_mAP_copypaste'] == ' '.join(f'{want[k]:.3f}' for k in E.MMDET_METRICS[:6])
    # not COCOeval's defaults (maxDets 1 / 10 / 100): one detection per image and class is a different number here
    assert E.coco_eval_bbox(E.dataset_gt_anns(ds), results, 3)['AR1'] != want['AR@100']
    assert ds.evaluate(results, metric=['bbox']) == got
    some = ds.evaluate(results, metric='bbox', metric_items=['mAP_50', 'AR@100'], proposal_nums=(100, 300, 1000))
    assert list(some) == ['bbox_mAP_50', 'bbox_AR@100', 'bbox_mAP_copypaste'] and some['bbox_mAP_50'] == got['bbox_mAP_50']
    with pytest.raises(NotImplementedError, match="'segm'.*SyntheticCityscapes"):
        ds.evaluate(results, metric='segm')
    with pytest.raises(NotImplementedError, match="'classwise'"):
        ds.evaluate(results, metric='bbox', classwise=True)
    with pytest.raises(KeyError, match='mAP_xl'):
        ds.evaluate(results, metric='bbox', metric_items=['mAP_xl'])


def test_dataset_evaluate_map_is_eval_map():
    ds, results = _three_image_set_and_results()
    anns = [ds.boxes(i) for i in range(len(ds))]
    m50, _ = E.eval_map(results, anns, 3, iou_thr=0.5)
    m75, _ = E.eval_map(results, anns, 3, iou_thr=0.75)
    assert 0 < m75 < m50 <= 1
    got = ds.evaluate(results, metric='mAP')
    assert list(got) == ['AP50', 'mAP'] and got['AP50'] == round(m50, 3) and got['mAP'] == m50
    two = ds.evaluate(results, metric='mAP', iou_thr=[0.5, 0.75])
    assert list(two) == ['AP50', 'AP75', 'mAP'] and two['AP75'] == round(m75, 3) and two['mAP'] == (m50 + m75) / 2
    # the tools import the same functions back
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location('oadg_tools_test_eval', os.path.join(ROOT, 'tools', 'test.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    assert mod.eval_map is E.eval_map and mod.evaluate is E.evaluate and mod.average_precision is E.average_precision


def test_file_datasets_carry_the_protocol_of_their_reference_class():
    from oadg_amd.datasets import CityscapesDataset, CocoDataset, SdgodDataset, XMLDataset
    for cls in (CocoDataset, CityscapesDataset):
        assert cls.EVAL_PROTOCOLS == (E.COCO_EVAL,) and callable(cls.evaluate)
    for cls in (XMLDataset, SdgodDataset):
        assert cls.EVAL_PROTOCOLS == (E.VOC_EVAL,) and callable(cls.evaluate)


# ------------------------------------------------------------------------------------------------ gather reordering
def test_merge_sharded_results_in_one_process():
    for n, world in ((5, 2), (4, 2), (1, 2), (7, 3), (0, 2)):
        parts = [[f'img{i}' for i in shard_indices(n, r, world)] for r in range(world)]
        assert merge_sharded_results(parts, n) == [f'img{i}' for i in range(n)]
    # the reference pads the shards to equal length (DistributedSampler): the surplus is cut
    assert merge_sharded_results([['a', 'c', 'a'], ['b', 'd', 'b']], 4) == ['a', 'b', 'c', 'd']


def _gather_worker(rank, world, port, q, sizes):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        import oadg_amd  # noqa: F401
        from oadg_amd.apis import collect_results, shard_indices
        out = {}
        for n in sizes:
            # a result per image as single_gpu_test returns it: a list over classes of [k, 5] arrays, here marked by index
            part = [[np.full((i % 3, 5), i, np.float32), np.full((1, 5), -i, np.float32)] for i in shard_indices(n, rank, world)]
            out[n] = (len(part), collect_results(part, n))
        q.put((rank, out))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_results_come_back_in_dataset_order_on_rank_0():
    """world of two over gloo: odd and even lengths, and a val set of ONE image (rank 1 tests nothing and must neither
    deadlock the gather nor shift the order)"""
    sizes = (5, 4, 1)
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q, sizes)) for r in range(2)]
    for p in procs:
        p.start()
    res, t0 = {}, time.time()
    try:
        while len(res) < 2:
            try:
                rank, out = q.get(timeout=2)
                res[rank] = out
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f'worker exited with {dead}'
                assert time.time() - t0 < 240, 'timed out waiting for the workers'
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for n in sizes:
        n0, merged = res[0][n]
        n1, other = res[1][n]
        assert (n0, n1) == ((n + 1) // 2, n // 2) and other is None          # rank 1 only waits
        assert len(merged) == n
        for i, r in enumerate(merged):
            assert r[0].shape == (i % 3, 5) and (r[0] == i).all() and (r[1] == -i).all(), (n, i)
