#!/usr/bin/env python
"""Inference entry point with the reference's CLI surface (tools/test.py:24-130, single-GPU ``single_gpu_test``
apis/test.py): CONFIG CHECKPOINT [--out results.pkl] [--eval bbox] [--cfg-options k=v ...].

Runs ``model(return_loss=False, rescale=True, **data)`` over the test split through the device test pipeline and
collects one ``list[np.ndarray [k, 5]]`` (per class) per image, the format ``--out`` pickles in the reference.
``--show-dir DIR [--show-score-thr T]`` also writes every tested image with its detections painted on it
(oadg_amd/visualization.py: painted and PNG-encoded on the device, ``DIR/<ori_filename>.png``).
``--eval bbox`` reports the COCO-style numbers the reference's Cityscapes / COCO datasets report (AP@[.50:.95], AP50,
AP75, APs/m/l, AR...: oadg_amd/evaluation.py, a restatement of pycocotools' COCOeval, which this image does not have);
``--eval mAP`` the VOC-style AP@0.5 of mmdet/core/evaluation/mean_ap.py ``eval_map`` (area mode).
``--eval proposal | proposal_fast | recall [--eval-options k=v ...]`` score PROPOSALS (an 'RPN' detector, configs/rpn/, returns
one [n, 5] array per image; 'proposal' also takes detections) through ``evaluation.proposal_evaluate``: AR@100 / 300 / 1000 ...
as ``CocoDataset.evaluate`` reports them, recall@num@thr as the VOC-style datasets do - matched on the GPU (csrc/recall.hip).
With a proposal metric ``cfg.data.test`` may be a LIST of splits (configs/rpn/rpn_r101_dc5_1x_dwd_sdgod_test.py: the five
Diverse-Weather domains): the model is built once, every split is tested and scored in turn ('split <i>: ...', its dict; ``--out
X.pkl`` writes X_<i>.pkl, ``eval.json`` holds the list of dicts), then one line holds the recall at the largest budget per split
(AR@num with several ``iou_thr``, else recall@num@thr) and its mean.  The detection metrics of a list of splits are
tools/test_dwd.py's.
``--format-only [--eval-options jsonfile_prefix=P]`` writes the detections as a COCO result file, ``P.bbox.json``
(``CocoDataset.format_results``: what tools/analysis_tools/coco_error_analysis.py reads), and evaluates nothing.
"""
import argparse
import os
import pickle
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from train import DictAction  # noqa: E402
from oadg_amd.evaluation import (PROPOSAL_METRICS, average_precision, eval_map, evaluate,  # noqa: E402,F401
                                 proposal_evaluate)                  # (the metric functions live there)


def parse_args():
    p = argparse.ArgumentParser(description='test (and eval) a model')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help="checkpoint file ('none' = random init, for smoke runs)")
    p.add_argument('--work-dir', help='the directory to save the evaluation metrics')
    p.add_argument('--out', help='output result file in pickle format')
    p.add_argument('--format-only', action='store_true',
                   help='write the detections as a COCO result file (--eval-options jsonfile_prefix=P -> P.bbox.json) without '
                        'evaluating them')
    p.add_argument('--eval', type=str, nargs='+',
                   help="evaluation metrics: 'bbox' (COCO style), 'mAP' (VOC style AP@0.5); for proposals 'proposal', "
                        "'proposal_fast' (COCO style) or 'recall' (VOC style)")
    p.add_argument('--eval-options', nargs='+', action=DictAction,
                   help="keywords of the proposal metrics, key=value: proposal_nums, iou_thrs, iou_thr, metric_items; with "
                        "--format-only: jsonfile_prefix")
    p.add_argument('--cfg-options', nargs='+', action=DictAction, help='override config entries, key=value')
    p.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none')
    p.add_argument('--local_rank', type=int, default=0)
    p.add_argument('--max-samples', type=int, default=None, help='stop after this many images (smoke runs)')
    p.add_argument('--amp', default='bf16', choices=['bf16', 'none'])
    p.add_argument('--allow-partial-checkpoint', action='store_true',
                   help='evaluate even if the checkpoint lacks (or mis-sizes) some model tensors')
    add_show_arguments(p)
    a = p.parse_args()
    os.environ.setdefault('LOCAL_RANK', str(a.local_rank))
    check_show_arguments(a)
    if a.eval and a.format_only:
        raise ValueError('--eval and --format_only cannot be both specified')
    return a


def add_show_arguments(p):
    """tools/test.py:52-60 of the reference: --show, --show-dir, --show-score-thr"""
    p.add_argument('--show', action='store_true', help='show results in a window (not built: use --show-dir)')
    p.add_argument('--show-dir', help='directory where the painted images will be saved (PNG, painted and encoded on the device)')
    p.add_argument('--show-score-thr', type=float, default=0.3, help='score threshold of the painted detections (default: 0.3)')


def check_show_arguments(a):
    if a.show:
        raise NotImplementedError('--show (a window per image) is not built: there is no display here; --show-dir DIR '
                                  'writes the painted images instead')


def build_model(cfg, checkpoint, dev, amp, allow_partial=False):
    from oadg_amd import build_detector, hip_conv
    cfg.model.pop('pretrained', None)
    model = build_detector(cfg.model, test_cfg=cfg.get('test_cfg'))
    if checkpoint != 'none':
        from oadg_amd.checkpoint import load_checkpoint
        rep = load_checkpoint(model, checkpoint, map_location='cpu', strict=False, logger=print)
        print(f'{rep["path"]}: {rep["loaded"]} tensors loaded, {len(rep["missing"])} missing, '
              f'{len(rep["unexpected"])} unexpected, {len(rep["mismatched"])} size-mismatched')
        lost = [k for k in rep['missing'] + [m[0] for m in rep['mismatched']]
                if k.startswith(('backbone.', 'neck.', 'rpn_head.', 'roi_head.'))]
        if lost and not allow_partial:
            raise RuntimeError(f'{len(lost)} model tensors are not provided by {checkpoint} (e.g. {lost[:4]}): they '
                               f'would be evaluated at their random initial values; pass --allow-partial-checkpoint to '
                               f'do that anyway')
    else:
        model.init_weights(allow_missing_pretrained=True)
    model = model.to(dev).to(memory_format=torch.channels_last).eval()
    if amp is not None:
        hip_conv.enable()
    return model


def run_test(model, data_cfg, dev, amp, samples_per_gpu=1, max_samples=None, show_dir=None, show_score_thr=0.3):
    """single_gpu_test (apis/test.py:15-70) over one test-split config: (results, dataset, seconds)"""
    from oadg_amd.apis import single_gpu_test
    from oadg_amd.datasets import build_dataset
    from oadg_amd.pipelines import DevicePipeline
    ds = build_dataset(data_cfg, default_args=dict(seed=12345, device=dev, test_mode=True), synthetic_fallback=True)
    pipe = DevicePipeline(data_cfg['pipeline'], dtype=amp or torch.float32)
    t0 = time.time()
    results = single_gpu_test(model, ds, pipe, amp, samples_per_gpu, max_samples, show_dir=show_dir,
                              show_score_thr=show_score_thr)
    torch.cuda.synchronize()
    return results, ds, time.time() - t0


def count_rows(results):
    """'<k> detections' for per-class results, '<k> proposals' for the one-array-per-image results of an RPN detector"""
    if results and all(hasattr(r, 'shape') for r in results):
        return f'{sum(len(r) for r in results)} proposals'
    return f'{sum(len(r) if hasattr(r, "shape") else sum(len(c) for c in r) for r in results)} detections'


def format_only(ds, results, eval_options):
    """tools/test.py:263-264 of the reference: ``dataset.format_results(outputs, **eval_options)`` on the images that were
    tested -> the files it wrote.  Without ``jsonfile_prefix`` the file lives in a temporary directory that goes with this
    call, as in the reference: name a prefix to keep it."""
    D = _dwd_tool()
    if not hasattr(ds, 'format_results'):
        raise NotImplementedError(f'--format-only: {type(ds).__name__} has no format_results()')
    files, tmp_dir = D.first_images(ds, len(results)).format_results(
        results, **{k: D._literal(v) for k, v in (eval_options or {}).items()})
    print(f'writing results to {files["bbox"]}' + (' (a temporary directory: pass --eval-options jsonfile_prefix=P to keep it)'
                                                   if tmp_dir is not None else ''))
    if tmp_dir is not None:
        tmp_dir.cleanup()
    return files


def _dwd_tool():
    """tools/test_dwd.py by path: the home of ``first_images`` (--max-samples: what was tested is what is scored) and of
    ``_literal`` (--eval-options values as Python literals) - one copy of each, used by both tools"""
    import importlib.util
    spec = importlib.util.spec_from_file_location('oadg_tools_test_dwd',
                                                  os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_dwd.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def score_proposals(ds, results, metric, eval_options):
    """``proposal_evaluate`` on the images that were tested (the first len(results) of ``ds``).  A ConcatDataset is scored as
    ``ConcatDataset.evaluate`` scores it - every dataset on its own slice of the results, keys prefixed ``{k}_`` - except that
    a concatenation of ONE dataset (a one-entry ``ann_file`` list) keeps that dataset's plain keys."""
    D = _dwd_tool()
    kw = {k: D._literal(v) for k, v in (eval_options or {}).items()}
    ds = D.first_images(ds, len(results))
    parts = [d for d in ds.datasets if len(d)] if hasattr(ds, 'datasets') else [ds]
    if len(parts) == 1:
        return proposal_evaluate(parts[0], results, metric, logger='silent', **kw)
    out, start = {}, 0
    for k, d in enumerate(parts):
        for name, v in proposal_evaluate(d, results[start:start + len(d)], metric, logger='silent', **kw).items():
            out[f'{k}_{name}'] = v
        start += len(d)
    return out


def check_splits_arguments(a, n_splits):
    """what tools/test.py does with a list of splits, checked before the model is built"""
    if a.format_only:
        raise NotImplementedError(f'--format-only: cfg.data.test is a list of {n_splits} splits and a COCO result file holds one '
                                  f'split; name one split with --cfg-options')
    if not a.eval or len(a.eval) != 1 or a.eval[0] not in PROPOSAL_METRICS:
        raise NotImplementedError(f'cfg.data.test is a list of {n_splits} splits: tools/test.py walks it for one proposal '
                                  f'metric (--eval {" | ".join(PROPOSAL_METRICS)}); the detection metrics of a list of '
                                  f'splits are tools/test_dwd.py\'s')
    if a.out:
        assert a.out.endswith(('.pkl', '.pickle')), 'The output file must be a pkl file.'


def test_splits(a, cfg, model, dev, amp):
    """``cfg.data.test`` as a list of splits, for ONE proposal metric: every split tested and scored in turn, then a line with
    the recall at the largest budget per split and its mean"""
    import json
    metric, dicts = a.eval[0], []
    for i, dcfg in enumerate(cfg.data.test):
        show_dir = os.path.join(a.show_dir, f'split_{i}') if a.show_dir else None
        results, ds, dt = run_test(model, dcfg, dev, amp, cfg.data.get('samples_per_gpu', 1), a.max_samples,
                                   show_dir=show_dir, show_score_thr=a.show_score_thr)
        n = len(results)
        print(f'split {i}: {n} images in {dt:.2f} s ({n / dt:.1f} img/s), {count_rows(results)}')
        if a.out:
            root, ext = os.path.splitext(a.out)
            path = f'{root}_{i}{ext}'
            with open(path, 'wb') as f:
                pickle.dump(results, f)
            print(f'writing results to {path}')
        dicts.append(score_proposals(ds, results, metric, a.eval_options))
        print(f'{metric}: {dicts[-1]}')
        if a.work_dir:
            os.makedirs(a.work_dir, exist_ok=True)
            with open(os.path.join(a.work_dir, 'eval.json'), 'w') as f:
                json.dump({metric: dicts}, f, indent=1)
    # the recall at the largest budget: AR@num over several thresholds, recall@num@thr with a single one
    keys = [k for k in dicts[0] if k.startswith('AR@')] or [k for k in dicts[0] if k.startswith('recall@')]
    if keys:
        vals = [d[keys[-1]] for d in dicts]
        print(f'{keys[-1]} per split: ' + ' '.join(f'{v:.3f}' for v in vals) + f'  mean {sum(vals) / len(vals):.3f}')


def main():
    a = parse_args()
    from oadg_amd import Config
    cfg = Config.fromfile(a.config)
    if a.cfg_options:
        cfg.merge_from_dict(a.cfg_options)
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)) % torch.cuda.device_count())
    dev = torch.device('cuda', torch.cuda.current_device())
    amp = torch.bfloat16 if a.amp == 'bf16' else None
    if isinstance(cfg.data.test, (list, tuple)):
        check_splits_arguments(a, len(cfg.data.test))
    model = build_model(cfg, a.checkpoint, dev, amp, a.allow_partial_checkpoint)
    dcfg = cfg.data.test
    if isinstance(dcfg, (list, tuple)):
        return test_splits(a, cfg, model, dev, amp)
    results, ds, dt = run_test(model, dcfg, dev, amp, cfg.data.get('samples_per_gpu', 1), a.max_samples,
                               show_dir=a.show_dir, show_score_thr=a.show_score_thr)
    n = len(results)
    print(f'{n} images in {dt:.2f} s ({n / dt:.1f} img/s), {count_rows(results)}')
    return report(a, results, ds, dcfg)


def report(a, results, ds, dcfg):
    """what follows the test of one split: --out, then --format-only (nothing is evaluated) or --eval"""
    if a.out:
        assert a.out.endswith(('.pkl', '.pickle')), 'The output file must be a pkl file.'
        with open(a.out, 'wb') as f:
            pickle.dump(results, f)
        print(f'writing results to {a.out}')
    if a.format_only:
        return format_only(ds, results, a.eval_options)
    if a.eval:
        assert set(a.eval) <= {'bbox', 'mAP'} | set(PROPOSAL_METRICS), \
            "--eval bbox (COCO style), mAP (VOC style AP@0.5), proposal / proposal_fast / recall (proposals)"
        nc = len(getattr(ds, 'CLASSES', None) or range(dcfg.get('num_classes', 8)))
        ev = evaluate(results, ds, [m for m in a.eval if m not in PROPOSAL_METRICS], nc, mmdet_style=True)
        for m in a.eval:
            if m in PROPOSAL_METRICS:
                ev[m] = score_proposals(ds, results, m, a.eval_options)
                print(f'{m}: {ev[m]}')                      # (the reference's dict, floats at full precision)
        if 'bbox' in ev:
            print('bbox (COCO style): ' + '  '.join(f'{k} {v:.3f}' for k, v in ev['bbox'].items()))
        if 'mAP' in ev:
            print(f"AP50 (eval_map, area): mAP {ev['mAP']['mAP']:.4f}  per class " +
                  ' '.join(f'{v:.3f}' for v in ev['mAP']['per_class']))
        if a.work_dir:
            import json
            os.makedirs(a.work_dir, exist_ok=True)
            with open(os.path.join(a.work_dir, 'eval.json'), 'w') as f:
                json.dump({k: (dict(mAP=v['mAP'], per_class=list(v['per_class'])) if k == 'mAP' else v)
                           for k, v in ev.items()}, f, indent=1)


if __name__ == '__main__':
    main()
