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
"""
import argparse
import os
import pickle
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from train import DictAction  # noqa: E402
from oadg_amd.evaluation import average_precision, eval_map, evaluate  # noqa: E402,F401  (the metric functions live there)


def parse_args():
    p = argparse.ArgumentParser(description='test (and eval) a model')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help="checkpoint file ('none' = random init, for smoke runs)")
    p.add_argument('--work-dir', help='the directory to save the evaluation metrics')
    p.add_argument('--out', help='output result file in pickle format')
    p.add_argument('--eval', type=str, nargs='+', help="evaluation metrics: 'bbox' (COCO style), 'mAP' (VOC style AP@0.5)")
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


def main():
    a = parse_args()
    from oadg_amd import Config
    cfg = Config.fromfile(a.config)
    if a.cfg_options:
        cfg.merge_from_dict(a.cfg_options)
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)) % torch.cuda.device_count())
    dev = torch.device('cuda', torch.cuda.current_device())
    amp = torch.bfloat16 if a.amp == 'bf16' else None
    model = build_model(cfg, a.checkpoint, dev, amp, a.allow_partial_checkpoint)
    dcfg = cfg.data.test
    results, ds, dt = run_test(model, dcfg, dev, amp, cfg.data.get('samples_per_gpu', 1), a.max_samples,
                               show_dir=a.show_dir, show_score_thr=a.show_score_thr)
    n = len(results)
    print(f'{n} images in {dt:.2f} s ({n / dt:.1f} img/s), {sum(len(c) for r in results for c in r)} detections')
    if a.out:
        assert a.out.endswith(('.pkl', '.pickle')), 'The output file must be a pkl file.'
        with open(a.out, 'wb') as f:
            pickle.dump(results, f)
        print(f'writing results to {a.out}')
    if a.eval:
        assert set(a.eval) <= {'bbox', 'mAP'}, "--eval bbox (COCO style) and / or mAP (VOC style AP@0.5)"
        nc = len(getattr(ds, 'CLASSES', None) or range(dcfg.get('num_classes', 8)))
        ev = evaluate(results, ds, a.eval, nc, mmdet_style=True)
        if 'bbox' in ev:
            print('bbox (COCO style): ' + '  '.join(f'{k} {v:.3f}' for k, v in ev['bbox'].items()))
        if 'mAP' in ev:
            print(f"AP50 (eval_map, area): mAP {ev['mAP']['mAP']:.4f}  per class " +
                  ' '.join(f'{v:.3f}' for v in ev['mAP']['per_class']))
        if a.work_dir:
            import json
            os.makedirs(a.work_dir, exist_ok=True)
            with open(os.path.join(a.work_dir, 'eval.json'), 'w') as f:
                json.dump({k: (v if k == 'bbox' else dict(mAP=v['mAP'], per_class=list(v['per_class'])))
                           for k, v in ev.items()}, f, indent=1)


if __name__ == '__main__':
    main()
