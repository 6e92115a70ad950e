#!/usr/bin/env python
"""The Diverse-Weather test loop with the reference's CLI surface (tools/test_dwd.py:23-113, 193-254): CONFIG CHECKPOINT
--eval mAP [--out X.pkl] [--work-dir D] [--cfg-options k=v ...] [--eval-options k=v ...], plus tools/test.py's
--max-samples, --amp and --allow-partial-checkpoint.

``cfg.data.test`` is a list of splits (configs/oadg/faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod_test.py: daytime-clear, foggy,
dusk-rainy, night-rainy, night-sunny).  The model is built and loaded ONCE (the reference rebuilds it per split); every
split is tested with tools/test.py's ``run_test`` and scored by ``dataset.evaluate`` with the config's ``evaluation``
keywords minus the EvalHook's own (test_dwd.py:242-250) - for SdgodDataset the VOC07 protocol, matched on the GPU
(csrc/voc_eval.hip).  Prints the reference's metric dict per split, then one summary line with
the per-split AP50 and their mean; ``--work-dir`` receives eval_<timestamp>.json with the list of per-split dicts;
``--out X.pkl`` with several splits writes X_<i>.pkl.
"""
import argparse
import ast
import copy
import importlib.util
import json
import os
import pickle
import sys
import time

import numpy as np
import torch

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(TOOLS))
sys.path.insert(0, TOOLS)
from train import DictAction  # noqa: E402

HOOK_KEYS = ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best', 'rule', 'dynamic_intervals')    # test_dwd.py:244-248


def _tools_test():
    """tools/test.py by path (its module name would be the standard library's ``test``)"""
    spec = importlib.util.spec_from_file_location('oadg_tools_test', os.path.join(TOOLS, 'test.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parse_args():
    p = argparse.ArgumentParser(description='test (and eval) a model on every split of cfg.data.test')
    p.add_argument('config', help='test config file path')
    p.add_argument('checkpoint', help="checkpoint file ('none' = random init, for smoke runs)")
    p.add_argument('--work-dir', help='the directory to save the file containing evaluation metrics')
    p.add_argument('--out', help='output result file in pickle format (several splits: X_<i>.pkl)')
    p.add_argument('--eval', type=str, nargs='+', help="evaluation metrics, e.g. 'mAP' for the VOC-style datasets")
    p.add_argument('--cfg-options', nargs='+', action=DictAction, help='override config entries, key=value')
    p.add_argument('--options', nargs='+', action=DictAction, help='deprecated alias of --eval-options')
    p.add_argument('--eval-options', nargs='+', action=DictAction, help='keywords for dataset.evaluate(), key=value')
    p.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none')
    p.add_argument('--local_rank', type=int, default=0)
    p.add_argument('--max-samples', type=int, default=None, help='stop after this many images per split (smoke runs)')
    p.add_argument('--amp', default='bf16', choices=['bf16', 'none'])
    p.add_argument('--allow-partial-checkpoint', action='store_true',
                   help='evaluate even if the checkpoint lacks (or mis-sizes) some model tensors')
    a = p.parse_args()
    os.environ.setdefault('LOCAL_RANK', str(a.local_rank))
    if a.options and a.eval_options:
        raise ValueError('--options and --eval-options cannot be both specified, --options is deprecated in favor of '
                         '--eval-options')
    if a.options:
        a.eval_options = a.options
    assert a.out or a.eval, 'Please specify at least one operation (save / eval the results) with "--out" or "--eval"'
    if a.out is not None and not a.out.endswith(('.pkl', '.pickle')):
        raise ValueError('The output file must be a pkl file.')
    return a


def _literal(v):
    try:
        return ast.literal_eval(v) if isinstance(v, str) else v
    except (ValueError, SyntaxError):
        return v


def first_images(ds, n):
    """a shallow copy of a dataset that holds its first ``n`` images (--max-samples: what was tested is what is scored)"""
    if n >= len(ds):
        return ds
    c = copy.copy(ds)
    if hasattr(ds, 'datasets'):
        c.datasets, left = [], n
        for d in ds.datasets:
            k = min(len(d), left)
            c.datasets.append(first_images(d, k))
            left -= k
        c.cumulative_sizes = np.cumsum([len(d) for d in c.datasets]).tolist()
    elif hasattr(ds, 'data_infos'):
        c.data_infos = ds.data_infos[:n]
    else:
        c.length = n
    return c


def eval_kwargs_of(cfg, metrics, eval_options):
    """test_dwd.py:242-249: the config's ``evaluation`` keywords without the hook's, the metric(s) of --eval, --eval-options"""
    kw = dict(cfg.get('evaluation', {}))
    for key in HOOK_KEYS:
        kw.pop(key, None)
    kw.update(dict(metric=metrics, **{k: _literal(v) for k, v in (eval_options or {}).items()}))
    return kw


def main():
    a = parse_args()
    from oadg_amd import Config
    T = _tools_test()
    cfg = Config.fromfile(a.config)
    if a.cfg_options:
        cfg.merge_from_dict(a.cfg_options)
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)) % torch.cuda.device_count())
    dev = torch.device('cuda', torch.cuda.current_device())
    amp = torch.bfloat16 if a.amp == 'bf16' else None
    splits = cfg.data.test if isinstance(cfg.data.test, (list, tuple)) else [cfg.data.test]
    json_file = None
    if a.work_dir is not None:
        os.makedirs(os.path.abspath(a.work_dir), exist_ok=True)
        json_file = os.path.join(a.work_dir, f"eval_{time.strftime('%Y%m%d_%H%M%S', time.localtime())}.json")
    model = T.build_model(cfg, a.checkpoint, dev, amp, a.allow_partial_checkpoint)
    metrics = []
    for i, dcfg in enumerate(splits):
        results, ds, dt = T.run_test(model, dcfg, dev, amp, cfg.data.get('samples_per_gpu', 1), a.max_samples)
        n = len(results)
        print(f'split {i}: {n} images in {dt:.2f} s ({n / dt:.1f} img/s), {sum(len(c) for r in results for c in r)} detections')
        if a.out:
            root, ext = os.path.splitext(a.out)
            path = a.out if len(splits) == 1 else f'{root}_{i}{ext}'
            print(f'\nwriting results to {path}')
            with open(path, 'wb') as f:
                pickle.dump(results, f)
        if a.eval:
            metric = first_images(ds, n).evaluate(results, **eval_kwargs_of(cfg, a.eval, a.eval_options))
            print(metric)
            metrics.append(dict(config=a.config, metric=metric))
            if json_file is not None:
                with open(json_file, 'w') as f:
                    json.dump(metrics, f, indent=1)
    if a.eval:
        ap50 = [next((v for k, v in m['metric'].items() if k.endswith('AP50')), None) for m in metrics]
        if all(v is not None for v in ap50):
            print('AP50 per split: ' + ' '.join(f'{v:.3f}' for v in ap50) + f'  mean {sum(ap50) / len(ap50):.3f}')


if __name__ == '__main__':
    main()
