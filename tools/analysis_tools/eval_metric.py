#!/usr/bin/env python
"""Evaluate saved detection results without running the model again, with the reference's CLI surface
(tools/analysis_tools/eval_metric.py:10-76):

    python tools/analysis_tools/eval_metric.py CONFIG PKL --eval bbox|mAP ... [--eval-options k=v ...] [--cfg-options k=v ...]
    python tools/analysis_tools/eval_metric.py CONFIG PKL --format-only [--eval-options jsonfile_prefix=P]

PKL is what ``tools/test.py --out`` wrote.  Builds ``data.test``, calls ``dataset.evaluate(results, metric=..., ...)`` with
the config's ``evaluation`` keywords (without the EvalHook's own) and ``--eval-options`` on top, and prints the dict it
returns.  The matching runs on the GPU when the library and a GPU are present (``device='auto'`` of the evaluators), on the
host otherwise - the same numbers.  ``--format-only`` calls ``dataset.format_results(results, **eval_options)`` instead (the
COCO-format datasets write ``P.bbox.json``, the file tools/analysis_tools/coco_error_analysis.py reads) and evaluates nothing.
"""
import argparse
import ast
import os
import pickle
import sys

TOOLS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TOOLS)
sys.path.insert(0, os.path.dirname(TOOLS))
from train import DictAction  # noqa: E402

HOOK_KEYS = ('interval', 'tmpdir', 'start', 'gpu_collect', 'save_best', 'rule', 'dynamic_intervals')   # eval_metric.py:70-74


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='Evaluate metric of the results saved in pkl format')
    p.add_argument('config', help='Config of the model')
    p.add_argument('pkl_results', help='Results in pickle format')
    p.add_argument('--format-only', action='store_true', help='Format the output results without perform evaluation: the COCO result file P.bbox.json of '
                        '--eval-options jsonfile_prefix=P')
    p.add_argument('--eval', type=str, nargs='+',
                   help='Evaluation metrics, which depends on the dataset: "bbox" for COCO / Cityscapes, "mAP" for PASCAL VOC')
    p.add_argument('--cfg-options', nargs='+', action=DictAction, help='override config entries, key=value')
    p.add_argument('--eval-options', nargs='+', action=DictAction,
                   help='custom options for evaluation, key=value: kwargs for dataset.evaluate()')
    a = p.parse_args(argv)
    if a.eval and a.format_only:
        raise ValueError('--eval and --format_only cannot be both specified')
    if not a.eval and not a.format_only:
        p.error('Please specify at least one metric with the argument "--eval"')
    return a


def _literal(v):
    try:
        return ast.literal_eval(v) if isinstance(v, str) else v
    except (ValueError, SyntaxError):
        return v


def main(argv=None):
    a = parse_args(argv)
    from oadg_amd import Config
    from oadg_amd.datasets import build_dataset
    cfg = Config.fromfile(a.config)
    if a.cfg_options:
        cfg.merge_from_dict(a.cfg_options)
    dataset = build_dataset(cfg.data.test, default_args=dict(device='cpu', test_mode=True))
    with open(a.pkl_results, 'rb') as f:
        outputs = pickle.load(f)
    if a.format_only:
        files, tmp_dir = dataset.format_results(outputs, **{k: _literal(v) for k, v in (a.eval_options or {}).items()})
        print(f'writing results to {files["bbox"]}' + (' (a temporary directory: pass --eval-options jsonfile_prefix=P to keep '
                                                       'it)' if tmp_dir is not None else ''))
        if tmp_dir is not None:
            tmp_dir.cleanup()
        return files
    eval_kwargs = dict(cfg.get('evaluation', {}))
    for key in HOOK_KEYS:
        eval_kwargs.pop(key, None)
    eval_kwargs.update(dict(metric=a.eval, **{k: _literal(v) for k, v in (a.eval_options or {}).items()}))
    print(dataset.evaluate(outputs, **eval_kwargs))


if __name__ == '__main__':
    main()
