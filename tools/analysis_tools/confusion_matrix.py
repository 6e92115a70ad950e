#!/usr/bin/env python
"""Confusion matrix of saved detection results, with the reference's CLI surface
(tools/analysis_tools/confusion_matrix.py:15-56, 226-257):

    python tools/analysis_tools/confusion_matrix.py CONFIG PKL SAVE_DIR [--color-theme plasma] [--score-thr 0.3]
        [--tp-iou-thr 0.5] [--nms-iou-thr T] [--cfg-options k=v ...]

PKL is what ``tools/test.py --out`` wrote.  The counts come from ``oadg_amd.evaluation.calculate_confusion_matrix``: the
split is packed once and counted in one launch of csrc/confusion.hip when the library and a GPU are present, on the host
otherwise - the same integers either way.  Written to SAVE_DIR: ``confusion_matrix.png``, the reference's matplotlib plot
(rows normalised to per cent), and - an addition - ``confusion_matrix.json`` with the raw counts and the class names plus
``background``.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TOOLS)
sys.path.insert(0, os.path.dirname(TOOLS))
from train import DictAction  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='Generate confusion matrix from detection results.  A row of the matrix whose sum is 0 (a class '
                    'without a box and, for the background row, a split without a background false positive) is printed '
                    'as 0%%; the reference raises there (int(nan)).')
    p.add_argument('config', help='test config file path')
    p.add_argument('prediction_path', help='prediction path where test .pkl result')
    p.add_argument('save_dir', help='directory where confusion matrix will be saved')
    p.add_argument('--show', action='store_true', help='show confusion matrix in a window (not built: the plot is saved)')
    p.add_argument('--color-theme', default='plasma', help='theme of the matrix color map')
    p.add_argument('--score-thr', type=float, default=0.3, help='score threshold to filter detection bboxes')
    p.add_argument('--tp-iou-thr', type=float, default=0.5, help='IoU threshold to be considered as matched')
    p.add_argument('--nms-iou-thr', type=float, default=None,
                   help='nms IoU threshold, only applied when users want to change the nms IoU threshold.')
    p.add_argument('--cfg-options', nargs='+', action=DictAction, help='override config entries, key=value')
    p.add_argument('--device', default='auto', choices=['auto', 'host'],
                   help="where the counts are made: 'auto' = the GPU when the library and a GPU are present, 'host'")
    a = p.parse_args(argv)
    if a.show:
        raise NotImplementedError('--show (a window) is not built: there is no display here; the plot is written to '
                                  'SAVE_DIR/confusion_matrix.png')
    return a


def plot_confusion_matrix(confusion_matrix, labels, save_dir=None, title='Normalized Confusion Matrix', color_theme='plasma'):
    """confusion_matrix.py:145-223 with the Agg backend; a row whose sum is 0 is a row of 0%"""
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from matplotlib.ticker import MultipleLocator
    per_label_sums = confusion_matrix.sum(axis=1)[:, np.newaxis]
    with np.errstate(divide='ignore', invalid='ignore'):
        confusion_matrix = confusion_matrix.astype(np.float32) / per_label_sums * 100
    confusion_matrix = np.where(per_label_sums > 0, confusion_matrix, np.float32(0))
    num_classes = len(labels)
    fig, ax = plt.subplots(figsize=(0.5 * num_classes, 0.5 * num_classes * 0.8), dpi=180)
    im = ax.imshow(confusion_matrix, cmap=plt.get_cmap(color_theme))
    plt.colorbar(mappable=im, ax=ax)
    ax.set_title(title, fontdict={'weight': 'bold', 'size': 12})
    label_font = {'size': 10}
    plt.ylabel('Ground Truth Label', fontdict=label_font)
    plt.xlabel('Prediction Label', fontdict=label_font)
    ax.xaxis.set_major_locator(MultipleLocator(1))
    ax.xaxis.set_minor_locator(MultipleLocator(0.5))
    ax.yaxis.set_major_locator(MultipleLocator(1))
    ax.yaxis.set_minor_locator(MultipleLocator(0.5))
    ax.grid(True, which='minor', linestyle='-')
    ax.set_xticks(np.arange(num_classes))
    ax.set_yticks(np.arange(num_classes))
    ax.set_xticklabels(labels)
    ax.set_yticklabels(labels)
    ax.tick_params(axis='x', bottom=False, top=True, labelbottom=False, labeltop=True)
    plt.setp(ax.get_xticklabels(), rotation=45, ha='left', rotation_mode='anchor')
    for i in range(num_classes):
        for j in range(num_classes):
            ax.text(j, i, '{}%'.format(int(confusion_matrix[i, j])), ha='center', va='center', color='w', size=7)
    ax.set_ylim(len(confusion_matrix) - 0.5, -0.5)
    fig.tight_layout()
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        plt.savefig(os.path.join(save_dir, 'confusion_matrix.png'), format='png')
    plt.close(fig)


def load_results(path):
    with open(path, 'rb') as f:
        results = pickle.load(f)
    assert isinstance(results, list)
    if results and isinstance(results[0], tuple):
        results = [r[0] for r in results]
    elif results and not isinstance(results[0], list):
        raise TypeError('invalid type of prediction results')
    return results


def main(argv=None):
    a = parse_args(argv)
    from oadg_amd import Config
    from oadg_amd import evaluation as E
    from oadg_amd.datasets import build_dataset
    cfg = Config.fromfile(a.config)
    if a.cfg_options:
        cfg.merge_from_dict(a.cfg_options)
    results = load_results(a.prediction_path)
    dataset = build_dataset(cfg.data.test, default_args=dict(device='cpu', test_mode=True))
    dev = E.voc_device() if a.device == 'auto' else None
    cm = E.calculate_confusion_matrix(dataset, results, a.score_thr, a.nms_iou_thr, a.tp_iou_thr, device=dev)
    names = list(dataset.CLASSES) + ['background']
    plot_confusion_matrix(cm, names, save_dir=a.save_dir, color_theme=a.color_theme)
    with open(os.path.join(a.save_dir, 'confusion_matrix.json'), 'w') as f:
        json.dump(dict(labels=names, counts=cm.astype(np.int64).tolist(), score_thr=a.score_thr, tp_iou_thr=a.tp_iou_thr,
                       nms_iou_thr=a.nms_iou_thr, device='host' if dev is None else str(dev)), f, indent=1)
    print(f'{len(results)} images, {int(cm.sum())} counts on {"the host" if dev is None else dev} -> '
          f'{os.path.join(a.save_dir, "confusion_matrix.png")}')


if __name__ == '__main__':
    main()
