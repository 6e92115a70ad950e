#!/usr/bin/env python
"""COCO error analysis of a result file, with the reference's CLI surface (tools/analysis_tools/coco_error_analysis.py:308-335):

    python tools/analysis_tools/coco_error_analysis.py RESULT.json OUT_DIR --ann ANN.json [--types bbox] [--extraplots]
        [--areas 1024 9216 10000000000] [--supercategories cityscapes | name=super ...] [--device auto|host]

RESULT.json is what ``tools/test.py --format-only --eval-options jsonfile_prefix=P`` wrote (``P.bbox.json``).  Per class and per
area range the precision-recall area is split into C75 / C50 (AP at IoU 0.75 / 0.5), Loc (AP at 0.1), Sim (confusion inside the
supercategory ignored), Oth (confusion with every class ignored), BG and FN.  The reference deep-copies the dataset twice per
class and runs COCOeval 1 + 2 K times on a pool of 48 processes; here ``oadg_amd.evaluation.coco_error_analysis`` packs the
split once and matches all of it in one launch of csrc/coco_error.hip when the library and a GPU are present, on the host
otherwise - the same array either way.  No process pool.  Written to OUT_DIR/bbox/: the reference's plots
(``bbox-<class>-<area>.png``, ``bbox-allclass-<area>.png``; with --extraplots the bar plots and the two ground-truth area
plots) and - an addition - ``error_analysis.json``: the mean of each band per class and area range, the numbers of the plots'
legends, unrounded.

Supercategories: ``categories[*].supercategory`` of ANN.json when every category has one (the reference dies with KeyError
otherwise; no Cityscapes json has the field).  Else ``--supercategories cityscapes`` (cityscapesscripts' grouping: person and
rider are 'human', the six others 'vehicle') or ``--supercategories name=super ...`` (refused beside a file that has the field).  With none of these every class is its
own supercategory, and Sim equals Loc.
"""
import argparse
import json
import os
import sys

import numpy as np

TOOLS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TOOLS)
sys.path.insert(0, os.path.dirname(TOOLS))

CITYSCAPES_SUPER = dict(person='human', rider='human', car='vehicle', truck='vehicle', bus='vehicle', train='vehicle',
                        motorcycle='vehicle', bicycle='vehicle')
AREA_LABELS = ('all', 'small', 'medium', 'large')                 # COCOeval.params.areaRngLbl
BAND_COLOURS = [(1, 1, 1), (1, 1, 1), (0.31, 0.51, 0.74), (0.75, 0.31, 0.30), (0.36, 0.90, 0.38), (0.50, 0.39, 0.64), (1, 0.6, 0)]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='COCO Error Analysis Tool')
    p.add_argument('result', help='result file (json format) path')
    p.add_argument('out_dir', help='dir to save analyze result images')
    p.add_argument('--ann', default='data/coco/annotations/instances_val2017.json', help='annotation file path')
    p.add_argument('--types', type=str, nargs='+', default=['bbox'], help="result types ('bbox'; masks are not built)")
    p.add_argument('--extraplots', action='store_true', help='export extra bar/stat plots')
    p.add_argument('--areas', type=int, nargs='+', default=[1024, 9216, 10000000000], help='area regions')
    p.add_argument('--supercategories', nargs='+', default=None, metavar='cityscapes|NAME=SUPER',
                   help="for an annotation file without categories[*].supercategory: 'cityscapes' (person, rider -> human; the "
                        "six others -> vehicle) or name=super pairs; default: every class is its own supercategory")
    p.add_argument('--device', default='auto', choices=['auto', 'host'],
                   help="where the matching runs: 'auto' = the GPU when the library and a GPU are present, 'host'")
    a = p.parse_args(argv)
    for t in a.types:
        if t == 'segm':
            raise NotImplementedError("--types segm is not built: this package has no masks; 'bbox' is")
        if t != 'bbox':
            raise ValueError(f"--types {t}: 'bbox' or 'segm'")
    if len(a.areas) != 3:
        raise ValueError('3 integers should be specified as areas, representing 3 area regions')
    return a


def supercategories(categories, option=None, log=print):
    """one supercategory per category, in the order of ``categories`` (the json records): the records' own field when every
    one has it; else --supercategories; else the class's own name (every class alone).  --supercategories beside a file that
    has the field is refused: the field is what the reference reads"""
    names = [c['name'] for c in categories]
    in_file = bool(categories) and all('supercategory' in c for c in categories)
    if option and in_file:
        raise ValueError('--supercategories: the annotation file names a supercategory for every category, and that field is '
                         'what the analysis uses; the option is for a file without it')
    if in_file:
        return [c['supercategory'] for c in categories]
    if option:
        table = dict(CITYSCAPES_SUPER) if list(option) == ['cityscapes'] else dict(o.split('=', 1) for o in option if '=' in o)
        if list(option) != ['cityscapes'] and len(table) != len(option):
            raise ValueError("--supercategories: 'cityscapes' or name=super pairs")
        missing = [n for n in names if n not in table]
        if missing:
            raise ValueError(f'--supercategories names no supercategory for {missing}')
        return [table[n] for n in names]
    log('no supercategory in the annotation file and no --supercategories: every class is its own supercategory, Sim equals Loc')
    return list(names)


def load_split(ann_file, res_file):
    """ANN.json and RESULT.json as COCO() / loadRes read them -> (categories, gt_anns, results, areas): the category records in
    file order; per image (file order) its annotations in file order as the evaluator's dicts; per image and category a float64
    array [k, 5] = x, y, w, h, score, the file's own numbers in the file's order; the area field of every annotation"""
    with open(ann_file) as f:
        gt = json.load(f)
    with open(res_file) as f:
        res = json.load(f)
    assert isinstance(res, list), 'results in not an array of objects'
    cats = list(gt.get('categories', []))
    label = {c['id']: k for k, c in enumerate(cats)}
    index = {im['id']: i for i, im in enumerate(gt.get('images', []))}
    gt_anns = [[] for _ in index]
    for a in gt.get('annotations', []):
        if a['image_id'] in index and a['category_id'] in label:
            gt_anns[index[a['image_id']]].append(dict(bbox=list(a['bbox']), category=label[a['category_id']], area=a['area'],
                                                      iscrowd=int(a.get('iscrowd', 0))))
    unknown = sorted({r['image_id'] for r in res} - set(index))
    assert not unknown, f'Results do not correspond to current coco set: image ids {unknown[:5]}'
    rows = [[[] for _ in cats] for _ in index]
    for r in res:
        if r['category_id'] in label:
            rows[index[r['image_id']]][label[r['category_id']]].append(list(r['bbox']) + [r['score']])
    results = [[np.array(c, np.float64).reshape(-1, 5) for c in per] for per in rows]
    return cats, gt_anns, results, [a['area'] for a in gt.get('annotations', [])]


def _canvas(title, xlabel=None, ylabel=None):
    """one Agg figure with one axes, titled and labelled (no pyplot state: the tool may be imported by a test process)"""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    ax.set_title(title)
    if xlabel:
        ax.set_xlabel(xlabel)
    if ylabel:
        ax.set_ylabel(ylabel)
    return fig, ax


def _save(fig, out_dir, title, tight=False):
    if tight:
        fig.tight_layout()
    fig.savefig(os.path.join(out_dir, f'{title}.png'))


def _value_labels(ax, bars):
    """the height above every bar: per cent for a share in (0, 1], the number itself otherwise"""
    for bar in bars:
        h = bar.get_height()
        ax.annotate(f'{h * 100 if 0 < h <= 1 else h:2.0f}', xy=(bar.get_x() + bar.get_width() / 2, h), xytext=(0, 3),
                    textcoords='offset points', ha='center', va='bottom', fontsize='x-small')


def band_curves(sub):
    """sub [7, R] (one class) or [7, R, K] (all): -> (the seven precision-over-recall curves, averaged over the classes, and the
    seven means - the legend's numbers)"""
    curves = [b.mean(axis=1) if b.ndim > 1 else b for b in sub]
    return curves, [float(b.mean()) for b in sub]


def plot_bands(recall, ps, out_dir, class_name, iou_type, names):
    """the reference's main plot, one per area range: the bands stacked between the curves, white up to C50, the legend
    '[mean]band'.  ps [7, R, 4, 1] (one class) or [7, R, K, 4, 1] (all)"""
    types, areas = names
    for a, area in enumerate(areas):
        title = f'{iou_type}-{class_name}-{area}'
        curves, means = band_curves(ps[..., a, 0])
        fig, ax = _canvas(title, 'recall', 'precision')
        below = np.zeros(len(recall))
        for curve, mean, band, colour in zip(curves, means, types, BAND_COLOURS):
            ax.plot(recall, curve, color='black', linewidth=0.5)
            ax.fill_between(recall, below, curve, color=colour, label=f'[{mean:.3f}]{band}')
            below = curve
        ax.set_xlim(0, 1.0)
        ax.set_ylim(0, 1.0)
        ax.legend()
        _save(fig, out_dir, title)


def plot_band_bars(ps, out_dir, class_name, iou_type, names):
    """--extraplots: the mean of every band below FN, grouped by area range"""
    types, areas = names
    title = f'{iou_type}-{class_name}-ap bar plot'
    fig, ax = _canvas(title, ylabel='Mean Average Precision (mAP)')
    at, group, n = np.arange(len(areas)), 0.60, len(types)
    drawn = []
    for b, band in enumerate(types[:-1]):
        heights = [band_curves(ps[..., a, 0])[1][b] for a in range(len(areas))]
        drawn.append(ax.bar(at - group / 2 + (b + 1) * group / n, heights, group / n, label=band))
    ax.set_xticks(at)
    ax.set_xticklabels(areas)
    ax.legend()
    for bars in drawn:
        _value_labels(ax, bars)
    _save(fig, out_dir, title)


def gt_area_group_numbers(gt_anns, num_classes, area_rng):
    """per area label the boxes that count in the plain evaluation: no crowd, area inside the range"""
    out = dict.fromkeys(AREA_LABELS, 0)
    for per in gt_anns:
        for g in per:
            for lbl, (lo, hi) in zip(AREA_LABELS, area_rng):
                if 0 <= g['category'] < num_classes and not (g['iscrowd'] or g['area'] < lo or g['area'] > hi):
                    out[lbl] += 1
    return out


def plot_gt_areas(gt_anns, all_areas, num_classes, area_rng, out_dir, log=print):
    """--extraplots: how many boxes count per area range, and the histogram of sqrt(area) over every annotation"""
    numbers = gt_area_group_numbers(gt_anns, num_classes, area_rng)
    log('number of annotations per area group:', numbers)
    title = 'number of annotations per area group'
    fig, ax = _canvas(title, ylabel='Number of annotations')
    at = np.arange(len(numbers))
    bars = ax.bar(at, list(numbers.values()), 0.60)
    ax.set_xticks(at)
    ax.set_xticklabels(list(numbers))
    _value_labels(ax, bars)
    _save(fig, out_dir, title, tight=True)
    title = 'gt annotation areas histogram plot'
    fig, ax = _canvas(title, 'Squareroot Area', 'Number of annotations')
    ax.hist(np.sqrt(np.asarray(all_areas, np.float64)), bins=100)
    _save(fig, out_dir, title, tight=True)
    return numbers


def analyze_results(res_file, ann_file, res_types, out_dir, extraplots=None, areas=None, supercats=None, device='auto',
                    log=print):
    from oadg_amd import evaluation as E
    areas = list(areas) if areas else [1024, 9216, 10000000000]
    cats, gt_anns, results, all_areas = load_split(ann_file, res_file)
    names, K = [c['name'] for c in cats], len(cats)
    sup = supercategories(cats, supercats, log=log)
    dev = E.voc_device() if device == 'auto' else None
    out = {}
    for res_type in res_types:
        res_out_dir = os.path.join(out_dir, res_type)
        os.makedirs(res_out_dir, exist_ok=True)
        ps = E.coco_error_analysis(gt_anns, results, K, sup, areas=areas, device=dev, xywh=True)
        labels = (E.ERROR_TYPES, E.ERROR_AREA_NAMES)
        for k, name in list(enumerate(names)) + [(None, 'allclass')]:
            sub = ps if k is None else ps[:, :, k]
            log(f'saving {name}' if k is None else f'saving {k + 1}-{name}')
            plot_bands(E.REC_THRS, sub, res_out_dir, name, res_type, labels)
            if extraplots:
                plot_band_bars(sub, res_out_dir, name, res_type, labels)
        if extraplots:
            plot_gt_areas(gt_anns, all_areas, K, E.error_area_rng(areas), res_out_dir, log=log)
        with open(os.path.join(res_out_dir, 'error_analysis.json'), 'w') as f:
            json.dump(dict(types=list(E.ERROR_TYPES), areas=areas, classes=names, supercategories=list(sup),
                           means=E.error_band_means(ps, names)), f, indent=1)
        log(f'{len(gt_anns)} images, {K} classes, matched on {"the host" if dev is None else dev} -> {res_out_dir}')
        out[res_type] = ps
    return out


def main(argv=None):
    a = parse_args(argv)
    return analyze_results(a.result, a.ann, a.types, out_dir=a.out_dir, extraplots=a.extraplots, areas=a.areas,
                           supercats=a.supercategories, device=a.device)


if __name__ == '__main__':
    main()
