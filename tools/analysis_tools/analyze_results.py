#!/usr/bin/env python
"""The best and the worst images of saved detection results, with the reference's CLI surface
(tools/analysis_tools/analyze_results.py:138-195):

    python tools/analysis_tools/analyze_results.py CONFIG PKL SHOW_DIR [--topk 20] [--show-score-thr 0] [--cfg-options k=v ...]

PKL is what ``tools/test.py --out`` wrote.  Every image gets the reference's ``bbox_map_eval`` - the mean over IoU .5 ... .95
of the one-image ``eval_map`` - from ``oadg_amd.evaluation.per_image_map``: ONE pack of the split, matched by
csrc/voc_eval.hip (two launches for the ten thresholds) when the library and a GPU are present.  The images are sorted by it
(stable, ascending); the first ``--topk`` go to SHOW_DIR/bad, the last to SHOW_DIR/good (``--topk`` becomes half the split
when the split is smaller than twice it), each painted with its ground truth (colour (255, 102, 61)) and its detections
((72, 101, 241)) on the device and written as ``<stem>_<round(mAP, 3)>.png`` - always a PNG, whatever the source's extension:
the device encoder (csrc/png_encode.hip) writes nothing else.  Painting and encoding need the GPU.
"""
import argparse
import os
import os.path as osp
import sys

TOOLS = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TOOLS)
sys.path.insert(0, os.path.dirname(TOOLS))
from train import DictAction  # noqa: E402

GT_COLOR, DET_COLOR = (255, 102, 61), (72, 101, 241)      # imshow_gt_det_bboxes' defaults


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='MMDet eval image prediction result for each.  The painted images are written '
                                            'as <stem>_<mAP>.png: PNG whatever the extension of the source image.')
    p.add_argument('config', help='test config file path')
    p.add_argument('prediction_path', help='prediction path where test pkl result')
    p.add_argument('show_dir', help='directory where painted images will be saved')
    p.add_argument('--show', action='store_true', help='show results in a window (not built: the images are saved)')
    p.add_argument('--wait-time', type=float, default=0, help='the interval of show (s): unused without --show')
    p.add_argument('--topk', default=20, type=int, help='saved Number of the highest topk and lowest topk after index sorting')
    p.add_argument('--show-score-thr', type=float, default=0, help='score threshold (default: 0.)')
    p.add_argument('--cfg-options', nargs='+', action=DictAction, help='override config entries, key=value')
    a = p.parse_args(argv)
    if a.show:
        raise NotImplementedError('--show (a window per image) is not built: there is no display here; the painted images '
                                  'are written to SHOW_DIR/good and SHOW_DIR/bad')
    return a


def picture_stem(dataset, index):
    """osp.splitext(osp.basename(filename))[0] of image ``index`` (analyze_results.py:72-78); ``<index:06d>`` for a dataset
    without files"""
    infos = getattr(dataset, 'data_infos', None)
    if infos is None:
        return f'{index:06d}'
    return osp.splitext(osp.basename(infos[index]['filename']))[0]


def save_image_gts_results(dataset, results, maps, out_dir, device, score_thr=0, encoder=None):
    """analyze_results.py:64-88: image by image, ground truth and detections painted together on the resident image
    (csrc/draw.hip), encoded on the device, written to ``out_dir``/<stem>_<round(mAP, 3)>.png -> the paths"""
    import torch
    import oadg_draw
    from oadg_amd import evaluation as E
    from oadg_amd import visualization as V
    os.makedirs(out_dir, exist_ok=True)
    names = getattr(dataset, 'CLASSES', None)
    enc = encoder or oadg_draw.PngEncoder(device, slots=1)
    paths = []
    with torch.cuda.device(device):
        for index, m in maps:
            img = dataset.batch([index])[0].to(device).contiguous().clone()
            ann = E.dataset_ann_infos(dataset, [index])[0]
            res = results[index][0] if isinstance(results[index], tuple) else results[index]
            # both lists on ONE image: the ground truth first, the detections over it
            items, off, text = V.join_lists([V.gt_items(ann['bboxes'], ann['labels'], names, color=GT_COLOR),
                                             V.det_items(res, names, score_thr, bbox_color=DET_COLOR, text_color=DET_COLOR)])
            drawn = oadg_draw.draw_items(img, items, off[[0, -1]].copy(), text)
            job = enc.launch(drawn, bgr=True)
            (address, nbytes), = enc.finish(job)
            path = osp.join(out_dir, f'{picture_stem(dataset, index)}_{round(m, 3)}.png')
            oadg_draw.write_png(enc.L, path, address, nbytes, job['H'], job['W'])
            paths.append(path)
    return paths


def main(argv=None):
    a = parse_args(argv)
    import pickle
    import torch
    from oadg_amd import Config
    from oadg_amd import evaluation as E
    from oadg_amd.datasets import build_dataset
    if not osp.isfile(a.prediction_path):
        raise FileNotFoundError(f'file "{a.prediction_path}" does not exist')
    cfg = Config.fromfile(a.config)
    if a.cfg_options:
        cfg.merge_from_dict(a.cfg_options)
    if not torch.cuda.is_available():
        raise RuntimeError('analyze_results.py paints and encodes the images on the GPU: none is available')
    dev = torch.device('cuda', torch.cuda.current_device())
    dataset = build_dataset(cfg.data.test, default_args=dict(device=dev, test_mode=True))
    with open(a.prediction_path, 'rb') as f:
        results = pickle.load(f)
    assert len(results) == len(dataset), f'{len(results)} results for {len(dataset)} images'
    match_dev = E.voc_device()
    maps = E.per_image_map(results, E.dataset_ann_infos(dataset), len(dataset.CLASSES), device=match_dev)
    good, bad = E.rank_images(maps, a.topk)
    n = 0
    for name, chosen in (('good', good), ('bad', bad)):
        n += len(save_image_gts_results(dataset, results, chosen, osp.abspath(osp.join(a.show_dir, name)), dev,
                                        a.show_score_thr))
    print(f'{len(results)} images, per-image mAP matched on {"the host" if match_dev is None else match_dev}: '
          f'min {min(maps, default=0.0):.3f} max {max(maps, default=0.0):.3f}; {n} images -> {a.show_dir}/good, {a.show_dir}/bad')


if __name__ == '__main__':
    main()
