#!/usr/bin/env python
"""Detect on one image file and write the picture (demo/image_demo.py of the reference):

    python demo/image_demo.py IMG CONFIG CHECKPOINT --out-file F [--device cuda:0] [--score-thr 0.3] [--palette]

``CHECKPOINT`` 'none' runs the detector at its initial weights (smoke runs).  The image goes through the config's test
pipeline on the device (``apis.inference_detector``), its detections above ``--score-thr`` are painted on it there
(``BaseDetector.show_result``: csrc/draw.hip) and the PNG is encoded there too.  The reference opens a window without
``--out-file``; there is no window here, so ``--out-file`` is required.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='detect on one image and write the painted picture')
    p.add_argument('img', help='image file')
    p.add_argument('config', help='config file')
    p.add_argument('checkpoint', help="checkpoint file ('none' = initial weights)")
    p.add_argument('--out-file', required=True, help='path of the PNG to write')
    p.add_argument('--device', default='cuda:0', help='device used for inference')
    p.add_argument('--palette', action='store_true', help='one colour per class instead of one colour for all')
    p.add_argument('--score-thr', type=float, default=0.3, help='bbox score threshold')
    p.add_argument('--amp', default='bf16', choices=['bf16', 'none'])
    return p.parse_args(argv)


def main(argv=None):
    a = parse_args(argv)
    import torch
    from oadg_amd.apis import inference_detector, init_detector
    if not torch.cuda.is_available():
        raise RuntimeError('demo/image_demo.py detects and draws on the MI355X only; there is no CPU fallback')
    model = init_detector(a.config, a.checkpoint, device=a.device, amp=None if a.amp == 'none' else a.amp)
    result = inference_detector(model, a.img)
    colour = 'palette' if a.palette else (72, 101, 241)
    model.show_result(a.img, result, score_thr=a.score_thr, bbox_color=colour, text_color=colour, out_file=a.out_file)
    print(f'{sum(len(c) for c in result)} detections, {sum(int((c[:, 4] > a.score_thr).sum()) for c in result)} drawn '
          f'-> {a.out_file}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
