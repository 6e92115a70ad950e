"""Write a Diverse-Weather-shaped synthetic dataset to DISK in the S-DGOD (VOC) layout - JPEG frames, XML annotations and
an id list with the DWD classes - so that tools/train.py can be run on JPEG FILES (entropy decode + upload + device
pixel stage + Resize / RandomFlip + OA-Mix + train) where the real S-DGOD tree is not available: the same images and
boxes as ``SyntheticCityscapes`` (the make_synthetic_coco.py counterpart).

usage: python tools/make_synthetic_voc.py OUT_DIR [--n 64] [--height 720] [--width 1280] [--boxes 12] [--quality 95]
                                          [--subsampling 4:2:0]
writes OUT_DIR/VOC2007/{JPEGImages/{id}.jpg, Annotations/{id}.xml, ImageSets/Main/train.txt}; run e.g.
  python tools/train.py configs/oadg/faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod.py --allow-missing-pretrained \\
      --cfg-options data.train.dataset.ann_file=OUT_DIR/VOC2007/ImageSets/Main/train.txt \\
                    data.train.dataset.img_prefix=OUT_DIR/VOC2007/
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oadg_amd  # noqa: F401,E402
from oadg_amd.pipelines import SyntheticCityscapes  # noqa: E402

CLASSES = ('bus', 'bike', 'car', 'motor', 'person', 'rider', 'truck')
SUBSAMPLING = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}


def write_xml(path, img_id, H, W, boxes, labels):
    objs = []
    for b, l in zip(boxes, labels):
        # VOC's 1-based pixel coordinates: XMLDataset subtracts 1 again (xml_style.py:144)
        x1, y1, x2, y2 = (int(round(float(v))) + 1 for v in b)
        objs.append(f'  <object>\n    <name>{CLASSES[int(l)]}</name>\n    <difficult>0</difficult>\n'
                    f'    <bndbox><xmin>{x1}</xmin><ymin>{y1}</ymin><xmax>{x2}</xmax><ymax>{y2}</ymax></bndbox>\n'
                    f'  </object>\n')
    with open(path, 'w') as f:
        f.write(f'<annotation>\n  <filename>{img_id}.jpg</filename>\n'
                f'  <size><width>{W}</width><height>{H}</height><depth>3</depth></size>\n{"".join(objs)}</annotation>\n')


def main():
    p = argparse.ArgumentParser()
    p.add_argument('out')
    p.add_argument('--n', type=int, default=64)
    p.add_argument('--height', type=int, default=720)
    p.add_argument('--width', type=int, default=1280)
    p.add_argument('--boxes', type=int, default=12)
    p.add_argument('--quality', type=int, default=95)
    p.add_argument('--subsampling', default='4:2:0', choices=sorted(SUBSAMPLING))
    a = p.parse_args()
    from PIL import Image
    dev = 'cuda' if torch.cuda.is_available() else 'cpu'
    ds = SyntheticCityscapes(img_shape=(a.height, a.width), num_boxes=a.boxes, num_classes=len(CLASSES), device=dev)
    root = os.path.join(a.out, 'VOC2007')
    for d in ('JPEGImages', 'Annotations', os.path.join('ImageSets', 'Main')):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    ids, nbytes = [], 0
    for i in range(a.n):
        img_id = f'{i:06d}'
        bgr = ds.image(i).cpu().numpy()
        path = os.path.join(root, 'JPEGImages', f'{img_id}.jpg')
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path, quality=a.quality,
                                                                    subsampling=SUBSAMPLING[a.subsampling])
        nbytes += os.path.getsize(path)
        boxes, labels = ds.boxes(i)
        write_xml(os.path.join(root, 'Annotations', f'{img_id}.xml'), img_id, a.height, a.width,
                  np.asarray(boxes), np.asarray(labels))
        ids.append(img_id)
    with open(os.path.join(root, 'ImageSets', 'Main', 'train.txt'), 'w') as f:
        f.write(''.join(f'{i}\n' for i in ids))
    print(f'{a.n} images of {a.height}x{a.width}, {nbytes / a.n / 1e6:.2f} MB per JPEG (q{a.quality}, {a.subsampling}) '
          f'-> {root}')


if __name__ == '__main__':
    main()
