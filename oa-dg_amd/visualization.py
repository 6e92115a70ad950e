"""Detections as a display list, and the pictures made of it (mmdet/core/visualization/image.py ``imshow_det_bboxes``,
``BaseDetector.show_result``, tools/test.py ``--show-dir``).

``det_items`` / ``gt_items`` are pure host code: boxes and labels -> the int32 rows and text bytes of csrc/draw.hip
(include/oadg_hip.h).  The reference hands every image to matplotlib on the host; here the rows are painted where the image
lives and the device PNG encoder turns the painted batch into files, so only the display list goes up and only zlib streams
come down.  The ctypes calls themselves are in the module next to the package's import shim (the rasteriser's wrapper and
``PngEncoder``; its docstring says why) and are imported on first use.

Colours are BGR tuples as in mmcv (the loaders' byte order), a colour name of mmcv, or 'palette': one fixed colour per
class index.  The label of a detection is a black plate with the text on it, in the fixed 6 x 11 bitmap font at the integer
scale nearest to ``font_size`` / 11; matplotlib's anti-aliased text and translucent plate are not reproduced.
"""
import os
import os.path as osp
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ._lib import DRAW_FILL, DRAW_ITEM_INTS, DRAW_OUTLINE, DRAW_TEXT

FONT_W, FONT_H = 6, 11
MAX_WRITERS = 16
COLOR_NAMES = dict(red=(0, 0, 255), green=(0, 255, 0), blue=(255, 0, 0), cyan=(255, 255, 0), yellow=(0, 255, 255),
                   magenta=(255, 0, 255), white=(255, 255, 255), black=(0, 0, 0))
# the Cityscapes colours of person, rider, car, truck, bus, train, motorcycle, bicycle (R, G, B in the dataset's label table)
_CITYSCAPES_RGB = ((220, 20, 60), (255, 0, 0), (0, 0, 142), (0, 0, 70), (0, 60, 100), (0, 80, 100), (0, 0, 230), (119, 11, 32))


def palette_color(index):
    """BGR colour of class ``index``: the Cityscapes colours for 0 .. 7, beyond them a fixed walk through the colour cube
    (an odd multiplier modulo 256 in the first byte: no two of 256 consecutive indices share a colour; none is black)"""
    index = int(index)
    if 0 <= index < len(_CITYSCAPES_RGB):
        return _CITYSCAPES_RGB[index][::-1]
    return (37 * index + 11) % 256, (101 * index + 97) % 256 | 32, (173 * index + 151) % 256


def color_val(color, index=0):
    """BGR tuple of ints of a colour argument (mmcv.color_val's forms that the configs use, and 'palette')"""
    if isinstance(color, str):
        if color == 'palette':
            return tuple(int(c) for c in palette_color(index))
        if color not in COLOR_NAMES:
            raise ValueError(f'colour {color!r}: one of {sorted(COLOR_NAMES)}, "palette" or a (B, G, R) tuple')
        return COLOR_NAMES[color]
    if isinstance(color, (int, np.integer)):
        color = (color, color, color)
    color = tuple(int(c) for c in color)
    if len(color) != 3 or not all(0 <= c <= 255 for c in color):
        raise ValueError(f'colour {color!r}: three values in 0 .. 255 (B, G, R)')
    return color


def _pack(color):
    return color[0] | color[1] << 8 | color[2] << 16


def font_scale(font_size):
    return max(1, int(round(font_size / FONT_H)))


def label_bytes(label_text):
    """the bytes of a label: latin-1, everything outside 32 .. 126 replaced by '?'"""
    return bytes(ord(ch) if 32 <= ord(ch) <= 126 else ord('?') for ch in label_text)


def _class_name(class_names, label):
    """image.py:143-144, and ``class <index>`` also for an index the names do not reach"""
    return class_names[label] if class_names is not None and 0 <= label < len(class_names) else f'class {label}'


def _boxes_to_rows(bboxes, labels, texts, bbox_color, text_color, thickness, font_size):
    s = font_scale(font_size)
    rows, text = [], bytearray()
    corners = bboxes[:, :4].astype(np.int32)                               # image.py:136 bbox.astype(np.int32): truncation
    for (x0, y0, x1, y1), label, label_text in zip(corners.tolist(), labels, texts):
        if x1 < x0 or y1 < y0:
            continue
        run = label_bytes(label_text)
        rows.append([DRAW_OUTLINE, x0, y0, x1, y1, int(thickness), _pack(color_val(bbox_color, label)), 0])
        rows.append([DRAW_FILL, x0, y0, x0 + FONT_W * s * len(run) + 1, y0 + FONT_H * s + 1, 0, 0, 0])
        rows.append([DRAW_TEXT, x0 + 1, y0 + 1, len(text), len(run), s, _pack(color_val(text_color, label)), 0])
        text += run
    items = np.asarray(rows, dtype=np.int64).clip(-2 ** 31, 2 ** 31 - 1).astype(np.int32).reshape(-1, DRAW_ITEM_INTS)
    return items, bytes(text)


def det_items(result, class_names, score_thr=0.3, bbox_color=(72, 101, 241), text_color=(72, 101, 241), thickness=2,
              font_size=13):
    """one image's ``list[ndarray [k, 5]]`` (per class) -> (items int32 [3 m, 8], text bytes) for its m drawn detections,
    in the order of ``np.vstack(result)``: rows with score > score_thr (no filter at score_thr <= 0: image.py:83-86),
    corners truncated to int32, inverted boxes dropped; per detection OUTLINE in the box colour, FILL in black from (x0, y0)
    to (x0 + 6 s len + 1, y0 + 11 s + 1), TEXT ``name|score`` at (x0 + 1, y0 + 1)."""
    result = [np.asarray(r, dtype=np.float32).reshape(-1, 5) for r in result]
    bboxes = np.vstack(result) if result else np.zeros((0, 5), np.float32)
    labels = np.concatenate([np.full(r.shape[0], i, dtype=np.int32) for i, r in enumerate(result)]) if result \
        else np.zeros(0, np.int32)
    if score_thr > 0:
        keep = bboxes[:, -1] > score_thr
        bboxes, labels = bboxes[keep], labels[keep]
    texts = [_class_name(class_names, l) + f'|{b[-1]:.02f}' for b, l in zip(bboxes, labels)]
    return _boxes_to_rows(bboxes, labels.tolist(), texts, bbox_color, text_color, thickness, font_size)


PROPOSAL_TOP_K = 20                    # RPN.show_result's default (rpn.py:142)


def proposal_items(proposals, top_k=PROPOSAL_TOP_K, **style):
    """one image's proposals (the [n, 5] array an RPN detector returns, best first) -> (items, text bytes): the first
    ``top_k`` of them (all when top_k <= 0) as the detections of ONE class named 'proposal', with no score threshold"""
    proposals = np.asarray(proposals, dtype=np.float32).reshape(-1, 5)
    return det_items([proposals[:top_k] if top_k > 0 else proposals], ('proposal',), 0, **style)


def gt_items(bboxes, labels, class_names, color=(0, 255, 0), thickness=2, font_size=13):
    """ground truth ``[k, 4]`` boxes and labels -> (items, text bytes): outline plus class name, the label geometry of
    ``det_items``"""
    bboxes = np.asarray(bboxes, dtype=np.float32).reshape(-1, 4)
    labels = [int(l) for l in np.asarray(labels).reshape(-1)]
    texts = [_class_name(class_names, l) for l in labels]
    return _boxes_to_rows(bboxes, labels, texts, color, color, thickness, font_size)


def join_lists(lists):
    """[(items, text bytes) per image] -> (items, item_off int32 [n + 1], text uint8) of the batch"""
    rows, off, text = [], [0], bytearray()
    for items, run in lists:
        items = items.copy()
        items[items[:, 0] == DRAW_TEXT, 3] += len(text)
        rows.append(items)
        text += run
        off.append(off[-1] + len(items))
    items = np.concatenate(rows) if rows else np.zeros((0, DRAW_ITEM_INTS), np.int32)
    return np.ascontiguousarray(items), np.asarray(off, dtype=np.int32), np.frombuffer(bytes(text), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------- device side
def draw_detections(imgs_u8, results, class_names, score_thr=0.3, **style):
    """a painted COPY of the resident uint8 batch [n, H, W, 3]: image i with the detections ``results[i]`` on it"""
    import oadg_draw
    drawn = imgs_u8.contiguous().clone()
    items, item_off, text = join_lists([proposal_items(r, **style) if isinstance(r, np.ndarray) else
                                        det_items(r, class_names, score_thr, **style) for r in results])
    return oadg_draw.draw_items(drawn, items, item_off, text)


def picture_name(dataset, index):
    """the file of image ``index`` under a show directory: its ``ori_filename`` with the extension replaced by .png, or
    ``<index:06d>.png`` for a dataset without files (a ConcatDataset / RepeatDataset: the file of the dataset it wraps)"""
    if hasattr(dataset, 'datasets') and hasattr(dataset, '_locate'):
        k, i = dataset._locate(index)
        return picture_name(dataset.datasets[k], i) if hasattr(dataset.datasets[k], 'data_infos') else f'{index:06d}.png'
    if hasattr(dataset, 'dataset') and hasattr(dataset, '_ori_len'):
        return picture_name(dataset.dataset, index % dataset._ori_len)
    infos = getattr(dataset, 'data_infos', None)
    if infos is None:
        return f'{index:06d}.png'
    # a name that is a whole path (no img_prefix) or climbs with '..' must still land BELOW the show directory - joined as
    # it is, an absolute name would discard the directory and the picture of a .png source would overwrite the source
    name = osp.normpath(osp.splitdrive(infos[index]['filename'])[1]).replace('\\', '/')
    name = '/'.join(p for p in name.split('/') if p not in ('', '.', '..'))
    return osp.splitext(name)[0] + '.png'


class ShowWriter:
    """``--show-dir``: paint a tested batch, encode it with csrc/png_encode.hip and write the files on writer threads.  The
    encode and the copy of the streams of one batch run behind the next batch's forward pass: ``add`` finishes the batch
    before and raises what a writer has raised by then (a full disk stops the loop, not the last image).  ``close``
    finishes the last batch and waits for the writes; ``abort`` only stops the threads (the loop is already failing)."""

    def __init__(self, show_dir, dataset, device, score_thr=0.3, workers=MAX_WRITERS, **style):
        import oadg_draw
        self._write = oadg_draw.write_png
        self.enc = oadg_draw.PngEncoder(device)
        self.show_dir, self.dataset, self.score_thr, self.style = show_dir, dataset, score_thr, style
        self.class_names = getattr(dataset, 'CLASSES', None)
        self.pool = ThreadPoolExecutor(max(1, min(int(workers), MAX_WRITERS)), thread_name_prefix='oadg-show-write')
        self._pending, self._futures, self._made, self.files = None, [], set(), 0

    def add(self, imgs_u8, results, indices):
        paths = [osp.join(self.show_dir, picture_name(self.dataset, i)) for i in indices]
        for p in paths:
            if osp.dirname(p) not in self._made:
                os.makedirs(osp.dirname(p), exist_ok=True)
                self._made.add(osp.dirname(p))
        drawn = draw_detections(imgs_u8, results, self.class_names, self.score_thr, **self.style)
        job = self.enc.launch(drawn, bgr=True)
        self._finish()
        self._pending = (job, paths)

    def _finish(self):
        if self._pending is None:
            return
        (job, paths), self._pending = self._pending, None
        streams = self.enc.finish(job)
        futures = [self.pool.submit(self._write, self.enc.L, p, addr, nb, job['H'], job['W'])
                   for p, (addr, nb) in zip(paths, streams)]
        self.enc.release(job, futures)
        earlier, self._futures = self._futures, futures                        # (bounded by what is in flight)
        self.files += len(paths)
        for f in earlier:
            if f.done():
                f.result()
            else:
                self._futures.append(f)

    def close(self):
        try:
            self._finish()
            for f in self._futures:
                f.result()
        finally:
            self._futures = []
            self.pool.shutdown(wait=True)

    def abort(self):
        self._pending, self._futures = None, []
        self.pool.shutdown(wait=True)


def resident_image(img, device):
    """a path, a uint8 HWC BGR numpy array or a resident tensor -> uint8 [1, H, W, 3] on ``device`` (a copy)"""
    if isinstance(img, (str, os.PathLike)):
        from PIL import Image
        with Image.open(img) as im:
            img = np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])       # mmcv.imread: colour, BGR
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError('img must be a uint8 [H, W, 3] (B, G, R) array')
        img = torch.from_numpy(np.ascontiguousarray(img)).to(device)
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('img must be a path, a uint8 [H, W, 3] numpy array or a uint8 [H, W, 3] tensor')
    return img.to(device).contiguous().clone()[None]


def show_result(img, result, class_names, device, score_thr=0.3, out_file=None, **style):
    """``BaseDetector.show_result`` without the window: paint ``result`` on a copy of ``img``; write a PNG to ``out_file``
    when given, else return the painted uint8 [H, W, 3] (B, G, R) numpy image"""
    import oadg_draw
    device = torch.device(device)
    with torch.cuda.device(device):
        drawn = draw_detections(resident_image(img, device), [result], class_names, score_thr, **style)
        if out_file is None:
            return drawn[0].cpu().numpy()
        if osp.dirname(out_file):
            os.makedirs(osp.dirname(out_file), exist_ok=True)
        enc = oadg_draw.PngEncoder(device, slots=1)
        job = enc.launch(drawn, bgr=True)
        (address, nbytes), = enc.finish(job)
        oadg_draw.write_png(enc.L, str(out_file), address, nbytes, job['H'], job['W'])
    return None
