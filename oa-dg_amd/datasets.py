"""Real input path: COCO-format annotation files + image files -> uint8 batches in HBM.

``CocoDataset`` / ``CityscapesDataset`` follow mmdet/datasets/{custom,coco,cityscapes}.py for what the training loop
needs (``load_annotations``, ``_filter_imgs``, ``_parse_ann_info``, ``get_ann_info``, ``prepare_train_img``'s
``img_info`` / ``ann_info``); the COCO index is a plain-json restatement of the few ``pycocotools.COCO`` lookups those
functions use (pycocotools is not installed).  Images are decoded on the host (PIL; PNG is lossless, so the bytes equal
``mmcv.imfrombytes(..., flag='color')`` = BGR order) by a small thread pool and uploaded through pinned memory; from
there on everything is the device pipeline.  ``batch(indices)`` has ``SyntheticCityscapes``' signature.

JPEG files of a dataset on the GPU take the native path (csrc/jpeg_decode.hip): the decode threads run the entropy stage
into one pinned coefficient buffer, one upload carries it to the device and the pixel stage writes the batch there,
byte-equal to PIL.  ``XMLDataset`` / ``SdgodDataset`` (mmdet/datasets/{xml_style,sdgod}.py: VOC-style id lists, XML
annotations, JPEG frames - the Diverse-Weather benchmark) reuse all of it.
"""
import bisect
import json
import os
import threading
import xml.etree.ElementTree as ET
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import evaluation, staging
from .registry import DATASETS, build_from_cfg


NATIVE_PNG = os.environ.get('OADG_NATIVE_PNG', '1') == '1'     # PNG files through csrc/png_decode.hip (else PIL)
NATIVE_JPEG = os.environ.get('OADG_NATIVE_JPEG', '1') == '1'   # JPEG files of a GPU dataset through csrc/jpeg_decode.hip
_JPEG_EXT = ('.jpg', '.jpeg')


class _CocoIndex:
    """The part of pycocotools.coco.COCO that CocoDataset calls (createIndex, getCatIds, getImgIds, getAnnIds, ...)."""

    def __init__(self, ann_file):
        with open(ann_file) as f:
            self.dataset = json.load(f)
        self.anns, self.imgs, self.cats = {}, {}, {}
        self.img_to_anns, self.cat_img_map = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get('annotations', []):
            self.img_to_anns[ann['image_id']].append(ann)
            self.anns[ann['id']] = ann
            self.cat_img_map[ann['category_id']].append(ann['image_id'])
        for img in self.dataset.get('images', []):
            self.imgs[img['id']] = img
        for cat in self.dataset.get('categories', []):
            self.cats[cat['id']] = cat

    def get_cat_ids(self, cat_names):
        # pycocotools filters the category list in FILE order: the result does not follow the order of cat_names
        return [c['id'] for c in self.dataset.get('categories', []) if c['name'] in cat_names]

    def get_img_ids(self):
        return list(self.imgs.keys())

    def get_ann_ids(self, img_ids):
        return [a['id'] for i in img_ids for a in self.img_to_anns.get(i, [])]

    def load_anns(self, ids):
        return [self.anns[i] for i in ids]


@DATASETS.register_module()
class CocoDataset:
    CLASSES = None

    def __init__(self, ann_file, pipeline=None, classes=None, data_root=None, img_prefix='', seg_prefix=None,
                 proposal_file=None, test_mode=False, filter_empty_gt=True, device='cuda', decode_workers=None, **kwargs):
        self.ann_file, self.data_root, self.img_prefix = ann_file, data_root, img_prefix
        self.test_mode, self.filter_empty_gt, self.device = test_mode, filter_empty_gt, device
        self.pipeline_cfg = pipeline
        if classes is not None:
            self.CLASSES = tuple(classes)
        if data_root is not None:
            if not os.path.isabs(self.ann_file):
                self.ann_file = os.path.join(data_root, self.ann_file)
            if self.img_prefix and not os.path.isabs(self.img_prefix):
                self.img_prefix = os.path.join(data_root, self.img_prefix)
        self.data_infos = self.load_annotations(self.ann_file)
        if not test_mode:
            valid = self._filter_imgs()
            self.data_infos = [self.data_infos[i] for i in valid]
        # Decode workers (PIL releases the interpreter lock inside its decoders, numpy inside the channel flip): a
        # 1024 x 2048 PNG costs 30 - 50 ms of inflate on one core and the step consumes a batch of four every ~27 ms, so
        # several BATCHES are decoded at once (tools/train.py keeps `loader_depth` of them in flight).  The workers run
        # on spare cores of the rank's slice of the host - NOT on the CCD the launch threads are pinned to
        # (apis.pin_rank_to_cores) - when there are any; default count: 12, or what the spare cores allow.
        from .apis import spare_cores
        want = 12 if decode_workers is None else int(decode_workers)
        self._decode_cores = spare_cores(want)
        if decode_workers is None and self._decode_cores is not None:
            want = max(4, len(self._decode_cores))
        self.decode_workers = want
        self.ring_slots = 6            # pinned batch buffers per (batch, shape): more than tools/train.py keeps in flight
        self._rings, self._ring_lock = {}, threading.Lock()     # staging.Ring per batch shape / per coefficient capacity
        self.jpeg_decodes = dict(native=0, pil=0)       # JPEG files decoded by csrc/jpeg_decode.hip / by PIL
        self._count_lock = threading.Lock()
        self._pool = ThreadPoolExecutor(want, thread_name_prefix='oadg-decode', initializer=self._place_worker)
        # custom.py:209-221 _set_group_flag: images with aspect ratio > 1 form group 1 (the samplers group by it)
        self.flag = np.array([1 if i['width'] / i['height'] > 1 else 0 for i in self.data_infos], dtype=np.uint8)

    # ---- coco.py:40-67
    def load_annotations(self, ann_file):
        self.coco = _CocoIndex(ann_file)
        self.cat_ids = self.coco.get_cat_ids(cat_names=self.CLASSES)
        self.cat2label = {cat_id: i for i, cat_id in enumerate(self.cat_ids)}
        self.img_ids = self.coco.get_img_ids()
        data_infos, total = [], []
        for i in self.img_ids:
            info = dict(self.coco.imgs[i])
            info['filename'] = info['file_name']
            data_infos.append(info)
            total.extend(self.coco.get_ann_ids(img_ids=[i]))
        assert len(set(total)) == len(total), f"Annotation ids in '{ann_file}' are not unique!"
        return data_infos

    # ---- coco.py:112-138
    def _filter_imgs(self, min_size=32):
        valid_inds, valid_img_ids = [], []
        ids_with_ann = set(a['image_id'] for a in self.coco.anns.values())
        ids_in_cat = set()
        for class_id in self.cat_ids:
            ids_in_cat |= set(self.coco.cat_img_map[class_id])
        ids_in_cat &= ids_with_ann
        for i, info in enumerate(self.data_infos):
            if self.filter_empty_gt and self.img_ids[i] not in ids_in_cat:
                continue
            if self._skip_all_crowd(info):
                continue
            if min(info['width'], info['height']) >= min_size:
                valid_inds.append(i)
                valid_img_ids.append(self.img_ids[i])
        self.img_ids = valid_img_ids
        return valid_inds

    def _skip_all_crowd(self, info):
        return False

    def __len__(self):
        return len(self.data_infos)

    EVAL_PROTOCOLS = (evaluation.COCO_EVAL,)

    def evaluate(self, results, metric='bbox', logger=None, **eval_kwargs):
        """coco.py:364-573 for 'bbox' (XMLDataset: voc.py:28-106 for 'mAP'): evaluation.dataset_evaluate"""
        return evaluation.dataset_evaluate(self, results, metric=metric, logger=logger, **eval_kwargs)

    # ---- coco.py:182-362, detections only (no masks here; proposals are scored by evaluation.proposal_evaluate)
    @staticmethod
    def xyxy2xywh(bbox):
        """one result row -> [x, y, w, h] as Python floats (the subtraction happens in double, on the row's own values)"""
        b = bbox.tolist()
        return [b[0], b[1], b[2] - b[0], b[3] - b[1]]

    def _det2json(self, results):
        """per image a list of [k, 5] arrays per class -> the records of a COCO result file, image after image, class after
        class, row after row"""
        return [dict(image_id=self.img_ids[idx], bbox=self.xyxy2xywh(row), score=float(row[4]), category_id=self.cat_ids[label])
                for idx in range(len(self)) for label, rows in enumerate(results[idx]) for row in rows]

    def results2json(self, results, outfile_prefix):
        """writes ``<outfile_prefix>.bbox.json`` -> dict(bbox=..., proposal=...) (both name that file, as in the reference)"""
        if results and not isinstance(results[0], list):
            raise TypeError('invalid type of results: format_results writes detections, a list of [k, 5] arrays per image '
                            '(masks and the one-array-per-image results of an RPN detector are not built)')
        path = f'{outfile_prefix}.bbox.json'
        if os.path.dirname(path):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(self._det2json(results), f)
        return dict(bbox=path, proposal=path)

    def format_results(self, results, jsonfile_prefix=None, **kwargs):
        """-> (result_files, tmp_dir): the json file of ``results2json`` under ``jsonfile_prefix`` ('a/b/prefix'), or in a
        ``tempfile.TemporaryDirectory`` - returned, the caller cleans it up - when there is no prefix"""
        assert isinstance(results, list), 'results must be a list'
        assert len(results) == len(self), \
            'The length of results is not equal to the dataset len: {} != {}'.format(len(results), len(self))
        tmp_dir = None
        if jsonfile_prefix is None:
            import tempfile
            tmp_dir = tempfile.TemporaryDirectory()
            jsonfile_prefix = os.path.join(tmp_dir.name, 'results')
        return self.results2json(results, jsonfile_prefix), tmp_dir

    def fast_eval_recall(self, results, proposal_nums, iou_thrs, logger=None, device='auto'):
        """coco.py:312-334: per budget the recall of one [n, 5] array of proposals per image, averaged over ``iou_thrs``
        (evaluation.fast_eval_recall; matched on the GPU when there is one)"""
        return evaluation.fast_eval_recall(self, results, proposal_nums, iou_thrs, logger=logger, device=device)

    def get_ann_info(self, idx):
        img_id = self.data_infos[idx]['id']
        return self._parse_ann_info(self.data_infos[idx], self.coco.load_anns(self.coco.get_ann_ids(img_ids=[img_id])))

    # ---- coco.py:140-199
    def _parse_ann_info(self, img_info, ann_info):
        gt_bboxes, gt_labels, gt_bboxes_ignore = [], [], []
        for ann in ann_info:
            if ann.get('ignore', False):
                continue
            x1, y1, w, h = ann['bbox']
            if self._degenerate(ann, img_info, x1, y1, w, h):
                continue
            if ann['category_id'] not in self.cat_ids:
                continue
            bbox = [x1, y1, x1 + w, y1 + h]
            if ann.get('iscrowd', False):
                gt_bboxes_ignore.append(bbox)
            else:
                gt_bboxes.append(bbox)
                gt_labels.append(self.cat2label[ann['category_id']])
        return dict(
            bboxes=np.array(gt_bboxes, dtype=np.float32) if gt_bboxes else np.zeros((0, 4), dtype=np.float32),
            labels=np.array(gt_labels, dtype=np.int64) if gt_labels else np.array([], dtype=np.int64),
            bboxes_ignore=np.array(gt_bboxes_ignore, dtype=np.float32) if gt_bboxes_ignore
            else np.zeros((0, 4), dtype=np.float32))

    @staticmethod
    def _degenerate(ann, img_info, x1, y1, w, h):
        inter_w = max(0, min(x1 + w, img_info['width']) - max(x1, 0))
        inter_h = max(0, min(y1 + h, img_info['height']) - max(y1, 0))
        return inter_w * inter_h == 0 or ann['area'] <= 0 or w < 1 or h < 1

    def _place_worker(self):
        if self._decode_cores and hasattr(os, 'sched_setaffinity'):
            try:
                os.sched_setaffinity(0, self._decode_cores)      # (pid 0 = the calling thread)
            except OSError:
                pass

    # ---- loading.py:33-78 LoadImageFromFile (color, BGR)
    def _path(self, idx):
        name = self.data_infos[idx]['filename']
        return os.path.join(self.img_prefix, name) if self.img_prefix else name

    def decode(self, idx):
        from PIL import Image
        with Image.open(self._path(idx)) as im:
            rgb = np.asarray(im.convert('RGB'))
        return np.ascontiguousarray(rgb[:, :, ::-1])

    def decode_into(self, idx, dst):
        """image ``idx`` as BGR bytes into ``dst`` (uint8 [H,W,3] view of host memory).  PNG files go through the native
        decoder (csrc/png_decode.hip: one call without the interpreter lock, pixels written at their final place); any other
        format, or a PNG variant it does not cover, through PIL."""
        path = self._path(idx)
        if path.lower().endswith(_JPEG_EXT):
            self._count('pil')
        if NATIVE_PNG and path.lower().endswith('.png'):
            from . import _lib
            rc = _lib.lib().oadg_png_decode_bgr(path.encode(), dst.ctypes.data, dst.shape[0], dst.shape[1])
            if rc == 0:
                return
            if rc not in (-4,):                   # (-4: a PNG variant for PIL; anything else is an error worth seeing)
                _lib.check(rc, f'oadg_png_decode_bgr({path})')
        np.copyto(dst, self.decode(idx))

    def _shape(self, idx):
        info = self.data_infos[idx]
        return int(info['height']), int(info['width'])

    def _count(self, path, k=1):
        with self._count_lock:
            self.jpeg_decodes[path] += k

    def _slot(self, n, H, W):
        """a reserved slot holding a pinned [n,H,W,3] batch, from a small ring per shape (allocated once per shape: pinning
        25 MB per batch costs more than decoding it); a slot is reused only after the upload that read it has finished"""
        return self._reserve((n, H, W), n * H * W * 3)

    def _coef_slot(self, nbytes):
        """a reserved slot of at least ``nbytes`` for the JPEG coefficients + descriptors of a batch, from a ring keyed by
        capacity (the next power of two, at least 1 MiB): a handful of rings whatever the image shapes"""
        cap = 1 << max(20, (int(nbytes) - 1).bit_length())
        return self._reserve(cap, cap)

    def _reserve(self, key, nbytes):
        with self._ring_lock:
            ring = self._rings.get(key)
            if ring is None:
                ring = self._rings[key] = staging.Ring(self.ring_slots, nbytes)
            ring.slots = self.ring_slots        # (tools/train.py raises it: holds for the slots not created yet)
        return ring.reserve(nbytes)

    def batch(self, indices):
        """(uint8 [N,H,W,3] on the device, list of float32 [n,4] boxes, list of int64 labels)."""
        indices = list(indices)
        shapes = {self._shape(i) for i in indices}
        assert len(shapes) == 1, 'one image shape per batch (Cityscapes: 1024x2048)'
        H, W = shapes.pop()
        if torch.device(self.device).type == 'cuda' and NATIVE_JPEG and \
                any(self._path(i).lower().endswith(_JPEG_EXT) for i in indices):
            dev = self._batch_jpeg(indices, H, W)
            anns = [self.get_ann_info(i) for i in indices]
            return dev, [a['bboxes'] for a in anns], [a['labels'] for a in anns]
        n = len(indices)
        slot = self._slot(n, H, W)
        views = slot.host[:n * H * W * 3].view(n, H, W, 3).numpy()
        try:
            list(self._pool.map(lambda a: self.decode_into(a[1], views[a[0]]), enumerate(indices)))
        except BaseException:
            slot.release()
            raise
        dev = slot.commit(n * H * W * 3, self.device).view(n, H, W, 3)
        anns = [self.get_ann_info(i) for i in indices]
        return dev, [a['bboxes'] for a in anns], [a['labels'] for a in anns]

    def _batch_jpeg(self, indices, H, W):
        """uint8 [N,H,W,3] on the device for a batch holding JPEG files: the decode threads run the entropy stage of each
        JPEG into its slot of one pinned buffer (descriptors first, then one coefficient slot per image), one upload, the
        pixel stage on the current stream.  A file the native path declines or fails on (and any other file) is decoded
        as ``decode_into`` does it and copied into its place, so its bytes - or its error - are the PIL path's."""
        from . import _lib, hip_ops
        L = _lib.lib()
        n, D = len(indices), hip_ops.JPEG_DESC_BYTES
        slot = int(L.oadg_jpeg_coef_capacity(H, W))
        dbytes = n * D                                   # (a multiple of 16: the coefficients stay 16-byte aligned)
        need = dbytes + 2 * n * slot
        cslot = self._coef_slot(need)
        arr = cslot.host.numpy()
        base = arr.ctypes.data

        def work(a):
            i, idx = a
            path = self._path(idx)
            arr[i * D:(i + 1) * D] = 0                   # ncomp 0: the pixel stage leaves this image alone
            if path.lower().endswith(_JPEG_EXT):
                rc = L.oadg_jpeg_entropy_decode(path.encode(), H, W, base + dbytes + 2 * i * slot, slot, base + i * D)
                if rc == 0:
                    return None
            img = np.empty((H, W, 3), dtype=np.uint8)
            self.decode_into(idx, img)
            return img
        try:
            host_imgs = list(self._pool.map(work, enumerate(indices)))
        except BaseException:
            cslot.release()
            raise
        native = sum(a is None for a in host_imgs)
        self._count('native', native)
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
        if native:
            dev = cslot.commit(need, self.device)
            hip_ops.jpeg_pixels_bgr(dev[dbytes:].view(torch.int16), dev[:dbytes], out, slot)
        else:
            cslot.release()
        for i, img in enumerate(host_imgs):
            if img is not None:
                out[i].copy_(torch.from_numpy(img))
        return out


@DATASETS.register_module()
class CityscapesDataset(CocoDataset):
    """cityscapes.py:19-110."""
    CLASSES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')

    def _skip_all_crowd(self, info):
        anns = self.coco.load_anns(self.coco.get_ann_ids(img_ids=[info['id']]))
        return self.filter_empty_gt and all(a['iscrowd'] for a in anns)

    @staticmethod
    def _degenerate(ann, img_info, x1, y1, w, h):
        return ann['area'] <= 0 or w < 1 or h < 1


@DATASETS.register_module()
class XMLDataset(CocoDataset):
    """xml_style.py:14-154: VOC-style ``ann_file`` (one image id per line), ``{img_prefix}/{ann_subdir}/{id}.xml``
    annotations and ``{img_subdir}/{id}.jpg`` images.  Each XML file is parsed once, here, instead of on every
    ``_filter_imgs`` / ``get_ann_info`` call (same results).  Decoding, rings, ``batch()`` and ``flag`` are CocoDataset's."""
    EVAL_PROTOCOLS = (evaluation.VOC_EVAL,)

    def evaluate(self, results, metric='mAP', logger=None, **eval_kwargs):
        return evaluation.dataset_evaluate(self, results, metric=metric, logger=logger, **eval_kwargs)

    def format_results(self, results, **kwargs):
        """custom.py:185-186 of the reference is an empty placeholder: a VOC-style dataset has no result file"""
        raise NotImplementedError(f'{type(self).__name__}.format_results is not built: the COCO result file belongs to the '
                                  f'COCO-format datasets (CocoDataset, CityscapesDataset)')

    def __init__(self, min_size=None, img_subdir='JPEGImages', ann_subdir='Annotations', **kwargs):
        assert self.CLASSES or kwargs.get('classes', None), 'CLASSES in `XMLDataset` can not be None.'
        self.img_subdir, self.ann_subdir = img_subdir, ann_subdir
        super().__init__(**kwargs)
        self.cat2label = {cat: i for i, cat in enumerate(self.CLASSES)}
        self.min_size = min_size

    # ---- xml_style.py:38-67
    def load_annotations(self, ann_file):
        with open(ann_file) as f:
            img_ids = [line.rstrip('\n\r') for line in f]          # mmcv.list_from_file
        data_infos = []
        for img_id in img_ids:
            filename = os.path.join(self.img_subdir, f'{img_id}.jpg')
            root = ET.parse(os.path.join(self.img_prefix, self.ann_subdir, f'{img_id}.xml')).getroot()
            size = root.find('size')
            if size is not None:
                width, height = int(size.find('width').text), int(size.find('height').text)
            else:
                from PIL import Image
                with Image.open(os.path.join(self.img_prefix, filename)) as img:
                    width, height = img.size
            objects = []
            for obj in root.findall('object'):
                difficult = obj.find('difficult')
                bnd = obj.find('bndbox')
                box = None if bnd is None else \
                    [int(float(bnd.find(t).text)) for t in ('xmin', 'ymin', 'xmax', 'ymax')]
                objects.append((obj.find('name').text, 0 if difficult is None else int(difficult.text), box))
            data_infos.append(dict(id=img_id, filename=filename, width=width, height=height, objects=objects))
        return data_infos

    # ---- xml_style.py:69-88
    def _filter_imgs(self, min_size=32):
        valid_inds = []
        for i, img_info in enumerate(self.data_infos):
            if min(img_info['width'], img_info['height']) < min_size:
                continue
            if self.filter_empty_gt:
                if any(name in self.CLASSES for name, _, _ in img_info['objects']):
                    valid_inds.append(i)
            else:
                valid_inds.append(i)
        return valid_inds

    # ---- xml_style.py:90-154
    def get_ann_info(self, idx):
        bboxes, labels, bboxes_ignore, labels_ignore = [], [], [], []
        for name, difficult, bbox in self.data_infos[idx]['objects']:
            if name not in self.CLASSES:
                continue
            label = self.cat2label[name]
            ignore = False
            if self.min_size:
                assert not self.test_mode
                if bbox[2] - bbox[0] < self.min_size or bbox[3] - bbox[1] < self.min_size:
                    ignore = True
            if difficult or ignore:
                bboxes_ignore.append(bbox)
                labels_ignore.append(label)
            else:
                bboxes.append(bbox)
                labels.append(label)
        if not bboxes:
            bboxes, labels = np.zeros((0, 4)), np.zeros((0,))
        else:
            bboxes, labels = np.array(bboxes, ndmin=2) - 1, np.array(labels)
        if not bboxes_ignore:
            bboxes_ignore, labels_ignore = np.zeros((0, 4)), np.zeros((0,))
        else:
            bboxes_ignore, labels_ignore = np.array(bboxes_ignore, ndmin=2) - 1, np.array(labels_ignore)
        return dict(bboxes=bboxes.astype(np.float32), labels=labels.astype(np.int64),
                    bboxes_ignore=bboxes_ignore.astype(np.float32), labels_ignore=labels_ignore.astype(np.int64))


@DATASETS.register_module()
class SdgodDataset(XMLDataset):
    """sdgod.py:12-106: the Diverse-Weather (S-DGOD) classes; the year is inferred from ``img_prefix``.  ``evaluate`` is the
    reference's VOC protocol (evaluation.sdgod_evaluate): legacy "+ 1" coordinates, ``difficult`` objects as ignore regions
    and, for a VOC2007 prefix, the 11-point AP - matched on the GPU (csrc/voc_eval.hip) when there is one."""
    CLASSES = ('bus', 'bike', 'car', 'motor', 'person', 'rider', 'truck')
    RECALL_LEGACY_COORDINATE = True      # sdgod.py:92-98: 'recall' with the VOC devkit's "+ 1" extents (evaluation.proposal_evaluate)

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if 'VOC2007' in self.img_prefix:
            self.year = 2007
        elif 'VOC2012' in self.img_prefix:
            self.year = 2012
        else:
            raise ValueError('Cannot infer dataset year from img_prefix')

    def evaluate(self, results, metric='mAP', logger=None, **eval_kwargs):
        return evaluation.sdgod_evaluate(self, results, metric=metric, logger=logger, **eval_kwargs)


@DATASETS.register_module()
class RepeatDataset:
    """dataset_wrappers.py RepeatDataset: ``times`` passes over the wrapped dataset per epoch."""

    def __init__(self, dataset, times):
        self.dataset, self.times = dataset, times
        self.CLASSES = getattr(dataset, 'CLASSES', None)
        self._ori_len = len(dataset)
        if hasattr(dataset, 'flag'):                      # dataset_wrappers.py:170-171
            self.flag = np.tile(dataset.flag, times)

    def __len__(self):
        return self.times * self._ori_len

    def batch(self, indices):
        return self.dataset.batch([i % self._ori_len for i in indices])

    def get_ann_info(self, idx):
        return self.dataset.get_ann_info(idx % self._ori_len)


@DATASETS.register_module()
class ConcatDataset:
    """dataset_wrappers.py:17-134 ConcatDataset: the datasets one after the other (length, ``batch``, ``get_ann_info``,
    the concatenated group flag) and ``evaluate`` with ``separate_eval=True``: every dataset on its own slice of the
    results, its keys prefixed ``{i}_``.  Evaluating the concatenation as a whole is not built."""

    def __init__(self, datasets, separate_eval=True):
        if not separate_eval:
            raise NotImplementedError("ConcatDataset(separate_eval=False) is not built")
        self.datasets, self.separate_eval = list(datasets), separate_eval
        self.CLASSES = getattr(self.datasets[0], 'CLASSES', None)
        self.cumulative_sizes = np.cumsum([len(d) for d in self.datasets]).tolist()
        if hasattr(self.datasets[0], 'flag'):
            self.flag = np.concatenate([d.flag for d in self.datasets])

    def __len__(self):
        return self.cumulative_sizes[-1]

    def _locate(self, idx):
        if idx < 0:
            if -idx > len(self):
                raise ValueError('absolute value of index should not exceed dataset length')
            idx = len(self) + idx
        k = bisect.bisect_right(self.cumulative_sizes, idx)
        return k, idx - (self.cumulative_sizes[k - 1] if k else 0)

    def get_ann_info(self, idx):
        k, i = self._locate(idx)
        return self.datasets[k].get_ann_info(i)

    def batch(self, indices):
        """one batch from ONE of the datasets (an image shape per batch, and a dataset per batch)"""
        where = [self._locate(i) for i in indices]
        assert len({k for k, _ in where}) == 1, 'a batch does not cross the seam between two concatenated datasets'
        return self.datasets[where[0][0]].batch([i for _, i in where])

    def evaluate(self, results, logger=None, **kwargs):
        assert len(results) == len(self), f'Dataset and results have different sizes: {len(self)} v.s. {len(results)}'
        total = {}
        for k, ds in enumerate(self.datasets):
            start = self.cumulative_sizes[k - 1] if k else 0
            for name, v in ds.evaluate(results[start:self.cumulative_sizes[k]], logger=logger, **kwargs).items():
                total[f'{k}_{name}'] = v
        return total


def _files_present(cfg):
    ann = cfg.get('ann_file')
    if isinstance(ann, (list, tuple)):
        return all(_files_present(dict(cfg, ann_file=a)) for a in ann)
    if ann is None:
        return True
    root = cfg.get('data_root')
    return os.path.exists(ann if (root is None or os.path.isabs(ann)) else os.path.join(root, ann))


def build_dataset(cfg, default_args=None, synthetic_fallback=False):
    """datasets/builder.py:31-82 (RepeatDataset, a list-valued ``ann_file`` -> ConcatDataset, plain datasets).
    ``synthetic_fallback``: a dataset whose annotation file does not exist on this machine (an unmodified reference
    config on a box without Cityscapes) is replaced by the Cityscapes-shaped synthetic source, loudly."""
    cfg = dict(cfg)
    if cfg.get('type') == 'RepeatDataset' and synthetic_fallback and not _files_present(cfg['dataset']):
        cfg = dict(cfg['dataset'])          # one synthetic pass is as good as eight
    if synthetic_fallback and cfg.get('type') != 'RepeatDataset' and not _files_present(cfg):
        from .pipelines import SyntheticCityscapes
        print(f"[oadg] {cfg.get('ann_file')} not found: using SyntheticCityscapes in place of {cfg.get('type')}", flush=True)
        keep = {k: v for k, v in (default_args or {}).items() if k in ('seed', 'device', 'test_mode')}
        cls = DATASETS.get(cfg.get('type')) if cfg.get('type') in DATASETS else None
        if isinstance(cls, type) and issubclass(cls, XMLDataset):     # labels within the head of a 7-class DWD config
            keep['num_classes'] = len(cfg.get('classes') or cls.CLASSES)
        return SyntheticCityscapes(pipeline=cfg.get('pipeline'), **keep)
    if cfg.get('type') == 'RepeatDataset':
        return RepeatDataset(build_dataset(cfg['dataset'], default_args, synthetic_fallback), cfg['times'])
    if isinstance(cfg.get('ann_file'), (list, tuple)):          # builder.py:31-55 _concat_dataset
        prefixes = cfg.get('img_prefix')
        parts = []
        for i, ann in enumerate(cfg['ann_file']):
            one = {k: v for k, v in cfg.items() if k != 'separate_eval'}
            one['ann_file'] = ann
            if isinstance(prefixes, (list, tuple)):
                assert len(prefixes) == len(cfg['ann_file']), 'one img_prefix per ann_file (or one string for all)'
                one['img_prefix'] = prefixes[i]
            parts.append(build_dataset(one, default_args))
        return ConcatDataset(parts, cfg.get('separate_eval', True))
    return build_from_cfg(cfg, DATASETS, default_args)
