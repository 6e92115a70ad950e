"""Cityscapes gtFine instance maps -> the COCO-style json every Cityscapes config here reads
(``instancesonly_filtered_gtFine_{train,val,test}.json``), with the per-pixel work on the device.

usage: python tools/dataset_converters/cityscapes.py cityscapes_path [--img-dir leftImg8bit] [--gt-dir gtFine] [-o OUT] [--nproc N]

The command line and the json are those of the reference's tools/dataset_converters/cityscapes.py, which needs
cityscapesscripts and pycocotools and visits the full map once per instance (``inst_img == inst_id`` -> encode, area,
toBbox).  Here the ``*_gtFine_instanceIds.png`` maps of one extent are decoded by ``--nproc`` threads (capped at 16; the
native 16-bit PNG decoder runs without the interpreter lock) straight into a pinned ring slot, uploaded as a batch, and
csrc/instance_maps.hip returns, for all instances of every map at once, (id, area, box) in ascending id order and the change
points of the column-major flattening; the run lengths of each kept instance are differences of its change points.  One
batch is decoded while the previous one is on the device.  The host reads PNG files and writes json, nothing else.

The tool needs the GPU: like every other device path of this project it has no host fallback.  (Its C-ABI calls live here,
not in the package: it is an offline tool, no training or inference step calls them - as tools/bench_decode.py does.)
"""
import argparse
import glob
import json
import os
import os.path as osp
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = osp.dirname(osp.dirname(osp.dirname(osp.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SUFFIX = 'leftImg8bit.png'
MIN_ID = 24                  # ids below are stuff labels: never an instance
MAX_THREADS = 16
BATCH = 8                    # maps per upload (8 x 1024 x 2048 x 2 bytes = 32 MiB of pinned memory per ring slot)
# cityscapesscripts.helpers.labels restricted to `hasInstances and not ignoreInEval`, in its order: the categories of the json
CATEGORIES = ((24, 'person'), (25, 'rider'), (26, 'car'), (27, 'truck'), (28, 'bus'), (31, 'train'), (32, 'motorcycle'),
              (33, 'bicycle'))
KEPT = frozenset(i for i, _ in CATEGORIES)
MAX_LABEL = 33               # labels 0..33 exist (29 caravan and 30 trailer have instances but are ignored in evaluation)
SET_NAME = dict(train='instancesonly_filtered_gtFine_train.json', val='instancesonly_filtered_gtFine_val.json',
                test='instancesonly_filtered_gtFine_test.json')


# ------------------------------------------------------------------------------------------------------------- files
def collect_files(img_dir, gt_dir):
    """[(image, instance map, label map)] for every ``**/*.png`` under img_dir, sorted (the reference's glob order is
    arbitrary); a file that does not end in leftImg8bit.png is an error that names it"""
    files = []
    for img_file in sorted(glob.glob(osp.join(img_dir, '**/*.png'))):
        if not img_file.endswith(SUFFIX):
            raise ValueError(f'{img_file}: not a *{SUFFIX} file')
        stem = img_file[len(img_dir):-len(SUFFIX)]
        files.append((img_file, gt_dir + stem + 'gtFine_instanceIds.png', gt_dir + stem + 'gtFine_labelIds.png'))
    if not files:
        raise ValueError(f'No images found in {img_dir}')
    print(f'Loaded {len(files)} images from {img_dir}')
    return files


# ---------------------------------------------------------------------------------------------------- annotations
def rle_to_string(counts):
    """COCO's compressed RLE string of the run lengths ``counts`` (zeros first) - a restatement of pycocotools' published
    rleToString (maskApi.c): each count after the third is stored as its difference from the count two places before it;
    a value goes out in 5-bit groups, low group first, taken from the signed value under arithmetic shift; bit 0x20 marks
    that more groups follow, which they do iff the remainder is not 0 - or not -1 when the group's 0x10 bit is set; every
    byte is offset by 48.
    PARITY UNPINNED: pycocotools is not available to this project's tests, so the string is checked against an independent
    decoder written from the format's description (tests/test_cityscapes_converter.py), not against pycocotools' bytes."""
    x = np.asarray(counts, dtype=np.int64).copy()
    if x.size > 3:
        x[3:] -= np.asarray(counts, dtype=np.int64)[1:-2]
    alive = np.ones(x.shape, dtype=bool)
    groups, valid = [], []
    while alive.any():
        c = x & 0x1f
        x = x >> 5                                            # (arithmetic on signed int64)
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        groups.append(c + np.where(more, 0x20, 0) + 48)
        valid.append(alive)
        alive = alive & more
    if not groups:
        return ''
    g, v = np.stack(groups, axis=1), np.stack(valid, axis=1)  # [value][group]: row-major order is the string's
    return g[v].astype(np.uint8).tobytes().decode('ascii')


def label_of(inst_id, where='<map>'):
    """instance id -> label id (``id // 1000`` from 1000 up, else the id itself: a crowd region); a label outside 0..33 is an
    error that names the file and the id"""
    inst_id = int(inst_id)
    label = inst_id // 1000 if inst_id >= 1000 else inst_id
    if not 0 <= label <= MAX_LABEL:
        raise ValueError(f'{where}: instance id {inst_id} gives label {label}, outside 0..{MAX_LABEL}')
    return label


def annotations_of_map(records, triples, f0, H, W, where='<map>'):
    """The reference's anno_info list of one map from what the device returns for it.
    records: int [r, 6] rows (id, pixel count, xmin, ymin, xmax, ymax) in ascending id; triples: int [m, 3] rows
    (p, f[p-1], f[p]) in ascending p over the column-major flattening f; f0 = f[0] = map[0, 0].
    The runs of instance k are the differences of [0, its change points..., H*W], with a leading 0 when f[0] == k."""
    records = np.asarray(records, dtype=np.int64).reshape(-1, 6)
    triples = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    HW = H * W
    # every change point under both ids it separates, grouped by id with p ascending inside a group
    ids = np.concatenate([triples[:, 1], triples[:, 2]])
    ps = np.concatenate([triples[:, 0], triples[:, 0]])
    order = np.lexsort((ps, ids))
    ids, ps = ids[order], ps[order]
    out = []
    for inst_id, area, xmin, ymin, xmax, ymax in records.tolist():
        if inst_id < MIN_ID:
            continue
        label = label_of(inst_id, where)
        if label not in KEPT:                                   # no instances, or ignored in evaluation
            continue
        lo, hi = np.searchsorted(ids, inst_id, 'left'), np.searchsorted(ids, inst_id, 'right')
        bounds = np.concatenate([[0], ps[lo:hi], [HW]])
        counts = np.diff(bounds)
        if int(f0) == inst_id:
            counts = np.concatenate([[0], counts])
        if int(counts[1::2].sum()) != area:
            raise RuntimeError(f'{where}: instance {inst_id}: runs cover {int(counts[1::2].sum())} pixels, area {area}')
        out.append(dict(iscrowd=int(inst_id < 1000), category_id=label,
                        bbox=[float(xmin), float(ymin), float(xmax - xmin + 1), float(ymax - ymin + 1)], area=int(area),
                        segmentation=dict(size=[H, W], counts=rle_to_string(counts))))
    return out


def image_info(files, H, W, anno_info):
    img_file, _, segm_file = files
    city = osp.basename(osp.dirname(img_file))
    return dict(file_name=osp.join(city, osp.basename(img_file)), height=int(H), width=int(W), anno_info=anno_info,
                segm_file=osp.join(city, osp.basename(segm_file)))


def cvt_annotations(image_infos, out_json_name):
    """image ids count from 0, annotation ids from 0 across the file; the `annotations` key is dropped when empty"""
    out = dict(images=[], categories=[], annotations=[])
    ann_id = 0
    for img_id, info in enumerate(image_infos):
        info = dict(info)
        annos = info.pop('anno_info')
        info['id'] = img_id
        out['images'].append(info)
        for a in annos:
            a = dict(a, image_id=img_id, id=ann_id)
            out['annotations'].append(a)
            ann_id += 1
    out['categories'] = [dict(id=i, name=n) for i, n in CATEGORIES]
    if not out['annotations']:
        out.pop('annotations')
    if out_json_name is not None:
        with open(out_json_name, 'w') as f:
            json.dump(out, f)
    return out


# ------------------------------------------------------------------------------------------------------- device path
class InstanceMaps:
    """csrc/instance_maps.hip on a batch of resident maps -> per map (records, triples) as numpy arrays.
    The capacities grow to what a batch needed: a short capacity is reported by the counts, never silently truncated."""

    def __init__(self, device):
        import torch
        from oadg_amd import _lib
        self.torch, self._lib, self.L, self.device = torch, _lib, _lib.lib(), torch.device(device)
        self.cap_records, self.cap_points = 1024, 1 << 16
        self.device_ms = 0.0

    def launch(self, maps, n, H, W):
        """enqueue both reductions of the uint8 device tensor ``maps`` (n*H*W uint16 samples) on the current stream"""
        torch, L, _lib = self.torch, self.L, self._lib
        i32 = dict(dtype=torch.int32, device=self.device)
        ws_bytes = int(L.oadg_instance_maps_workspace_bytes(n, H, W))
        if ws_bytes == 0:
            raise ValueError(f'maps of {H} x {W}: H * W must stay below 2^31')
        job = dict(maps=maps, n=n, H=H, W=W, ws=torch.empty(ws_bytes, dtype=torch.uint8, device=self.device),
                   records=torch.empty((n, self.cap_records, 6), **i32), triples=torch.empty((n, self.cap_points, 3), **i32),
                   counts=torch.empty((2, n), **i32), caps=(self.cap_records, self.cap_points),
                   t0=torch.cuda.Event(enable_timing=True), t1=torch.cuda.Event(enable_timing=True))
        job['t0'].record()
        s = _lib.stream_ptr()
        _lib.check(L.oadg_instance_stats(_lib.ptr(maps), n, H, W, MIN_ID, _lib.ptr(job['records']), job['caps'][0],
                                         _lib.ptr(job['counts'][0]), _lib.ptr(job['ws']), ws_bytes, s), 'oadg_instance_stats')
        _lib.check(L.oadg_instance_change_points(_lib.ptr(maps), n, H, W, MIN_ID, _lib.ptr(job['triples']), job['caps'][1],
                                                 _lib.ptr(job['counts'][1]), _lib.ptr(job['ws']), ws_bytes, s),
                   'oadg_instance_change_points')
        job['t1'].record()
        from oadg_amd import staging
        job['back'] = staging.readback(job['counts'])
        return job

    def finish(self, job):
        """-> [(records [r, 6], triples [m, 3])] per map; launches again with more room when a capacity was short"""
        counts = job['back'].wait().numpy()
        self.device_ms += job['t0'].elapsed_time(job['t1'])
        need_r, need_p = int(counts[0].max()), int(counts[1].max())
        if need_r > job['caps'][0] or need_p > job['caps'][1]:
            self.cap_records = max(self.cap_records, 1 << max(need_r - 1, 1).bit_length())
            self.cap_points = max(self.cap_points, 1 << max(need_p - 1, 1).bit_length())
            return self.finish(self.launch(job['maps'], job['n'], job['H'], job['W']))
        return [(job['records'][i, :int(counts[0, i])].cpu().numpy(), job['triples'][i, :int(counts[1, i])].cpu().numpy())
                for i in range(job['n'])]


def decode_map(L, path, dst):
    """one instance map into the uint16 [H, W] view ``dst`` of a pinned slot (native decoder; PIL for a PNG variant it
    does not cover)"""
    H, W = dst.shape
    rc = L.oadg_png_decode_gray16(path.encode(), dst.ctypes.data, H, W)
    if rc == 0:
        return
    if rc == -3:
        raise FileNotFoundError(f'{path}: cannot be read')
    if rc != -4:
        raise RuntimeError(f'{path}: oadg_png_decode_gray16 failed with {rc} (expected a {H} x {W} map)')
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.shape != (H, W) or a.min() < 0 or a.max() > 65535:
        raise ValueError(f'{path}: not a {H} x {W} greyscale map of 16 bits')
    np.copyto(dst, a.astype(np.uint16))


def map_extent(L, path):
    import ctypes
    h, w = ctypes.c_int(0), ctypes.c_int(0)
    rc = L.oadg_png_size(path.encode(), ctypes.byref(h), ctypes.byref(w))
    if rc == -3:
        raise FileNotFoundError(f'{path}: cannot be read')
    if rc != 0:
        from PIL import Image
        with Image.open(path) as im:
            return im.size[1], im.size[0]
    return h.value, w.value


def collect_annotations(files, nproc=1, device='cuda', timers=None):
    """the reference's image infos (with anno_info) of ``files``, in their order"""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('tools/dataset_converters/cityscapes.py runs its per-pixel work on the MI355X only; '
                           'there is no CPU fallback')
    from oadg_amd import staging
    timers = timers if timers is not None else {}
    for k in ('decode_s', 'device_wait_s', 'assemble_s'):
        timers.setdefault(k, 0.0)
    ops = InstanceMaps(device)
    L = ops.L
    threads = max(1, min(int(nproc), MAX_THREADS))
    infos = []
    with ThreadPoolExecutor(threads, thread_name_prefix='oadg-gtfine') as pool:
        extents = list(pool.map(lambda f: map_extent(L, f[1]), files))
        # consecutive files of one extent form batches: a map of another extent ends up in a batch of its own
        batches, i = [], 0
        while i < len(files):
            j = i + 1
            while j < len(files) and j - i < BATCH and extents[j] == extents[i]:
                j += 1
            batches.append((i, j))
            i = j
        ring = staging.Ring(2, 1 << 20)

        def finish(pending):
            job, lo, hi, f0s = pending
            t = time.perf_counter()
            per_map = ops.finish(job)
            timers['device_wait_s'] += time.perf_counter() - t
            t = time.perf_counter()
            for k, (records, triples) in enumerate(per_map):
                annos = annotations_of_map(records, triples, f0s[k], job['H'], job['W'], files[lo + k][1])
                infos.append(image_info(files[lo + k], job['H'], job['W'], annos))
            timers['assemble_s'] += time.perf_counter() - t

        pending = None
        for lo, hi in batches:
            (H, W), n = extents[lo], hi - lo
            t = time.perf_counter()
            slot = ring.reserve(n * H * W * 2)
            views = slot.host[:n * H * W * 2].numpy().view(np.uint16).reshape(n, H, W)
            try:
                list(pool.map(lambda k: decode_map(L, files[lo + k][1], views[k]), range(n)))
            except BaseException:
                slot.release()
                raise
            f0s = [int(views[k, 0, 0]) for k in range(n)]
            timers['decode_s'] += time.perf_counter() - t
            job = ops.launch(slot.commit(n * H * W * 2, ops.device), n, H, W)
            if pending is not None:
                finish(pending)                                  # (the batch before: it ran while this one was decoded)
            pending = (job, lo, hi, f0s)
        if pending is not None:
            finish(pending)
    timers['device_ms'] = timers.get('device_ms', 0.0) + ops.device_ms
    return infos


# ------------------------------------------------------------------------------------------------------ command line
def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Convert Cityscapes annotations to COCO format')
    parser.add_argument('cityscapes_path', help='cityscapes data path')
    parser.add_argument('--img-dir', default='leftImg8bit', type=str)
    parser.add_argument('--gt-dir', default='gtFine', type=str)
    parser.add_argument('-o', '--out-dir', help='output path')
    parser.add_argument('--nproc', default=1, type=int, help=f'number of decode threads (at most {MAX_THREADS})')
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    out_dir = args.out_dir if args.out_dir else args.cityscapes_path
    os.makedirs(out_dir, exist_ok=True)
    img_dir = osp.join(args.cityscapes_path, args.img_dir)
    gt_dir = osp.join(args.cityscapes_path, args.gt_dir)
    for split, json_name in SET_NAME.items():
        if not osp.isdir(osp.join(img_dir, split)):
            print(f'Skipping {split}: {osp.join(img_dir, split)} does not exist')
            continue
        print(f'Converting {split} into {json_name}')
        t = time.perf_counter()
        files = collect_files(osp.join(img_dir, split), osp.join(gt_dir, split))
        infos = collect_annotations(files, nproc=args.nproc)
        cvt_annotations(infos, osp.join(out_dir, json_name))
        print(f'It took {time.perf_counter() - t:.1f}s to convert Cityscapes annotation')


if __name__ == '__main__':
    main()
