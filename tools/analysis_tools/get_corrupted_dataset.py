#!/usr/bin/env python
"""Write the corrupted benchmark trees (Cityscapes-C, COCO-C, ...) that ``test_robustness.py --load-dataset corrupted``
reads, with the reference's command line (tools/analysis_tools/get_corrupted_dataset.py:32-231):

    python tools/analysis_tools/get_corrupted_dataset.py CONFIG --show-dir OUT
        [--corruptions benchmark|all|noise|blur|weather|digital|holdout|None|<names...>] [--severities 0 1 2 3 4 5]
        [--workers 32] [--seed 0] [--debug] [--cfg-options k=v ...]

For every (corruption, severity) - severity 0 once, under the first corruption - and every image of ``cfg.data.test`` in
dataset order, ``OUT/<corruption>/<severity>/<ori_filename>`` is written (sub-directories created, ``.jpg`` renamed
``.png``).  The file decodes to exactly the array ``Corrupt(corruption, severity)`` makes of the loaded image, so loading
it gives the bytes the on-the-fly ``--load-dataset original`` path feeds the model; numpy's global stream is seeded once
with ``--seed`` and consumed in this order.  With a ``/cityscapes/`` or ``/coco/`` image prefix, ``--show-dir`` is what
``evaluation.corrupted_img_prefix`` makes of that prefix without the trailing ``<corruption>/<severity>/``.

The reference decodes, corrupts and ``PIL.Image.save``s image by image in data-loader workers.  Here the split is decoded
once and stays on the device; a batch goes through ``Corrupt.batch`` (csrc/corrupt.hip for the names of
DEVICE_CORRUPTIONS, the host transform for the rest), then csrc/png_encode.hip turns it into one zlib stream per image
(row filters + literal-only dynamic-Huffman deflate), the streams are copied into a pinned slot and ``oadg_png_write_rgb8``
wraps them into files on up to ``--workers`` threads (at most 16; the call takes no interpreter lock).  Encoding, the copy
and the writes of one batch run while the next one is corrupted.

The tool needs the GPU: like every other device path of this project it has no host fallback.  (``PngEncoder`` and
``write_png`` - the C-ABI calls - live in oadg_draw.py next to the package's import shim, which the test loop's
``--show-dir`` uses too; they are importable from here under the same names.)
"""
import argparse
import copy
import os
import os.path as osp
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = osp.dirname(osp.dirname(osp.dirname(osp.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# the device PNG encoder (csrc/png_encode.hip) and the file writer, re-exported under the names they had here; the test
# loop's --show-dir uses them too.  (Imports torch and the package: the library itself is loaded at first use.)
from oadg_draw import BATCH, PINNED_SLOTS, PngEncoder, write_png  # noqa: E402,F401

MAX_THREADS = 16
CHOICES = ['all', 'benchmark', 'noise', 'blur', 'weather', 'digital', 'holdout', 'None', 'gaussian_noise', 'shot_noise',
           'impulse_noise', 'defocus_blur', 'glass_blur', 'motion_blur', 'zoom_blur', 'snow', 'frost', 'fog', 'brightness',
           'contrast', 'elastic_transform', 'pixelate', 'jpeg_compression', 'speckle_noise', 'gaussian_blur', 'spatter',
           'saturate']


class DictAction(argparse.Action):
    """key=value pairs -> dict (mmcv.DictAction); Config.merge_from_dict parses the values"""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, dict(kv.split('=', maxsplit=1) for kv in values))


# ------------------------------------------------------------------------------------------------------ command line
def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Write the corrupted copies of a test split')
    parser.add_argument('config', help='test config file path')
    parser.add_argument('--show-dir', required=True, help='directory where the corrupted images will be saved')
    parser.add_argument('--corruptions', type=str, nargs='+', default='benchmark', choices=CHOICES, help='corruptions')
    parser.add_argument('--severities', type=int, nargs='+', default=[0, 1, 2, 3, 4, 5], help='corruption severity levels')
    parser.add_argument('--workers', type=int, default=32, help=f'writer threads (at most {MAX_THREADS} are used)')
    parser.add_argument('--debug', action='store_true')
    parser.add_argument('--seed', type=int, default=0, help='random seed')
    parser.add_argument('--launcher', choices=['none', 'pytorch', 'slurm', 'mpi'], default='none', help='job launcher')
    parser.add_argument('--local_rank', type=int, default=0)
    parser.add_argument('--cfg-options', nargs='+', action=DictAction, help='override some settings in the used config')
    args = parser.parse_args(argv)
    if 'LOCAL_RANK' not in os.environ:
        os.environ['LOCAL_RANK'] = str(args.local_rank)
    return args


# -------------------------------------------------------------------------------------------------------- the tree
def plan(corruptions, severities):
    """[(corruption, severity)] in the reference's loop order; severity 0 (= no corruption) once, under the first name"""
    return [(c, s) for ci, c in enumerate(corruptions) for s in severities if not (ci > 0 and s == 0)]


def out_dir_of(show_dir, corruption, severity):
    return osp.join(show_dir, corruption, str(severity))


def out_path(out_dir, ori_filename):
    """get_corrupted_dataset.py:95-104: the file keeps its sub-directory, ``.jpg`` becomes ``.png``"""
    path = f'{out_dir}/{ori_filename}'
    if '.jpg' in path:
        path = path.replace('.jpg', '.png')
    return path


def writer_threads(workers, debug=False):
    return 1 if debug else max(1, min(int(workers), MAX_THREADS))


# ------------------------------------------------------------------------------------------------------ device path
def resident_split(ds):
    """the decoded split on the device: [(dataset indices, uint8 [n, H, W, 3] as the loader yields it: B, G, R)] - consecutive
    images of one extent form batches of at most BATCH"""
    shapes = [ds._shape(i) for i in range(len(ds))]
    out, i = [], 0
    while i < len(ds):
        j = i + 1
        while j < len(ds) and j - i < BATCH and shapes[j] == shapes[i]:
            j += 1
        out.append((list(range(i, j)), ds.batch(range(i, j))[0]))
        i = j
    return out


def generate(ds, show_dir, corruptions, severities, workers=MAX_THREADS, debug=False, timers=None):
    """write the tree for ``plan(corruptions, severities)``; -> the number of files"""
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt
    timers = timers if timers is not None else {}
    for k in ('corrupt_s', 'wait_s', 'bytes'):
        timers.setdefault(k, 0)
    dev = torch.device(ds.device)
    enc = PngEncoder(dev)
    split = resident_split(ds)
    made, files, futures_all = set(), 0, []
    with ThreadPoolExecutor(writer_threads(workers, debug), thread_name_prefix='oadg-png-write') as pool:

        def finish(pending):
            job, paths = pending
            t = time.perf_counter()
            streams = enc.finish(job)
            timers['wait_s'] += time.perf_counter() - t
            futures = [pool.submit(write_png, enc.L, p, addr, nb, job['H'], job['W']) for p, (addr, nb) in zip(paths, streams)]
            enc.release(job, futures)
            futures_all.extend(futures)
            if debug:
                for p in paths:
                    print(p)

        pending = None
        for corruption, severity in plan(corruptions, severities):
            print(f'\nWriting {corruption} at severity {severity}', flush=True)
            out_dir = out_dir_of(show_dir, corruption, severity)
            os.makedirs(out_dir, exist_ok=True)
            transform = Corrupt(corruption, severity) if severity > 0 else None
            for indices, imgs in split:
                paths = [out_path(out_dir, ds.data_infos[i]['filename']) for i in indices]
                for p in paths:
                    if osp.dirname(p) not in made:
                        os.makedirs(osp.dirname(p), exist_ok=True)
                        made.add(osp.dirname(p))
                t = time.perf_counter()
                batch = transform.batch(imgs) if transform is not None else imgs
                timers['corrupt_s'] += time.perf_counter() - t
                job = enc.launch(batch, bgr=True)
                if pending is not None:
                    finish(pending)                                # (the batch before: encoded and copied meanwhile)
                pending = (job, paths)
                files += len(paths)
        if pending is not None:
            finish(pending)
        for f in futures_all:
            timers['bytes'] += f.result()                          # (raises what a writer raised)
    timers['device_ms'] = timers.get('device_ms', 0.0) + enc.device_ms
    return files


def main(argv=None):
    args = parse_args(argv)
    import torch
    from oadg_amd import Config
    from oadg_amd import evaluation as E
    from oadg_amd.apis import set_random_seed
    from oadg_amd.datasets import build_dataset
    cfg = Config.fromfile(args.config)
    if args.cfg_options is not None:
        cfg.merge_from_dict(args.cfg_options)
    if args.workers == 0:
        args.workers = cfg.data.get('workers_per_gpu', 1)
    if args.debug:
        args.launcher = 'none'
    if args.launcher != 'none':
        raise TypeError('It does not support distribution mode')
    if not torch.cuda.is_available():
        raise RuntimeError('tools/analysis_tools/get_corrupted_dataset.py corrupts and encodes on the MI355X only; '
                           'there is no CPU fallback')
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', 0)) % torch.cuda.device_count())
    dev = torch.device('cuda', torch.cuda.current_device())
    if args.seed is not None:
        set_random_seed(args.seed)
    corruptions, severities = E.select_corruptions(args.corruptions, args.severities)
    dcfg = copy.deepcopy(cfg.data.test.to_dict() if hasattr(cfg.data.test, 'to_dict') else dict(cfg.data.test))
    dcfg['test_mode'] = True
    ds = build_dataset(dcfg, default_args=dict(device=dev))
    if not hasattr(ds, 'data_infos'):
        raise TypeError(f"{dcfg.get('type')} has no image files to corrupt")
    t = time.perf_counter()
    files = generate(ds, args.show_dir, corruptions, severities, args.workers, args.debug)
    print(f'\n{files} files in {time.perf_counter() - t:.1f}s under {args.show_dir}')
    return 0


if __name__ == '__main__':
    main()
