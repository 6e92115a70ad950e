"""GPU: csrc/confusion.hip (oadg_confusion.confusion_count, evaluation.calculate_confusion_matrix(device=...)) against the
host functions of oadg_amd.evaluation with == - hand cases with their matrices written out, degenerate splits, the kernel's
capacities straddled, a seeded sweep, the reference's fixture -, the NMS rerun against oracle/nms.py, per_image_map on the
device, the bad arguments of the C ABI, and the confusion_matrix.py / analyze_results.py tools on a 4-image tree."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import confusion_cases as K
import oadg_confusion
from oadg_amd import _lib
from oadg_amd import evaluation as E

pytestmark = pytest.mark.gpu
ROOT = K.ROOT
GARBAGE = -0x0101010101010102          # what the output holds before the call: every byte set


def _device(pack, thr, dev, workspace=None):
    up = [torch.from_numpy(pack[k]).to(dev) for k in oadg_confusion.KEYS]
    C = pack['num_classes']
    out = torch.full((C + 1, C + 1), GARBAGE, dtype=torch.int64, device=dev)
    oadg_confusion.confusion_count(*up, C, thr, out=out, workspace=workspace)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(anns, results, C, score_thr, thr, dev):
    pack = E.pack_confusion_segments(results, anns, C, score_thr)
    want, got = E.confusion_counts_host(pack, thr), _device(pack, thr, dev)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


def test_hand_cases(dev):
    for name, (C, anns, results, score_thr, thr, want) in K.HAND.items():
        assert _check(anns, results, C, score_thr, thr, dev).tolist() == want, name
    # all of them as one split of C = 3 where they fit: the matrices add up
    names = ('a', 'c')
    anns = [a for n in names for a in K.HAND[n][1]]
    results = [r for n in names for r in K.HAND[n][2]]
    total = _check(anns, results, 3, 0.3, 0.5, dev)
    assert total.tolist() == (np.array(K.HAND['a'][5]) + np.array(K.HAND['c'][5])).tolist()


def test_degenerate_splits_overwrite_a_garbage_output(dev):
    box = K._ann([[10, 10, 50, 50]], [1])
    none = K._ann([], [])
    det = K._res(2, c0=[[10, 10, 50, 50, 0.9]])
    assert _check([none], [det], 2, 0, 0.5, dev).tolist() == [[0, 0, 0], [0, 0, 0], [1, 0, 0]]       # image without boxes
    assert _check([box], [K._res(2)], 2, 0, 0.5, dev).tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]  # without detections
    assert _check([none], [K._res(2)], 2, 0, 0.5, dev).sum() == 0                                    # both empty
    assert _check([none, box, none], [K._res(2), det, det], 2, 0, 0.5, dev).tolist() == [[0, 0, 0], [1, 0, 1], [1, 0, 0]]
    assert _check([], [], 2, 0, 0.5, dev).tolist() == [[0] * 3] * 3                                  # S = 0
    assert _check([box, box], [K._res(2)] * 2, 2, 0, 0.5, dev)[1, 2] == 2                            # D = 0
    assert _check([none, none], [det, det], 2, 0, 0.5, dev)[2, 0] == 2                               # G = 0
    assert _check([box], [K._res(2, c0=[[10, 10, 50, 50, 0.2]])], 2, 0.3, 0.5, dev).tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 0]]


def _grid(k, step=40.0, side=30.0, cols=40):
    j = np.arange(k)
    x, y = (j % cols) * step, (j // cols) * step
    return np.stack([x, y, x + side, y + side], 1).astype(np.float32)


@pytest.mark.parametrize('n_det', [63, 64, 65, oadg_confusion.CHUNK - 1, oadg_confusion.CHUNK, oadg_confusion.CHUNK + 1])
def test_detections_across_the_wave_and_the_chunk(dev, n_det):
    """n_det detections of one image: the lanes' passes and the staging chunk's size - 1, exactly and + 1, over boxes that
    fill a chunk but for one, exactly, and one more"""
    rs = np.random.RandomState(n_det)
    C = 4
    for k in (oadg_confusion.CHUNK - 1, oadg_confusion.CHUNK, oadg_confusion.CHUNK + 1):
        g = _grid(k)
        gl = rs.randint(0, C, k)
        src = rs.randint(0, k, n_det)
        d = np.concatenate([g[src] + rs.uniform(-4, 4, (n_det, 4)), rs.uniform(0.1, 1, (n_det, 1))], 1).astype(np.float32)
        far = np.zeros(n_det, bool)
        far[:-1:7] = True
        d[far, :4] += 10000                                          # background false positives
        dl = np.where(rs.randint(2, size=n_det) > 0, gl[src], rs.randint(0, C, n_det))
        # the LAST box of the image is matched by the last detection: the chunk's tail is read
        d[-1, :4], dl[-1] = g[-1], gl[-1]
        got = _check([dict(bboxes=g, labels=gl)], [[d[dl == c] for c in range(C)]], C, 0, 0.5, dev)
        assert got[:C, :C].sum() == n_det - far.sum() and got[C, :C].sum() == far.sum() and got[:C, C].sum() > 0


@pytest.mark.parametrize('k', [oadg_confusion.LDS_BOXES - 1, oadg_confusion.LDS_BOXES, oadg_confusion.LDS_BOXES + 1])
def test_boxes_across_the_lds_found_capacity(dev, k):
    """k boxes in one image (beyond the capacity the "found" words live in the workspace), next to a small image before and
    after it; every other box found, the last box found by one detection alone"""
    rs = np.random.RandomState(k)
    C = 3
    g = _grid(k)
    gl = rs.randint(0, C, k)
    hit = np.concatenate([np.arange(0, k, 2), [k - 1]])
    d = np.concatenate([g[hit], rs.uniform(0.5, 1, (len(hit), 1))], 1).astype(np.float32)
    big = (dict(bboxes=g, labels=gl), [d[gl[hit] == c] for c in range(C)])
    small = (K.HAND['a'][1][0], K.HAND['a'][2][0])
    anns, results = zip(small, big, small)
    got = _check(list(anns), list(results), C, 0.3, 0.5, dev)
    n_found = len(np.unique(hit))
    assert got[:C, C].sum() == (k - n_found) + 2 and np.trace(got[:C, :C]) == len(hit) + 2
    # a workspace one byte short of the boxes' words is refused
    pack = E.pack_confusion_segments(list(results), list(anns), C, 0.3)
    with pytest.raises(RuntimeError, match='argument error -2'):
        _device(pack, 0.5, dev, workspace=torch.empty(4 * len(pack['gts']) - 4, dtype=torch.uint8, device=dev))


@pytest.mark.parametrize('C', [1, 8, 80, 90])
def test_class_counts_up_to_and_beyond_the_lds_histogram(dev, C):
    """(C + 1)^2 cells: 4, 81 and 6561 are counted in LDS, 8281 (C = 90) with global atomic adds"""
    assert (81 ** 2 <= oadg_confusion.LDS_CELLS < 91 ** 2)
    anns, results = K.random_split(100 + C, 24, C, max_boxes=20, max_dets=60)
    if C >= 80:                                                      # the last class and the last label are used
        i0 = next(i for i, a in enumerate(anns) if len(a['labels']))
        anns[i0]['labels'][:] = C - 1
        results[i0][C - 1] = np.concatenate([anns[i0]['bboxes'][:1], [[0.9]]], 1).astype(np.float32)
    got = _check(anns, results, C, 0.3, 0.5, dev)
    assert got[C, :C].sum() > 0 and got[:C, C].sum() > 0 and np.trace(got[:C, :C]) > 0
    if C >= 80:
        assert got[C - 1, C - 1] >= 1


@pytest.mark.parametrize('fractional', [False, True])
def test_seeded_sweep_equals_the_host(dev, fractional):
    anns, results = K.random_split(31 + fractional, 200, 8, fractional=fractional)
    for score_thr, thr in ((0, 0.5), (0.3, 0.5), (0.3, 0.75)):
        got = _check(anns, results, 8, score_thr, thr, dev)
        off = got[:8, :8].sum() - np.trace(got[:8, :8])
        assert off > 0 and got[8, :8].sum() > 0 and got[:8, 8].sum() > 0
    a = _check(anns, results, 8, 0, 0.5, dev)
    assert a.tobytes() == _check(anns, results, 8, 0, 0.5, dev).tobytes()                # the same numbers from run to run


def test_device_equals_the_reference_fixture(dev):
    z, anns, results, n, C = K.load_fixture()
    for k, (score_thr, thr) in enumerate(z['cases'].tolist()):
        pack = E.pack_confusion_segments(results, anns, C, score_thr)
        assert np.array_equal(_device(pack, thr, dev), z[f'cm_{k}']), k
        assert np.array_equal(E.confusion_counts_device(pack, thr, dev), z[f'cm_{k}']), k


def test_calculate_confusion_matrix_with_and_without_nms(dev):
    from oracle import nms as O
    from test_result_analysis import _Split
    anns, results = K.random_split(77, 40, 5, max_boxes=10, max_dets=60)
    for res in results:                                              # close copies, so that the suppression has work
        for c in range(5):
            if len(res[c]):
                twin = res[c].copy()
                twin[:, :4] += 1.5
                twin[:, 4] *= 0.9
                res[c] = np.concatenate([res[c], twin]).astype(np.float32)
    ds = _Split(anns, 5)
    plain = E.calculate_confusion_matrix(ds, results, 0.3, None, 0.5, device=dev)
    assert plain.dtype == np.float64 and np.array_equal(plain, E.calculate_confusion_matrix(ds, results, 0.3, None, 0.5, device=None))
    assert np.array_equal(E.calculate_confusion_matrix(ds, results, 0.3, device='auto'), plain) and E.voc_device() is not None
    for iou_thr in (0.5, 0.3):
        # the yardstick of the NMS path: oracle/nms.py over the rows with score > score_thr, then the host counts
        kept = []
        for res in results:
            per_class = []
            for d in res:
                d = d[d[:, 4] > np.float32(0.3)]
                per_class.append(O.nms(torch.from_numpy(d[:, :4].copy()), torch.from_numpy(d[:, 4].copy()), iou_thr)[0].numpy())
            kept.append(per_class)
        want = E.calculate_confusion_matrix(ds, kept, 0.3, None, 0.5, device=None)
        got = E.calculate_confusion_matrix(ds, results, 0.3, iou_thr, 0.5, device=dev)
        assert np.array_equal(got, want), iou_thr
        assert np.array_equal(E.calculate_confusion_matrix(ds, results, 0.3, iou_thr, 0.5, device=None), want)
        assert got.sum() < plain.sum()
        assert sum(len(d) for r in kept for d in r) < sum(int((d[:, 4] > np.float32(0.3)).sum()) for r in results for d in r)


def test_per_image_map_on_the_device(dev):
    z, anns, results, n, C = K.load_fixture()
    assert np.array_equal(E.per_image_map(results, anns, C, device=dev), z['per_image_map'])
    anns, results = K.random_split(5, 60, 4)
    host = E.per_image_map(results, anns, 4, device=None)
    assert np.array_equal(E.per_image_map(results, anns, 4, device=dev), host) and len(np.unique(host)) > 10


def test_bad_arguments_return_the_code_and_launch_nothing(dev):
    """tests/test_cabi.py's question of this entry point: every refusal returns OADG_EARG / OADG_ESIZE, and the output - full
    of garbage before - is left as it was, so nothing was zeroed and nothing was launched"""
    L = _lib.lib()
    pack = E.pack_confusion_segments(K.HAND['a'][2], K.HAND['a'][1], 3, 0.3)
    up = {k: torch.from_numpy(pack[k]).to(dev) for k in oadg_confusion.KEYS}
    out = torch.full((4, 4), GARBAGE, dtype=torch.int64, device=dev)
    need = int(L.oadg_confusion_workspace_bytes(1, 2, 2, 3))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)
    assert need == 8 and L.oadg_confusion_workspace_bytes(1, 2, 3000, 3) == 12000
    for bad in ((-1, 2, 2, 3), (1, -1, 2, 3), (1, 2, -1, 3), (1, 2, 2, 0), (1, 2, 2, _lib.CONFUSION_MAX_CLASSES + 1)):
        assert L.oadg_confusion_workspace_bytes(*bad) == 0

    def call(S=1, D=2, G=2, C=3, counts=out, workspace=ws, nbytes=None, **swap):
        p = {k: _lib.ptr(swap.get(k, up[k])) for k in oadg_confusion.KEYS}
        return L.oadg_confusion_count(p['dets'], p['det_cls'], p['det_off'], p['gts'], p['gt_lab'], p['gt_off'], S, D, G, C,
                                      0.5, _lib.ptr(counts), _lib.ptr(workspace),
                                      workspace.numel() if nbytes is None and workspace is not None else (nbytes or 0),
                                      _lib.stream_ptr())
    EARG, ESIZE = -1, -2
    assert call(S=-1) == EARG and call(D=-1) == EARG and call(G=-1) == EARG
    assert call(C=0) == EARG and call(C=_lib.CONFUSION_MAX_CLASSES + 1) == EARG
    assert call(counts=None) == EARG and call(workspace=None) == EARG
    for k in oadg_confusion.KEYS:
        assert call(**{k: None}) == EARG, k
    assert call(dets=up['dets'].view(-1)[1:5].view(1, 4), D=1) == EARG            # boxes not 16-byte aligned
    assert call(gts=up['gts'].view(-1)[1:5].view(1, 4), G=1) == EARG
    assert call(workspace=ws[1:]) == EARG                                        # workspace not 4-byte aligned
    assert call(nbytes=need - 1) == ESIZE
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == GARBAGE).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == K.HAND['a'][5]
    # the Python wrapper's own refusals
    t = [up[k] for k in oadg_confusion.KEYS]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_confusion.confusion_count(*[torch.from_numpy(pack[k]) for k in oadg_confusion.KEYS], 3, 0.5)
    with pytest.raises(ValueError, match='num_classes'):
        oadg_confusion.confusion_count(*t, 0, 0.5)
    with pytest.raises(ValueError, match='counts must be'):
        oadg_confusion.confusion_count(*t, 3, 0.5, out=torch.empty((3, 3), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match='contiguous'):
        oadg_confusion.confusion_count(t[0].double(), *t[1:], 3, 0.5)


def test_labels_outside_the_classes_stay_in_bounds(dev):
    """the pack refuses them; handed to the kernel all the same, a class or label outside [0, C) takes no part"""
    pack = E.pack_confusion_segments(K.HAND['a'][2], K.HAND['a'][1], 3, 0.3)
    pack = dict(pack, gt_lab=np.array([0, 7], np.int32), det_cls=np.array([0, -5], np.int32),
                det_off=np.array([-3, 99], np.int32), gt_off=np.array([0, 1 << 30], np.int32))
    assert _device(pack, 0.5, dev).tolist() == [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]]


def test_tools_on_a_synthetic_tree_take_the_device_path(dev, tmp_path, monkeypatch):
    from PIL import Image
    from oadg_amd.datasets import CityscapesDataset
    t = K.synthetic_tree(tmp_path, monkeypatch)
    ds = CityscapesDataset(ann_file=t['ann'], img_prefix=t['prefix'], test_mode=True, device='cpu')
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = tmp_path / 'cm'
    r = subprocess.run([sys.executable, os.path.join(K.TOOLS, 'confusion_matrix.py'), t['cfg'], t['pkl'], str(out),
                        '--nms-iou-thr', '0.5'], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    js = json.load(open(out / 'confusion_matrix.json'))
    assert js['device'].startswith('cuda')
    assert js['counts'] == E.calculate_confusion_matrix(ds, t['results'], 0.3, 0.5, 0.5, device=None).astype(np.int64).tolist()
    with Image.open(out / 'confusion_matrix.png') as im:
        im.load()
    # ---- analyze_results.py: topk 3 of 4 images becomes 2; the names carry the host's per-image mAP
    show = tmp_path / 'show'
    r = subprocess.run([sys.executable, os.path.join(K.TOOLS, 'analyze_results.py'), t['cfg'], t['pkl'], str(show), '--topk', '3'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'matched on cuda' in r.stdout
    maps = E.per_image_map(t['results'], [ds.get_ann_info(i) for i in range(t['n'])], len(ds.CLASSES), device=None)
    assert maps[0] == 1.0 and maps[-1] == 0.0 and all(0.0 < m < 1.0 for m in maps[1:-1])
    good, bad = E.rank_images(maps, 3)
    assert len(good) == len(bad) == 2 and [i for i, _ in bad][0] == t['n'] - 1 and [i for i, _ in good][-1] == 0
    for name, chosen in (('good', good), ('bad', bad)):
        assert sorted(os.listdir(show / name)) == sorted(f'{i}_{round(m, 3)}.png' for i, m in chosen)
        for i, m in chosen:
            with Image.open(show / name / f'{i}_{round(m, 3)}.png') as im:
                im.load()
                assert im.size == (t['W'], t['H']) and im.mode == 'RGB'
                painted = np.asarray(im)[:, :, ::-1]
            src = ds.batch([i])[0][0].numpy()
            assert painted.shape == src.shape and not np.array_equal(painted, src)           # the boxes are on it
            b = ds.get_ann_info(i)['bboxes'][0].astype(np.int32)
            assert tuple(painted[b[1], (b[0] + b[2]) // 2]) in ((255, 102, 61), (72, 101, 241), (0, 0, 0))
