"""GPU: csrc/coco_error.hip (oadg_coco_error.coco_error_match, evaluation.coco_error_analysis(device=...)) against the host
yardstick ``coco_error_flags_host`` (= ``_evaluate_img`` on the reference's relabelled box lists), byte for byte: the hand cases,
the seeded split in all 20 lanes, images and segments across the kernel's staging capacities, empty inputs, repeatability over
a garbage workspace, the refused arguments, and the tool with ``--device auto``.  Output buffers are pre-filled with 0xFF."""
import numpy as np
import pytest
import torch

import coco_error_cases as C
import oadg_coco_error
from oadg_amd import evaluation as E

pytestmark = pytest.mark.gpu
KEYS = oadg_coco_error.KEYS
LDS_GTS, LDS_DETS = oadg_coco_error.LDS_GTS, oadg_coco_error.LDS_DETS


def _device(pack, dev, thrs=C.THRS, sim=C.SIM, area_rng=C.AREA_RNG, fill=0xFF, workspace=None):
    up = [torch.from_numpy(pack[k]).to(dev) for k in KEYS]
    flags = torch.full((len(area_rng), len(thrs) + 2, len(pack['dets'])), fill, dtype=torch.uint8, device=dev)
    oadg_coco_error.coco_error_match(*up, [min(float(t), 1 - 1e-10) for t in thrs], sim, area_rng, out=flags, workspace=workspace)
    torch.cuda.synchronize()
    return flags.cpu().numpy()


def _check(pack, dev, **kw):
    want = E.coco_error_flags_host(pack, kw.get('thrs', C.THRS), kw.get('sim', C.SIM), kw.get('area_rng', C.AREA_RNG))
    got = _device(pack, dev, **kw)
    assert got.shape == want.shape and np.array_equal(got, want)
    return got


# ------------------------------------------------------------------------------------------------------------ hand cases
@pytest.mark.parametrize('name', sorted(C.hand_cases()))
def test_hand_case_flags(dev, name):
    images, K, sup, want = C.hand_cases()[name]
    flags = _check(C.pack_images(images, K, sup), dev)
    for a, rows in want.items():
        assert flags[a].T.tolist() == rows, (name, a)


# ------------------------------------------------------------------------------------------------------------ seeded split
def test_seeded_split_flags_and_ps_equal_the_host(dev):
    gt_anns, results = C.seeded_split()
    pack = E.pack_coco_error(gt_anns, results, 6, C.SUPERCATS)
    flags = _check(pack, dev)
    assert flags.shape[:2] == (4, 5)                                     # 20 lanes
    for a in range(4):
        assert set(np.unique(flags[a]).tolist()) == {0, 1, 2}, a
    assert (flags[:, 2] != flags[:, 3]).any() and (flags[:, 3] != flags[:, 4]).any()      # the three 0.1 rows all differ
    assert np.array_equal(E.coco_error_flags_device(pack, C.THRS, C.SIM, C.AREA_RNG, dev), flags)
    want = E.coco_error_analysis(gt_anns, results, 6, C.SUPERCATS, device=None)
    got = E.coco_error_analysis(gt_anns, results, 6, C.SUPERCATS, device=dev)
    assert got.dtype == np.float64 and np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ capacities
def _grid(n):
    """n boxes of 30 x 30, 40 apart"""
    xs, ys = np.meshgrid(np.arange(20) * 40.0, np.arange(16) * 40.0)
    assert n <= xs.size
    return np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 30.0), np.full(xs.size, 30.0)], 1)[:n]


def _big_image(n, n_det, rs):
    """an image of ``n`` boxes: class 0 on the even places, class 1 on the odd ones, so both classes have boxes on either
    side of every chunk border; every ninth a crowd, every fourth 'medium' by its area field.  ``n_det`` detections per class
    on boxes near the borders (first boxes, both sides of LDS_GTS, last boxes), two per box so that boxes get taken"""
    g = _grid(n)
    boxes = [(g[j, 0], g[j, 1], 30, 30, j % 2, 5000.0 if j % 4 == 0 else 900.0, int(j % 9 == 0)) for j in range(n)]
    near = np.array([j for j in list(range(8)) + list(range(n // 2 - 6, n // 2 + 6)) + list(range(LDS_GTS - 6, LDS_GTS + 6)) +
                     list(range(n - 10, n)) if 0 <= j < n])
    dets = {}
    for k in (0, 1):
        src = near[rs.randint(0, len(near), n_det)]
        dets[k] = np.concatenate([g[src] + rs.uniform(-3, 3, (n_det, 4)), np.round(rs.uniform(0, 1, (n_det, 1)), 1)], 1)
    return boxes, dets


def test_an_image_of_one_box_more_than_fits(dev):
    """LDS_GTS + 1 boxes: the own-class boxes of either class fall in both chunks, and two segments read the same image - each
    keeps the taken words of its own class in the shared workspace"""
    rs = np.random.RandomState(7)
    boxes, dets = _big_image(LDS_GTS + 1, 24, rs)
    assert boxes[LDS_GTS][4] == 0 and boxes[LDS_GTS - 1][4] == 1 and boxes[0][4] == 0 and boxes[1][4] == 1
    small = ([(0, 0, 40, 40, 1), (100, 0, 40, 40, 0)], {0: [[1, 0, 40, 40, 0.9]], 1: [[0, 1, 40, 40, 0.8]]})
    pack = C.pack_images([small, (boxes, dets), small], 2, [0, 0])
    flags = _check(pack, dev)
    big = slice(2, 2 + 48)
    assert {0, 1, 2} <= set(np.unique(flags[C.ALL][:, big]).tolist())
    assert 0 < (flags[C.ALL, 2, big] == 1).sum() < 48                     # some boxes were contested: taken words matter


def test_more_detections_than_fit_on_3_boxes(dev):
    rs = np.random.RandomState(8)
    boxes = [(10, 10, 40, 40, 0), (100, 10, 40, 40, 1), (10, 100, 60, 60, 0)]
    g = np.array([b[:4] for b in boxes], np.float64)
    n = LDS_DETS + 1
    d = np.concatenate([g[rs.randint(0, 3, n)] + rs.uniform(-6, 6, (n, 4)), np.round(rs.uniform(0, 1, (n, 1)), 1)], 1)
    flags = _check(C.pack_images([(boxes, {0: d, 1: d[:5]})], 2, [0, 0]), dev)
    assert (flags[C.ALL, 2, :n] == 1).sum() == 2 and (flags[C.ALL, 3, :n] == 2).sum() > 0


def test_boxes_and_detections_both_beyond_the_capacities(dev):
    rs = np.random.RandomState(9)
    boxes, dets = _big_image(LDS_GTS + 1, LDS_DETS + 1, rs)
    pack = C.pack_images([(boxes, dets)], 2, [0, 0])
    flags = _check(pack, dev)
    assert flags.shape[2] == 2 * (LDS_DETS + 1) and {0, 1, 2} <= set(np.unique(flags[C.ALL]).tolist())
    _check(C.pack_images([(boxes, dets)], 2, [0, 1]), dev)                # (another supercategory: row 3 loses the foreign boxes)


# ------------------------------------------------------------------------------------------------------------ empty inputs
def test_empty_inputs(dev):
    empty = E.pack_coco_error([], [], 3, [0, 0, 1])
    assert _device(empty, dev).shape == (4, 5, 0)
    assert E.coco_error_flags_device(empty, C.THRS, C.SIM, C.AREA_RNG, dev).shape == (4, 5, 0)
    det = [[10, 10, 40, 40, 0.9], [300, 300, 20, 20, 0.2]]
    images = [([], {0: det, 1: det[:1]}),                                 # detections in an image without boxes
              ([(10, 10, 40, 40, 0), (60, 60, 40, 40, 1)], {}),           # boxes and no detections
              ([], {}),
              ([(10, 10, 40, 40, 1)], {0: det})]
    flags = _check(C.pack_images(images, 2, [0, 0]), dev)
    assert flags.shape == (4, 5, 5)
    assert flags[C.ALL].T.tolist() == [[0] * 5] * 3 + [[0, 0, 0, 2, 2], [0] * 5]
    assert flags[C.MEDIUM].T.tolist() == [[0] * 5, [2] * 5, [0] * 5, [0, 0, 0, 2, 2], [2] * 5]      # (1600 and 400 pixels)
    only_boxes = C.pack_images(images[1:3], 2, [0, 0])
    assert len(only_boxes['gts']) == 2 and _device(only_boxes, dev).shape == (4, 5, 0)


# ------------------------------------------------------------------------------------------------ arguments, repeatability
def test_arguments_short_workspace_and_repeatability(dev):
    rs = np.random.RandomState(10)
    boxes, dets = _big_image(LDS_GTS + 12, 40, rs)
    pack = C.pack_images([(boxes, dets), (boxes[:9], {0: dets[0][:20]})], 2, [0, 0])
    G = len(pack['gts'])
    a = _check(pack, dev)
    for fill in (0xFF, 0x5A):                                            # the workspace's contents do not matter
        ws = torch.full((8 * G,), fill, dtype=torch.uint8, device=dev)
        assert _device(pack, dev, workspace=ws).tobytes() == a.tobytes()
    assert _device(pack, dev, fill=0x7F).tobytes() == a.tobytes()        # every element of the output is written
    with pytest.raises(RuntimeError, match='argument error -2'):         # OADG_ESIZE
        _device(pack, dev, workspace=torch.empty(8 * G - 8, dtype=torch.uint8, device=dev))
    L = oadg_coco_error._lib.lib()
    assert L.oadg_coco_error_workspace_bytes(2, 2, len(pack['dets']), G, 3, 4) == 8 * G
    assert L.oadg_coco_error_workspace_bytes(2, 2, 0, 0, 3, 4) == 8
    # (n_thr + 2) * n_area <= 64: 14 thresholds x 4 ranges fill all 64 lanes, 15 are refused (OADG_EARG)
    fourteen = [0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75]
    assert L.oadg_coco_error_workspace_bytes(2, 2, len(pack['dets']), G, 15, 4) == 0
    with pytest.raises(RuntimeError, match='argument error -1'):
        _device(pack, dev, thrs=fourteen + [0.9])
    full = _device(pack, dev, thrs=fourteen)
    assert np.array_equal(full[:, [13, 8, 0, 14, 15]], a)
    one = _check(pack, dev, thrs=[], area_rng=[C.AREA_RNG[C.SMALL]])      # no plain row, one range: two lanes
    assert np.array_equal(one[0], a[C.SMALL, 3:])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_coco_error.coco_error_match(*[torch.from_numpy(pack[k]) for k in KEYS], C.THRS, C.SIM, C.AREA_RNG)
    with pytest.raises(ValueError, match='contiguous'):
        up = [torch.from_numpy(pack[k]).to(dev) for k in KEYS]
        oadg_coco_error.coco_error_match(up[0].float(), *up[1:], C.THRS, C.SIM, C.AREA_RNG)


# ------------------------------------------------------------------------------------------------------------ the tool
def test_tool_with_device_auto_writes_the_host_runs_bytes(dev, tmp_path, capsys):
    T = C.load_tool('tools/analysis_tools/coco_error_analysis.py')
    gt_anns, results = C.seeded_split(3, n_img=6, n_cls=3)
    names = C.NAMES[:3]
    ann = C.write_ann(tmp_path / 'ann.json', gt_anns, names, supercategory=['human', 'human', 'vehicle'])
    res = C.coco_dataset(ann, names).format_results(results, jsonfile_prefix=str(tmp_path / 'r'))[0]['bbox']
    assert E.voc_device() is not None
    auto = T.main([res, str(tmp_path / 'auto'), '--ann', ann])
    assert 'matched on cuda' in capsys.readouterr().out
    host = T.main([res, str(tmp_path / 'host'), '--ann', ann, '--device', 'host'])
    assert 'matched on the host' in capsys.readouterr().out
    assert np.array_equal(auto['bbox'], host['bbox'])
    a = open(tmp_path / 'auto' / 'bbox' / 'error_analysis.json', 'rb').read()
    assert a == open(tmp_path / 'host' / 'bbox' / 'error_analysis.json', 'rb').read() and len(a) > 1000
