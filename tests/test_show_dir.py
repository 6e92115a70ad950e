"""GPU: ``single_gpu_test(show_dir=...)`` and ``BaseDetector.show_result`` - the written pictures decode to exactly what
Pillow makes (tests/draw_cases.py ``draw_expect``) of the image the network was fed and ``visualization.det_items`` of its
result; the results are those of a run without ``show_dir``; the dataset's resident images stay as they were.

Two 64 x 128 ``SyntheticCityscapes`` images, the R50-FPN detector of the Cityscapes config at its random initial weights,
``show_score_thr=0``.  A randomly initialised box head scores every class near 1 / 9, above the config's
``test_cfg.rcnn.score_thr`` of 0.05, so the config is used as it is: every image comes back with detections (asserted
below - a condition of the test, not a measurement - and seen on the MI355X: 100 per image, ``max_per_img``)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_cases as C  # noqa: E402

CFG = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes_oadg.py')
H, W = 64, 128
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _pipeline(corrupt=None):
    steps = [dict(type='LoadImageFromFile'),
             dict(type='MultiScaleFlipAug', img_scale=(W, H), flip=False,
                  transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **NORM),
                              dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                              dict(type='Collect', keys=['img'])])]
    if corrupt is not None:
        steps.insert(1, dict(type='Corrupt', corruption=corrupt, severity=3))   # where test_robustness.py puts it
    return steps


def _same(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(x, y))
                                    for x, y in zip(a, b))


def _decode(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == 'RGB'
        return np.asarray(im)[:, :, ::-1]                                    # the loaders' byte order: B, G, R


def _expect(source_bgr, result, names):
    from oadg_amd import visualization as V
    items, text = V.det_items(result, names, score_thr=0)
    assert len(items) >= 3, 'no detection to draw: the test would pass on an empty picture'
    return C.draw_expect(source_bgr, items, np.frombuffer(text, np.uint8))


@pytest.fixture(scope='module')
def setup(dev, tmp_path_factory):
    """the model, the dataset, the reference results (no show_dir) and one run with show_dir"""
    import torch
    from oadg_amd import Config, build_detector, hip_conv
    from oadg_amd.apis import set_random_seed, single_gpu_test
    from oadg_amd.pipelines import DevicePipeline, SyntheticCityscapes
    cfg = Config.fromfile(CFG)
    cfg.model.pop('pretrained', None)
    set_random_seed(0)
    model = build_detector(cfg.model, test_cfg=cfg.get('test_cfg'))
    model.init_weights(allow_missing_pretrained=True)
    model = model.to(dev).to(memory_format=torch.channels_last).eval()
    ds = SyntheticCityscapes(img_shape=(H, W), num_boxes=3, num_classes=8, length=2, box_size=(8, 40), seed=3, device=dev,
                             test_mode=True)
    ds.CLASSES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')
    pipe = DevicePipeline(_pipeline(), dtype=torch.bfloat16)
    show_dir = tmp_path_factory.mktemp('show')
    hip_conv.enable()
    try:
        def run(dataset=ds, pipeline=pipe, **kw):
            out = single_gpu_test(model, dataset, pipeline, torch.bfloat16, 2, **kw)
            torch.cuda.synchronize()
            return out
        before = [ds.image(i).cpu().numpy() for i in range(2)]
        plain = run()
        shown = run(show_dir=str(show_dir), show_score_thr=0)
        yield dict(model=model, ds=ds, run=run, plain=plain, shown=shown, show_dir=show_dir, before=before, dev=dev)
    finally:
        hip_conv.enable(False)


@pytest.mark.gpu
def test_pictures_are_what_pillow_draws_and_results_do_not_change(setup):
    s = setup
    counts = [sum(len(c) for c in r) for r in s['plain']]
    print('detections per image at the config\'s test_cfg.rcnn.score_thr:', counts)
    assert all(n >= 1 for n in counts), counts
    assert _same(s['shown'], s['plain'])
    assert sorted(os.listdir(s['show_dir'])) == ['000000.png', '000001.png']
    for i in range(2):
        got = _decode(s['show_dir'] / f'{i:06d}.png')
        want = _expect(s['before'][i], s['plain'][i], s['ds'].CLASSES)
        assert not np.array_equal(want, s['before'][i])
        assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:5].tolist()


@pytest.mark.gpu
def test_source_images_are_untouched(setup):
    s = setup
    assert _same(s['run'](), s['plain'])                                      # again, after the run that drew
    for i in range(2):
        assert np.array_equal(s['ds'].image(i).cpu().numpy(), s['before'][i])


@pytest.mark.gpu
def test_a_show_dir_that_cannot_be_made_raises_its_own_error_and_leaves_no_thread(setup, tmp_path):
    import threading
    s = setup
    blocker = tmp_path / 'a_file'
    blocker.write_text('not a directory')
    with pytest.raises(OSError, match='a_file'):
        s['run'](show_dir=str(blocker / 'pics'), show_score_thr=0)
    assert not [t.name for t in threading.enumerate() if t.name.startswith('oadg-show-write')]
    assert _same(s['run'](), s['plain'])


@pytest.mark.gpu
def test_show_result_returns_the_bytes_of_the_file(setup, tmp_path):
    import torch
    s = setup
    src, res = s['before'][1], s['plain'][1]
    s['model'].CLASSES = s['ds'].CLASSES
    want = _expect(src, res, s['ds'].CLASSES)
    keep = src.copy()
    got = s['model'].show_result(src, res, score_thr=0)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(src, keep)
    resident = torch.from_numpy(src).to(s['dev'])
    assert s['model'].show_result(resident, res, score_thr=0, out_file=str(tmp_path / 'sub' / 'one.png')) is None
    assert np.array_equal(resident.cpu().numpy(), keep)                       # drawn on a copy
    assert np.array_equal(_decode(tmp_path / 'sub' / 'one.png'), want)
    assert np.array_equal(_decode(s['show_dir'] / '000001.png'), want)        # and the file --show-dir wrote
    # a path; a threshold and a style of the caller's
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(src[:, :, ::-1])).save(tmp_path / 'src.png')
    from oadg_amd import visualization as V
    items, text = V.det_items(res, s['ds'].CLASSES, score_thr=0.1, bbox_color='palette', text_color='white', thickness=1, font_size=22)
    got = s['model'].show_result(str(tmp_path / 'src.png'), res, score_thr=0.1, bbox_color='palette', text_color='white',
                                 thickness=1, font_size=22)
    assert np.array_equal(got, C.draw_expect(src, items, np.frombuffer(text, np.uint8)))


@pytest.mark.gpu
def test_the_picture_behind_a_corrupt_step_is_the_corrupted_image(setup, tmp_path):
    import torch
    from oadg_amd.pipelines import DevicePipeline
    s = setup
    pipe = DevicePipeline(_pipeline('brightness'), dtype=torch.bfloat16)     # (on the device, draws no random number)
    assert pipe.corrupt is not None
    results = s['run'](pipeline=pipe, show_dir=str(tmp_path), show_score_thr=0)
    assert _same(results, s['run'](pipeline=pipe))
    imgs = s['ds'].batch([0, 1])[0]
    fed = pipe.corrupt.batch(imgs).cpu().numpy()
    for i in range(2):
        assert not np.array_equal(fed[i], s['before'][i])
        assert np.array_equal(_decode(tmp_path / f'{i:06d}.png'), _expect(fed[i], results[i], s['ds'].CLASSES))


@pytest.mark.gpu
def test_file_names_follow_the_dataset(setup, tmp_path, monkeypatch):
    """a VOC tree of tools/make_synthetic_voc.py: JPEGImages/000000.jpg -> <show_dir>/JPEGImages/000000.png"""
    import torch
    from oadg_amd.datasets import build_dataset
    from oadg_amd.pipelines import DevicePipeline
    s = setup
    spec = importlib.util.spec_from_file_location('oadg_make_synthetic_voc', os.path.join(ROOT, 'tools', 'make_synthetic_voc.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    monkeypatch.setattr(sys, 'argv', ['make_synthetic_voc.py', str(tmp_path / 'voc'), '--n', '2', '--height', str(H), '--width',
                                      str(W), '--boxes', '2'])
    tool.main()
    voc = tmp_path / 'voc' / 'VOC2007'
    dcfg = dict(type='SdgodDataset', ann_file=str(voc / 'ImageSets' / 'Main' / 'train.txt'), img_prefix=str(voc) + '/',
                pipeline=_pipeline())
    ds = build_dataset(dcfg, default_args=dict(device=s['dev'], test_mode=True))
    assert [info['filename'] for info in ds.data_infos] == ['JPEGImages/000000.jpg', 'JPEGImages/000001.jpg']
    pipe = DevicePipeline(dcfg['pipeline'], dtype=torch.bfloat16)
    out = tmp_path / 'pics'
    results = s['run'](dataset=ds, pipeline=pipe, show_dir=str(out), show_score_thr=0)
    assert sorted(os.listdir(out)) == ['JPEGImages'] and sorted(os.listdir(out / 'JPEGImages')) == ['000000.png', '000001.png']
    fed = ds.batch([0, 1])[0].cpu().numpy()
    for i in range(2):
        assert np.array_equal(_decode(out / 'JPEGImages' / f'{i:06d}.png'), _expect(fed[i], results[i], ds.CLASSES))
