"""GPU: ``apis.init_detector`` / ``apis.inference_detector`` and demo/image_demo.py on a PNG file the test writes - the
result of ``inference_detector`` is the result of ``single_gpu_test`` on a one-image dataset of that file, and the demo's
picture is what Pillow makes (tests/draw_cases.py) of that file and that result.  The R50-FPN Cityscapes detector at its
initial weights (every image comes back with detections: tests/test_show_dir.py), one 64 x 128 image."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_cases as C  # noqa: E402

BASE = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes_oadg.py')
H, W = 64, 128
CONFIG = """_base_ = ['{base}']
test_pipeline = [
    dict(type='LoadImageFromFile'),
    dict(type='MultiScaleFlipAug', img_scale=({W}, {H}), flip=False,
         transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'),
                     dict(type='Normalize', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
                     dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),
                     dict(type='Collect', keys=['img'])])]
data = dict(test=dict(_delete_=True, type='CityscapesDataset', ann_file='{ann}', img_prefix='{prefix}/',
                      pipeline=test_pipeline))
"""


def _same(a, b):
    return len(a) == len(b) and all(p.dtype == q.dtype and np.array_equal(p, q) for p, q in zip(a, b))


@pytest.fixture(scope='module')
def setup(dev, tmp_path_factory):
    import torch
    from PIL import Image
    from oadg_amd import hip_conv
    from oadg_amd.apis import init_detector, set_random_seed, single_gpu_test
    from oadg_amd.datasets import CityscapesDataset, build_dataset
    from oadg_amd.pipelines import DevicePipeline
    d = tmp_path_factory.mktemp('inference')
    os.makedirs(d / 'imgs' / 'town')
    bgr = C.random_images('inference_detector', 1, H, W)[0]
    bgr[8:40, 16:90] //= 3                                                   # (some structure besides the noise)
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(d / 'imgs' / 'town' / 'one.png')
    ann = dict(images=[dict(id=1, file_name='town/one.png', height=H, width=W)],
               annotations=[dict(id=1, image_id=1, category_id=i + 1, bbox=[10, 10, 30, 20], area=600, iscrowd=0)
                            for i in range(1)],
               categories=[dict(id=i + 1, name=n) for i, n in enumerate(CityscapesDataset.CLASSES)])
    with open(d / 'ann.json', 'w') as f:
        json.dump(ann, f)
    cfg = d / 'cfg.py'
    cfg.write_text(CONFIG.format(base=BASE, W=W, H=H, ann=d / 'ann.json', prefix=d / 'imgs'))
    set_random_seed(0)
    try:
        model = init_detector(str(cfg), 'none', device=dev)
        # the yardstick of both tests: single_gpu_test on the one-image dataset of that file
        test = model.cfg.data.test.to_dict() if hasattr(model.cfg.data.test, 'to_dict') else dict(model.cfg.data.test)
        ds = build_dataset(test, default_args=dict(device=dev, test_mode=True))
        assert len(ds) == 1
        want, = single_gpu_test(model, ds, DevicePipeline(test['pipeline'], dtype=torch.bfloat16), torch.bfloat16, 1)
        assert sum(len(c) for c in want) >= 1
        yield dict(model=model, cfg=cfg, dir=d, bgr=bgr, path=str(d / 'imgs' / 'town' / 'one.png'), dev=dev, want=want)
    finally:
        hip_conv.enable(False)


@pytest.mark.gpu
def test_inference_detector_is_single_gpu_test_on_that_file(setup):
    import torch
    from oadg_amd.apis import inference_detector
    s = setup
    model, want = s['model'], s['want']
    assert model.CLASSES[2] == 'car' and not model.training and model.amp is torch.bfloat16
    got = inference_detector(model, s['path'])
    assert _same(got, want)
    assert _same(inference_detector(model, s['bgr']), want)                       # the decoded array
    both = inference_detector(model, [s['path'], s['bgr']])
    assert isinstance(both, list) and len(both) == 2 and _same(both[0], want) and _same(both[1], want)


@pytest.mark.gpu
def test_image_demo_writes_the_expected_picture(setup, tmp_path, monkeypatch):
    from PIL import Image
    from oadg_amd import apis
    from oadg_amd import visualization as V
    s = setup
    spec = importlib.util.spec_from_file_location('oadg_image_demo', os.path.join(ROOT, 'demo', 'image_demo.py'))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    a = demo.parse_args(['i.png', 'c.py', 'ck.pth', '--out-file', 'o.png'])
    assert (a.img, a.config, a.checkpoint, a.out_file, a.score_thr, a.device) == ('i.png', 'c.py', 'ck.pth', 'o.png', 0.3, 'cuda:0')
    with pytest.raises(SystemExit):
        demo.parse_args(['i.png', 'c.py', 'ck.pth'])                               # no window: --out-file is required
    # the demo builds its own detector: hand it the one of this module (the same initial weights would need the same seed)
    monkeypatch.setattr(apis, 'init_detector', lambda *args, **kw: s['model'])
    out = tmp_path / 'demo' / 'out.png'
    assert demo.main([s['path'], str(s['cfg']), 'none', '--out-file', str(out), '--score-thr', '0.05', '--device', str(s['dev'])]) == 0
    items, text = V.det_items(s['want'], s['model'].CLASSES, score_thr=0.05)
    assert len(items) >= 3
    with Image.open(out) as im:
        got = np.asarray(im)[:, :, ::-1]
    assert np.array_equal(got, C.draw_expect(s['bgr'], items, np.frombuffer(text, np.uint8)))
