"""XMLDataset / SdgodDataset (mmdet/datasets/{xml_style,sdgod}.py) on a VOC tree written at test time, the S-DGOD
config, and - on the GPU - the native JPEG batch path, a train step and tools/train.py on JPEG files."""
import os
import sys

import numpy as np
import pytest
import torch

from inputs import lowpass_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDGOD_CFG = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod.py')


def _obj(name, box, difficult=None):
    d = '' if difficult is None else f'<difficult>{difficult}</difficult>'
    return (f'<object><name>{name}</name>{d}<bndbox><xmin>{box[0]}</xmin><ymin>{box[1]}</ymin>'
            f'<xmax>{box[2]}</xmax><ymax>{box[3]}</ymax></bndbox></object>')


def write_voc(root, images, year='VOC2007', quality=90):
    """images: id -> (H, W, write <size>?, [object xml]); JPEG frames of lowpass noise"""
    from PIL import Image
    base = os.path.join(root, year)
    for d in ('JPEGImages', 'Annotations', os.path.join('ImageSets', 'Main')):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    for k, (img_id, (H, W, with_size, objs)) in enumerate(images.items()):
        rs = np.random.RandomState(k)
        Image.fromarray(lowpass_image(rs, H, W, 4)).save(os.path.join(base, 'JPEGImages', f'{img_id}.jpg'), quality=quality)
        size = f'<size><width>{W}</width><height>{H}</height><depth>3</depth></size>' if with_size else ''
        with open(os.path.join(base, 'Annotations', f'{img_id}.xml'), 'w') as f:
            f.write(f'<annotation><filename>{img_id}.jpg</filename>{size}{"".join(objs)}</annotation>')
    with open(os.path.join(base, 'ImageSets', 'Main', 'train.txt'), 'w') as f:
        f.write(''.join(f'{i}\n' for i in images))
    return base + '/'


TREE = {
    'a': (80, 100, True, [_obj('car', ('10.6', 20, 50, 60)), _obj('person', (5, 5, 30, 30), 1), _obj('dog', (1, 1, 9, 9)),
                          _obj('bus', (40, 30, 90, 75), 0), _obj('rider', (60, 60, 66, 64))]),
    'b': (40, 64, False, [_obj('truck', (2, 3, 40, 38))]),
    'c': (48, 64, True, [_obj('bike', (1, 2, 20, 30), 1), _obj('motor', (20, 2, 60, 40), 1)]),
    'd': (48, 64, True, [_obj('dog', (1, 1, 30, 30))]),
    'e': (20, 100, True, [_obj('car', (1, 1, 10, 10))]),
}


def test_xml_dataset_restates_the_reference_rules(tmp_path):
    from oadg_amd.datasets import SdgodDataset, XMLDataset, build_dataset
    prefix = write_voc(str(tmp_path), TREE)
    ann = prefix + 'ImageSets/Main/train.txt'
    ds = build_dataset(dict(type='SdgodDataset', ann_file=ann, img_prefix=prefix), default_args=dict(device='cpu'))
    assert isinstance(ds, SdgodDataset) and ds.year == 2007
    # filter: 'd' has no known class, 'e' is under 32 px; the all-difficult 'c' stays (difficult objects count)
    assert [i['id'] for i in ds.data_infos] == ['a', 'b', 'c']
    assert [(i['filename'], i['height'], i['width']) for i in ds.data_infos] == \
        [('JPEGImages/a.jpg', 80, 100), ('JPEGImages/b.jpg', 40, 64), ('JPEGImages/c.jpg', 48, 64)]   # b: no <size>
    assert ds.flag.tolist() == [1, 1, 1]
    a = ds.get_ann_info(0)
    # int(float(text)) - 1; unknown 'dog' skipped; 'bus' with difficult 0 kept; classes index CLASSES
    np.testing.assert_array_equal(a['bboxes'], np.array([[9, 19, 49, 59], [39, 29, 89, 74], [59, 59, 65, 63]], np.float32))
    np.testing.assert_array_equal(a['labels'], np.array([2, 0, 5]))
    np.testing.assert_array_equal(a['bboxes_ignore'], np.array([[4, 4, 29, 29]], np.float32))
    np.testing.assert_array_equal(a['labels_ignore'], np.array([4]))
    assert a['bboxes'].dtype == np.float32 and a['labels'].dtype == np.int64
    assert a['bboxes_ignore'].dtype == np.float32 and a['labels_ignore'].dtype == np.int64
    c = ds.get_ann_info(2)
    assert c['bboxes'].shape == (0, 4) and c['bboxes'].dtype == np.float32
    assert c['labels'].shape == (0,) and c['labels'].dtype == np.int64
    np.testing.assert_array_equal(c['bboxes_ignore'], np.array([[0, 1, 19, 29], [19, 1, 59, 39]], np.float32))
    np.testing.assert_array_equal(c['labels_ignore'], np.array([1, 3]))
    # min_size: the 6 x 4 'rider' box goes to the ignored set
    m = SdgodDataset(ann_file=ann, img_prefix=prefix, min_size=5, device='cpu')
    am = m.get_ann_info(0)
    np.testing.assert_array_equal(am['labels'], np.array([2, 0]))
    np.testing.assert_array_equal(am['labels_ignore'], np.array([4, 5]))
    np.testing.assert_array_equal(am['bboxes_ignore'][1], np.array([59, 59, 65, 63], np.float32))
    # without filter_empty_gt only the size rule applies
    nf = SdgodDataset(ann_file=ann, img_prefix=prefix, filter_empty_gt=False, device='cpu')
    assert [i['id'] for i in nf.data_infos] == ['a', 'b', 'c', 'd']
    assert nf.get_ann_info(3)['bboxes'].shape == (0, 4)
    # XMLDataset with its own classes; img_subdir / ann_subdir
    x = XMLDataset(ann_file=ann, img_prefix=prefix, classes=('truck',), device='cpu')
    assert [i['id'] for i in x.data_infos] == ['b']
    np.testing.assert_array_equal(x.get_ann_info(0)['bboxes'], np.array([[1, 2, 39, 37]], np.float32))
    os.rename(prefix + 'Annotations', prefix + 'xml')
    y = SdgodDataset(ann_file=ann, img_prefix=prefix, ann_subdir='xml', device='cpu')
    assert len(y) == 3
    with pytest.raises(AssertionError):
        XMLDataset(ann_file=ann, img_prefix=prefix, ann_subdir='xml', device='cpu')       # no CLASSES


def test_sdgod_year_rule_and_cpu_batch(tmp_path):
    from PIL import Image
    from oadg_amd.datasets import SdgodDataset
    p12 = write_voc(str(tmp_path / 'x'), {'b': TREE['b']}, year='VOC2012')
    assert SdgodDataset(ann_file=p12 + 'ImageSets/Main/train.txt', img_prefix=p12, device='cpu').year == 2012
    p = write_voc(str(tmp_path / 'y'), {'b': TREE['b']}, year='VOC')
    with pytest.raises(ValueError, match='year'):
        SdgodDataset(ann_file=p + 'ImageSets/Main/train.txt', img_prefix=p, device='cpu')
    p07 = write_voc(str(tmp_path / 'z'), {'b': TREE['b'], 'c': (40, 64, True, TREE['c'][3])})
    ds = SdgodDataset(ann_file=p07 + 'ImageSets/Main/train.txt', img_prefix=p07, device='cpu')
    imgs, boxes, labels = ds.batch([0, 1])
    for k, n in enumerate(('b', 'c')):
        with Image.open(p07 + f'JPEGImages/{n}.jpg') as im:
            assert np.array_equal(imgs[k].numpy(), np.asarray(im.convert('RGB'))[:, :, ::-1])
    assert ds.jpeg_decodes == dict(native=0, pil=2)       # a CPU dataset keeps the PIL path


def test_sdgod_config_loads_and_falls_back_to_synthetic(capsys):
    from oadg_amd import Config
    from oadg_amd.datasets import build_dataset
    from oadg_amd.pipelines import SyntheticCityscapes
    cfg = Config.fromfile(SDGOD_CFG)
    tr = cfg.data.train
    assert tr.type == 'RepeatDataset' and tr.times == 2 and set(tr.keys()) == {'type', 'times', 'dataset'}
    assert tr.dataset.type == 'SdgodDataset'
    assert tr.dataset.ann_file.endswith('Daytime_Sunny/daytime_clear/VOC2007/ImageSets/Main/train.txt')
    assert tr.dataset.img_prefix.endswith('Daytime_Sunny/daytime_clear/VOC2007/')
    types = [t['type'] for t in tr.dataset.pipeline]
    assert types == ['LoadImageFromFile', 'LoadAnnotations', 'Resize', 'RandomFlip', 'OAMix', 'Normalize', 'Pad',
                     'DefaultFormatBundle', 'Collect']
    assert [tuple(s) for s in tr.dataset.pipeline[2]['img_scale']] == [(1280, 600), (1280, 720)]
    assert tr.dataset.pipeline[4]['version'] == 'augmix.all'
    assert cfg.model.roi_head.bbox_head.num_classes == 7
    ds = build_dataset(tr, default_args=dict(device='cpu', seed=0), synthetic_fallback=True)
    assert isinstance(ds, SyntheticCityscapes) and 'not found' in capsys.readouterr().out
    assert ds.num_classes == 7                # the synthetic labels stay within the 7-class head


def test_native_jpeg_switch_follows_the_environment():
    import subprocess
    code = 'import oadg_amd.datasets as d; print(d.NATIVE_JPEG)'
    for val, want in (('0', 'False'), ('1', 'True')):
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT, timeout=120,
                           env=dict(os.environ, OADG_NATIVE_JPEG=val, PYTHONPATH=ROOT))
        assert r.returncode == 0 and r.stdout.strip() == want, r.stderr[-1000:]


@pytest.mark.gpu
def test_native_batch_equals_the_pil_batch(dev, tmp_path, monkeypatch):
    from oadg_amd import datasets
    imgs = {f'{i:03d}': (72, 120, True, [_obj('car', (5, 5, 60, 50))]) for i in range(6)}
    prefix = write_voc(str(tmp_path), imgs)
    ds = datasets.SdgodDataset(ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix, device=dev)
    native, b1, l1 = ds.batch([0, 3, 5, 1])
    assert ds.jpeg_decodes == dict(native=4, pil=0)
    monkeypatch.setattr(datasets, 'NATIVE_JPEG', False)
    pil, b2, l2 = ds.batch([0, 3, 5, 1])
    assert ds.jpeg_decodes == dict(native=4, pil=4)
    torch.cuda.synchronize()
    assert native.device.type == 'cuda' and torch.equal(native, pil)
    assert all(np.array_equal(x, y) for x, y in zip(b1, b2)) and all(np.array_equal(x, y) for x, y in zip(l1, l2))


@pytest.mark.gpu
def test_jpeg_files_through_the_sdgod_pipeline_and_a_train_step(dev, tmp_path):
    """JPEG files + VOC XML -> SdgodDataset (native path) -> the S-DGOD config's train pipeline list (Resize, RandomFlip,
    OAMix 'augmix.all', Normalize, Pad) on the device -> one bf16 train step of the DWD OA-DG model with finite losses."""
    from oadg_amd import Config, build_detector, hip_conv
    from oadg_amd.apis import TrainEngine, build_optimizer
    from oadg_amd.datasets import build_dataset
    from oadg_amd.pipelines import DevicePipeline
    cfg = Config.fromfile(SDGOD_CFG)
    names = ('bus', 'bike', 'car', 'motor', 'person', 'rider', 'truck')
    imgs = {f'{i}': (256, 448, True, [_obj(names[(i + j) % 7], (20 + 40 * j, 30 + 20 * j, 120 + 40 * j, 140 + 20 * j))
                                      for j in range(5)]) for i in range(2)}
    prefix = write_voc(str(tmp_path), imgs)
    dcfg = dict(cfg.data.train.dataset, ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix)
    ds = build_dataset(dict(type='RepeatDataset', times=2, dataset=dcfg), default_args=dict(device=dev))
    pipeline = [dict(t) for t in dcfg['pipeline']]
    pipeline[2] = dict(type='Resize', img_scale=[(448, 224), (448, 256)], keep_ratio=True)
    pipe = DevicePipeline(pipeline, dtype=torch.bfloat16, one_scale_per_batch=True)
    np.random.seed(0)
    torch.manual_seed(0)
    data = pipe(*ds.batch([0, 3]))
    assert ds.dataset.jpeg_decodes['native'] == 2
    assert data['img'].shape[0] == 2 and data['img'].shape[2] % 32 == 0 and data['img2'].shape == data['img'].shape
    det = build_detector(cfg.model)
    det.init_weights(allow_missing_pretrained=True)
    det = det.to(dev).to(memory_format=torch.channels_last).train()
    hip_conv.enable()
    out = TrainEngine(det, build_optimizer(det, cfg.optimizer), amp_dtype=torch.bfloat16).step(data)
    assert np.isfinite(float(out['loss'])) and float(out['loss']) > 0


@pytest.mark.gpu
def test_train_cli_on_a_synthetic_voc_tree(dev, tmp_path):
    """tools/make_synthetic_voc.py -> tools/train.py on the S-DGOD config: a few iterations on JPEG files, no fallback"""
    import subprocess
    out = tmp_path / 'voc'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'make_synthetic_voc.py'), str(out), '--n', '6',
                        '--height', '256', '--width', '448', '--boxes', '6'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    voc = out / 'VOC2007'
    assert len(os.listdir(voc / 'JPEGImages')) == 6 and (voc / 'ImageSets' / 'Main' / 'train.txt').exists()
    cfg = tmp_path / 'tiny.py'
    cfg.write_text(
        f"_base_ = ['{SDGOD_CFG}']\n"
        "log_config = dict(interval=1, hooks=[dict(type='TextLoggerHook')])\n"
        "data = dict(samples_per_gpu=2, train=dict(times=1, dataset=dict(\n"
        f"    ann_file='{voc}/ImageSets/Main/train.txt', img_prefix='{voc}/')))\n")
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'train.py'), str(cfg), '--work-dir', str(tmp_path / 'w'),
                        '--seed', '0', '--max-iters', '3'], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'not found' not in r.stdout and 'SyntheticCityscapes' not in r.stdout
    lines = [l for l in r.stdout.splitlines() if l.startswith('Epoch [')]
    assert len(lines) == 3 and all('loss:' in l and 'nan' not in l for l in lines), r.stdout[-3000:]
