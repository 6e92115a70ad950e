"""GPU: Corrupt.batch of a resident batch through csrc/corrupt.hip equals corrupt() on the host image by image, byte
for byte, and leaves numpy's global stream where the host loop leaves it (pipelines/corrupt_device.py)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from inputs import lowpass_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('gaussian_blur', 'glass_blur', 'defocus_blur', 'motion_blur', 'zoom_blur', 'snow', 'brightness', 'saturate',
         'elastic_transform')

pytestmark = pytest.mark.gpu


def _compare(imgs, name, severity, seed=0):
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt, corrupt
    np.random.seed(seed)
    ref = np.stack([corrupt(im, name, severity) for im in imgs])
    state = np.random.get_state()
    before = Corrupt.runs['device']
    np.random.seed(seed)
    out = Corrupt(name, severity).batch(torch.from_numpy(imgs).cuda()).cpu().numpy()
    after = np.random.get_state()
    assert Corrupt.runs['device'] == before + len(imgs)
    bad = np.argwhere(out != ref)
    assert bad.size == 0, (name, severity, imgs.shape, len(bad), bad[:5].tolist(),
                           [(int(out[tuple(b)]), int(ref[tuple(b)])) for b in bad[:5]])
    assert after[2:] == state[2:] and np.array_equal(after[1], state[1]), 'numpy stream differs after the batch'


def _pair(h, w, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, 256, (h, w, 3)).astype(np.uint8), np.full((h, w, 3), 128, np.uint8)])


@pytest.mark.parametrize('severity', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('name', NAMES)
def test_severity_sweep_random_and_grey(name, severity):
    _compare(_pair(61, 97, severity), name, severity)


@pytest.mark.parametrize('severity', [1, 3, 5])
@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('h,w', [(9, 13), (33, 47), (5, 3)])
def test_small_and_odd_sides(name, severity, h, w):
    """9 x 13: the motion blur breaks early; odd sides: the zoom crops round; 5 x 3: kernels wider than the image"""
    rs = np.random.RandomState(h * w + severity)
    _compare(rs.randint(0, 256, (2, h, w, 3)).astype(np.uint8), name, severity)


@pytest.mark.parametrize('name', NAMES)
def test_batch_of_three_in_order(name):
    rs = np.random.RandomState(11)
    imgs = np.stack([lowpass_image(rs, 40, 56, 4), rs.randint(0, 256, (40, 56, 3)).astype(np.uint8),
                     np.full((40, 56, 3), 7, np.uint8)])
    _compare(imgs, name, 3, seed=123)


@pytest.mark.parametrize('name,severity', [(n, 3) for n in NAMES] + [('zoom_blur', 5), ('defocus_blur', 5)])
def test_full_size(name, severity):
    rs = np.random.RandomState(7)
    img = lowpass_image(rs, 1024, 2048, 6)
    img[::37] = rs.randint(0, 256, img[::37].shape)                 # some sharp rows as well
    _compare(img[None], name, severity, seed=1)


def test_routing_counter_and_escape_hatch(monkeypatch):
    import torch
    from oadg_amd.pipelines.corrupt import Corrupt
    x = torch.from_numpy(_pair(17, 23, 0)).cuda()
    d0, h0 = Corrupt.runs['device'], Corrupt.runs['host']
    a = Corrupt('zoom_blur', 2).batch(x)
    assert (Corrupt.runs['device'], Corrupt.runs['host']) == (d0 + 2, h0)
    Corrupt('contrast', 2).batch(x)                                 # a host-only name
    assert (Corrupt.runs['device'], Corrupt.runs['host']) == (d0 + 2, h0 + 2)
    monkeypatch.setenv('OADG_DEVICE_CORRUPT', '0')
    b = Corrupt('zoom_blur', 2).batch(x)
    assert (Corrupt.runs['device'], Corrupt.runs['host']) == (d0 + 2, h0 + 4)
    assert a.is_cuda and b.is_cuda and torch.equal(a, b)


def test_robustness_cli_identical_with_and_without_the_device_path(tmp_path):
    cfg = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r50_fpn_1x_cityscapes_oadg.py')
    res = []
    for flag in ('1', '0'):
        out = tmp_path / f'rob{flag}.pkl'
        env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1', OADG_DEVICE_CORRUPT=flag)
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'analysis_tools', 'test_robustness.py'), cfg,
                            'none', '--load-dataset', 'original', '--corruptions', 'zoom_blur', 'defocus_blur',
                            '--severities', '0', '3', '--max-samples', '2', '--seed', '0', '--out', str(out)],
                           capture_output=True, text=True, env=env, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        res.append(open(tmp_path / f'rob{flag}_results.pkl', 'rb').read())
    assert set(pickle.loads(res[0])) == {'zoom_blur', 'defocus_blur'}
    assert res[0] == res[1]
