"""PhotoMetricDistortion / CutOut of the reference's train pipeline (mmdet/datasets/pipelines/transforms.py:941-1041 and
:1874-1944): the augmentation baselines OA-DG is compared against.

The two classes own the DRAWS - the reference's calls in the reference's order, through the random stream the other
transforms use (pipelines.oa_mix.rng) - and hand back small parameter records.  The pixels are ``DevicePipeline``'s: one
launch of csrc/photo.hip applies both steps, Normalize and Pad to the whole batch (oadg_photo.photo_normalize_batch), so no
float image is ever stored.
"""
import numpy as np

from .._lib import (PHOTO_ALPHA_POST, PHOTO_ALPHA_PRE, PHOTO_DELTA, PHOTO_HUE, PHOTO_PERM, PHOTO_PRESENT, PHOTO_SAT)
from ..registry import PIPELINES
from .oa_mix import rng


@PIPELINES.register_module()
class PhotoMetricDistortion:
    """transforms.py:941-1041.  Every sub-step is applied with probability 0.5; the contrast step comes before the HSV
    round trip in mode 1 and after it in mode 0 (the reference's CODE - its docstring says the opposite)."""

    def __init__(self, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18):
        self.brightness_delta = brightness_delta
        self.contrast_lower, self.contrast_upper = contrast_range
        self.saturation_lower, self.saturation_upper = saturation_range
        self.hue_delta = hue_delta

    def draw(self):
        """:987-1028, same draws in the same order -> dict(flags, mode, delta, alpha_pre, sat, hue, alpha_post, perm).
        ``flags``: PHOTO_PRESENT and one PHOTO_* bit per drawn sub-step; every scalar is rounded to float32 once (the
        reference applies a Python float in place to a float32 array); a sub-step that was not drawn keeps its neutral
        value.  ``perm``: output channel c is input channel perm[c]."""
        f32 = np.float32
        p = dict(flags=PHOTO_PRESENT, mode=0, delta=f32(0), alpha_pre=f32(1), sat=f32(1), hue=f32(0), alpha_post=f32(1),
                 perm=(0, 1, 2))

        def contrast(key, bit):
            if rng.randint(2):
                p[key] = f32(rng.uniform(self.contrast_lower, self.contrast_upper))
                p['flags'] |= bit
        if rng.randint(2):
            p['delta'] = f32(rng.uniform(-self.brightness_delta, self.brightness_delta))
            p['flags'] |= PHOTO_DELTA
        p['mode'] = int(rng.randint(2))
        if p['mode'] == 1:
            contrast('alpha_pre', PHOTO_ALPHA_PRE)
        if rng.randint(2):
            p['sat'] = f32(rng.uniform(self.saturation_lower, self.saturation_upper))
            p['flags'] |= PHOTO_SAT
        if rng.randint(2):
            p['hue'] = f32(rng.uniform(-self.hue_delta, self.hue_delta))
            p['flags'] |= PHOTO_HUE
        if p['mode'] == 0:
            contrast('alpha_post', PHOTO_ALPHA_POST)
        if rng.randint(2):
            p['perm'] = tuple(int(v) for v in rng.permutation(3))
            p['flags'] |= PHOTO_PERM
        return p


@PIPELINES.register_module()
class CutOut:
    """transforms.py:1874-1944."""

    def __init__(self, n_holes, cutout_shape=None, cutout_ratio=None, fill_in=(0, 0, 0)):
        assert (cutout_shape is None) ^ (cutout_ratio is None), 'Either cutout_shape or cutout_ratio should be specified.'
        assert isinstance(cutout_shape, (list, tuple)) or isinstance(cutout_ratio, (list, tuple))
        if isinstance(n_holes, tuple):
            assert len(n_holes) == 2 and 0 <= n_holes[0] < n_holes[1]
        else:
            n_holes = (n_holes, n_holes)
        fill = np.broadcast_to(np.asarray(fill_in, dtype=np.float64), (3,))
        if not (np.isfinite(fill).all() and (fill >= 0).all() and (fill <= 255).all()):
            raise ValueError(f'CutOut: fill_in must lie in [0, 255] (got {fill_in})')
        self.n_holes, self.fill_in = n_holes, fill_in
        self.with_ratio = cutout_ratio is not None
        self.candidates = cutout_ratio if self.with_ratio else cutout_shape
        if not isinstance(self.candidates, list):
            self.candidates = [self.candidates]

    def draw(self, h, w):
        """:1921-1933 for an h x w image, same draws in the same order -> int32 [n, 4] = x1, y1, x2, y2 (exclusive).
        A hole that would leave the image is clipped; an empty one (x2 == x1 or y2 == y1) is legal."""
        n = int(rng.randint(self.n_holes[0], self.n_holes[1] + 1))
        rects = np.zeros((n, 4), np.int32)
        for i in range(n):
            x1 = int(rng.randint(0, w))
            y1 = int(rng.randint(0, h))
            index = int(rng.randint(0, len(self.candidates)))
            if not self.with_ratio:
                cutout_w, cutout_h = self.candidates[index]
            else:
                cutout_w = int(self.candidates[index][0] * w)
                cutout_h = int(self.candidates[index][1] * h)
            rects[i] = x1, y1, int(np.clip(x1 + cutout_w, 0, w)), int(np.clip(y1 + cutout_h, 0, h))
        return rects

    def fill(self, on_uint8):
        """the three values a hole pixel takes, float32.  ``on_uint8``: the step precedes any photometric step, so the
        reference assigns into a uint8 image and numpy truncates the fill to an integer; behind a photometric step the
        image is float32 and takes the fill as it is."""
        fill = np.broadcast_to(np.asarray(self.fill_in, dtype=np.float64), (3,))
        return (fill.astype(np.uint8) if on_uint8 else fill).astype(np.float32)
