"""GPU: csrc/draw.hip through ``oadg_draw.draw_items`` - every case of tests/draw_cases.py byte for byte against Pillow
(``draw_expect``), the WHOLE batch compared, so a stray write anywhere fails.  Images are random bytes: painting nothing
is not painting black.  The answering suite for the ``oadg_draw_items_u8`` / ``oadg_draw_tile_capacity`` call sites."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_cases as C  # noqa: E402

GROUPS = {'size': C.size_cases, 'box': C.box_cases, 'text': C.text_cases, 'batch': C.batch_cases, 'extreme': C.extreme_cases,
          'fuzz': lambda: [C.fuzz_case(0)]}


@functools.lru_cache(None)
def _expected(group, capacity):
    """[(case, images, expected)]: the oracle runs once per group"""
    if group == 'order':
        cases = C.order_cases(capacity)
    elif group == 'fuzz_capacity':
        cases = [C.fuzz_case(1, count=2 * capacity + 37)]
    else:
        cases = GROUPS[group]()
    return [(case,) + C.expected(case) for case in cases]


def _draw(dev, case, imgs):
    import torch
    import oadg_draw
    items, off, text = C.batch_arrays(case.lists)
    t = torch.from_numpy(imgs).to(dev)
    out = oadg_draw.draw_items(t, items, off, text)
    assert out is t                                                         # in place
    return t.cpu().numpy()


def _check(dev, group, capacity=0):
    failed = []
    for case, imgs, want in _expected(group, capacity):
        got = _draw(dev, case, imgs)
        if not np.array_equal(got, want):
            bad = np.argwhere((got != want).any(-1))
            failed.append((case.name, len(bad), bad[:4].tolist()))
    assert not failed, failed


@pytest.mark.gpu
@pytest.mark.parametrize('group', sorted(GROUPS))
def test_draw_matches_pillow(dev, group):
    _check(dev, group)


@pytest.mark.gpu
def test_painters_order_and_the_tile_list_capacity(dev):
    """three overlapping rows in both orders; capacity, capacity + 1 and 2 * capacity + 1 rows that all cover one tile (the
    last one wins); two tiles taking turns in 3 * capacity + 1 rows; 2 * capacity + 37 random rows"""
    import oadg_draw
    capacity = oadg_draw.tile_capacity()
    assert capacity >= 64
    names = [c.name for c, _, _ in _expected('order', capacity)]
    assert f'capacity_{2 * capacity + 1}_rows_on_one_tile' in names and 'order_reversed' in names
    _check(dev, 'order', capacity)
    _check(dev, 'fuzz_capacity', capacity)


@pytest.mark.gpu
def test_an_image_without_rows_is_left_alone_and_rows_stay_with_their_image(dev):
    (case, imgs, want), = [e for e in _expected('batch', 0) if e[0].name == 'batch_counts_0_k_1']
    got = _draw(dev, case, imgs)
    assert np.array_equal(got[0], imgs[0]) and not np.array_equal(got[1], imgs[1]) and not np.array_equal(got[2], imgs[2])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_draws_into_a_slice_of_a_larger_allocation(dev):
    """the batch is a contiguous slice in the middle of a buffer: the bytes before and behind it do not change"""
    import torch
    import oadg_draw
    case = C.Case('slice', 21, 67, [C.generic(21, 67), C.DL().fill(-5, -5, 100, 100, C.ODD)])
    imgs, want = C.expected(case)
    rs = np.random.RandomState(5)
    whole = rs.randint(0, 256, (4, 21, 67, 3), dtype=np.uint8)
    whole[1:3] = imgs
    t = torch.from_numpy(whole).to(dev)
    items, off, text = C.batch_arrays(case.lists)
    oadg_draw.draw_items(t[1:3], items, off, text)
    got = t.cpu().numpy()
    assert np.array_equal(got[1:3], want) and np.array_equal(got[0], whole[0]) and np.array_equal(got[3], whole[3])


@pytest.mark.gpu
def test_refusals_launch_nothing(dev):
    import torch
    import oadg_draw
    items, off, text = C.batch_arrays([C.overlap_list(), C.DL()])
    imgs = C.random_images('refusals', 2, 20, 70)
    t = torch.from_numpy(imgs).to(dev)
    wide = torch.from_numpy(C.random_images('refusals wide', 2, 20, 140)).to(dev)
    bad_off = off.copy()
    bad_off[1] = len(items) + 1
    past = items.copy()
    past[2, 4] = len(text) + 1                                              # the TEXT row runs past the buffer
    refused = [
        ('imgs', (torch.from_numpy(imgs), items, off, text)),               # a CPU tensor
        ('imgs', (wide[:, :, ::2], items, off, text)),                      # not contiguous
        ('imgs', (t.to(torch.int8), items, off, text)), ('imgs', (t.float(), items, off, text)),
        ('imgs', (t[0], items, off, text)),
        ('items', (t, items.astype(np.int64), off, text)), ('items', (t, torch.from_numpy(items).to(dev), off, text)),
        ('item_off', (t, items, bad_off, text)), ('item_off', (t, items, off[:2], text)),
        ('item_off', (t, items, off[::-1].copy(), text)),
        ('text', (t, past, off, text)), ('text', (t, items, off, text[:3])),
    ]
    for name, args in refused:
        with pytest.raises(ValueError, match=name):
            oadg_draw.draw_items(*args)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), imgs)                            # nothing was painted on the way
