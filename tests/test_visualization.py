"""CPU: the host side of drawing detections - the glyph table against the installed Pillow, ``visualization.det_items`` by
hand, what is refused by name, the wrapper's argument checks that need no GPU, and the oracle of tests/draw_cases.py
itself (it must be able to tell a wrong painter's order and an outline that grows outward)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import draw_cases as C  # noqa: E402


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))                         # (the tools import each other by file name)
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.path.pop(0)
    return mod


def _vis():
    from oadg_amd import visualization
    return visualization


# ------------------------------------------------------------------------------------------------------ glyph table
def test_committed_font_header_is_what_the_generator_makes_of_the_installed_pillow():
    gen = _load(('tools', 'make_font6x11.py'), 'oadg_make_font')
    assert open(gen.HEADER).read() == gen.header_text()
    rows = gen.glyph_rows()
    assert len(rows) == 95 and all(len(r) == 11 and all(0 <= b < 64 for b in r) for r in rows)
    for code in (33, 65, 103, 124, 126):                                    # bit 5 is the leftmost column
        mask = C.glyph_mask(code, 1)
        assert [[(b >> (5 - c)) & 1 for c in range(6)] for b in rows[code - 32]] == mask.astype(int).tolist()
    assert rows[0] == [0] * 11                                              # the space


def test_case_constants_are_the_headers():
    from oadg_amd import _lib
    assert (C.OUTLINE, C.FILL, C.TEXT, C.ITEM_INTS) == (_lib.DRAW_OUTLINE, _lib.DRAW_FILL, _lib.DRAW_TEXT, _lib.DRAW_ITEM_INTS)


# ------------------------------------------------------------------------------------------------------- det_items
NAMES = ('person', 'rider', 'car')


def _rows(items):
    return [tuple(r) for r in items.tolist()]


def test_det_items_by_hand():
    V = _vis()
    result = [np.array([[10.9, 20.2, 50.7, 60.99, 0.984], [0, 0, 5, 5, 0.3]], np.float32),        # person: 0.3 is NOT > 0.3
              np.zeros((0, 5), np.float32),
              np.array([[-3.7, -0.5, 8.2, 9.9, 0.31], [30, 30, 29.5, 40, 0.9], [5, 9, 7, 8.5, 0.9]], np.float32)]
    items, text = V.det_items(result, NAMES, score_thr=0.3, bbox_color=(1, 2, 3), text_color=(4, 5, 6), thickness=2, font_size=13)
    assert items.dtype == np.int32 and items.shape == (6, 8)
    colour, ink = 1 | 2 << 8 | 3 << 16, 4 | 5 << 8 | 6 << 16
    # person|0.98: corners truncated; the plate is 6 * 11 + 1 wide and 11 + 1 high from the corner; the text one pixel in
    assert text == b'person|0.98car|0.31'
    assert _rows(items) == [
        (C.OUTLINE, 10, 20, 50, 60, 2, colour, 0), (C.FILL, 10, 20, 10 + 66 + 1, 20 + 12, 0, 0, 0), (C.TEXT, 11, 21, 0, 11, 1, ink, 0),
        # negative and fractional corners truncate toward zero (astype(np.int32)); rows with x1 < x0 or y1 < y0 are dropped
        (C.OUTLINE, -3, 0, 8, 9, 2, colour, 0), (C.FILL, -3, 0, -3 + 48 + 1, 12, 0, 0, 0), (C.TEXT, -2, 1, 11, 8, 1, ink, 0)]


def test_det_items_threshold_rules():
    V = _vis()
    result = [np.array([[0, 0, 4, 4, 0.5], [0, 0, 4, 4, 0.0], [1, 1, 3, 3, -1.0]], np.float32)]
    assert len(V.det_items(result, NAMES, score_thr=0.5)[0]) == 0                    # strict >
    assert len(V.det_items(result, NAMES, score_thr=0.49)[0]) == 3
    assert len(V.det_items(result, NAMES, score_thr=0)[0]) == 9                      # score_thr == 0: no filter at all
    assert V.det_items(result, NAMES, score_thr=0)[1] == b'person|0.50person|0.00person|-1.00'
    assert V.det_items([], NAMES)[0].shape == (0, 8) and V.det_items([np.zeros((0, 5))], None)[1] == b''


def test_det_items_label_text_and_scale():
    V = _vis()
    one = [np.array([[2, 3, 40, 50, 0.975]], np.float32)]
    items, text = V.det_items(one, ('café ☃',), score_thr=0, font_size=22)          # s = round(22 / 11) = 2
    assert text == b'caf? ?|0.98'                                           # (float32 0.975 is 0.97500002...)
    n = len(text)
    assert _rows(items)[1] == (C.FILL, 2, 3, 2 + 6 * 2 * n + 1, 3 + 11 * 2 + 1, 0, 0, 0)
    assert _rows(items)[2][:6] == (C.TEXT, 3, 4, 0, n, 2)
    assert [V.font_scale(f) for f in (1, 11, 13, 16, 17, 22, 33)] == [1, 1, 1, 1, 2, 2, 3]
    assert V.det_items(one, None, score_thr=0)[1] == b'class 0|0.98'
    assert V.det_items([np.zeros((0, 5)), one[0]], ('only',), score_thr=0)[1].startswith(b'class 1|')   # no name for the index


def test_palette_is_fixed():
    V = _vis()
    assert V.palette_color(0) == (60, 20, 220) and V.palette_color(2) == (142, 0, 0) and V.palette_color(7) == (32, 11, 119)
    many = [V.color_val('palette', i) for i in range(8, 264)]
    assert len(set(many)) == 256 and (0, 0, 0) not in many and many == [V.color_val('palette', i) for i in range(8, 264)]
    assert all(isinstance(c, int) and 0 <= c <= 255 for col in many for c in col)
    res = [np.array([[0, 0, 9, 9, 0.9]], np.float32), np.array([[0, 0, 9, 9, 0.9]], np.float32)]
    items, _ = V.det_items(res, NAMES, bbox_color='palette', text_color='green')
    assert items[0, 6] == 60 | 20 << 8 | 220 << 16 and items[3, 6] == 0 | 0 << 8 | 255 << 16 and items[2, 6] == 255 << 8
    with pytest.raises(ValueError, match='chartreuse'):
        V.color_val('chartreuse')


def test_gt_items():
    V = _vis()
    items, text = V.gt_items(np.array([[1.5, 2.5, 30, 40], [9, 9, 8, 12]], np.float32), [2, 0], NAMES, color=(0, 255, 0), thickness=1)
    assert text == b'car'
    assert _rows(items) == [(C.OUTLINE, 1, 2, 30, 40, 1, 255 << 8, 0), (C.FILL, 1, 2, 1 + 18 + 1, 2 + 12, 0, 0, 0),
                            (C.TEXT, 2, 3, 0, 3, 1, 255 << 8, 0)]


def test_join_lists_moves_text_offsets():
    V = _vis()
    a = V.det_items([np.array([[0, 0, 9, 9, 0.9]], np.float32)], NAMES)
    b = V.det_items([np.zeros((0, 5), np.float32)], NAMES)
    c = V.det_items([np.zeros((0, 5), np.float32), np.array([[1, 1, 9, 9, 0.8]], np.float32)], NAMES)
    items, off, text = V.join_lists([a, b, c])
    assert off.tolist() == [0, 3, 3, 6] and off.dtype == np.int32 and bytes(text) == b'person|0.90rider|0.80'
    assert items[2, 3] == 0 and items[5, 3] == 11 and items.flags.c_contiguous
    assert a[0][2, 3] == 0 and c[0][2, 3] == 0                                        # the inputs are left alone


def test_picture_names():
    V = _vis()

    class Files:
        data_infos = [dict(filename='JPEGImages/000012.jpg'), dict(filename='frankfurt/f_000000_000294_leftImg8bit.png'),
                      dict(filename='a.b/c.d.jpeg')]
    assert [V.picture_name(Files, i) for i in range(3)] == ['JPEGImages/000012.png', 'frankfurt/f_000000_000294_leftImg8bit.png',
                                                            'a.b/c.d.png']
    assert V.picture_name(object(), 7) == '000007.png'

    class Absolute:                                                          # no img_prefix: the names are whole paths
        data_infos = [dict(filename='/data/city/a.png'), dict(filename='//x/b.jpg'), dict(filename='../../up/c.png'),
                      dict(filename='d/../../e.png')]
    names = [V.picture_name(Absolute, i) for i in range(4)]
    assert names == ['data/city/a.png', 'x/b.png', 'up/c.png', 'e.png']
    for n in names:                                                          # always below the show directory
        assert os.path.normpath(os.path.join('/pics', n)).startswith('/pics/')
    from oadg_amd.datasets import ConcatDataset, RepeatDataset

    class Two(Files):
        data_infos = Files.data_infos[:2]

        def __len__(self):
            return 2
    both = ConcatDataset([Two(), Two()])                                     # a list-valued ann_file: the DWD test splits
    assert [V.picture_name(both, i) for i in (1, 2)] == ['frankfurt/f_000000_000294_leftImg8bit.png', 'JPEGImages/000012.png']
    assert V.picture_name(RepeatDataset(Two(), 3), 5) == 'frankfurt/f_000000_000294_leftImg8bit.png'


# ------------------------------------------------------------------------------------------------ refused by name
def test_show_and_mask_color_are_reported_by_name():
    from oadg_amd.detectors import BaseDetector
    det = BaseDetector()
    img = np.zeros((4, 4, 3), np.uint8)
    with pytest.raises(NotImplementedError, match='show=True'):
        det.show_result(img, [np.zeros((0, 5))], show=True)
    with pytest.raises(NotImplementedError, match='mask_color'):
        det.show_result(img, [np.zeros((0, 5))], mask_color=(1, 2, 3))


@pytest.mark.parametrize('tool', [('tools', 'test.py')])
def test_command_lines_take_show_dir_and_report_show(tool, monkeypatch):
    mod = _load(tool, 'oadg_tool_' + tool[-1][:-3])
    monkeypatch.setenv('LOCAL_RANK', '0')
    monkeypatch.setattr(sys, 'argv', [tool[-1], 'cfg.py', 'none', '--show-dir', '/pics', '--show-score-thr', '0.15', '--eval', 'bbox'])
    a = mod.parse_args()
    assert a.show_dir == '/pics' and a.show_score_thr == 0.15 and a.show is False
    monkeypatch.setattr(sys, 'argv', [tool[-1], 'cfg.py', 'none', '--eval', 'bbox'])
    a = mod.parse_args()
    assert a.show_dir is None and a.show_score_thr == 0.3
    monkeypatch.setattr(sys, 'argv', [tool[-1], 'cfg.py', 'none', '--show', '--eval', 'bbox'])
    with pytest.raises(NotImplementedError, match='--show '):
        mod.parse_args()


# ------------------------------------------------------------------------------- wrapper arguments, without a GPU
def _good():
    items, off, text = C.batch_arrays([C.overlap_list(), C.DL()])
    return items, off, text


def test_wrapper_refuses_a_cpu_tensor():
    import torch
    import oadg_draw
    items, off, text = _good()
    with pytest.raises(ValueError, match='imgs'):
        oadg_draw.draw_items(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), items, off, text)
    with pytest.raises(ValueError, match='imgs'):
        oadg_draw.draw_items(np.zeros((2, 8, 8, 3), np.uint8), items, off, text)


def test_display_list_checks():
    import oadg_draw
    items, off, text = _good()
    got = oadg_draw.check_display_list(2, items, off, text)
    assert got[0] is items and got[1] is off and bytes(got[2]) == bytes(text)
    assert bytes(oadg_draw.check_display_list(2, items, off, bytes(text))[2]) == bytes(text)
    bad = [
        ('items', (items.astype(np.int64), off, text)), ('items', (items[:, :7], off, text)), ('items', (items[::2], off, text)),
        ('items', (items.reshape(-1), off, text)),
        ('item_off', (items, off.astype(np.int64), text)), ('item_off', (items, off[:-1], text)),
        ('item_off', (items, np.array([1, 4, 4], np.int32), text)), ('item_off', (items, np.array([0, 4, 3], np.int32), text)),
        ('item_off', (items, np.array([0, 5, 4], np.int32), text)), ('item_off', (items, np.array([0, 2, 5], np.int32), text)),
        ('text', (items, off, text[:-1])), ('text', (items, off, text.astype(np.int8))), ('text', (items, off, 'car|0.98')),
    ]
    for name, args in bad:
        with pytest.raises(ValueError, match=name):
            oadg_draw.check_display_list(2, *args)
    for column, value in ((3, -1), (4, -1), (3, 2 ** 31 - 1), (4, len(text) + 1)):
        doctored = items.copy()
        doctored[2, column] = value                                       # row 2 of the overlap list is its TEXT row
        assert doctored[2, 0] == C.TEXT
        with pytest.raises(ValueError, match='text'):
            oadg_draw.check_display_list(2, doctored, off, text)
    for scale in (0, -1, -2 ** 31):                                       # legal rows that paint nothing (the header's rule)
        doctored = items.copy()
        doctored[2, 5] = scale
        oadg_draw.check_display_list(2, doctored, off, text)


def test_tool_keeps_the_encoder_under_its_name():
    import oadg_draw
    tool = _load(('tools', 'analysis_tools', 'get_corrupted_dataset.py'), 'oadg_tool_gcd')
    assert tool.PngEncoder is oadg_draw.PngEncoder and tool.write_png is oadg_draw.write_png
    assert tool.BATCH == 8 and tool.PINNED_SLOTS == 3


def test_nothing_in_the_package_calls_the_draw_entries_directly():
    import re
    for d, _, files in os.walk(os.path.join(ROOT, 'oa-dg_amd')):
        for f in files:
            if f.endswith('.py'):
                assert not re.search(r'\.oadg_(draw|png_encode|png_write)', open(os.path.join(d, f)).read()), f


# ---------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_tells_a_wrong_order_and_an_outline_grown_outward():
    case = next(c for c in C.order_cases(256) if c.name == 'order_forward')
    dl = case.lists[0]
    img = C.random_images(case.name, 1, case.H, case.W)[0]
    right = C.draw_expect(img, dl.items(), dl.text)
    assert not np.array_equal(right, img)
    assert not np.array_equal(right, C.draw_expect(img, dl.reversed().items(), dl.text))
    grown = C.grown_outward(dl)
    assert not np.array_equal(right, C.draw_expect(img, grown.items(), grown.text))
    assert np.array_equal(right, C.draw_expect(img, dl.items(), dl.text, masks=True))


def test_oracle_paints_unscaled_characters_the_same_both_ways_and_every_case_builds():
    cases = C.all_cases(256)
    assert len({c.name for c in cases}) == len(cases) > 100
    for case in cases:
        imgs, want = C.expected(case)
        assert want.shape == imgs.shape and want.dtype == np.uint8
        if case.name.startswith('text_') and case.expect_lists is None:
            again = np.stack([C.draw_expect(imgs[i], dl.items(), dl.text, masks=True) for i, dl in enumerate(case.lists)])
            assert np.array_equal(want, again), case.name
        if case.name.startswith(('size_', 'order_', 'capacity_', 'fuzz_', 'text_all', 'text_scale', 'text_over')):
            assert not np.array_equal(want, imgs), case.name             # the case paints something
    nothing = [c for c in cases if c.name in ('box_inverted_x_fill', 'box_outside_left_outline_w2', 'text_clip_outside_top',
                                              'text_empty_run', 'box_width_side12_w0', 'batch_no_rows_at_all')]
    assert len(nothing) == 6
    for case in nothing:
        imgs, want = C.expected(case)
        if case.name == 'text_empty_run':
            want[:, 0:2, 0:2] = imgs[:, 0:2, 0:2]                          # (its fill)
        assert np.array_equal(want, imgs), case.name


def test_extreme_cases_state_lists_the_oracle_can_draw():
    for case in C.extreme_cases():
        assert case.expect_lists is not None
        for dl in case.expect_lists:
            assert np.abs(dl.items()[:, 1:6]).max(initial=0) <= C.LIMIT
        assert any(np.abs(dl.items()[:, 1:6].astype(np.int64)).max(initial=0) > C.LIMIT for dl in case.lists)
