"""The pixel oracle and the case lists of csrc/draw.hip (tests/test_hip_draw.py on the GPU, tests/test_visualization.py and
tests/test_show_dir.py use them too).

``draw_expect`` applies a display list row by row with Pillow: ``ImageDraw.rectangle(outline=, width=)``,
``rectangle(fill=)`` and the built-in 6 x 11 bitmap font (``ImageFont.load_default_imagefont()``).  Pillow raises for
x1 < x0 (the kernel paints nothing), so such rows are skipped; a run is drawn character by character, each alone in its
cell (Pillow's glyphs of the bytes below 32 and of 127 have no width: the kernel keeps the cell and paints nothing), and a
scaled character is its glyph mask under ``np.kron``.  Pillow walks every row of an outline, so ``draw_expect`` refuses
coordinates beyond +-2^20; the int32 extremes are cases of their own, each with an equivalent list of modest rows that is
worked out from the painting rule in its comment.

A case is ``Case(name, H, W, lists, expect_lists)``: one DisplayList per image; ``expect_lists`` (default: the same) is
what the oracle draws.  Images are random uint8 seeded by the case name, so "painted nothing" differs from "painted
black".  The shapes are the smallest that reach every path of the kernel: its tile is 64 x 16 pixels, a thread owns 4
adjacent pixels, a workgroup lists at most ``capacity`` rows before it paints.
"""
import zlib
from collections import namedtuple

import numpy as np

OUTLINE, FILL, TEXT = 0, 1, 2
ITEM_INTS = 8
TILE_W, TILE_H, GROUP = 64, 16, 4
LIMIT = 1 << 20
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
RED, GREEN, BLUE, WHITE, BLACK, ODD = (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255), (0, 0, 0), (1, 128, 254)


def pack(colour):
    return int(colour[0]) | int(colour[1]) << 8 | int(colour[2]) << 16


class DisplayList:
    """rows of one image and the bytes its TEXT rows point into"""

    def __init__(self):
        self.rows, self.text = [], bytearray()

    def outline(self, x0, y0, x1, y1, w, colour):
        self.rows.append([OUTLINE, x0, y0, x1, y1, w, pack(colour), 0])
        return self

    def fill(self, x0, y0, x1, y1, colour):
        self.rows.append([FILL, x0, y0, x1, y1, 0, pack(colour), 0])
        return self

    def write(self, x, y, scale, colour, run):
        run = run.encode('latin-1') if isinstance(run, str) else bytes(run)
        self.rows.append([TEXT, x, y, len(self.text), len(run), scale, pack(colour), 0])
        self.text += run
        return self

    def raw(self, row):
        self.rows.append(list(row))
        return self

    def reversed(self):
        out = DisplayList()
        out.rows, out.text = self.rows[::-1], bytearray(self.text)
        return out

    def items(self):
        return np.asarray(self.rows, dtype=np.int64).astype(np.int32).reshape(-1, ITEM_INTS)


def batch_arrays(lists):
    """[DisplayList per image] -> items int32 [k, 8] (text offsets moved into the joint buffer), item_off int32 [n + 1],
    text uint8"""
    rows, off, text = [], [0], bytearray()
    for dl in lists:
        it = dl.items().copy()
        it[it[:, 0] == TEXT, 3] += len(text)
        rows.append(it)
        text += dl.text
        off.append(off[-1] + len(it))
    return (np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, ITEM_INTS), np.int32)),
            np.asarray(off, dtype=np.int32), np.frombuffer(bytes(text), dtype=np.uint8))


# ------------------------------------------------------------------------------------------------------------ oracle
def _font():
    from PIL import ImageFont
    return ImageFont.load_default_imagefont()


def glyph_mask(code, scale):
    """bool [11 s, 6 s] of one printable character, from Pillow's font"""
    m = np.asarray(_font().getmask(chr(code)), dtype=np.uint8).reshape(11, 6) != 0
    return np.kron(m, np.ones((scale, scale), dtype=bool))


def _paint_mask(out, x, y, mask, colour):
    H, W = out.shape[:2]
    h, w = mask.shape
    xa, ya, xb, yb = max(x, 0), max(y, 0), min(x + w, W), min(y + h, H)
    if xa < xb and ya < yb:
        out[ya:yb, xa:xb][mask[ya - y:yb - y, xa - x:xb - x]] = colour


def draw_expect(img, items, text, masks=False):
    """uint8 [H, W, 3], int32 [k, 8] rows, the text bytes -> the painted copy, row after row with Pillow.
    ``masks=True``: also unscaled characters are painted from their glyph mask (the two ways must agree)"""
    from PIL import Image, ImageDraw
    text = bytes(bytearray(text))
    out = np.array(img, dtype=np.uint8, copy=True)
    for kind, a, b, c, d, e, colour, _ in np.asarray(items).reshape(-1, ITEM_INTS).tolist():
        col = (colour & 255, (colour >> 8) & 255, (colour >> 16) & 255)
        assert max(abs(a), abs(b)) <= LIMIT, 'draw_expect: coordinates beyond 2^20 are the extreme cases'
        if kind in (OUTLINE, FILL):
            assert max(abs(c), abs(d)) <= LIMIT and e <= 4096
            if c < a or d < b:
                continue
            pil = Image.fromarray(out)
            if kind == FILL or e >= d - b + 1 or e > c - a + 1:
                # (an outline at least as wide as the box is high, or wider than the box: every pixel of the box is within
                #  w of an edge, a fill by the rule.  Pillow's own outline leaves the rectangle there - its vertical strokes
                #  run from y0 + w to y1 - w + 1 in whichever direction, its horizontal ones to y0 + w - 1)
                ImageDraw.Draw(pil).rectangle([a, b, c, d], fill=col)
            else:
                ImageDraw.Draw(pil).rectangle([a, b, c, d], outline=col, width=e)
            out = np.array(pil)
        elif kind == TEXT:
            run = text[c:c + d]
            assert 0 <= c and c + d <= len(text) and e <= 64
            if e < 1:                                                     # a scale below 1 paints nothing
                continue
            # character by character, each in its own 6 s x 11 s cell: Pillow draws a character alone exactly as its
            # 6 x 11 mask (a RUN is not the concatenation of those - 45 pixels of 29 glyphs sit one column left of their
            # cell and replace the last column of the character before; the kernel keeps to the cells)
            for k, ch in enumerate(run):
                if not 32 <= ch <= 126:
                    continue
                if e == 1 and not masks:
                    pil = Image.fromarray(out)
                    ImageDraw.Draw(pil).text((a + 6 * k, b), chr(ch), font=_font(), fill=col)
                    out = np.array(pil)
                else:
                    _paint_mask(out, a + 6 * e * k, b, glyph_mask(ch, e), col)
    return out


def random_images(name, n, H, W):
    rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    return rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)


def expected(case):
    imgs = random_images(case.name, len(case.lists), case.H, case.W)
    want = np.stack([draw_expect(imgs[i], dl.items(), dl.text) for i, dl in enumerate(case.expect_lists or case.lists)]) \
        if len(imgs) else imgs.copy()
    return imgs, want


# ------------------------------------------------------------------------------------------------------------- cases
Case = namedtuple('Case', 'name H W lists expect_lists', defaults=(None,))


def DL():
    return DisplayList()


def generic(H, W):
    """something of every kind over every border of an H x W image"""
    return (DL().outline(-3, -2, W // 2, H // 2, 2, RED).fill(W // 2 - 1, H // 2 - 1, W + 5, H + 5, GREEN)
            .outline(0, 0, W - 1, H - 1, 1, BLUE).write(1, 1, 1, WHITE, 'Hq|0.5').write(W - 8, H - 6, 1, ODD, 'gy')
            .outline(W - 3, -1, W + 2, H, 2, ODD).write(-2, H - 12, 2, RED, '@j').fill(0, H - 1, 0, H - 1, BLACK))


def size_cases():
    sizes = [(1, 1), (5, 7), (TILE_H, TILE_W), (TILE_H + 1, TILE_W + 1), (TILE_H, TILE_W + GROUP - 1), (9, 2 * TILE_W + 2),
             (2 * TILE_H + 3, 7)]
    out = [Case(f'size_{H}x{W}', H, W, [generic(H, W)]) for H, W in sizes]
    out.append(Case('size_1x1_fill', 1, 1, [DL().fill(0, 0, 0, 0, ODD)]))
    return out


BOX_H, BOX_W = 20, 70
BOXES = {
    'outside_left': (-10, 2, -1, 8), 'outside_right': (BOX_W, 2, BOX_W + 10, 8), 'outside_top': (5, -9, 20, -1),
    'outside_bottom': (5, BOX_H, 20, BOX_H + 10),
    'straddle_left': (-4, 3, 6, 12), 'straddle_right': (62, 3, 75, 12), 'straddle_top': (10, -4, 30, 5),
    'straddle_bottom': (10, 14, 30, 25), 'corner_tl': (-4, -4, 5, 5), 'corner_tr': (64, -4, 75, 5),
    'corner_bl': (-4, 15, 5, 25), 'corner_br': (64, 15, 75, 25),
    'whole_exact': (0, 0, BOX_W - 1, BOX_H - 1), 'whole_beyond': (-5, -5, BOX_W + 10, BOX_H + 10),
    'whole_far': (-LIMIT, -LIMIT, LIMIT, LIMIT),
    'inverted_x': (10, 5, 9, 8), 'inverted_y': (5, 10, 20, 9), 'single_pixel': (7, 7, 7, 7),
    'across_tiles': (60, 12, 68, 18), 'tile_corner_pixels': (63, 15, 64, 16),
}


def box_cases():
    out = []
    for name, (x0, y0, x1, y1) in BOXES.items():
        out.append(Case(f'box_{name}_fill', BOX_H, BOX_W, [DL().fill(x0, y0, x1, y1, ODD)]))
        for w in (1, 2):
            if name == 'whole_far' and w == 2:
                continue
            out.append(Case(f'box_{name}_outline_w{w}', BOX_H, BOX_W, [DL().outline(x0, y0, x1, y1, w, ODD)]))
    for w in (0, 1, 5, 6, 7, 40):           # side 12: 2w = side at 6; side 11 (below): 2w = side + 1 at 6, a 1-pixel hollow at 5
        out.append(Case(f'box_width_side12_w{w}', BOX_H, BOX_W, [DL().outline(10, 2, 21, 13, w, ODD)]))
        out.append(Case(f'box_width_side11_w{w}', BOX_H, BOX_W, [DL().outline(10, 2, 20, 12, w, ODD)]))
    out.append(Case('box_width_negative', BOX_H, BOX_W, [DL().outline(10, 2, 21, 13, -3, ODD)], [DL()]))
    out.append(Case('box_hollow_holds_a_tile', 3 * TILE_H + 4, 3 * TILE_W + 4,
                    [DL().outline(TILE_W - 3, TILE_H - 3, 2 * TILE_W + 2, 2 * TILE_H + 2, 3, ODD)
                     .outline(TILE_W - 2, TILE_H - 2, 2 * TILE_W + 1, 2 * TILE_H + 1, 3, RED)]))
    out.append(Case('box_unknown_kind', BOX_H, BOX_W, [DL().raw([7, 2, 2, 30, 12, 2, pack(ODD), 0]).fill(1, 1, 3, 3, RED)
                                                      .raw([-1, 0, 0, 9, 9, 1, pack(ODD), 0])], [DL().fill(1, 1, 3, 3, RED)]))
    return out


def overlap_list():
    return (DL().fill(5, 2, 40, 12, RED).outline(20, 5, 60, 18, 3, GREEN).write(16, 4, 1, WHITE, 'car|0.98')
            .fill(30, 0, 36, 19, BLUE))


def grown_outward(dl):
    """the planted defect of tests/test_visualization.py: every outline grows outward instead of inward"""
    out = DisplayList()
    out.text = bytearray(dl.text)
    out.rows = [[k, a - e + 1, b - e + 1, c + e - 1, d + e - 1, e, col, z] if k == OUTLINE else [k, a, b, c, d, e, col, z]
                for k, a, b, c, d, e, col, z in dl.rows]
    return out


def order_cases(capacity):
    out = [Case('order_forward', BOX_H, BOX_W, [overlap_list()]), Case('order_reversed', BOX_H, BOX_W, [overlap_list().reversed()])]

    def covering(count):       # every row covers most of tile (0, 0), every row another colour: the last one wins
        dl = DL()
        for i in range(count):
            dl.fill(i % 13, i % 7, TILE_W - 1 - i % 5, TILE_H - 1 - i % 3, (i % 251 + 1, (i * 7) % 256, (i * 13) % 256))
        return dl
    for count in (capacity, capacity + 1, 2 * capacity + 1):
        out.append(Case(f'capacity_{count}_rows_on_one_tile', TILE_H, TILE_W, [covering(count)]))

    dl = DL()                   # two tiles take turns, one row in three misses the image: ragged hits in every wave
    for i in range(3 * capacity + 1):
        col = ((i * 3) % 256, i % 256, (i * 11) % 256)
        if (i * 7) % 3 == 0:
            dl.fill(-40, i % 5, -1 - i % 3, 9, col)
        elif i % 2:
            dl.outline(i % 9, i % 4, TILE_W - 1, TILE_H - 1, 1 + i % 3, col)
        else:
            dl.fill(TILE_W + i % 11, i % 6, 2 * TILE_W + 5, TILE_H + 4, col)
    dl.write(TILE_W - 9, 3, 1, WHITE, 'ab').fill(2, 2, 2, 2, ODD)
    out.append(Case('capacity_two_tiles_take_turns', TILE_H + 2, 2 * TILE_W + 3, [dl]))
    return out


PRINTABLE = bytes(range(32, 127))


def text_cases():
    H, W = 24, 80
    out = [Case('text_all_printable', 13, 6 * 95 + 2, [DL().write(1, 1, 1, ODD, PRINTABLE)]),
           Case('text_all_printable_scale2_two_lines', 2 * 22 + 3, 6 * 2 * 48 + 1,
                [DL().write(0, 0, 2, ODD, PRINTABLE[:48]).write(0, 23, 2, RED, PRINTABLE[48:])])]
    where = {'left': (-7, 3), 'right': (W - 10, 3), 'top': (5, -5), 'bottom': (5, H - 5), 'corner': (W - 4, H - 3),
             'outside_left': (-100, 3), 'outside_right': (W, 3), 'outside_top': (5, -11), 'outside_bottom': (5, H),
             'just_inside_left': (-41, 3), 'just_outside_left': (-42, 3)}
    for name, (x, y) in where.items():
        out.append(Case(f'text_clip_{name}', H, W, [DL().write(x, y, 1, ODD, 'Wg|0.87')]))
    for s in (1, 2, 3):
        out.append(Case(f'text_scale_{s}', 40, 150, [DL().write(3, 2, s, ODD, 'aQ|1.0j').write(-5 * s, 40 - 7 * s, s, RED, 'Mg')]))
    out.append(Case('text_empty_run', H, W, [DL().write(3, 3, 1, ODD, b'').write(3, 3, 2, RED, b'').fill(0, 0, 1, 1, GREEN)]))
    out.append(Case('text_bytes_that_paint_nothing', H, W, [DL().write(2, 2, 1, ODD, b'A\x00B\x1fC\x7fD\xffE\x80')
                                                            .write(2, 13, 1, RED, b'\x00\x1f\x7f\xff')]))
    out.append(Case('text_scale_below_one', H, W, [DL().write(3, 3, 0, ODD, 'Wg|0.87').write(3, 3, -1, RED, 'Wg').write(0, 0, INT_MIN, RED, '|')
                                                   .fill(0, 0, 1, 1, GREEN)], [DL().fill(0, 0, 1, 1, GREEN)]))
    out.append(Case('text_over_boxes', H, W, [DL().fill(0, 0, W - 1, H - 1, BLACK).write(1, 1, 1, WHITE, 'person|0.31')
                                              .outline(0, 0, 50, 12, 1, RED).write(30, 6, 2, GREEN, 'Xy')]))
    return out


def batch_cases():
    k = DL().outline(2, 2, 60, 15, 2, RED).fill(3, 3, 20, 12, BLACK).write(4, 4, 1, WHITE, 'bus|0.77').fill(66, 17, 80, 30, BLUE)
    return [Case('batch_counts_0_k_1', BOX_H, BOX_W, [DL(), k, DL().write(1, 5, 1, ODD, 'z')]),
            Case('batch_no_rows_at_all', BOX_H, BOX_W, [DL()]),
            Case('batch_text_offsets_per_image', BOX_H, BOX_W, [DL().write(1, 1, 1, RED, 'first'), DL(),
                                                                DL().write(1, 1, 1, GREEN, 'second').write(30, 8, 1, BLUE, '3rd')])]


def extreme_cases():
    """int32 extremes; the modest list on the right paints the same pixels by the rule
    x0 <= x <= x1, y0 <= y <= y1, and for an outline (x - x0 < w or x1 - x < w or y - y0 < w or y1 - y < w)"""
    H, W = BOX_H, BOX_W
    whole = [DL().fill(0, 0, W - 1, H - 1, ODD)]
    bar = glyph_mask(ord('|'), 1)
    assert not bar[0, 0]
    bar_row, bar_col = (int(v) for v in np.argwhere(bar)[0])
    edge, edge_row = next((chr(c), int(np.argmax(glyph_mask(c, 1)[:7, 0]))) for c in range(33, 127) if glyph_mask(c, 1)[:7, 0].any())
    return [
        Case('extreme_fill_everything', H, W, [DL().fill(INT_MIN, INT_MIN, INT_MAX, INT_MAX, ODD)], whole),
        Case('extreme_fill_far_away', H, W, [DL().fill(INT_MIN, INT_MIN, INT_MIN + 5, INT_MAX, ODD)
                                             .fill(INT_MAX - 5, 0, INT_MAX, 5, ODD)], [DL()]),
        # rows 3 .. 8 over the whole width; the vertical edges are 2^31 pixels away: only the two horizontal bands
        Case('extreme_outline_band', H, W, [DL().outline(INT_MIN, 3, INT_MAX, 8, 2, ODD)],
             [DL().fill(0, 3, W - 1, 4, ODD).fill(0, 7, W - 1, 8, ODD)]),
        # w = 2^31 - 1: x - x0 = x + 2^31 >= w always; x1 - x = 2^31 - 1 - x < w iff x > 0; the same in y: all but (0, 0)
        Case('extreme_outline_width', H, W, [DL().outline(INT_MIN, INT_MIN, INT_MAX, INT_MAX, INT_MAX, ODD)],
             [DL().fill(1, 0, W - 1, H - 1, ODD).fill(0, 1, 0, H - 1, ODD)]),
        Case('extreme_outline_hollow', H, W, [DL().outline(INT_MIN, INT_MIN, INT_MAX, INT_MAX, 1000, ODD)], [DL()]),
        Case('extreme_outline_inverted', H, W, [DL().outline(INT_MAX, 0, INT_MIN, 5, 3, ODD).fill(0, INT_MAX, 5, INT_MIN, ODD)], [DL()]),
        Case('extreme_text_far_away', H, W, [DL().write(INT_MIN, 3, 1, ODD, 'abc').write(INT_MAX, 3, 3, ODD, 'abc')
                                             .write(3, INT_MIN, 1, ODD, 'abc').write(3, INT_MAX, 2, ODD, 'abc')], [DL()]),
        # at scale 10^8 one glyph bit covers the image: a set bit of '|' paints all of it, its clear bit (0, 0) nothing
        Case('extreme_text_scale_set_bit', H, W, [DL().write(-bar_col * 10 ** 8, -bar_row * 10 ** 8, 10 ** 8, ODD, '|')], whole),
        Case('extreme_text_scale_clear_bit', H, W, [DL().write(0, 0, INT_MAX, ODD, '|||')], [DL()]),
        # the second character of a run whose cells are 6 * 3.5 * 10^8 = 2.1 * 10^9 wide, from x = -2^31: the image lies
        # 2^31 - 2.1 * 10^9 < 3.5 * 10^8 into that cell, in its column 0, where `edge` has a set bit in row edge_row
        Case('extreme_text_second_cell', H, W, [DL().write(INT_MIN, -edge_row * 35 * 10 ** 7, 35 * 10 ** 7, ODD, ' ' + edge)], whole),
    ]


def fuzz_case(seed=0, count=200, H=37, W=150):
    rs, dl = np.random.RandomState(seed), DL()
    for _ in range(count):
        kind = rs.randint(3)
        col = tuple(int(v) for v in rs.randint(0, 256, 3))
        x0, y0 = int(rs.randint(-30, W + 10)), int(rs.randint(-20, H + 10))
        if kind == TEXT:
            run = bytes(rs.randint(0, 256, rs.randint(0, 9)).astype(np.uint8)) if rs.rand() < 0.3 else \
                bytes(rs.randint(32, 127, rs.randint(0, 9)).astype(np.uint8))
            dl.write(x0, y0, int(rs.randint(1, 4)), col, run)
        else:
            x1, y1 = x0 + int(rs.randint(-2, 60)), y0 + int(rs.randint(-2, 25))
            dl.fill(x0, y0, x1, y1, col) if kind == FILL and rs.rand() < 0.3 else dl.outline(x0, y0, x1, y1, int(rs.randint(0, 5)), col)
    return Case(f'fuzz_{seed}', H, W, [dl])


def all_cases(capacity):
    return (size_cases() + box_cases() + order_cases(capacity) + text_cases() + batch_cases() + extreme_cases()
            + [fuzz_case(0), fuzz_case(1, count=2 * capacity + 37)])
