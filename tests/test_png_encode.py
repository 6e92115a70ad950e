"""csrc/png_encode.hip and tools/analysis_tools/get_corrupted_dataset.py: resident batches -> zlib streams -> PNG files.

CPU: the host-side file writer around streams made by Python's zlib, the tool's command line and path mapping, and the
capacity / segment queries.  GPU (-m gpu): every stream of the device encoder is inflated by zlib (which also checks the
Adler-32), compared with the numpy oracle below - exactly in the forced filter modes, through the oracle's un-filtering in
every mode - written to a file and read back through PIL and the native decoder, and encoded a second time; and the tool
end to end.

The oracle is numpy: the five PNG filters over whole images at once, and un-filtering along the wavefronts x + 2y = d
(a pixel needs its left, upper and upper-left neighbours: d - 1, d - 2, d - 3)."""
import ctypes
import functools
import heapq
import importlib.util
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5


@pytest.fixture(autouse=True)
def _local_rank(monkeypatch):
    monkeypatch.setenv('LOCAL_RANK', '0')                         # (the tool's parser sets it when it is missing)


@functools.lru_cache(None)
def tool():
    spec = importlib.util.spec_from_file_location('get_corrupted_dataset_tool',
                                                  os.path.join(ROOT, 'tools', 'analysis_tools', 'get_corrupted_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lib():
    from oadg_amd import _lib as B
    return B, B.lib()


# ----------------------------------------------------------------------------------------------------------- oracle
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def _predict(t, a, b, c):
    """the predictor of filter type ``t`` (an array broadcast against the pixels) from left, up and upper-left"""
    return np.select([t == 0, t == 1, t == 2, t == 3, t == 4], [np.zeros_like(a), a, b, (a + b) >> 1, _paeth(a, b, c)])


def filter_rows(rgb, types):
    """uint8 [H, W, 3] and one filter type per row (or one for all) -> the PNG scanlines uint8 [H, 3W + 1]"""
    H, W, _ = rgb.shape
    types = np.broadcast_to(np.asarray(types, dtype=np.int32), (H,))
    pad = np.zeros((H + 1, W + 1, 3), dtype=np.int32)                 # zero outside the image
    pad[1:, 1:] = rgb
    x, a, b, c = pad[1:, 1:], pad[1:, :-1], pad[:-1, 1:], pad[:-1, :-1]
    out = np.empty((H, 3 * W + 1), dtype=np.uint8)
    out[:, 0] = types
    out[:, 1:] = ((x - _predict(types[:, None, None], a, b, c)) & 255).reshape(H, 3 * W)
    return out


def unfilter(scanlines, H, W):
    """PNG scanlines (bytes or uint8 [H, 3W + 1]) -> uint8 [H, W, 3]"""
    s = np.frombuffer(bytes(scanlines), dtype=np.uint8).reshape(H, 3 * W + 1)
    types, f = s[:, 0].astype(np.int32), s[:, 1:].reshape(H, W, 3).astype(np.int32)
    assert types.max() <= 4
    out = np.zeros((H + 1, W + 1, 3), dtype=np.int32)
    for d in range(W + 2 * (H - 1)):
        y = np.arange(max(0, -((W - 1 - d) // 2)), min(H - 1, d // 2) + 1)
        x = d - 2 * y
        a, b, c = out[y + 1, x], out[y, x + 1], out[y, x]
        out[y + 1, x + 1] = (f[y, x] + _predict(types[y][:, None], a, b, c)) & 255
    return out[1:, 1:].astype(np.uint8)


def test_the_oracle_unfilters_what_it_filters_and_agrees_with_pil(tmp_path):
    from PIL import Image
    rgb = smooth(3, 9, 14)
    for t in (0, 1, 2, 3, 4, np.arange(9) % 5):
        assert np.array_equal(unfilter(filter_rows(rgb, t), 9, 14), rgb)
    # PIL's own file: its IDAT, inflated, un-filters to the picture
    Image.fromarray(rgb).save(tmp_path / 'p.png')
    data = open(tmp_path / 'p.png', 'rb').read()
    idat, at = b'', 8
    while at < len(data):
        n = int.from_bytes(data[at:at + 4], 'big')
        if data[at + 4:at + 8] == b'IDAT':
            idat += data[at + 8:at + 8 + n]
        at += 12 + n
    assert np.array_equal(unfilter(zlib.decompress(idat), 9, 14), rgb)
    # hand values: Sub, Up, Average and Paeth of the second pixel of the second row
    two = np.array([[[10, 20, 30], [40, 60, 90]], [[50, 0, 250], [100, 7, 3]]], dtype=np.uint8)
    assert filter_rows(two, 1)[1].tolist() == [1, 50, 0, 250, 50, 7, 9]
    assert filter_rows(two, 2)[1].tolist() == [2, 40, 236, 220, 60, 203, 169]
    assert filter_rows(two, 3)[1].tolist() == [3, 45, 246, 235, 55, 233, 89]
    assert filter_rows(two, 4)[1].tolist() == [4, 40, 236, 220, 50, 203, 9]


# ------------------------------------------------------------------------------------------------------------ content
def smooth(seed, H, W):
    """a random walk along every row: neighbouring bytes are close, so filters and Huffman codes have something to do"""
    rs = np.random.RandomState(seed)
    steps = rs.randint(-3, 4, (H, W, 3))
    steps[:, 0] = rs.randint(0, 256, (H, 3))
    return (np.cumsum(steps, axis=1) & 255).astype(np.uint8)


def content(kind, H, W):
    rs = np.random.RandomState(H * 1000 + W)
    if kind == 'zeros':
        a = np.zeros((H, W, 3), np.uint8)
    elif kind == 'full':
        a = np.full((H, W, 3), 255, np.uint8)
    elif kind == 'two_values':
        a = rs.choice([17, 200], (H, W, 3)).astype(np.uint8)
    elif kind == 'hramp':
        a = ((np.arange(W)[None, :, None] * 3 + np.arange(3)[None, None, :] * 5 + np.zeros((H, 1, 1), int)) & 255).astype(np.uint8)
    elif kind == 'vramp':
        a = ((np.arange(H)[:, None, None] * 7 + np.zeros((1, W, 3), int)) & 255).astype(np.uint8)
    elif kind == 'random':
        a = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    elif kind == 'smooth':
        a = smooth(H * 1000 + W, H, W)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a)


def huffman_depth(counts):
    """the depth of an unlimited Huffman code over the non-zero counts"""
    heap = [(c, 0) for c in counts if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        (c1, d1), (c2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (c1 + c2, max(d1, d2) + 1))
    return heap[0][1]


def fibonacci_row():
    """One row under filter None whose symbol counts - its bytes, the row's filter-type byte (a zero) and end-of-block - are
    the Fibonacci numbers F1 .. F20, strictly (no two partial sums tie, so the Huffman tree is one chain of depth 19), plus
    a twentieth byte value with 1000 occurrences that makes the row length a multiple of 3.  18,708 bytes: more would not
    fit one segment.  -> uint8 [1, W, 3]"""
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    # F1 = end-of-block, F2 = value 1, F3 = value 0 (one of its two is the filter-type byte), F4 .. F20 = values 2 .. 18
    counts = {0: fib[2] - 1, 1: fib[1]}
    counts.update({v: fib[v + 1] for v in range(2, 19)})
    counts[19] = 1000
    data = np.concatenate([np.full(c, v, np.uint8) for v, c in counts.items()])
    assert len(data) % 3 == 0 and len(counts) == 20
    data = np.random.RandomState(4).permutation(data)
    hist = np.bincount(data, minlength=257)
    hist[0] += 1
    hist[256] = 1
    return data.reshape(1, -1, 3), hist


# ------------------------------------------------------------------------------------------------- CPU: file writer
def _write(path, stream, H, W):
    B, L = _lib()
    buf = ctypes.create_string_buffer(bytes(stream), len(stream))
    return L.oadg_png_write_rgb8(str(path).encode(), ctypes.addressof(buf), len(stream), H, W)


def _decode_bgr(path, H, W):
    B, L = _lib()
    out = np.full((H, W, 3), 0x5a, dtype=np.uint8)
    return L.oadg_png_decode_bgr(str(path).encode(), out.ctypes.data, H, W), out


def check_file(path, rgb):
    from PIL import Image
    H, W, _ = rgb.shape
    with Image.open(path) as im:
        im.verify()                                               # every chunk's CRC
    with Image.open(path) as im:
        assert im.mode == 'RGB' and im.size == (W, H)
        assert np.array_equal(np.asarray(im), rgb)
    rc, bgr = _decode_bgr(path, H, W)
    assert rc == 0 and np.array_equal(bgr, rgb[:, :, ::-1])


@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (64, 33)])
def test_writer_wraps_a_zlib_stream_into_a_png_file(tmp_path, H, W):
    rgb = smooth(H + W, H, W)
    for k, level in enumerate((6, 0)):
        stream = zlib.compress(filter_rows(rgb, np.arange(H) % 5).tobytes(), level)
        path = tmp_path / f'{k}.png'
        assert _write(path, stream, H, W) == 0
        check_file(path, rgb)
        data = open(path, 'rb').read()
        assert data[:8] == b'\x89PNG\r\n\x1a\n' and data[12:16] == b'IHDR' and data[-12:-8] == b'\x00\x00\x00\x00'
        assert data[-8:-4] == b'IEND' and data[16:29] == W.to_bytes(4, 'big') + H.to_bytes(4, 'big') + bytes([8, 2, 0, 0, 0])
    assert _write(tmp_path / 'no_such_dir' / 'a.png', stream, H, W) == -3          # OADG_EIO
    assert _write(tmp_path / 'x.png', stream, 0, W) == -1 and not os.path.exists(tmp_path / 'x.png')


# -------------------------------------------------------------------------------------- CPU: the tool's command line
def test_argument_parser_is_the_reference_surface():
    T = tool()
    a = T.parse_args(['cfg.py', '--show-dir', '/out'])
    assert vars(a) == dict(config='cfg.py', show_dir='/out', corruptions='benchmark', severities=[0, 1, 2, 3, 4, 5],
                           workers=32, debug=False, seed=0, launcher='none', local_rank=0, cfg_options=None)
    a = T.parse_args(['cfg.py', '--show-dir', '/o', '--corruptions', 'noise', 'fog', '--severities', '1', '5', '--workers', '4',
                      '--debug', '--seed', '7', '--launcher', 'slurm', '--local_rank', '2', '--cfg-options', 'a.b=1', 'c=x'])
    assert (a.corruptions, a.severities, a.workers, a.debug, a.seed, a.launcher, a.local_rank, a.cfg_options) == (
        ['noise', 'fog'], [1, 5], 4, True, 7, 'slurm', 2, {'a.b': '1', 'c': 'x'})
    with pytest.raises(SystemExit):
        T.parse_args(['cfg.py'])                                   # --show-dir is required
    with pytest.raises(SystemExit):
        T.parse_args(['cfg.py', '--show-dir', '/o', '--corruptions', 'rain'])
    assert len(T.CHOICES) == 27 and T.CHOICES[:8] == ['all', 'benchmark', 'noise', 'blur', 'weather', 'digital', 'holdout', 'None']
    from oadg_amd import evaluation as E
    assert E.select_corruptions(a.corruptions, a.severities)[0] == ['gaussian_noise', 'shot_noise', 'impulse_noise']
    assert len(E.select_corruptions(T.parse_args(['c', '--show-dir', 'o']).corruptions, [1])[0]) == 15
    assert T.writer_threads(32) == 16 and T.writer_threads(0) == 1 and T.writer_threads(5) == 5 and T.writer_threads(9, True) == 1


def test_launcher_other_than_none_is_refused(tmp_path):
    cfg = tmp_path / 'cfg.py'
    cfg.write_text("data = dict(test=dict(type='CityscapesDataset', ann_file='a.json', img_prefix='x/', pipeline=[]))\n")
    with pytest.raises(TypeError, match='distribution'):
        tool().main([str(cfg), '--show-dir', str(tmp_path / 'o'), '--launcher', 'pytorch'])
    assert not os.path.exists(tmp_path / 'o')


def test_path_mapping_and_severity_zero_once():
    T = tool()
    assert T.plan(['fog', 'snow', 'frost'], [0, 1, 5]) == [('fog', 0), ('fog', 1), ('fog', 5), ('snow', 1), ('snow', 5),
                                                            ('frost', 1), ('frost', 5)]
    assert T.plan(['None'], [0]) == [('None', 0)] and T.plan(['fog'], [2]) == [('fog', 2)]
    d = T.out_dir_of('/data/cityscapes-c/leftImg8bit/val', 'fog', 3)
    assert d == '/data/cityscapes-c/leftImg8bit/val/fog/3'
    assert T.out_path(d, 'frankfurt/frankfurt_000000_000294_leftImg8bit.png') == d + '/frankfurt/frankfurt_000000_000294_leftImg8bit.png'
    assert T.out_path(d, 'JPEGImages/000012.jpg') == d + '/JPEGImages/000012.png'
    assert T.out_path(d, '0.png') == d + '/0.png'


def test_the_tool_writes_where_the_robustness_loop_reads():
    from oadg_amd import evaluation as E
    T = tool()
    for prefix in ('/data/cityscapes/leftImg8bit/val/', '/tmp/x/cityscapes/val/img/', '/data/coco/val2017/'):
        clean = 'cityscapes' if '/cityscapes/' in prefix else 'coco'
        show_dir = prefix.replace(clean, clean + '-c').rstrip('/')
        for corruption, severity in T.plan(['gaussian_noise', 'jpeg_compression'], [0, 1, 5]):
            if severity:
                assert T.out_dir_of(show_dir, corruption, severity) + '/' == E.corrupted_img_prefix(prefix, corruption, severity)
        assert T.out_path(T.out_dir_of(show_dir, 'fog', 2), 'a/b.png') == E.corrupted_img_prefix(prefix, 'fog', 2) + 'a/b.png'


# -------------------------------------------------------------------------------------------------- CPU: the queries
def test_capacity_and_segment_queries():
    B, L = _lib()
    for W in (1, 2, 21, 683, 2048, 6314, 6315, 7000, 100000):
        segs = []
        for H in (1, 2, 3, 15, 16, 17, 100, 513, 1024, 5000):
            n, cap, ln = L.oadg_png_encode_segments(H, W), L.oadg_png_encode_stream_capacity(H, W), (3 * W + 1) * H
            assert n >= 1 and ln + 8 + 5 <= cap <= ln + ln // 64 + 64, (H, W, n, cap)
            assert cap >= ln + 5 * n + 8                          # every segment stored: 5 bytes each (it is at most 65,535)
            assert L.oadg_png_encode_workspace_bytes(2, H, W) >= 2 * cap - 16
            segs.append(n)
        assert segs == sorted(segs) and segs[-1] > segs[0], (W, segs)
    assert L.oadg_png_encode_segments(1024, 2048) * 3 >= 1024                      # (three rows of 6145 bytes per segment)
    for H, W in ((0, 5), (5, 0), (-1, 1), (1, -1), (1 << 16, 1 << 15), (1, 1 << 30)):
        assert L.oadg_png_encode_segments(H, W) == 0 and L.oadg_png_encode_stream_capacity(H, W) == 0
        assert L.oadg_png_encode_workspace_bytes(1, H, W) == 0
    assert L.oadg_png_encode_workspace_bytes(0, 4, 4) == 0 and L.oadg_png_encode_workspace_bytes(1 << 16, 4, 4) == 0


def test_fibonacci_row_is_deeper_than_deflate_allows():
    row, hist = fibonacci_row()
    assert row.shape[0] == 1 and 3 * row.shape[1] + 1 <= 18944 and len(np.unique(row)) >= 20
    assert huffman_depth(hist.tolist()) > 15


# -------------------------------------------------------------------------------------------------------------- GPU
def encode(dev, imgs, bgr=0, mode=-1, capacity=None, guard=64):
    """oadg_png_encode_rgb8 on uint8 [n, H, W, 3] -> (the whole output buffer incl. the guard as numpy, sizes, capacity)"""
    import torch
    B, L = _lib()
    n, H, W, _ = imgs.shape
    cap = int(L.oadg_png_encode_stream_capacity(H, W)) if capacity is None else capacity
    ws_bytes = int(L.oadg_png_encode_workspace_bytes(n, H, W))
    assert ws_bytes > 0
    d = torch.from_numpy(np.ascontiguousarray(imgs)).to(dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.full((n * cap + guard,), FILL, dtype=torch.uint8, device=dev)
    sizes = torch.full((n,), -7, dtype=torch.int64, device=dev)
    B.check(L.oadg_png_encode_rgb8(B.ptr(d), n, H, W, bgr, mode, B.ptr(out), cap, B.ptr(sizes), B.ptr(ws), ws_bytes,
                                   B.stream_ptr()), 'oadg_png_encode_rgb8')
    return out.cpu().numpy(), sizes.cpu().numpy(), cap


def streams_of(buf, sizes, cap):
    n = len(sizes)
    assert (sizes >= 8).all() and (sizes <= cap).all(), (sizes, cap)               # stream_bytes <= capacity
    for i in range(n):
        assert (buf[i * cap + sizes[i]:(i + 1) * cap] == FILL).all()               # nothing behind a stream
    assert (buf[n * cap:] == FILL).all()
    return [buf[i * cap:i * cap + sizes[i]].tobytes() for i in range(n)]


def check_case(dev, tmp_path, rgb, modes=(-1, 0, 1, 2, 3, 4), tag='c'):
    """all the checks of one case on one RGB image, per filter mode -> {mode: stream}"""
    B, L = _lib()
    H, W, _ = rgb.shape
    bound = (3 * W + 1) * H + (3 * W + 1) * H // 64 + 64
    out = {}
    for mode in modes:
        buf, sizes, cap = encode(dev, rgb[None], 0, mode)
        stream, = streams_of(buf, sizes, cap)
        assert len(stream) <= cap <= bound
        raw = zlib.decompress(stream)                                              # (raises on a wrong Adler-32)
        assert len(raw) == (3 * W + 1) * H
        assert np.array_equal(unfilter(raw, H, W), rgb), mode
        if mode >= 0:
            assert raw == filter_rows(rgb, mode).tobytes(), mode
        path = tmp_path / f'{tag}_{mode}.png'
        assert _write(path, stream, H, W) == 0
        check_file(path, rgb)
        buf2, sizes2, _ = encode(dev, rgb[None], 0, mode)
        assert buf2.tobytes() == buf.tobytes() and sizes2.tolist() == sizes.tolist()          # a second run: the same bytes
        out[mode] = stream
    return out


def first_change(W):
    """the smallest H with more segments than H = 1 has"""
    B, L = _lib()
    H = 2
    while L.oadg_png_encode_segments(H, W) == L.oadg_png_encode_segments(1, W):
        H += 1
    return H


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', [(1, 1), (1, 5), (2, 21), (7, 683), (33, 64), (2, 7001), (1, 6500)])
def test_extents(dev, tmp_path, H, W):
    check_case(dev, tmp_path, content('smooth', H, W))


@pytest.mark.gpu
@pytest.mark.parametrize('W', [21, 683])
@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_extents_either_side_of_the_first_segment_boundary(dev, tmp_path, W, delta):
    B, L = _lib()
    H = first_change(W) + delta
    assert L.oadg_png_encode_segments(H, W) == (1 if delta < 0 else 2)
    check_case(dev, tmp_path, content('smooth', H, W), modes=(-1, 3, 4))


@pytest.mark.gpu
def test_three_segments_and_a_ragged_last_one(dev, tmp_path):
    B, L = _lib()
    rows = first_change(683) - 1                                                   # rows of a full segment
    H = 2 * rows + max(1, rows // 2)
    assert L.oadg_png_encode_segments(H, 683) == 3 and H % rows != 0
    check_case(dev, tmp_path, content('smooth', H, 683))
    H = 3 * rows + 1
    assert L.oadg_png_encode_segments(H, 683) == 4
    check_case(dev, tmp_path, content('smooth', H, 683), modes=(-1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', [(5, 21), (40, 683)])
@pytest.mark.parametrize('kind', ['zeros', 'full', 'two_values', 'hramp', 'vramp', 'random'])
def test_content(dev, tmp_path, kind, H, W):
    rgb = content(kind, H, W)
    streams = check_case(dev, tmp_path, rgb)
    ln = (3 * W + 1) * H
    if kind == 'hramp':
        assert len(streams[-1]) <= len(streams[0])                                 # adaptive is not larger than None
    if kind == 'random':                                                           # nothing to gain: stored blocks
        for mode in (-1, 0):
            assert ln < len(streams[mode]) <= ln + ln // 64 + 64
        B, L = _lib()
        assert len(streams[0]) == ln + 5 * L.oadg_png_encode_segments(H, W) + 8
    if kind in ('zeros', 'two_values'):
        assert len(streams[0]) < ln // 4 + 200 * (1 + ln // 18944)                 # one or two used literals: <= 2 bits each
    if kind == 'zeros':
        assert zlib.decompress(streams[-1]) == bytes(ln)


@pytest.mark.gpu
def test_fibonacci_counts_need_the_length_limit(dev, tmp_path):
    B, L = _lib()
    row, hist = fibonacci_row()
    assert L.oadg_png_encode_segments(1, row.shape[1]) == 1 and huffman_depth(hist.tolist()) > 15
    streams = check_case(dev, tmp_path, row, modes=(0,))
    assert np.array_equal(np.bincount(np.frombuffer(zlib.decompress(streams[0]), np.uint8), minlength=256), hist[:256])
    assert len(streams[0]) < row.size // 2                                         # coded, not stored


@pytest.mark.gpu
def test_batch_equals_single_images_and_both_channel_orders(dev, tmp_path):
    B, L = _lib()
    H, W = 22, 683
    assert L.oadg_png_encode_segments(H, W) >= 3
    imgs = np.stack([content('smooth', H, W), content('random', H, W), content('vramp', H, W)])
    for mode in (-1, 4):
        buf, sizes, cap = encode(dev, imgs, 0, mode)
        batch = streams_of(buf, sizes, cap)
        assert len(set(batch)) == 3
        for i in range(3):
            b1, s1, _ = encode(dev, imgs[i:i + 1], 0, mode)
            assert streams_of(b1, s1, cap)[0] == batch[i], (mode, i)
            assert np.array_equal(unfilter(zlib.decompress(batch[i]), H, W), imgs[i])
        buf, sizes, cap = encode(dev, imgs[..., ::-1], 1, mode)                    # the same pictures stored B, G, R
        assert streams_of(buf, sizes, cap) == batch
    path = tmp_path / 'bgr.png'
    assert _write(path, batch[0], H, W) == 0
    check_file(path, imgs[0])


@pytest.mark.gpu
@pytest.mark.parametrize('which', ['one_byte', 'half_of_the_first', 'between_first_and_third'])
def test_a_short_capacity_is_reported_and_nothing_is_written_past_it(dev, which):
    H, W = 22, 683
    imgs = np.stack([content('smooth', H, W), content('zeros', H, W), content('random', H, W)])
    buf, sizes, cap = encode(dev, imgs, 0, -1)
    full = streams_of(buf, sizes, cap)
    assert len(full[1]) < len(full[0]) // 2 and len(full[0]) + 2 < len(full[2])
    short = dict(one_byte=1, half_of_the_first=len(full[0]) // 2, between_first_and_third=(len(full[0]) + len(full[2])) // 2)[which]
    got, need, _ = encode(dev, imgs, 0, -1, capacity=short)
    assert need.tolist() == sizes.tolist()                                         # the full need
    for i in range(3):
        k = min(short, len(full[i]))
        assert got[i * short:i * short + k].tobytes() == full[i][:k]               # the other images' streams are intact
        assert (got[i * short + k:(i + 1) * short] == FILL).all()
    assert (got[3 * short:] == FILL).all()                                         # the guard behind the last slot


@pytest.mark.gpu
def test_refusals(dev):
    import torch
    B, L = _lib()
    need = L.oadg_png_encode_workspace_bytes(1, 5, 7)
    assert need > 0
    imgs = torch.zeros(5 * 7 * 3, dtype=torch.uint8, device=dev)
    out = torch.zeros(1 << 12, dtype=torch.uint8, device=dev)
    work = torch.zeros(need, dtype=torch.uint8, device=dev)
    sizes = torch.zeros(4, dtype=torch.int64, device=dev)

    def call(n=1, H=5, W=7, bgr=0, mode=-1, ws_bytes=need, imgs=imgs, out=out, ws=work):
        return L.oadg_png_encode_rgb8(B.ptr(imgs), n, H, W, bgr, mode, B.ptr(out), 1 << 12, B.ptr(sizes), B.ptr(ws), ws_bytes,
                                      B.stream_ptr())
    assert call(ws_bytes=need - 1) == -2 and call(ws_bytes=16) == -2 and call(ws_bytes=0) == -2      # OADG_ESIZE
    for bad in (dict(n=0), dict(n=1 << 16), dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 16, W=1 << 15), dict(bgr=2),
                dict(mode=5), dict(mode=-2), dict(imgs=None), dict(out=None), dict(ws=None)):
        assert call(**bad) == -1, bad                                              # OADG_EARG
    torch.cuda.synchronize()
    assert sizes.tolist() == [0, 0, 0, 0] and int(out.max()) == 0                  # a refused call launches nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert 8 < sizes[0].item() <= 1 << 12


@pytest.mark.gpu
def test_workload_extent(dev, tmp_path):
    B, L = _lib()
    rgb = content('smooth', 1024, 2048)
    streams = check_case(dev, tmp_path, rgb, modes=(-1, 1))
    assert L.oadg_png_encode_segments(1024, 2048) > 256
    assert len(streams[-1]) < rgb.size // 2


CFG = "data = dict(test=dict(type='CityscapesDataset', ann_file={ann!r}, img_prefix={prefix!r}, pipeline=[]))\n"


@pytest.mark.gpu
def test_tool_writes_the_tree_end_to_end(dev, tmp_path, monkeypatch, capsys):
    from PIL import Image
    from oadg_amd import evaluation as E
    from oadg_amd.datasets import CityscapesDataset
    from oadg_amd.pipelines.corrupt import corrupt
    T = tool()
    root = tmp_path / 'cityscapes' / 'val'
    spec = importlib.util.spec_from_file_location('make_synthetic_coco_tool', os.path.join(ROOT, 'tools', 'make_synthetic_coco.py'))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    monkeypatch.setattr(sys, 'argv', ['make_synthetic_coco.py', str(root), '--n', '3', '--height', '64', '--width', '128',
                                      '--boxes', '3'])
    maker.main()
    prefix, ann = str(root / 'img') + '/', str(root / 'train.json')
    assert '/cityscapes/' in prefix and prefix.count('cityscapes') == 1
    source = []
    for i in range(3):
        with Image.open(root / 'img' / f'{i}.png') as im:
            source.append(np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1]))      # as LoadImageFromFile: B, G, R
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(CFG.format(ann=ann, prefix=prefix))
    show_dir = prefix.replace('cityscapes', 'cityscapes-c').rstrip('/')
    T.main([str(cfg), '--show-dir', show_dir, '--corruptions', 'gaussian_blur', 'brightness', '--severities', '0', '3',
            '--workers', '2'])
    want = {('gaussian_blur', 0), ('gaussian_blur', 3), ('brightness', 3)}
    found = {os.path.relpath(os.path.join(d, f), show_dir) for d, _, fs in os.walk(show_dir) for f in fs}
    assert found == {f'{c}/{s}/{i}.png' for c, s in want for i in range(3)}
    for c, s in want:
        for i in range(3):
            rc, got = _decode_bgr(os.path.join(show_dir, c, str(s), f'{i}.png'), 64, 128)
            assert rc == 0 and np.array_equal(got, corrupt(source[i], c, s)), (c, s, i)
            if s:
                assert not np.array_equal(got, source[i])
    # the robustness loop's --load-dataset corrupted reads exactly these files
    ds = CityscapesDataset(ann_file=ann, img_prefix=E.corrupted_img_prefix(prefix, 'brightness', 3), test_mode=True, device=dev)
    loaded = ds.batch(range(3))[0].cpu().numpy()
    assert np.array_equal(loaded, np.stack([corrupt(source[i], 'brightness', 3) for i in range(3)]))
    # a host-path corruption with random draws: the tool's seed and order are the host loop's
    noisy = str(tmp_path / 'noisy')
    T.main([str(cfg), '--show-dir', noisy, '--corruptions', 'gaussian_noise', '--severities', '1', '--seed', '0'])
    np.random.seed(0)
    for i in range(3):
        expect = corrupt(source[i], 'gaussian_noise', 1)
        rc, got = _decode_bgr(os.path.join(noisy, 'gaussian_noise', '1', f'{i}.png'), 64, 128)
        assert rc == 0 and np.array_equal(got, expect), i
    assert '9 files' in capsys.readouterr().out
