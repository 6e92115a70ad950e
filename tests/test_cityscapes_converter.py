"""tools/dataset_converters/cityscapes.py: gtFine instance maps -> COCO json with the per-pixel work on the device.

CPU: the 16-bit PNG decoder against PIL, the annotation assembly and the compressed RLE string from numpy-computed statistics
and change points, the file listing and the command line.  GPU (-m gpu): csrc/instance_maps.hip byte-equal to the numpy
oracle below, twice, and the tool end to end.

The oracle is numpy: per id ``np.nonzero(map == id)`` for the box and the area, ``np.diff`` over ``map.T.reshape(-1)`` (the
column-major flattening, COCO RLE's order) for the change points."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_ID = 24


@functools.lru_cache(None)
def tool():
    spec = importlib.util.spec_from_file_location('cityscapes_converter_tool',
                                                  os.path.join(ROOT, 'tools', 'dataset_converters', 'cityscapes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lib():
    from oadg_amd import _lib as B
    return B, B.lib()


# ----------------------------------------------------------------------------------------------------------- oracle
def oracle_stats(m, min_id=MIN_ID):
    """int32 [r, 6]: (id, pixel count, xmin, ymin, xmax, ymax) for every id >= min_id of the map, ascending (np.unique)"""
    ids = np.unique(m[m >= min_id])
    if len(ids) <= 512:
        rows = []
        for k in ids:
            ys, xs = np.nonzero(m == k)
            rows.append((int(k), len(ys), xs.min(), ys.min(), xs.max(), ys.max()))
        return np.array(rows, dtype=np.int32).reshape(-1, 6)
    # thousands of ids (the permutation case): the same minima and maxima, grouped by one stable sort instead of one
    # comparison of the whole map per id
    ys, xs = np.nonzero(m >= min_id)
    v = m[ys, xs].astype(np.int64)
    order = np.argsort(v, kind='stable')
    v, ys, xs = v[order], ys[order], xs[order]
    first = np.nonzero(np.r_[True, v[1:] != v[:-1]])[0]
    assert np.array_equal(v[first], ids)
    cnt = np.diff(np.r_[first, len(v)])
    return np.stack([v[first], cnt, np.minimum.reduceat(xs, first), np.minimum.reduceat(ys, first),
                     np.maximum.reduceat(xs, first), np.maximum.reduceat(ys, first)], axis=1).astype(np.int32)


def oracle_points(m, min_id=MIN_ID):
    """int32 [c, 3]: (p, f[p-1], f[p]) for every p >= 1 where the column-major flattening f changes and either side is
    >= min_id, ascending p"""
    f = m.T.reshape(-1).astype(np.int64)
    p = np.nonzero(np.diff(f))[0] + 1
    p = p[np.maximum(f[p], f[p - 1]) >= min_id]
    return np.stack([p, f[p - 1], f[p]], axis=1).astype(np.int32).reshape(-1, 3)


def direct_runs(mask):
    """COCO run lengths (zeros first) of a binary mask by walking its column-major pixels one by one"""
    counts, value, run = [], 0, 0
    for b in mask.T.reshape(-1).tolist():
        if b != value:
            counts.append(run)
            value, run = b, 0
        run += 1
    counts.append(run)
    return counts


def runs_from_points(points, f0, k, HW):
    """the issue's construction: differences of [0, the change points of k..., H*W], a leading 0 when f[0] == k"""
    pts = [int(p) for p, a, b in points.tolist() if a == k or b == k]
    counts = np.diff([0] + pts + [HW]).tolist()
    return ([0] if f0 == k else []) + counts


def rle_from_string(s):
    """independent decoder of COCO's compressed RLE string, from the format's description: bytes minus 48 are groups of 5
    payload bits (low group first) with 0x20 = another group follows; the last group's 0x10 bit is the sign, extended
    upwards; from the fourth value on, the value is a difference from the count two places back"""
    counts, data, i = [], s.encode('ascii'), 0
    while i < len(data):
        x, k = 0, 0
        while True:
            c = data[i] - 48
            assert 0 <= c < 64
            i += 1
            x |= (c & 0x1f) << (5 * k)
            k += 1
            if not c & 0x20:
                if c & 0x10:
                    x -= 1 << (5 * k)
                break
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def mask_from_runs(counts, H, W):
    flat = np.zeros(H * W, dtype=np.uint8)
    pos, value = 0, 0
    for c in counts:
        flat[pos:pos + c] = value
        pos, value = pos + c, 1 - value
    assert pos == H * W
    return flat.reshape(W, H).T


# ------------------------------------------------------------------------------------------------------------ cases
def blobs(seed, H, W, ids, max_size, background=(7, 8, 11, 21, 23)):
    """stuff stripes with one ellipse per id painted over them (later blobs may cover earlier ones)"""
    rs = np.random.RandomState(seed)
    m = np.empty((H, W), dtype=np.uint16)
    edges = np.linspace(0, H, len(background) + 1).astype(int)
    for k, b in enumerate(background):
        m[edges[k]:edges[k + 1]] = b
    for k in ids:
        h, w = rs.randint(1, max_size + 1, 2)
        y0, x0 = rs.randint(0, max(1, H - h + 1)), rs.randint(0, max(1, W - w + 1))
        h, w = min(h, H - y0), min(w, W - x0)
        yy, xx = np.mgrid[0:h, 0:w]
        inside = ((yy - (h - 1) / 2) / (h / 2)) ** 2 + ((xx - (w - 1) / 2) / (w / 2)) ** 2 <= 1.0
        m[y0:y0 + h, x0:x0 + w][inside] = k
    return m


def instance_ids(seed, count):
    rs = np.random.RandomState(seed)
    labels = rs.choice([24, 25, 26, 27, 28, 29, 31, 32, 33], count)
    return [int(l) * 1000 + i for i, l in enumerate(labels)]


def hand_case():
    """13 x 9 (H x W): see test_hand_case_construction_equals_a_direct_run_length_pass"""
    m = np.full((13, 9), 7, dtype=np.uint16)
    m[:, 5:] = 11
    m[8:, 6:] = 23                                   # stuff ids below 24: never reported
    m[0:3, 0:2] = 26001                              # an instance at pixel 0
    m[10:13, 3] = 24002                              # the bottom of column 3 ...
    m[0:3, 4] = 24002                                # ... runs on into the top of column 4: ONE run, box height H
    m[11:13, 8] = 33005                              # an instance at the last pixel
    m[6, 6] = 25                                     # a one-pixel crowd region
    m[5, 1] = 65535                                  # the largest id
    return m


@functools.lru_cache(None)
def case(name):
    """name -> (maps uint16 [n, H, W], [oracle_stats per map], [oracle_points per map]); computed once, never modified"""
    if name == '1x1':
        maps = np.array([[[26001]]], dtype=np.uint16)
    elif name == '1x1_stuff':
        maps = np.array([[[7]]], dtype=np.uint16)
    elif name == '5x7':
        maps = np.random.RandomState(1).choice([7, 23, 24, 25, 26001, 26002, 33000], (1, 5, 7)).astype(np.uint16)
    elif name == 'hand':
        maps = hand_case()[None]
    elif name == '64x33':
        maps = blobs(2, 64, 33, instance_ids(2, 12) + [24, 26], 20)[None]
    elif name == '33x64':
        maps = blobs(3, 33, 64, instance_ids(3, 12) + [25], 20)[None]
    elif name == '257x130':
        maps = blobs(4, 257, 130, instance_ids(4, 300), 12)[None]
        assert len(np.unique(maps[maps >= MIN_ID])) > 256
    elif name == 'permutation':
        maps = np.random.RandomState(5).permutation(65536).astype(np.uint16).reshape(1, 256, 256)
    elif name == 'batch3':                           # 13 * 9 is odd: maps 1 and 2 start off a 16-byte boundary
        maps = np.stack([hand_case(), blobs(6, 13, 9, instance_ids(6, 5), 6), blobs(7, 13, 9, [25, 31007], 9)])
    elif name == 'batch3_33x64':
        maps = np.stack([blobs(8 + i, 33, 64, instance_ids(8 + i, 6 + 5 * i), 16) for i in range(3)])
    elif name == '1024x2048':
        maps = blobs(9, 1024, 2048, instance_ids(9, 60) + [24, 25], 300,
                     background=(23, 21, 11, 8, 7, 7))[None]
    else:
        raise KeyError(name)
    maps = np.ascontiguousarray(maps)
    maps.setflags(write=False)
    return maps, [oracle_stats(m) for m in maps], [oracle_points(m) for m in maps]


# ------------------------------------------------------------------------------------------------- CPU: PNG decoder
def _decode16(path, H, W):
    B, L = _lib()
    out = np.full((H, W), 0xabcd, dtype=np.uint16)
    rc = L.oadg_png_decode_gray16(str(path).encode(), out.ctypes.data, H, W)
    return rc, out


@pytest.mark.parametrize('H,W', [(1, 1), (5, 7), (64, 33), (1024, 2048)])
def test_gray16_png_equals_pil(tmp_path, H, W):
    from PIL import Image
    if H * W > 10000:
        a = blobs(11, H, W, instance_ids(11, 40), 300)
    else:
        a = np.random.RandomState(H * W).randint(0, 65536, (H, W)).astype(np.uint16)
        a.flat[0] = 0x0102                                                    # byte order shows
    p = tmp_path / 'a.png'
    Image.fromarray(a).save(p)
    with Image.open(p) as im:
        assert im.mode == 'I;16'
        want = np.asarray(im).astype(np.uint16)
    assert np.array_equal(want, a)
    rc, got = _decode16(p, H, W)
    assert rc == 0 and np.array_equal(got, want)


def test_gray16_png_widens_8_bit_and_reports_what_it_declines(tmp_path):
    from PIL import Image
    a = np.random.RandomState(0).randint(0, 256, (9, 13)).astype(np.uint8)
    Image.fromarray(a).save(tmp_path / 'g8.png')
    rc, got = _decode16(tmp_path / 'g8.png', 9, 13)
    assert rc == 0 and np.array_equal(got, a.astype(np.uint16))
    Image.fromarray(np.zeros((9, 13, 3), np.uint8)).save(tmp_path / 'rgb.png')
    assert _decode16(tmp_path / 'rgb.png', 9, 13)[0] == -4                    # OADG_EUNSUPPORTED
    assert _decode16(tmp_path / 'g8.png', 13, 9)[0] == -2                     # OADG_ESIZE
    assert _decode16(tmp_path / 'missing.png', 9, 13)[0] == -3                # OADG_EIO
    rc, untouched = _decode16(tmp_path / 'rgb.png', 9, 13)
    assert (untouched == 0xabcd).all()


# ------------------------------------------------------------------------------------- CPU: annotations and the string
def test_hand_case_construction_equals_a_direct_run_length_pass():
    m = hand_case()
    H, W = m.shape
    stats, points = oracle_stats(m), oracle_points(m)
    assert stats[:, 0].tolist() == [25, 24002, 26001, 33005, 65535]           # no stuff id, ascending
    by_id = {r[0]: r[1:].tolist() for r in stats}
    assert by_id[24002] == [6, 3, 0, 4, 12]                                   # ymin 0, ymax H - 1: box height H
    assert by_id[25] == [1, 6, 6, 6, 6]
    assert not (set(points[:, 1]) | set(points[:, 2])) - {7, 11, 23, 25, 24002, 26001, 33005, 65535}
    for k in stats[:, 0].tolist():
        want = direct_runs(m == k)
        assert runs_from_points(points, int(m[0, 0]), k, H * W) == want, k
    assert direct_runs(m == 24002) == [3 * 13 + 10, 6, H * W - 3 * 13 - 16]   # the wrap is one run
    assert direct_runs(m == 26001)[0] == 0 and direct_runs(m == 33005)[-1] == 2


def assembly_map(extra=()):
    m = np.full((40, 50), 7, dtype=np.uint16)
    m[:, 30:] = 21
    for i, k in enumerate((23, 24, 25, 29, 30, 33, 26001, 29003, 30001, 33999) + tuple(extra)):
        m[3 * i:3 * i + 4 + i % 3, 4 * i:4 * i + 5] = k
    m[0, 0] = 26001                                                            # the car's mask starts at pixel 0
    return m


def test_annotations_keep_drop_crowd_types_and_order():
    T = tool()
    m = assembly_map()
    H, W = m.shape
    annos = T.annotations_of_map(oracle_stats(m), oracle_points(m), int(m[0, 0]), H, W, 'x_gtFine_instanceIds.png')
    kept = [24, 25, 33, 26001, 33999]                                          # ascending ids; 23 stuff, 29/30 ignored in eval
    assert [a['category_id'] for a in annos] == [24, 25, 33, 26, 33]
    assert [a['iscrowd'] for a in annos] == [1, 1, 1, 0, 0]
    for a, k in zip(annos, kept):
        ys, xs = np.nonzero(m == k)
        assert a['bbox'] == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
        assert all(type(v) is float for v in a['bbox']) and type(a['area']) is int and a['area'] == len(ys)
        assert a['segmentation']['size'] == [H, W] and isinstance(a['segmentation']['counts'], str)
        runs = rle_from_string(a['segmentation']['counts'])
        assert runs == direct_runs(m == k)
        assert np.array_equal(mask_from_runs(runs, H, W), m == k)
        assert set(a) == {'iscrowd', 'category_id', 'bbox', 'area', 'segmentation'}
    assert rle_from_string(annos[3]['segmentation']['counts'])[0] == 0


def test_a_label_outside_the_table_names_the_file_and_the_id():
    T = tool()
    m = assembly_map(extra=(65535,))
    with pytest.raises(ValueError, match=r'some_gtFine_instanceIds\.png.*65535'):
        T.annotations_of_map(oracle_stats(m), oracle_points(m), int(m[0, 0]), 40, 50, 'some_gtFine_instanceIds.png')
    with pytest.raises(ValueError, match='34'):
        T.label_of(34)
    assert [T.label_of(k) for k in (24, 33, 26001, 33999, 1000)] == [24, 33, 26, 33, 1]


def test_json_assembly_running_ids_categories_and_the_dropped_key(tmp_path):
    T = tool()
    m = assembly_map()
    annos = T.annotations_of_map(oracle_stats(m), oracle_points(m), int(m[0, 0]), 40, 50)
    files = [(f'/d/leftImg8bit/train/{c}/{c}_{i}_leftImg8bit.png', f'/d/gtFine/train/{c}/{c}_{i}_gtFine_instanceIds.png',
              f'/d/gtFine/train/{c}/{c}_{i}_gtFine_labelIds.png') for c, i in (('aachen', 0), ('aachen', 1), ('bochum', 0))]
    infos = [T.image_info(files[0], 40, 50, annos), T.image_info(files[1], 40, 50, []), T.image_info(files[2], 40, 50, annos)]
    out = T.cvt_annotations(infos, str(tmp_path / 'o.json'))
    assert json.load(open(tmp_path / 'o.json')) == out
    assert out['images'][2] == dict(file_name='bochum/bochum_0_leftImg8bit.png', height=40, width=50, id=2,
                                    segm_file='bochum/bochum_0_gtFine_labelIds.png')
    assert [a['id'] for a in out['annotations']] == list(range(10))
    assert [a['image_id'] for a in out['annotations']] == [0] * 5 + [2] * 5
    assert out['categories'] == [dict(id=i, name=n) for i, n in (
        (24, 'person'), (25, 'rider'), (26, 'car'), (27, 'truck'), (28, 'bus'), (31, 'train'), (32, 'motorcycle'),
        (33, 'bicycle'))]
    empty = T.cvt_annotations([T.image_info(files[1], 40, 50, [])], None)
    assert 'annotations' not in empty and len(empty['images']) == 1 and len(empty['categories']) == 8


def test_file_listing_is_sorted_and_refuses_another_suffix(tmp_path):
    T = tool()
    img, gt = tmp_path / 'leftImg8bit' / 'val', tmp_path / 'gtFine' / 'val'
    for city, name in (('munster', 'munster_000002_000019'), ('frankfurt', 'frankfurt_000001_000019'),
                       ('frankfurt', 'frankfurt_000000_000294')):
        (img / city).mkdir(parents=True, exist_ok=True)
        (img / city / f'{name}_leftImg8bit.png').write_bytes(b'')
    files = T.collect_files(str(img), str(gt))
    assert [os.path.basename(f[0]) for f in files] == [
        'frankfurt_000000_000294_leftImg8bit.png', 'frankfurt_000001_000019_leftImg8bit.png',
        'munster_000002_000019_leftImg8bit.png']
    assert files[0][1] == str(gt / 'frankfurt' / 'frankfurt_000000_000294_gtFine_instanceIds.png')
    assert files[0][2] == str(gt / 'frankfurt' / 'frankfurt_000000_000294_gtFine_labelIds.png')
    (img / 'munster' / 'munster_000003_000019_rightImg8bit.png').write_bytes(b'')
    with pytest.raises(ValueError, match='munster_000003_000019_rightImg8bit.png'):
        T.collect_files(str(img), str(gt))
    with pytest.raises(ValueError, match='No images found'):
        T.collect_files(str(tmp_path / 'nothing'), str(gt))


def test_argument_parser_is_the_reference_surface():
    T = tool()
    a = T.parse_args(['/data/cityscapes'])
    assert vars(a) == dict(cityscapes_path='/data/cityscapes', img_dir='leftImg8bit', gt_dir='gtFine', out_dir=None, nproc=1)
    a = T.parse_args(['/d', '--img-dir', 'i', '--gt-dir', 'g', '-o', '/o', '--nproc', '8'])
    assert (a.img_dir, a.gt_dir, a.out_dir, a.nproc) == ('i', 'g', '/o', 8)
    assert T.parse_args(['/d', '--out-dir', '/p']).out_dir == '/p'
    assert T.SET_NAME == dict(train='instancesonly_filtered_gtFine_train.json', val='instancesonly_filtered_gtFine_val.json',
                              test='instancesonly_filtered_gtFine_test.json')


@pytest.mark.parametrize('counts', [
    [0, 5, 3],                                        # a mask that starts at pixel 0
    [40000, 70000, 33, 1 << 15, 1, 2, 1 << 20, 5],    # counts >= 2^15, negative and positive differences of every width
    [3, 1000, 2, 1, 900, 1016, 4, 15, 20, 16, 4, 31, 36],   # differences around the group boundaries: -16, -17, 15, 16, ...
    [7],
    [0, 1 << 30],
])
def test_rle_string_round_trips_through_an_independent_decoder(counts):
    s = tool().rle_to_string(counts)
    assert all(48 <= ord(ch) < 112 for ch in s)
    assert rle_from_string(s) == counts


def test_rle_string_of_known_small_values():
    # one group per value below 16: the byte is value + 48; 16 needs a second group (0x10 would read as a sign)
    assert tool().rle_to_string([0, 1, 15]) == '01?'
    assert tool().rle_to_string([16]) == chr(48 + 0x30) + chr(48)
    # the fourth value is stored as a difference: 2 - 5 = -3 -> 0x1d, no continuation
    assert tool().rle_to_string([4, 5, 6, 2]) == '456' + chr(48 + 0x1d)


# -------------------------------------------------------------------------------------------------------------- GPU
def run_kernels(dev, maps, cap_records, cap_points, min_id=MIN_ID, guard=64):
    """both entries on uint16 [n, H, W] -> (records int32 [n, cap, 6], counts, triples [n, cap, 3], counts, the guard words
    behind each output, which must still hold the fill value)"""
    import torch
    B, L = _lib()
    n, H, W = maps.shape
    d = torch.from_numpy(maps.view(np.int16).copy()).to(dev)
    ws_bytes = int(L.oadg_instance_maps_workspace_bytes(n, H, W))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rec = torch.full((n * cap_records * 6 + guard,), -7, dtype=torch.int32, device=dev)
    tri = torch.full((n * cap_points * 3 + guard,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((2, n), -7, dtype=torch.int32, device=dev)
    s = B.stream_ptr()
    B.check(L.oadg_instance_stats(B.ptr(d), n, H, W, min_id, B.ptr(rec), cap_records, B.ptr(counts[0]), B.ptr(ws), ws_bytes, s),
            'oadg_instance_stats')
    B.check(L.oadg_instance_change_points(B.ptr(d), n, H, W, min_id, B.ptr(tri), cap_points, B.ptr(counts[1]), B.ptr(ws),
                                          ws_bytes, s), 'oadg_instance_change_points')
    rec, tri, counts = rec.cpu().numpy(), tri.cpu().numpy(), counts.cpu().numpy()
    return (rec[:n * cap_records * 6].reshape(n, cap_records, 6), counts[0], tri[:n * cap_points * 3].reshape(n, cap_points, 3),
            counts[1], np.concatenate([rec[n * cap_records * 6:], tri[n * cap_points * 3:]]))


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['1x1', '1x1_stuff', '5x7', 'hand', '64x33', '33x64', '257x130', 'permutation', 'batch3',
                                  'batch3_33x64', '1024x2048'])
def test_kernels_equal_the_numpy_oracle_twice(dev, name):
    maps, stats, points = case(name)
    cap_r = max(1, max(len(s) for s in stats))
    cap_p = max(1, max(len(p) for p in points))
    first = run_kernels(dev, maps, cap_r, cap_p)
    rec, nrec, tri, ntri, guard = first
    assert nrec.tolist() == [len(s) for s in stats] and ntri.tolist() == [len(p) for p in points]
    for i in range(len(maps)):
        assert rec[i, :nrec[i]].tobytes() == stats[i].tobytes(), (name, i)
        assert tri[i, :ntri[i]].tobytes() == points[i].tobytes(), (name, i)
        assert (rec[i, nrec[i]:] == -7).all() and (tri[i, ntri[i]:] == -7).all()      # nothing behind the last entry
    assert (guard == -7).all()
    second = run_kernels(dev, maps, cap_r, cap_p)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    if name == 'permutation':
        assert nrec[0] == 65536 - MIN_ID and ntri[0] >= 65500                    # every pixel a change point
    if name == '1024x2048':
        assert 40 <= nrec[0] <= 62


@pytest.mark.gpu
@pytest.mark.parametrize('name,cap_r,cap_p', [('hand', 2, 5), ('257x130', 100, 1000), ('batch3_33x64', 7, 40),
                                              ('5x7', 0, 0)])
def test_a_short_capacity_is_reported_and_nothing_is_written_past_it(dev, name, cap_r, cap_p):
    maps, stats, points = case(name)
    rec, nrec, tri, ntri, guard = run_kernels(dev, maps, cap_r, cap_p)
    assert nrec.tolist() == [len(s) for s in stats] and ntri.tolist() == [len(p) for p in points]     # the needed counts
    assert max(nrec) > cap_r and max(ntri) > cap_p
    for i in range(len(maps)):
        kr, kp = min(cap_r, len(stats[i])), min(cap_p, len(points[i]))
        assert rec[i, :kr].tobytes() == stats[i][:kr].tobytes() and (rec[i, kr:] == -7).all()
        assert tri[i, :kp].tobytes() == points[i][:kp].tobytes() and (tri[i, kp:] == -7).all()
    assert (guard == -7).all()


@pytest.mark.gpu
def test_min_id_is_honoured_and_bad_shapes_are_refused(dev):
    import torch
    B, L = _lib()
    maps = case('5x7')[0]
    rec, nrec, tri, ntri, _ = run_kernels(dev, maps, 16, 64, min_id=0)
    assert rec[0, :nrec[0]].tobytes() == oracle_stats(maps[0], 0).tobytes()
    assert tri[0, :ntri[0]].tobytes() == oracle_points(maps[0], 0).tobytes()
    t = torch.zeros(64, dtype=torch.int32, device=dev)
    big = (1 << 16, 1 << 15)                                                   # H * W = 2^31: no launch, OADG_EARG
    assert L.oadg_instance_maps_workspace_bytes(1, *big) == 0
    for fn in (L.oadg_instance_stats, L.oadg_instance_change_points):
        assert fn(B.ptr(t), 1, big[0], big[1], 24, B.ptr(t), 1, B.ptr(t), B.ptr(t), 1 << 40, B.stream_ptr()) == -1
        assert fn(B.ptr(t), 1, 5, 7, 24, B.ptr(t), 1, B.ptr(t), B.ptr(t), 16, B.stream_ptr()) == -2      # workspace too small
        assert fn(B.ptr(t), 1, 5, 7, 1 << 16, B.ptr(t), 1, B.ptr(t), B.ptr(t), 1 << 40, B.stream_ptr()) == -1
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_tool_end_to_end_on_a_two_city_tree(dev, tmp_path, capsys):
    from PIL import Image
    from oadg_amd.datasets import CityscapesDataset
    T = tool()
    root = tmp_path / 'cityscapes'
    maps = {}
    for c, (city, stem) in enumerate((('aachen', 'aachen_000000_000019'), ('aachen', 'aachen_000001_000019'),
                                      ('bochum', 'bochum_000000_000313'), ('bochum', 'bochum_000000_000600'))):
        m = blobs(20 + c, 48, 64, instance_ids(20 + c, 5) + [24 + c % 3, 29001, 30002], 24).copy()
        m[40:48, 56:64] = 26000 + 900 + c                                      # at least one car that nothing covers
        m[0:4, 0:4] = 24 + c % 3                                               # and one crowd region
        (root / 'leftImg8bit' / 'train' / city).mkdir(parents=True, exist_ok=True)
        (root / 'gtFine' / 'train' / city).mkdir(parents=True, exist_ok=True)
        Image.fromarray(np.full((48, 64, 3), 90 + c, np.uint8)).save(root / 'leftImg8bit' / 'train' / city / f'{stem}_leftImg8bit.png')
        Image.fromarray(m).save(root / 'gtFine' / 'train' / city / f'{stem}_gtFine_instanceIds.png')
        Image.fromarray(np.minimum(m, 255).astype(np.uint8)).save(root / 'gtFine' / 'train' / city / f'{stem}_gtFine_labelIds.png')
        maps[f'{city}/{stem}_leftImg8bit.png'] = m
    out = tmp_path / 'annotations'
    T.main([str(root), '-o', str(out), '--nproc', '2'])
    said = capsys.readouterr().out
    assert 'Skipping val' in said and 'Skipping test' in said and 'Loaded 4 images' in said
    assert os.listdir(out) == ['instancesonly_filtered_gtFine_train.json']
    ann_file = str(out / 'instancesonly_filtered_gtFine_train.json')
    data = json.load(open(ann_file))
    assert [i['file_name'] for i in data['images']] == sorted(maps) and [i['id'] for i in data['images']] == [0, 1, 2, 3]
    assert [a['id'] for a in data['annotations']] == list(range(len(data['annotations'])))
    for a in data['annotations']:                                              # masks: the string decodes to map == id
        m = maps[data['images'][a['image_id']]['file_name']]
        mask = mask_from_runs(rle_from_string(a['segmentation']['counts']), 48, 64)
        ids = np.unique(m[mask.astype(bool)])
        assert len(ids) == 1 and np.array_equal(mask, m == ids[0]) and a['area'] == int(mask.sum())
    ds = CityscapesDataset(ann_file=ann_file, img_prefix=str(root / 'leftImg8bit' / 'train'), device='cpu')
    assert len(ds) == 4
    kept = {24, 25, 26, 27, 28, 31, 32, 33}
    for idx in range(len(ds)):
        m = maps[ds.data_infos[idx]['file_name']]
        want, want_ignore, labels = [], [], []
        for r in oracle_stats(m).tolist():
            label = r[0] // 1000 if r[0] >= 1000 else r[0]
            if label in kept:
                box = [r[2], r[3], r[4] + 1, r[5] + 1]
                (want_ignore if r[0] < 1000 else want).append(box)
                if r[0] >= 1000:
                    labels.append(CityscapesDataset.CLASSES.index(dict(T.CATEGORIES)[label]))
        info = ds.get_ann_info(idx)
        assert np.array_equal(info['bboxes'], np.array(want, np.float32).reshape(-1, 4))
        assert np.array_equal(info['bboxes_ignore'], np.array(want_ignore, np.float32).reshape(-1, 4))
        assert info['labels'].tolist() == labels and len(want) >= 1 and len(want_ignore) >= 1
