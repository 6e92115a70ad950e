"""csrc/jpeg_decode.hip and csrc/png_decode.hip on the files of tests/jpeg_cases.py: legal files no common encoder writes,
files the decoders decline, malformed files, every prefix of a JPEG and every single-byte damage to its header.  PIL
(libjpeg-turbo, zlib) is the judge: a decode that returns OADG_OK equals PIL's bytes, anything else is an exact return code
(or, for malformed files, one of the three rejecting codes).  Every call writes into buffers with 64 guard bytes of 0xA5 on
each side, checked after every call.  The CPU half runs the host stages; the GPU half gives the device pixel stage the
descriptors those produce - rare files, batches mixed with rejected files, output pointers that are only byte-aligned."""
import ctypes
import json

import numpy as np
import pytest

import jpeg_cases as J
from jpeg_cases import EUNSUPPORTED, OK, REJECT

GUARD, FILL = 64, 0xA5
DESC_BYTES = 672


def _lib():
    from oadg_amd import _lib as lib
    return lib.lib()


class Guarded:
    """``n`` bytes in the middle of an allocation filled with 0xA5, 64 guard bytes on each side"""

    def __init__(self, n):
        self.n = n
        self.whole = np.full(n + 2 * GUARD, FILL, np.uint8)
        self.data = self.whole[GUARD:GUARD + n]

    @property
    def ptr(self):
        return self.data.ctypes.data

    def intact(self):
        return bool((self.whole[:GUARD] == FILL).all() and (self.whole[GUARD + self.n:] == FILL).all())


class Host:
    """the host entry points on one file, every buffer guarded"""

    def __init__(self, tmp_path):
        self.L = _lib()
        self.path = str(tmp_path / 'case.bin')

    def write(self, raw):
        with open(self.path, 'wb') as f:
            f.write(raw)
        return self.path.encode()

    def jpeg(self, raw, h, w):
        """(rc of the host twin, its pixels, rc of the entropy stage, ncomp it left)"""
        p = self.write(raw)
        out = Guarded(h * w * 3)
        rc = self.L.oadg_jpeg_decode_bgr(p, out.ptr, h, w)
        assert out.intact(), 'oadg_jpeg_decode_bgr wrote outside out'
        cap = int(self.L.oadg_jpeg_coef_capacity(h, w))
        coef, desc = Guarded(2 * cap), Guarded(DESC_BYTES)
        rc2 = self.L.oadg_jpeg_entropy_decode(p, h, w, coef.ptr, cap, desc.ptr)
        assert coef.intact() and desc.intact(), 'oadg_jpeg_entropy_decode wrote outside its buffers'
        return rc, out.data.reshape(h, w, 3), rc2, int(desc.data[8:12].view(np.int32)[0])

    def jpeg_size(self, raw):
        hh, ww = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = self.L.oadg_jpeg_size(self.write(raw), ctypes.byref(hh), ctypes.byref(ww))
        return rc, (ww.value, hh.value)

    def png(self, raw, kind, h, w):
        p = self.write(raw)
        if kind == 'png16':
            out = Guarded(h * w * 2)
            rc = self.L.oadg_png_decode_gray16(p, out.ptr, h, w)
            px = out.data.view(np.uint16).reshape(h, w)
        else:
            out = Guarded(h * w * 3)
            rc = self.L.oadg_png_decode_bgr(p, out.ptr, h, w)
            px = out.data.reshape(h, w, 3)
        assert out.intact(), 'the PNG decoder wrote outside out'
        return rc, px


@pytest.fixture
def host(tmp_path):
    return Host(tmp_path)


# ---------------------------------------------------------------------------------------------------------------- JPEG
def test_editor_round_trip():
    """split + join give the file back, and the bases are what the tables assume"""
    for h, w in J.SIZES:
        for sub in (2, 1, 0, 'L'):
            raw = J.base(h, w, sub)
            assert J.join(*J.split(raw)) == raw
            assert b'\xff\xdd' in raw


def test_legal_rare_jpegs_equal_pil(host):
    bad = []
    for name, raw, h, w, want in J.legal_cases():
        assert want == OK
        ref = J.pil_bgr(raw)
        assert ref is not None and ref.shape == (h, w, 3), name
        rc, px, rc2, ncomp = host.jpeg(raw, h, w)
        size = host.jpeg_size(raw)
        if rc != OK or rc2 != OK or ncomp not in (1, 3) or not np.array_equal(px, ref) or size != (OK, J.pil_size(raw)):
            bad.append((name, rc, rc2, ncomp, size))
    assert not bad, bad


def test_edited_files_decode_to_the_unedited_pixels():
    """the edits of the legal table change no pixel for PIL either (so they test the parser, not the picture)"""
    for h, w in J.SIZES:
        tag = f'_{h}x{w}'
        cases = {n[:-len(tag)]: raw for n, raw, hh, ww, _ in J.legal_cases() if n.endswith(tag)}
        refs = {k: J.pil_bgr(cases['base_' + k]) for k in ('420', '444', 'grey')}
        for name, raw in cases.items():
            if name.startswith(('base_', 'dri_', 'hand_')):
                continue
            k = 'grey' if name.startswith('grey_') else ('444' if name.endswith('_444') else '420')
            assert np.array_equal(J.pil_bgr(raw), refs[k]), name


def test_declined_jpegs(host):
    bad = []
    for name, raw, h, w, want in J.declined_cases():
        assert want == EUNSUPPORTED
        rc, _, rc2, ncomp = host.jpeg(raw, h, w)
        if (rc, rc2, ncomp) != (EUNSUPPORTED, EUNSUPPORTED, 0):
            bad.append((name, rc, rc2, ncomp))
    assert not bad, bad


def test_malformed_jpegs_are_never_decoded(host):
    bad = []
    for name, raw, h, w, want in J.malformed_cases():
        want = want if isinstance(want, tuple) else (want,)
        assert OK not in want
        rc, _, rc2, ncomp = host.jpeg(raw, h, w)
        if rc not in want or rc2 not in want or ncomp != 0:
            bad.append((name, rc, rc2, ncomp))
    assert not bad, bad


def _swept(host, raw):
    """the rule of both sweeps: OK implies that PIL loads the file and the bytes are equal; True = decoded"""
    rc, px, rc2, ncomp = host.jpeg(raw, 16, 16)
    assert rc == rc2 and (ncomp != 0) == (rc == OK)
    if rc == OK:
        ref = J.pil_bgr(raw)
        assert ref is not None, 'decoded a file PIL does not load'
        assert ref.shape == px.shape and np.array_equal(px, ref), 'decoded other bytes than PIL'
        return True
    assert rc in REJECT, rc
    return False


def test_no_prefix_of_a_file_decodes(host):
    for n, raw in enumerate(J.prefix_sweep()):
        assert not _swept(host, raw), n


def test_header_byte_sweep(host):
    """every header byte set to 0x00, 0xFF, b ^ 1, b ^ 0x80: decoded exactly as PIL decodes it, or rejected - and both
    happen at least 100 times (the quantizer bytes give the first, counts, lengths and markers the second)"""
    accepted = rejected = 0
    for p, v, raw in J.header_sweep():
        try:
            if _swept(host, raw):
                accepted += 1
            else:
                rejected += 1
        except AssertionError as e:
            raise AssertionError(f'offset {p} set to {v:#04x}: {e}') from None
    print(f'header sweep: {accepted} mutants decoded and equal to PIL, {rejected} rejected')
    assert accepted >= 100 and rejected >= 100, (accepted, rejected)


def test_coefficient_sweep(host):
    """coefficients and quantizers far beyond an encoder's, where libjpeg-turbo's C and SIMD IDCT stop agreeing (16-bit
    lanes and saturating packs against ints and a wrapping range limit): whatever is decoded equals PIL, the rest is
    declined; both happen"""
    accepted = rejected = 0
    for n, raw in enumerate(J.coefficient_sweep()):
        try:
            if _swept(host, raw):
                accepted += 1
            else:
                rejected += 1
        except AssertionError as e:
            raise AssertionError(f'file {n}: {e}') from None
    print(f'coefficient sweep: {accepted} files decoded and equal to PIL, {rejected} rejected')
    assert accepted >= 100 and rejected >= 100, (accepted, rejected)


# ----------------------------------------------------------------------------------------------------------------- PNG
def _png_table(host, cases):
    bad = []
    for name, kind, raw, h, w, want in cases:
        rc, px = host.png(raw, kind, h, w)
        if want == OK:
            ref = J.pil_png(raw, kind)
            assert ref is not None and ref.shape == px.shape, name
            if rc != OK or not np.array_equal(px, ref):
                bad.append((name, rc))
        elif rc not in (want if isinstance(want, tuple) else (want,)):
            bad.append((name, rc))
    assert not bad, bad


def test_png_writer_is_read_by_pil_as_written():
    """the pure-Python writer's filters are right: PIL reads back the raw rows for every filter type"""
    rows = J.png_rows(1, 7, 9, 3)
    for ft in range(5):
        got = J.pil_png(J.png_file(7, 9, J.RGB, 8, J.png_stream(rows, [ft] * 7, 3)), 'png')
        assert np.array_equal(got[:, :, ::-1].reshape(7, -1), np.frombuffer(b''.join(rows), np.uint8).reshape(7, -1)), ft


def test_png_every_filter_at_every_pixel_width(host):
    cases = J.png_filter_cases()
    assert len(cases) == 4 * 4 * 5 * 2
    _png_table(host, cases)


def test_png_split_idat_and_ancillary_chunks(host):
    _png_table(host, J.png_legal_cases())


def test_png_chunks_between_idats_are_declined_as_pil_rejects_them(host):
    cases = J.png_between_cases()
    for name, kind, raw, h, w, _ in cases:
        assert J.pil_png(raw, kind) is None, name
    _png_table(host, cases)


def test_png_declined(host):
    _png_table(host, J.png_declined_cases())
    # the 16-bit entry point takes grey only
    name, kind, raw, h, w, _ = [c for c in J.png_filter_cases() if c[0] == 'rgb_7x9_f4_all'][0]
    assert host.png(raw, 'png16', h, w)[0] == EUNSUPPORTED


def test_png_malformed(host):
    _png_table(host, J.png_malformed_cases())


# ------------------------------------------------------------------------------------------------------------- GPU half
def _entropy_batch(files, h, w):
    """pinned descriptors + coefficient slots of a batch, as CocoDataset._batch_jpeg lays them out; the return codes"""
    import torch
    L = _lib()
    n, slot = len(files), int(L.oadg_jpeg_coef_capacity(h, w))
    host = torch.zeros(n * DESC_BYTES + 2 * n * slot, dtype=torch.uint8).pin_memory()
    base = host.numpy().ctypes.data
    rcs = [L.oadg_jpeg_entropy_decode(p.encode(), h, w, base + n * DESC_BYTES + 2 * i * slot, slot, base + i * DESC_BYTES)
           for i, p in enumerate(files)]
    return host, slot, rcs


def _write_all(tmp_path, cases):
    paths = []
    for k, (name, raw, h, w, _) in enumerate(cases):
        p = tmp_path / f'{k}_{name}.jpg'
        p.write_bytes(raw)
        paths.append(str(p))
    return paths


def _pixels(dev, host, slot, out):
    import torch
    from oadg_amd import hip_ops
    assert hip_ops.JPEG_DESC_BYTES == DESC_BYTES
    n = out.shape[0]
    d = host.to(dev)
    hip_ops.jpeg_pixels_bgr(d[n * DESC_BYTES:].view(torch.int16), d[:n * DESC_BYTES], out, slot)
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', J.SIZES)
def test_device_stage_on_rare_legal_files(dev, tmp_path, h, w):
    import torch
    cases = [c for c in J.legal_cases() if (c[2], c[3]) == (h, w)]
    paths = _write_all(tmp_path, cases)
    host, slot, rcs = _entropy_batch(paths, h, w)
    assert rcs == [OK] * len(cases)
    got = _pixels(dev, host, slot, torch.zeros((len(cases), h, w, 3), dtype=torch.uint8, device=dev))
    bad = [c[0] for i, c in enumerate(cases) if not np.array_equal(got[i], J.pil_bgr(c[1]))]
    assert not bad, bad


@pytest.mark.gpu
def test_device_batch_of_good_and_rejected_files(dev, tmp_path):
    """good files interleaved with declined and malformed ones: the good images equal PIL, the rows of the others keep
    the pattern the output held"""
    import torch
    good = [c for c in J.legal_cases() if (c[2], c[3]) == (16, 16)]
    rejected = [c for c in J.declined_cases() + J.malformed_cases() if (c[2], c[3]) == (16, 16)]
    assert len(rejected) > len(good) > 30
    cases = [c for pair in zip(good, rejected) for c in pair] + rejected[len(good):]
    paths = _write_all(tmp_path, cases)
    host, slot, rcs = _entropy_batch(paths, 16, 16)
    n = len(cases)
    ncomp = host.numpy()[:n * DESC_BYTES].reshape(n, DESC_BYTES)[:, 8:12].copy().view(np.int32)[:, 0]
    for c, rc, k in zip(cases, rcs, ncomp):
        assert (rc == OK and k in (1, 3)) if c[4] == OK else (rc in REJECT and k == 0), (c[0], rc, k)
    pattern = (np.arange(n * 16 * 16 * 3, dtype=np.int64) * 7 % 251).astype(np.uint8).reshape(n, 16, 16, 3)
    got = _pixels(dev, host, slot, torch.from_numpy(pattern).to(dev))
    bad = [c[0] for i, c in enumerate(cases)
           if not np.array_equal(got[i], J.pil_bgr(c[1]) if c[4] == OK else pattern[i])]
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize('offset', [1, 2, 3])
def test_device_stage_into_a_byte_aligned_output(dev, tmp_path, offset):
    """W % 4 == 0 with an output pointer that is not 4-byte aligned: the byte-store branch of the colour kernel"""
    import torch
    cases = [c for c in J.legal_cases() if c[0] in ('base_420_16x16', 'base_422_16x16', 'base_444_16x16', 'base_grey_16x16',
                                                    'fill2_16x16')]
    assert len(cases) == 5
    paths = _write_all(tmp_path, cases)
    host, slot, rcs = _entropy_batch(paths, 16, 16)
    assert rcs == [OK] * 5
    nbytes = 5 * 16 * 16 * 3
    whole = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 4 == 0
    out = whole[GUARD + offset:GUARD + offset + nbytes].view(5, 16, 16, 3)
    assert out.data_ptr() % 4 == offset
    got = _pixels(dev, host, slot, out)
    for i, c in enumerate(cases):
        assert np.array_equal(got[i], J.pil_bgr(c[1])), c[0]
    w = whole.cpu().numpy()
    assert (w[:GUARD + offset] == FILL).all() and (w[GUARD + offset + nbytes:] == FILL).all()


@pytest.mark.gpu
def test_dataset_batch_counts_native_and_pil(dev, tmp_path):
    """CocoDataset.batch over a plain file, rare legal ones, every declined file PIL still decodes, and a PNG"""
    from oadg_amd.datasets import CocoDataset
    legal = {c[0]: c for c in J.legal_cases()}
    files = [('plain.jpg', legal['base_420_16x16'][1], True)]
    files += [(f'{n}.jpg', legal[n][1], True) for n in ('fill3_16x16', 'dht_twice_16x16', 'grey_factors_41_16x16',
                                                        'adobe0_with_jfif_420_16x16', 'no_jfif_ids123_444_16x16')]
    declined = [(f'{c[0]}.jpg', c[1], False) for c in J.declined_cases() if (c[2], c[3]) == (16, 16) and
                J.pil_bgr(c[1]) is not None]
    assert {'no_jfif_ids_rgb_16x16.jpg', 'adobe0_no_jfif_16x16.jpg', 'keep_rgb_16x16.jpg'} <= {d[0] for d in declined}
    files += declined
    files.append(('average.png', J.png_file(16, 16, J.RGB, 8, J.png_stream(J.png_rows(5, 16, 16, 3), [3] * 16, 3)), False))
    for name, raw, _ in files:
        (tmp_path / name).write_bytes(raw)
    images = [dict(id=i, file_name=f[0], height=16, width=16) for i, f in enumerate(files)]
    anns = [dict(id=i, image_id=i, category_id=1, iscrowd=0, area=16.0, bbox=[1.0, 1.0, 4.0, 4.0]) for i in range(len(files))]
    with open(tmp_path / 'ann.json', 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name='car')]), f)
    # (test_mode: the training filter drops images under 32 pixels)
    ds = CocoDataset(ann_file=str(tmp_path / 'ann.json'), img_prefix=str(tmp_path), classes=('car',), device=dev,
                     test_mode=True)
    assert len(ds.data_infos) == len(files)
    imgs, _, _ = ds.batch(range(len(files)))
    got = imgs.cpu().numpy()
    for i, (name, raw, _) in enumerate(files):
        ref = J.pil_png(raw, 'png') if name.endswith('.png') else J.pil_bgr(raw)
        assert np.array_equal(got[i], ref), name
    assert ds.jpeg_decodes == dict(native=sum(f[2] for f in files), pil=len(declined))
