"""Inputs of tests/test_decoder_robustness.py and of tests/native/decoder_corpus_main.cpp: JPEG files PIL's plain ``save``
never writes - legal ones that are rarely written, ones csrc/jpeg_decode.hip declines, malformed ones - made by editing the
segments of PIL-written baseline files, two sweeps over one base file, and PNG files from a small writer that puts a chosen
filter on every row.  Everything is generated (seeded); PIL (libjpeg-turbo, zlib) is the judge of every file.

A JPEG is handled as ``(segments, ecs)``: the ``(marker, payload)`` segments after SOI up to and including SOS, and the
entropy-coded bytes (restart markers included) up to EOI.  A segment given as plain ``bytes`` is written as it stands
(for length fields that lie).

Each case is ``(name, bytes, H, W, expected return code)``; ``REJECT`` as the code of a malformed file means "any of
OADG_EFORMAT, OADG_EUNSUPPORTED, OADG_ESIZE".
A PNG case is ``(name, kind, bytes, H, W, code)``, kind ``png`` (oadg_png_decode_bgr) or ``png16`` (oadg_png_decode_gray16).

    python tests/jpeg_cases.py --write DIR      every case, the sweeps and the PNG files, with DIR/manifest.txt
                                                (one ``kind path H W`` per line; kind = jpeg | png | png16)
"""
import io
import re
import struct
import sys
import zlib

import numpy as np

OK, EARG, ESIZE, EIO, EUNSUPPORTED, EFORMAT = 0, -1, -2, -3, -4, -5
REJECT = (EFORMAT, EUNSUPPORTED, ESIZE)
SOI, EOI = b'\xff\xd8', b'\xff\xd9'
SOF0, DHT, DQT, DRI, SOS, DNL, COM, APP0, APP1, APP13, APP14 = 0xC0, 0xC4, 0xDB, 0xDD, 0xDA, 0xDC, 0xFE, 0xE0, 0xE1, 0xED, 0xEE
SIZES = [(16, 16), (17, 33)]
BASE_KW = dict(quality=90, restart_marker_blocks=1)


# ------------------------------------------------------------------------------------------------------- segment editor
def split(raw):
    """JPEG bytes -> (segments up to and including SOS, entropy-coded bytes); the file ends with EOI"""
    assert raw[:2] == SOI and raw[-2:] == EOI
    segs, p = [], 2
    while True:
        assert raw[p] == 0xFF and raw[p + 1] not in (0x00, 0xFF), p
        m, n = raw[p + 1], struct.unpack('>H', raw[p + 2:p + 4])[0]
        segs.append((m, bytes(raw[p + 4:p + 2 + n])))
        p += 2 + n
        if m == SOS:
            return segs, bytes(raw[p:-2])


def segment_bytes(seg, length=None):
    if isinstance(seg, bytes):
        return seg
    m, payload = seg
    return bytes([0xFF, m]) + struct.pack('>H', len(payload) + 2 if length is None else length) + payload


def join(segs, ecs, tail=EOI, fill=0):
    """the file again; ``fill``: that many 0xFF fill bytes before every marker (RSTn and EOI included)"""
    pad = b'\xff' * fill
    if fill:
        ecs = re.sub(b'\xff([\xd0-\xd7])', lambda m: pad + m.group(0), ecs)
        tail = pad + tail
    return SOI + b''.join(pad + segment_bytes(s) for s in segs) + ecs + tail


def find(segs, marker, nth=0):
    return [i for i, s in enumerate(segs) if not isinstance(s, bytes) and s[0] == marker][nth]


def without(segs, marker):
    return [s for s in segs if isinstance(s, bytes) or s[0] != marker]


def patch(segs, i, offset, value):
    """a copy of segs with byte ``offset`` of segment i's payload set"""
    m, p = segs[i]
    p = bytearray(p)
    p[offset] = value
    return segs[:i] + [(m, bytes(p))] + segs[i + 1:]


def dqt_tables(segs):
    """every quantization table of the file, in order: (Pq, Tq, 64 values in zig-zag order)"""
    out = []
    for s in segs:
        if s[0] != DQT:
            continue
        p, i = s[1], 0
        while i < len(p):
            pq, tq = p[i] >> 4, p[i] & 15
            n = 64 * (pq + 1)
            v = list(struct.unpack('>64H', p[i + 1:i + 1 + n])) if pq else list(p[i + 1:i + 1 + n])
            out.append((pq, tq, v))
            i += 1 + n
    return out


def dqt_payload(tables):
    return b''.join(bytes([pq << 4 | tq]) + (struct.pack('>64H', *v) if pq else bytes(v)) for pq, tq, v in tables)


def dht_tables(segs):
    """every Huffman table of the file, in order: (Tc, Th, 16 counts, symbols)"""
    out = []
    for s in segs:
        if s[0] != DHT:
            continue
        p, i = s[1], 0
        while i < len(p):
            counts = list(p[i + 1:i + 17])
            out.append((p[i] >> 4, p[i] & 15, counts, bytes(p[i + 17:i + 17 + sum(counts)])))
            i += 17 + sum(counts)
    return out


def dht_payload(tables):
    return b''.join(bytes([tc << 4 | th]) + bytes(counts) + bytes(vals) for tc, th, counts, vals in tables)


def replace_tables(segs, marker, new_segments):
    """segs with every segment of ``marker`` removed and ``new_segments`` put where the first one stood"""
    at = find(segs, marker)
    rest = without(segs, marker)
    return rest[:at] + list(new_segments) + rest[at:]


# ------------------------------------------------------------------------------------------------------------ base files
def image(seed, h, w):
    """uint8 [h, w, 3]: a smooth ramp per channel plus noise"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[:h, :w]
    ramp = np.stack([(9 * x + 5 * y) % 256, (255 - 6 * x + 3 * y) % 256, (4 * x * y + 17) % 256], -1)
    return np.clip(ramp + rs.randint(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def pil_jpeg(a, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def base(h, w, sub=2, **kw):
    """the PIL-written base file: quality 90, a restart marker after every MCU; sub: 2 = 4:2:0, 1 = 4:2:2, 0 = 4:4:4,
    'L' = grey"""
    a = image(h * 100 + w, h, w)
    kw = dict(BASE_KW, **kw)
    return pil_jpeg(a[:, :, 1], **kw) if sub == 'L' else pil_jpeg(a, subsampling=sub, **kw)


def pil_bgr(raw):
    """PIL's pixels of the file as BGR, or None when PIL does not load it"""
    from PIL import Image
    try:
        with Image.open(io.BytesIO(raw)) as im:
            return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
    except Exception:       # noqa: BLE001 (PIL raises OSError, SyntaxError, ValueError, ... for broken files)
        return None


def pil_size(raw):
    from PIL import Image
    with Image.open(io.BytesIO(raw)) as im:
        return im.size


ADOBE = lambda transform: (APP14, b'Adobe\x00\x64\x00\x00\x00\x00' + bytes([transform]))        # noqa: E731


def with_ids(segs, ids):
    """component ids rewritten in SOF and SOS"""
    f, s = find(segs, SOF0), find(segs, SOS)
    for k, v in enumerate(ids):
        segs = patch(patch(segs, f, 6 + 3 * k, v), s, 1 + 2 * k, v)
    return segs


# --------------------------------------------------------------------------------------- hand-written entropy-coded data
# A 16 x 16 grey file (four blocks) whose Huffman tables and bits are written here, for streams no encoder emits.
HAND_DC = (0, 0, [0, 0, 0, 13] + [0] * 12, bytes(range(13)))                            # categories 0 .. 12, 4-bit codes
HAND_AC = (1, 0, [0, 0, 0, 8] + [0] * 12, bytes([0x00, 0xF0, 0x01, 0xF1, 0x11, 0x32, 0x0A, 0xE1]))


def canonical(table):
    """symbol -> (code, length) of a DHT table (T.81 annex C)"""
    out, code, k = {}, 0, 0
    for length, n in enumerate(table[2], 1):
        for _ in range(n):
            out[table[3][k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def amplitude(v):
    """(size, bits) of a coefficient value"""
    s = abs(v).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def hand_ecs(blocks):
    """blocks: list of (dc difference or ('cat', category, bits), [(run, value) or ('sym', symbol)], eob) -> stuffed bytes"""
    dc, ac = canonical(HAND_DC), canonical(HAND_AC)
    bits = []

    def put(v, n):
        bits.extend((v >> (n - 1 - i)) & 1 for i in range(n))
    for d, acs, eob in blocks:
        s, v = (d[1], d[2]) if isinstance(d, tuple) else amplitude(d)
        put(*dc[s])
        put(v, s)
        for item in acs:
            if item[0] == 'sym':
                put(*ac[item[1]])
            else:
                s, v = amplitude(item[1])
                put(*ac[item[0] << 4 | s])
                put(v, s)
        if eob:
            put(*ac[0x00])
    bits += [1] * (-len(bits) % 8)
    raw = bytes(int(''.join(map(str, bits[i:i + 8])), 2) for i in range(0, len(bits), 8))
    return raw.replace(b'\xff', b'\xff\x00')


def hand_file(blocks, q0=16, qt=None):
    qt = qt or [q0] + [64 if k == 18 else 1 + k % 3 for k in range(1, 64)]      # (zig-zag order)
    segs = [(APP0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00'), (DQT, dqt_payload([(0, 0, qt)])),
            (SOF0, struct.pack('>BHHB', 8, 16, 16, 1) + b'\x01\x11\x00'), (DHT, dht_payload([HAND_DC])),
            (DHT, dht_payload([HAND_AC])), (SOS, b'\x01\x01\x00\x00\x3f\x00')]
    return join(segs, hand_ecs(blocks))


PLAIN_BLOCKS = [(30, [(0, 1), (0, -1), (3, 2)], True), (-12, [(15, 1), (0, 513)], True), (0, [], True),
                (5, [('sym', 0xF0), ('sym', 0xF0), ('sym', 0xF0), (14, 1)], False)]      # (the last one ends at k = 63)


# ------------------------------------------------------------------------------------------------------------ the tables
def legal_cases():
    """decoded by PIL; csrc/jpeg_decode.hip must return OADG_OK and PIL's bytes"""
    out = []
    for h, w in SIZES:
        tag = f'{h}x{w}'
        raw = base(h, w)
        segs, ecs = split(raw)
        add = lambda name, data: out.append((f'{name}_{tag}', data, h, w, OK))      # noqa: E731
        for k in (1, 2, 3):
            add(f'fill{k}', join(segs, ecs, fill=k))
        add('trailing', raw + b'\x00\x01trailing bytes\xff\xd9\xff')
        extra = [(COM, b'a comment'), (APP1, b'Exif\x00\x00' + bytes(40)), (APP13, b'Photoshop 3.0\x008BIM' + bytes(20))]
        add('com_app1_app13', join(segs[:1] + extra + segs[1:], ecs))
        add('com_before_sos', join(segs[:-1] + extra + segs[-1:], ecs))
        icc = base(h, w, icc_profile=bytes(np.random.RandomState(1).randint(0, 256, 70000, dtype=np.uint8)))
        assert icc.count(b'ICC_PROFILE\x00') >= 2
        add('icc70k', icc)
        inner = base(24, 40)
        add('app1_holds_a_jpeg', join(segs[:1] + [(APP1, inner)] + segs[1:], ecs))
        # tables repacked
        q, t = dqt_tables(segs), dht_tables(segs)
        add('dqt_in_one', join(replace_tables(segs, DQT, [(DQT, dqt_payload(q))]), ecs))
        add('dht_in_one', join(replace_tables(segs, DHT, [(DHT, dht_payload(t))]), ecs))
        one_each = replace_tables(replace_tables(segs, DQT, [(DQT, dqt_payload([x])) for x in q]), DHT,
                                  [(DHT, dht_payload([x])) for x in t])
        add('table_per_segment', join(one_each, ecs))
        other_q = [(pq, tq, [min(255, v + 1 + k % 3) for k, v in enumerate(vals)]) for pq, tq, vals in q]
        add('dqt_twice', join(replace_tables(segs, DQT, [(DQT, dqt_payload(other_q)), (DQT, dqt_payload(q))]), ecs))
        add('dqt_twice_in_one', join(replace_tables(segs, DQT, [(DQT, dqt_payload(other_q + q))]), ecs))
        # (first definition of every slot: the table of the other slot of its class - valid, different)
        other_t = [(tc, 1 - th, c, v) for tc, th, c, v in t]
        add('dht_twice', join(replace_tables(segs, DHT, [(DHT, dht_payload(other_t)), (DHT, dht_payload(t))]), ecs))
        add('dht_twice_in_one', join(replace_tables(segs, DHT, [(DHT, dht_payload(other_t + t))]), ecs))
        tabs = [s for s in segs if s[0] in (DQT, DHT)]
        rest = [s for s in segs if s[0] not in (DQT, DHT)]
        f = find(rest, SOF0)
        add('tables_after_sof', join(rest[:f + 1] + tabs + rest[f + 1:], ecs))
        slot3 = [(DQT, dqt_payload([(0, 3, q[0][2])])), (DHT, dht_payload([(0, 3, t[0][2], t[0][3]), (1, 3, t[1][2], t[1][3])]))]
        add('unused_slot3', join(segs[:1] + slot3 + segs[1:], ecs))
        add('dqt16_in_sof0', join(replace_tables(segs, DQT, [(DQT, dqt_payload([(1, tq, v) for _, tq, v in q]))]), ecs))
        # restart intervals
        d = find(segs, DRI)
        add('dri_twice', join(segs[:d] + [(DRI, b'\x00\x07')] + segs[d:], ecs))
        plain_segs, plain_ecs = split(base(h, w, restart_marker_blocks=0))
        assert DRI not in [s[0] for s in plain_segs] and not re.search(b'\xff[\xd0-\xd7]', plain_ecs)
        add('dri_zero', join(plain_segs[:-1] + [(DRI, b'\x00\x00')] + plain_segs[-1:], plain_ecs))
        add('dri_beyond_mcus', join(plain_segs[:-1] + [(DRI, b'\x03\xe8')] + plain_segs[-1:], plain_ecs))
        # grey: the sampling factors of a one-component file mean nothing
        gsegs, gecs = split(base(h, w, 'L'))
        gf = find(gsegs, SOF0)
        assert gsegs[gf][1][5] == 1 and gsegs[gf][1][7] == 0x11
        for factors in (0x22, 0x12, 0x41, 0x44):
            add(f'grey_factors_{factors:02x}', join(patch(gsegs, gf, 7, factors), gecs))
        # colour space inference (jdapimin.c default_decompress_parms)
        for sub, stag in ((2, '420'), (0, '444')):
            ssegs, secs = split(base(h, w, sub))
            assert ssegs[0][0] == APP0 and ssegs[0][1][:5] == b'JFIF\x00'
            add(f'jfif_ids012_{stag}', join(with_ids(ssegs, (0, 1, 2)), secs))
            add(f'no_jfif_ids123_{stag}', join(ssegs[1:], secs))
            add(f'adobe0_with_jfif_{stag}', join(ssegs[:1] + [ADOBE(0)] + ssegs[1:], secs))
            add(f'adobe1_no_jfif_{stag}', join([ADOBE(1)] + ssegs[1:], secs))
        add('base_422', base(h, w, 1))
        add('base_444', base(h, w, 0))
        add('base_grey', base(h, w, 'L'))
        add('base_420', raw)
    out.append(('hand_written_16x16', hand_file(PLAIN_BLOCKS), 16, 16, OK))
    # four ZRL codes carry a block past coefficient 63 without writing one: libjpeg ends the block there, as we do
    out.append(('hand_written_zrl_to_the_end_16x16', hand_file(PLAIN_BLOCKS[:3] + [(5, [('sym', 0xF0)] * 4, False)]), 16, 16, OK))
    return out


def declined_cases():
    """OADG_EUNSUPPORTED: the data set decodes these with PIL (where PIL can)"""
    out = []
    for h, w in SIZES:
        tag = f'{h}x{w}'
        add = lambda name, data: out.append((f'{name}_{tag}', data, h, w, EUNSUPPORTED))      # noqa: E731
        segs, ecs = split(base(h, w, 0))
        add('no_jfif_ids_rgb', join(with_ids(segs[1:], b'RGB'), ecs))
        add('adobe0_no_jfif', join([ADOBE(0)] + segs[1:], ecs))
        add('keep_rgb', pil_jpeg(image(7, h, w), keep_rgb=True, **BASE_KW))
        segs, ecs = split(base(h, w))
        f = find(segs, SOF0)
        add('precision12', join(patch(segs, f, 0, 12), ecs))
        for m in (0xC9, 0xC3, 0xC5):
            add(f'sof_marker_{m:02x}', join(segs[:f] + [(m, segs[f][1])] + segs[f + 1:], ecs))
        add('height0', join(patch(patch(segs, f, 1, 0), f, 2, 0), ecs))
        add('dnl_after_scan', join(segs, ecs, tail=segment_bytes((DNL, struct.pack('>H', h))) + EOI))
        add('dnl_before_scan', join(segs[:-1] + [(DNL, struct.pack('>H', h))] + segs[-1:], ecs))
        s422, e422 = split(base(h, w, 1))
        f2 = find(s422, SOF0)
        assert s422[f2][1][7] == 0x21
        add('luma12_440', join(patch(s422, f2, 7, 0x12), e422))
        add('chroma21', join(patch(segs, f, 10, 0x21), ecs))
        add('chroma12_both', join(patch(patch(segs, f, 10, 0x12), f, 13, 0x12), ecs))
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(image(9, h, w)).convert('CMYK').save(buf, 'JPEG', **BASE_KW)
        add('cmyk', buf.getvalue())
        add('second_scan', join(segs, ecs, tail=segment_bytes(segs[-1]) + ecs + EOI))
    return out


def malformed_cases():
    """never OADG_OK; the entropy stage leaves ncomp 0"""
    out = []
    h, w = 16, 16
    raw = base(h, w)
    segs, ecs = split(raw)
    add = lambda name, data, rc=REJECT: out.append((name, data, h, w, rc))      # noqa: E731
    t = dht_tables(segs)
    assert [x[:2] for x in t] == [(0, 0), (1, 0), (0, 1), (1, 1)] and t[0][2][:3] == [0, 1, 5]

    def dht_with(k, table, **kw):
        """the file with Huffman table k replaced"""
        new = [(DHT, dht_payload([table if i == k else x])) for i, x in enumerate(t)]
        return join(replace_tables(segs, DHT, new), ecs, **kw)
    tc, th, counts, vals = t[0]
    add('dht_three_1bit_codes', dht_with(0, (tc, th, [3, 1, 2] + counts[3:], vals)))
    add('dht_255_1bit_codes_dc', dht_with(0, (0, 0, [255] + [0] * 15, bytes(255))))
    add('dht_255_1bit_codes_ac', dht_with(1, (1, 0, [255] + [0] * 15, bytes(range(255)))))
    add('dht_five_2bit_codes', dht_with(0, (tc, th, [0, 5, 1] + counts[3:], vals)))
    add('dht_three_1bit_codes_ac', dht_with(3, (1, 1, [sum(t[3][2][:3]), 0, 0] + t[3][2][3:], t[3][3])))
    big = (1, 0, [0] * 7 + [29] * 8 + [25], bytes(range(256)) + b'\x00')
    assert sum(big[2]) == 257
    add('dht_total_257', dht_with(1, big))
    d0 = find(segs, DHT)
    add('dht_shorter_than_counts', join(segs[:d0] + [(DHT, segs[d0][1][:-3])] + segs[d0 + 1:], ecs))
    add('dht_shorter_than_17', join(segs[:d0] + [(DHT, segs[d0][1][:9])] + segs[d0 + 1:], ecs))
    add('dht_tc2', dht_with(0, (2, 0, counts, vals)))
    add('dht_th4', dht_with(0, (0, 4, counts, vals)))
    add('dht_dc_symbol_16', dht_with(0, (tc, th, counts, vals[:-1] + b'\x10')))
    add('dht_all_ones_code', dht_with(0, (tc, th, [2] + [0] * 15, vals[:2])))
    add('dht_all_ones_code_8bit', dht_with(1, (1, 0, [1] * 7 + [2] + [0] * 8, t[1][3][:9])))
    q0 = find(segs, DQT)
    add('dqt_tq4', join(patch(segs, q0, 0, 0x04), ecs))
    add('dqt_pq2', join(patch(segs, q0, 0, 0x20), ecs))
    add('dqt_short', join(segs[:q0] + [(DQT, segs[q0][1][:40])] + segs[q0 + 1:], ecs))
    add('dqt_pq1_short', join(patch(segs, q0, 0, 0x10), ecs))
    f = find(segs, SOF0)
    sof = segs[f][1]
    put = lambda payload: join(segs[:f] + [(SOF0, payload)] + segs[f + 1:], ecs)      # noqa: E731
    add('sof_short_5', put(sof[:5]))
    add('sof_short_components', put(sof[:-1]))
    add('sof_0_components', put(sof[:5] + b'\x00'))
    add('sof_factor_0', join(patch(segs, f, 7, 0x02), ecs))
    add('sof_factor_5', join(patch(segs, f, 7, 0x52), ecs))
    add('sof_chroma_factor_0', join(patch(segs, f, 10, 0x10), ecs))
    add('sof_tq4', join(patch(segs, f, 8, 4), ecs))
    add('sof_width0', join(patch(patch(segs, f, 3, 0), f, 4, 0), ecs))
    add('sof_longer_than_its_components', put(sof + b'\x00'))
    add('sof_twice', join(segs[:f + 1] + [segs[f]] + segs[f + 1:], ecs))
    s = len(segs) - 1
    add('sos_before_sof', join(segs[:f] + [segs[s]] + segs[f:s], ecs))
    add('sos_before_sof_and_after', join(segs[:f] + [segs[s]] + segs[f:], ecs))
    add('sos_one_component', join(segs[:s] + [(SOS, b'\x01\x01\x00\x00\x3f\x00')], ecs))
    add('sos_count_2_of_3', join(patch(segs, s, 0, 2), ecs))
    add('sos_count_0', join(patch(segs, s, 0, 0), ecs))
    add('sos_unknown_id', join(patch(segs, s, 3, 9), ecs))
    add('sos_td4', join(patch(segs, s, 2, 0x40), ecs))
    add('sos_ta4', join(patch(segs, s, 4, 0x14), ecs))
    add('sos_table_never_defined', join(patch(segs, s, 4, 0x13), ecs))
    add('sos_dc_table_never_defined', join(patch(segs, s, 6, 0x21), ecs))
    add('sos_no_dht_at_all', join(without(segs, DHT), ecs))
    add('sos_no_dqt_at_all', join(without(segs, DQT), ecs))
    add('sos_ss1', join(patch(segs, s, 7, 1), ecs))
    add('sos_se62', join(patch(segs, s, 8, 62), ecs))
    add('sos_ahal', join(patch(segs, s, 9, 0x10), ecs))
    add('sos_longer_than_its_components', join(segs[:s] + [(SOS, segs[s][1] + b'\x00')], ecs))
    add('sos_short', join(segs[:s] + [(SOS, segs[s][1][:-2])], ecs))
    com = (COM, b'four')
    for n, name in ((0, 'length_0'), (1, 'length_1'), (0xFFFF, 'length_past_the_end')):
        add(f'segment_{name}', join(segs[:1] + [segment_bytes(com, n)] + segs[1:], ecs))
        add(f'sos_{name}', join(segs[:s] + [segment_bytes(segs[s], n)], ecs))
    add('dqt_length_past_the_end', join(segs[:q0] + [segment_bytes(segs[q0], 0x4000)] + segs[q0 + 1:], ecs))
    # restart markers: the 4:4:4 file has four MCUs, RST0 RST1 RST2 between them
    rsegs, recs = split(base(h, w, 0))
    rst = [m.start() for m in re.finditer(b'\xff[\xd0-\xd7]', recs)]
    assert [recs[p + 1] for p in rst] == [0xD0, 0xD1, 0xD2]
    e = bytearray(recs)
    e[rst[1] + 1] = 0xD2
    add('rst_out_of_order', join(rsegs, bytes(e)))
    e = bytearray(recs)
    e[rst[0] + 1], e[rst[1] + 1] = 0xD1, 0xD0
    add('rst_swapped', join(rsegs, bytes(e)))
    add('rst_one_missing', join(rsegs, recs[:rst[1]] + recs[rst[1] + 2:]))
    add('rst_one_too_many', join(rsegs, recs + b'\xff\xd3'))
    add('rst_doubled', join(rsegs, recs[:rst[1]] + b'\xff\xd1' + recs[rst[1]:]))
    add('rst_without_dri', join(without(rsegs, DRI), recs))
    add('rst_with_dri_2', join(patch(rsegs, find(rsegs, DRI), 1, 2), recs))
    d = find(segs, DRI)
    add('dri_length_5', join(segs[:d] + [(DRI, segs[d][1] + b'\x00')] + segs[d + 1:], ecs))
    add('dri_length_3', join(segs[:d] + [(DRI, b'\x00')] + segs[d + 1:], ecs))
    add('garbage_after_soi', join([b'\x00\x00'] + segs, ecs))
    for m in (0x01, 0x02, 0x60, 0xBF, 0xDE, 0xDF, 0xF0, 0xFD):
        add(f'reserved_marker_{m:02x}', join(segs[:1] + [(m, b'four')] + segs[1:], ecs))
    add('reserved_marker_f0_after_scan', join(segs, ecs, tail=segment_bytes((0xF0, b'four')) + EOI))
    add('soi_twice', join([SOI] + segs, ecs))
    add('eoi_missing', join(segs, ecs, tail=b''))
    add('eoi_missing_ff_last', join(segs, ecs, tail=b'\xff'))
    add('no_entropy_data', join(segs, b''))
    add('soi_only', SOI)
    add('soi_eoi', SOI + EOI)
    add('empty_file', b'')
    add('not_a_jpeg', b'\x89PNG\r\n\x1a\n' + bytes(40))
    # streams no encoder writes
    zrl3 = [('sym', 0xF0)] * 3
    add('ac_run_past_63', hand_file(PLAIN_BLOCKS[:3] + [(5, zrl3 + [(15, 1)], False)]))
    add('dc_category_12', hand_file(PLAIN_BLOCKS[:2] + [(('cat', 12, 0xABC), [], True)] + PLAIN_BLOCKS[3:]))
    add('huffman_code_unassigned', hand_file(PLAIN_BLOCKS[:3])[:-2] + b'\xff\x00\xff\x00' + EOI)
    add('data_one_block_short', hand_file(PLAIN_BLOCKS[:3]))
    add('coefficient_times_quantizer_above_32767', hand_file([(2047, [], True)] + PLAIN_BLOCKS[1:], q0=255), EUNSUPPORTED)
    add('ac_times_quantizer_above_32767', hand_file([(3, [(0, 1), (15, 1), (0, 513)], True)] + PLAIN_BLOCKS[1:]), EUNSUPPORTED)
    return out


def sweep_base():
    """the 16 x 16 4:2:0 file both sweeps work on, and the offset of its first entropy-coded byte"""
    raw = base(16, 16)
    segs, ecs = split(raw)
    return raw, len(raw) - 2 - len(ecs)


def prefix_sweep():
    raw, _ = sweep_base()
    return [raw[:n] for n in range(len(raw))]


def header_sweep():
    """every header byte from offset 2 set to 0x00, 0xFF, b ^ 0x01, b ^ 0x80 (mutants equal to the file are left out)"""
    raw, start = sweep_base()
    out = []
    for p in range(2, start):
        for v in sorted({0x00, 0xFF, raw[p] ^ 0x01, raw[p] ^ 0x80} - {raw[p]}):
            out.append((p, v, raw[:p] + bytes([v]) + raw[p + 1:]))
    return out


def coefficient_sweep(n=1500, seed=0):
    """hand-written files whose dequantized coefficients run far beyond what an encoder writes (quantizers up to 255, DC up
    to +-1023, 10-bit AC values), where the forms of libjpeg's IDCT stop agreeing: swept under the rule of the other two"""
    rs = np.random.RandomState(seed)
    codes = [(0, 1), (15, 1), (0, 10), (1, 1), (3, 2), (14, 1)]
    out = []
    for _ in range(n):
        qt = [int(v) for v in rs.choice([1, 2, 4, 8, 16, 32, 64, 128, 255][:rs.randint(1, 10)], 64)]
        blocks, prev = [], 0
        for _ in range(4):
            dc, acs, k = int(rs.randint(-1023, 1024)), [], 1
            for _ in range(rs.randint(0, 6)):
                run, size = codes[rs.randint(len(codes))]
                if k + run > 63:
                    break
                k += run + 1
                acs.append((run, int(rs.randint(1 << (size - 1), 1 << size)) * int(rs.choice([-1, 1]))))
            blocks.append((dc - prev, acs, k < 64))
            prev = dc
        out.append(hand_file(blocks, qt=qt))
    return out


# -------------------------------------------------------------------------------------------------------------------- PNG
PNG_SIG = b'\x89PNG\r\n\x1a\n'
GREY, RGB, PALETTE, GREY_ALPHA, RGBA = 0, 2, 3, 4, 6
CHANNELS = {GREY: 1, RGB: 3, PALETTE: 1, GREY_ALPHA: 2, RGBA: 4}


def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data))


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_row(ft, cur, prev, bpp):
    """PNG filter type ft over the raw bytes of one row (prev: the raw row above, zeros for the first)"""
    left = lambda i: cur[i - bpp] if i >= bpp else 0                   # noqa: E731
    upleft = lambda i: prev[i - bpp] if i >= bpp else 0                # noqa: E731
    pred = {0: lambda i: 0, 1: left, 2: lambda i: prev[i], 3: lambda i: (left(i) + prev[i]) >> 1,
            4: lambda i: paeth(left(i), prev[i], upleft(i))}[ft]
    return bytes((cur[i] - pred(i)) & 255 for i in range(len(cur)))


def png_stream(rows, filters, bpp):
    """the filtered scanlines (filter byte + bytes) of raw rows; a filter value above 4 is written with a zero predictor"""
    out, prev = b'', bytes(len(rows[0]))
    for row, ft in zip(rows, filters):
        out += bytes([ft]) + filter_row(ft if ft <= 4 else 0, row, prev, bpp)
        prev = row
    return out


def png_file(h, w, ctype, depth, stream, split_at=None, between=(), before=(), interlace=0, level=6, empty_idats=False):
    """a PNG from an (uncompressed) scanline stream.  split_at: IDAT payload sizes (None: one IDAT; 1: a chunk per byte);
    ``before``: chunks between IHDR and the first IDAT; ``between``: chunks put after the first IDAT; ``empty_idats``:
    a zero-length IDAT before, between and after the others"""
    z = zlib.compress(stream, level)
    pieces = [z] if split_at is None else [z[i:i + split_at] for i in range(0, len(z), split_at)]
    out = PNG_SIG + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, depth, ctype, 0, 0, interlace)) + b''.join(before)
    for k, piece in enumerate(pieces):
        if empty_idats:
            out += chunk(b'IDAT', b'')
        out += chunk(b'IDAT', piece)
        if k == 0:
            out += b''.join(between)
    if empty_idats:
        out += chunk(b'IDAT', b'')
    return out + chunk(b'IEND', b'')


def png_rows(seed, h, w, bpp):
    rs = np.random.RandomState(seed)
    return [bytes(rs.randint(0, 256, w * bpp, dtype=np.uint8)) for _ in range(h)]


PNG_FORMATS = [('grey8', GREY, 8, 1), ('grey16', GREY, 16, 2), ('rgb', RGB, 8, 3), ('rgba', RGBA, 8, 4)]
PNG_SIZES = [(1, 1), (1, 5), (5, 1), (7, 9)]


def png_filter_cases():
    """(name, kind, bytes, H, W, OK): each filter on every row / on the first row only (filter 0 below it), bytes per
    pixel 1, 2, 3, 4"""
    out = []
    for (fmt, ctype, depth, bpp), (h, w), ft in [(f, s, t) for f in PNG_FORMATS for s in PNG_SIZES for t in range(5)]:
        rows = png_rows(h * 31 + w * 7 + bpp + ft, h, w, bpp)
        kind = 'png16' if depth == 16 else 'png'
        for tag, filters in (('all', [ft] * h), ('first', [ft] + [0] * (h - 1))):
            data = png_file(h, w, ctype, depth, png_stream(rows, filters, bpp))
            out.append((f'{fmt}_{h}x{w}_f{ft}_{tag}', kind, data, h, w, OK))
    return out


TEXT = chunk(b'tEXt', b'Comment\x00made by hand')
GAMA = chunk(b'gAMA', struct.pack('>I', 45455))


def png_legal_cases():
    out = []
    h, w = 7, 9
    for fmt, ctype, depth, bpp in PNG_FORMATS:
        if depth == 16:
            continue
        rows = png_rows(bpp, h, w, bpp)
        stream = png_stream(rows, [y % 5 for y in range(h)], bpp)
        trns = [] if ctype == RGBA else [chunk(b'tRNS', b'\x00\x07' if ctype == GREY else b'\x00\x01\x00\x02\x00\x03')]
        add = lambda name, data: out.append((f'{fmt}_{name}', 'png', data, h, w, OK))      # noqa: E731
        add('idat_per_byte', png_file(h, w, ctype, 8, stream, split_at=1))
        add('idat_per_3_bytes_level0', png_file(h, w, ctype, 8, stream, split_at=3, level=0))
        add('empty_idats', png_file(h, w, ctype, 8, stream, split_at=5, empty_idats=True))
        add('ancillary_before', png_file(h, w, ctype, 8, stream, before=[GAMA, TEXT] + trns))
        # (more scanline data than the image holds: zlib's and PIL's readers stop at the last row)
        add('idat_long_by_one_row', png_file(h, w, ctype, 8, stream + stream[:bpp * w + 1]))
        add('ancillary_before_split', png_file(h, w, ctype, 8, stream, split_at=4, before=[TEXT, GAMA] + trns))
    return out


def png_between_cases():
    """ancillary chunks BETWEEN the IDAT chunks: not a legal PNG (the IDAT chunks must be consecutive) and PIL does not
    load such a file, so csrc/png_decode.hip declines it"""
    out = []
    h, w = 7, 9
    for fmt, ctype, depth, bpp in PNG_FORMATS:
        if depth == 16:
            continue
        stream = png_stream(png_rows(bpp, h, w, bpp), [y % 5 for y in range(h)], bpp)
        for name, c in (('text', TEXT), ('gama', GAMA), ('trns', chunk(b'tRNS', b'\x00\x07' if ctype == GREY else bytes(6)))):
            if name == 'trns' and ctype == RGBA:
                continue
            out.append((f'{fmt}_{name}_between_idats', 'png', png_file(h, w, ctype, 8, stream, split_at=6, between=[c]),
                        h, w, EUNSUPPORTED))
    return out


def png_declined_cases():
    out = []
    h, w = 7, 9
    add = lambda name, data: out.append((name, 'png', data, h, w, EUNSUPPORTED))      # noqa: E731
    rgb = png_rows(3, h, w, 3)
    add('interlaced', png_file(h, w, RGB, 8, png_stream(rgb, [0] * h, 3), interlace=1))
    pal = png_rows(4, h, w, 1)
    add('palette', png_file(h, w, PALETTE, 8, png_stream(pal, [0] * h, 1),
                            before=[chunk(b'PLTE', bytes(range(256)) * 3)]))
    for depth in (1, 2, 4):
        rows = png_rows(depth, h, (w * depth + 7) // 8, 1)
        add(f'grey_depth{depth}', png_file(h, w, GREY, depth, png_stream(rows, [0] * h, 1)))
    add('rgb16', png_file(h, w, RGB, 16, png_stream(png_rows(5, h, w, 6), [1] * h, 6)))
    add('grey_alpha', png_file(h, w, GREY_ALPHA, 8, png_stream(png_rows(6, h, w, 2), [4] * h, 2)))
    add('filter_byte_5', png_file(h, w, RGB, 8, png_stream(rgb, [0, 1, 5, 2, 3, 4, 0], 3)))
    add('filter_byte_5_first_row', png_file(h, w, RGB, 8, png_stream(rgb, [5] + [0] * (h - 1), 3)))
    add('filter_byte_255_last_row', png_file(h, w, GREY, 8, png_stream(pal, [0] * (h - 1) + [255], 1)))
    return out


def png_malformed_cases():
    """never OADG_OK"""
    out = []
    h, w = 7, 9
    add = lambda name, data: out.append((name, 'png', data, h, w, REJECT))      # noqa: E731
    rows = png_rows(3, h, w, 3)
    stream = png_stream(rows, [y % 5 for y in range(h)], 3)
    good = png_file(h, w, RGB, 8, stream)
    ihdr = chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, RGB, 0, 0, 0))
    idat = good.index(b'IDAT') - 4
    add('chunk_length_past_the_end', good[:idat] + struct.pack('>I', 4000) + good[idat + 4:])
    add('chunk_length_4g', good[:idat] + b'\xff\xff\xff\xff' + good[idat + 4:])
    add('idat_short_by_one_row', png_file(h, w, RGB, 8, stream[:-(3 * w + 1)]))
    add('idat_one_byte', PNG_SIG + ihdr + chunk(b'IDAT', zlib.compress(stream)[:1]) + chunk(b'IEND', b''))
    add('idat_missing', PNG_SIG + ihdr + chunk(b'IEND', b''))
    add('ihdr_not_first', PNG_SIG + TEXT + good[8:])
    add('signature_damaged', b'\x89PNG\r\n\x1a\r' + good[8:])
    small = png_file(1, 1, GREY, 8, b'\x00\x07', level=0)
    assert len(small) > 56
    out.append(('file_of_56_bytes', 'png', small[:56], 1, 1, REJECT))
    garbage = bytes(np.random.RandomState(8).randint(0, 256, 60, dtype=np.uint8))
    add('zlib_garbage', PNG_SIG + ihdr + chunk(b'IDAT', garbage) + chunk(b'IEND', b''))
    add('zlib_cut_in_half', PNG_SIG + ihdr + chunk(b'IDAT', zlib.compress(stream)[:40]) + chunk(b'IEND', b''))
    add('empty_file', b'')
    return out


def png_cases():
    return png_filter_cases() + png_legal_cases() + png_between_cases() + png_declined_cases() + png_malformed_cases()


def pil_png(raw, kind):
    """PIL's pixels (BGR uint8, or uint16 for kind png16), None when PIL does not load the file"""
    from PIL import Image
    try:
        with Image.open(io.BytesIO(raw)) as im:
            if kind == 'png16':
                return np.asarray(im).astype(np.uint16)
            return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
    except Exception:       # noqa: BLE001
        return None


# ------------------------------------------------------------------------------------------------------------ the corpus
def write_corpus(root):
    """every file above under ``root`` and root/manifest.txt for tests/native/decoder_corpus_main.cpp"""
    import os
    os.makedirs(root, exist_ok=True)
    lines = []

    def put(kind, name, data, h, w):
        path = os.path.join(root, name)
        with open(path, 'wb') as f:
            f.write(data)
        lines.append(f'{kind} {path} {h} {w}')
    for table in (legal_cases, declined_cases, malformed_cases):
        for name, data, h, w, _ in table():
            put('jpeg', f'{table.__name__[:-6]}_{name}.jpg', data, h, w)
    for n, data in enumerate(prefix_sweep()):
        put('jpeg', f'prefix_{n:04d}.jpg', data, 16, 16)
    for p, v, data in header_sweep():
        put('jpeg', f'header_{p:04d}_{v:02x}.jpg', data, 16, 16)
    for n, data in enumerate(coefficient_sweep()):
        put('jpeg', f'coefficients_{n:04d}.jpg', data, 16, 16)
    for name, kind, data, h, w, _ in png_cases():
        put(kind, f'png_{name}.png', data, h, w)
    with open(os.path.join(root, 'manifest.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return len(lines)


if __name__ == '__main__':
    if len(sys.argv) != 3 or sys.argv[1] != '--write':
        sys.exit(__doc__)
    print(write_corpus(sys.argv[2]), 'files')
