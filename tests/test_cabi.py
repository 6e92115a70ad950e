"""CPU: the C-ABI library loads and exports every symbol include/oadg_hip.h declares, and oadg_amd._lib - the only Python
restatement of that header - agrees with it: struct fields, offsets and sizes, constants, the kind of every parameter (no
compute, no compiler: the header is read as text)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'oadg_hip.h')


def _declared():
    src = open(os.path.join(ROOT, 'include', 'oadg_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(oadg_[a-z0-9_]+)\s*\(', src)))


def test_header_declares_something():
    assert len(_declared()) >= 10


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    from oadg_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    h = _lib.lib()
    for name in _declared():
        assert hasattr(h, name), name
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature'
    assert sorted(_lib.SIGNATURES) == _declared()


def test_hot_ops_refuse_cpu_tensors():
    import torch
    from oadg_amd import hip_ops
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip_ops.supcon_loss(torch.zeros(4, 64), torch.zeros(4, 1, dtype=torch.long), 2, 0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip_ops.roi_align_fpn([torch.zeros(1, 4, 8, 8)], torch.zeros(1, 5), 7, [0.25])


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, 'oa-dg_amd')
    for dp, _, fn in os.walk(pkg):
        for f in fn:
            if f.endswith('.py'):
                s = open(os.path.join(dp, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', s, flags=re.M), os.path.join(dp, f)


# ---- include/oadg_hip.h against oadg_amd._lib -----------------------------------------------------------------------------
_C = ctypes
SCALARS = {'int': _C.c_int, 'long': _C.c_long, 'long long': _C.c_longlong, 'float': _C.c_float, 'double': _C.c_double,
           'unsigned': _C.c_uint, 'unsigned char': _C.c_ubyte, 'char': _C.c_char, 'size_t': _C.c_size_t,
           'int16_t': _C.c_int16, 'int32_t': _C.c_int32, 'int64_t': _C.c_int64, 'uint8_t': _C.c_uint8,
           'uint16_t': _C.c_uint16, 'uint32_t': _C.c_uint32, 'uint64_t': _C.c_uint64}
STRUCT_RE = re.compile(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;', re.S)
FIRST_RE = re.compile(r'^([\w\s]+?)\s*(\**)\s*(\w+)\s*((?:\[\d+\])*)$')       # base type, stars, name, array extents
NEXT_RE = re.compile(r'^(\**)\s*(\w+)\s*((?:\[\d+\])*)$')
EXPECTED_STRUCTS = {'oadg_rpn_level', 'oadg_rpn_loss_level', 'oadg_roi_assign_image', 'oadg_roi_target_entry',
                    'oadg_roi_sample_image', 'oadg_region_op', 'oadg_colsum_job', 'oadg_wgrad_job', 'oadg_prep_bwd_job',
                    'oadg_prep_desc', 'oadg_select_job', 'oadg_sgd_tensor', 'oadg_mix_target', 'oadg_bbox_step',
                    'oadg_bbox_chain', 'oadg_jpeg_desc'}
REQUIRED_CONSTANTS = ('OP_COPY OP_LUT_AUTOCONTRAST OP_LUT_EQUALIZE OP_POSTERIZE OP_SOLARIZE OP_IMAGE OP_BG_WARP OP_WARP_NEG '
                      'OP_ENH_BRIGHTNESS OP_ENH_COLOR OP_ENH_CONTRAST OP_ENH_SHARPNESS ROI_ASSIGN_MAX_IMAGES '
                      'ROI_TARGET_MAX_ENTRIES ROI_SAMPLE_MAX_IMAGES RPN_MAX_LEVELS PARSE_LOSSES_MAX CORRUPT_NEAREST '
                      'CORRUPT_REFLECT CORRUPT_MIRROR').split()


def _scalar(base):
    return SCALARS[' '.join(w for w in base.split() if w != 'const')]


def _parse(text):
    """header text -> ({struct: [(field, ctypes type)]}, {constant: value}, {function: (return kind, [parameter kinds])})"""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    text = re.sub(r'//[^\n]*', '', text)
    structs = {}
    for body, name in STRUCT_RE.findall(text):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            first, *rest = [p.strip() for p in decl.split(',')]
            base, stars, fname, dims = FIRST_RE.match(first).groups()
            for stars, fname, dims in [(stars, fname, dims)] + [NEXT_RE.match(p).groups() for p in rest]:
                t = _C.c_void_p if stars else _scalar(base)
                for d in reversed(re.findall(r'\d+', dims)):
                    t = t * int(d)
                fields.append((fname, t))
        structs[name] = fields
    consts = {m.group(1): int(m.group(2), 0) for m in re.finditer(r'^#define\s+(OADG_\w+)\s+(-?\w+)\s*$', text, re.M)
              if re.fullmatch(r'-?(0x[0-9a-fA-F]+|\d+)', m.group(2))}
    for body in re.findall(r'\benum\s*\{(.*?)\}', text, re.S):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(','))):
            name, _, v = (x.strip() for x in item.partition('='))
            value = int(v, 0) if v else value + 1
            consts[name] = value
    protos = {}
    rest = re.sub(r'\benum\s*\{.*?\}\s*;', '', STRUCT_RE.sub('', text), flags=re.S)
    rest = re.sub(r'^\s*#[^\n]*', '', rest, flags=re.M)
    for ret, name, params in re.findall(r'([\w\s*]+?)\b(oadg_\w+)\s*\(([^)]*)\)\s*;', rest):
        params = [p.strip() for p in params.split(',')]
        if params == ['void']:
            params = []
        protos[name] = (_kind_c(ret + ' _'), [_kind_c(p) for p in params])
    return structs, consts, protos


def _kind_c(decl):
    """'const float* x' -> 'ptr'; 'long long n' -> ('scalar', bytes, signed, float) (the last word is the name)"""
    return 'ptr' if '*' in decl else _kind(_scalar(decl.rsplit(None, 1)[0]))


def _kind(t):
    if t in (_C.c_void_p, _C.c_char_p) or (isinstance(t, type) and issubclass(t, _C._Pointer)):
        return 'ptr'
    is_float = t in (_C.c_float, _C.c_double)
    return ('scalar', _C.sizeof(t), is_float or t(-1).value < 0, is_float)


def _same_type(a, b):
    if hasattr(a, '_length_') or hasattr(b, '_length_'):
        return getattr(a, '_length_', None) == getattr(b, '_length_', None) and _same_type(a._type_, b._type_)
    return a is b


def _problems(text):
    """every disagreement between the header text and oadg_amd._lib (+ hip_ops.CORRUPT_MODES), as a list of sentences"""
    from oadg_amd import _lib, hip_ops
    structs, consts, protos = _parse(text)
    out = []
    if set(structs) != set(_lib.STRUCTS):
        out.append(f'structs: header and _lib.STRUCTS differ in {sorted(set(structs) ^ set(_lib.STRUCTS))}')
    for name in sorted(set(structs) & set(_lib.STRUCTS)):
        mine, fields = _lib.STRUCTS[name], structs[name]
        theirs = type(name, (_C.Structure,), {'_fields_': fields})
        if [n for n, _ in mine._fields_] != [n for n, _ in fields]:
            out.append(f'struct {name}: fields {[n for n, _ in mine._fields_]}, header {[n for n, _ in fields]}')
            continue
        bad = [n for (n, a), (_, b) in zip(mine._fields_, fields)
               if not _same_type(a, b) or getattr(mine, n).offset != getattr(theirs, n).offset]
        if bad or _C.sizeof(mine) != _C.sizeof(theirs):
            out.append(f'struct {name}: type or offset of {bad}, size {_C.sizeof(mine)} against {_C.sizeof(theirs)}')
    held = {k: v for k, v in vars(_lib).items() if k.isupper() and isinstance(v, int)}
    for k in REQUIRED_CONSTANTS:
        if k not in held:
            out.append(f'constant {k}: not in _lib')
    held.update({'CORRUPT_' + k.upper(): v for k, v in hip_ops.CORRUPT_MODES.items()})
    for k, v in sorted(held.items()):
        if consts.get('OADG_' + k) != v:
            out.append(f'constant {k}: {v}, header {consts.get("OADG_" + k)}')
    for name, (res, args) in sorted(_lib.SIGNATURES.items()):
        if name not in protos:
            out.append(f'signature {name}: not declared')
        elif (_kind(res), [_kind(a) for a in args]) != protos[name]:
            ret, params = protos[name]
            where = ['return'] * (_kind(res) != ret) + [i for i, (a, b) in enumerate(zip(args, params)) if _kind(a) != b]
            out.append(f'signature {name}: {len(args)} parameters against {len(params)}, differing at {where}')
    return out


def test_parser_reads_the_whole_header():
    structs, consts, protos = _parse(open(HEADER).read())
    assert set(structs) >= EXPECTED_STRUCTS and len(structs) >= 16
    assert len(protos) >= 119 and sorted(protos) == _declared()
    assert len(consts) >= 24 and consts['OADG_OP_ENH_SHARPNESS'] == 11 and consts['OADG_ROI_SAMPLE_MAX_IMAGES'] == 8
    # what the header really uses: multi-declarator pointers, 1-D and 2-D arrays, struct pointers, every scalar width
    assert structs['oadg_prep_bwd_job'][:2] == [('part', _C.c_void_p), ('gbias', _C.c_void_p)]
    assert dict(structs['oadg_bbox_chain'])['steps_dev'] is _C.c_void_p
    jd = dict(structs['oadg_jpeg_desc'])
    assert _same_type(jd['v'], _C.c_int32 * 4) and _same_type(jd['qt'], _C.c_uint16 * 64 * 4)
    assert dict(structs['oadg_bbox_step'])['scratch_off'] is _C.c_longlong
    assert dict(structs['oadg_wgrad_job'])['P'] is _C.c_long
    assert protos['oadg_sgd_blocks'] == (('scalar', 8, True, False), [('scalar', 8, True, False)])
    assert protos['oadg_supcon_workspace_bytes'][0] == ('scalar', 8, False, False)
    assert protos['oadg_cls_loss_workspace_bytes'][1] == []


def test_structs_constants_and_signatures_match_the_header():
    assert _problems(open(HEADER).read()) == []


def _doctor(text, old, new):
    assert text.count(old) == 1, old
    return text.replace(old, new)


@pytest.mark.parametrize('old,new,reported', [
    ('int splits, K, C, R, S, w_krsc, first_block;\n} oadg_prep_bwd_job',
     'int K, splits, C, R, S, w_krsc, first_block;\n} oadg_prep_bwd_job', 'struct oadg_prep_bwd_job'),
    ('float *dw, *dgamma;\n    float eps;', 'float *dw;\n    float eps;\n    float *dgamma;', 'struct oadg_prep_bwd_job'),
    ('int rows, K, first_block;', 'long rows, K, first_block;', 'struct oadg_colsum_job'),
    ('long long total_blocks, float lr, float momentum,', 'long long total_blocks, float momentum,',
     'signature oadg_sgd_step_multi'),
    ('int n, long long total_blocks, float lr,', 'int n, int total_blocks, float lr,', 'signature oadg_sgd_step_multi'),
    ('#define OADG_ROI_TARGET_MAX_ENTRIES 32', '#define OADG_ROI_TARGET_MAX_ENTRIES 33', 'constant ROI_TARGET_MAX_ENTRIES'),
    ('OADG_OP_IMAGE = 5,', 'OADG_OP_IMAGE = 6,', 'constant OP_IMAGE'),
    ('} oadg_sgd_tensor;', '} oadg_sgd_entry;', 'structs:'),
])
def test_the_comparison_reports_a_doctored_header(old, new, reported):
    found = _problems(_doctor(open(HEADER).read(), old, new))
    assert found and all(p.startswith(reported) for p in found), found


def test_only_lib_restates_the_header():
    """a Structure or a record dtype anywhere else in the product is a copy of a C layout that nothing checks"""
    pkg = os.path.join(ROOT, 'oa-dg_amd')
    for dp, _, fn in os.walk(pkg):
        for f in fn:
            if f.endswith('.py') and f != '_lib.py':
                s = open(os.path.join(dp, f)).read()
                assert not re.search(r'\bStructure\b|np\.dtype\(\[', s), os.path.join(dp, f)
