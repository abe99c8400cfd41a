"""CPU: the whole C-ABI binding, once.  depth-from-motion_amd/_capi.py is written by hand; here every header of
include/ is parsed (tests/capi_header.py) and held against it -- the names each header declares, return types, the
type of EVERY parameter, every descriptor struct field by field, the integer constants _capi mirrors -- and against
the built library.  A comparison returns its findings as messages that name the symbol and the parameter or field;
the three tests at the end show on in-memory copies that a swapped parameter pair, a moved field and a constant off
by one are found."""
import collections
import ctypes
import importlib
import itertools
import re

import pytest

from tests import capi_header as H

RESTYPES = {'int': ctypes.c_int, 'size_t': ctypes.c_size_t, 'const char *': ctypes.c_char_p, 'void': None}
SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t,
           'float': ctypes.c_float, 'double': ctypes.c_double}
# (function, parameter): why its binding may break the parameter rule.  An entry that is not needed fails the test.
EXCEPTIONS = {('dfm_point_sample_mv_fwd_batched', 'descs'): 'an ARRAY of dfm_mv_desc, one per sample, passed as '
              '(MvDesc * batch)(): bound as c_void_p'}
CODE = {h: H.code(h) for h in H.HEADERS}
DECLS = {h: H.declarations(CODE[h]) for h in H.HEADERS}
KNOWN = {k: v for c in CODE.values() for k, v in H.constants(c).items()}      # an array length may use any of them


@pytest.fixture(scope='module')
def capi():
    importlib.import_module('depth-from-motion_amd.build').build_hip()
    return importlib.import_module('depth-from-motion_amd')._capi


def name_of(t):
    return getattr(t, '__name__', repr(t))


def is_pointer(t):
    return t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


def signature_problems(header, decls, table, struct_classes, exceptions=EXCEPTIONS):
    """one header's declarations against its table {name: (restype, argtypes)}.  A scalar parameter is bound as exactly
    its class, a single pointer to a header struct as POINTER(its class), any other pointer as c_void_p or a ctypes
    pointer type"""
    out = [f'{n}: declared in {header}, not bound under it' for n in decls if n not in table]
    out += [f'{n}: bound under {header}, which does not declare it' for n in table if n not in decls]
    for name in (n for n in decls if n in table):
        (ret, params), (restype, argtypes) = decls[name], table[name]
        if restype is not RESTYPES[ret]:
            out.append(f'{name}: restype {name_of(restype)}, the header returns {ret}')
        if not isinstance(argtypes, list) or len(argtypes) != len(params):
            out.append(f'{name}: {len(argtypes)} argtypes, the header declares {len(params)} parameters')
        for i, ((pname, ctype, depth), bound) in enumerate(zip(params, argtypes)):
            want = ctypes.POINTER(struct_classes[ctype]) if depth == 1 and ctype in struct_classes else \
                SCALARS[ctype] if depth == 0 else None
            holds = bound is want if want else is_pointer(bound)
            if (name, pname) in exceptions:
                if holds:
                    out.append(f'{name}: parameter {i} ({pname}) is listed as an exception and needs none')
                holds = is_pointer(bound)
            if not holds:
                out.append(f'{name}: parameter {i} ({ctype} {"*" * depth}{pname}) is bound as {name_of(bound)}, the '
                           f'header asks for {name_of(want) if want else "c_void_p or a ctypes pointer"}')
    return out


def struct_problems(parsed, struct_classes):
    """the structs parsed from the headers against {C name: ctypes class}, both ways, field by field in order"""
    out = [f'struct {s}: defined in a header, not in _capi.STRUCTS' for s in parsed if s not in struct_classes]
    out += [f'struct {s}: in _capi.STRUCTS, defined in no header' for s in struct_classes if s not in parsed]
    for s, cls in ((s, struct_classes[s]) for s in parsed if s in struct_classes):
        header = [(n, name_of(SCALARS[c]), length) for n, c, length in parsed[s]]
        mirror = [(n, name_of(t._type_), t._length_) if issubclass(t, ctypes.Array) else (n, name_of(t), None)
                  for n, t in cls._fields_]
        for i, (h, m) in enumerate(itertools.zip_longest(header, mirror)):
            if h != m:
                h, m = ('%s %s[%s]' % (f[1], f[0], f[2]) if f else 'nothing' for f in (h, m))
                out.append(f'struct {s}: field {i} is {h} in the header, {m} in {cls.__name__}'.replace('[None]', ''))
    return out


def constant_problems(known, namespace):
    """DFM_NAME is mirrored as DFM_NAME or as NAME; a constant without a mirror is ignored, a mirror that is no plain
    int is none"""
    return [f'{name}: {value} in the header, _capi.{mirror} is {namespace[mirror]}'
            for name, value in known.items() for mirror in (name, name[len('DFM_'):])
            if type(namespace.get(mirror)) is int and namespace[mirror] != value]


def test_parser_on_known_declarations():
    d = DECLS['dfm_hip.h']
    short = {n: (ret, len(params)) for n, (ret, params) in d.items()}
    assert short['dfm_version'] == ('int', 0) and short['dfm_last_error'] == ('const char *', 0)
    assert short['dfm_plane_sweep_reset_tuning'] == ('void', 0)
    assert short['dfm_profile_end'] == ('int', 2) and short['dfm_camera_prepare'] == ('int', 7)
    assert short['dfm_plane_sweep_workspace_bytes'] == ('size_t', 1)
    assert d['dfm_profile_end'][1] == [('total_ms', 'double', 1), ('launches', 'int', 1)]
    assert d['dfm_plane_sweep_fwd'][1][::9] == [('desc', 'dfm_sweep_desc', 1), ('workspace_bytes', 'size_t', 0)]
    assert d['dfm_point_sample_mv_fwd'][1][6] == ('valid', 'unsigned char', 1)
    s = H.structs(CODE['dfm_hip.h'], KNOWN)
    assert s['dfm_sweep_desc'][2:4] == [('h_in', 'int32_t', None), ('w_in', 'int32_t', None)]     # one line, two names
    assert s['dfm_sweep_opts'][-1] == ('reserved', 'int32_t', 1) and s['dfm_vs_desc'][14] == ('voxel_range', 'float', 6)
    assert H.structs(CODE['dfm_hip_sparse_conv.h'], KNOWN)['dfm_voxel_desc'][-1] == ('offset', 'int64_t', 65)
    assert (KNOWN['DFM_ERR_UNSUPPORTED'], KNOWN['DFM_VS_PAIR_FLOATS']) == (-2, 24) and 'DFM_VOXEL_NO_KEY' not in KNOWN
    text = H.strip_comments('/* DFM_API int dfm_a(int a);\n*/ // DFM_API int dfm_b(void);\n'
                            'DFM_API int dfm_c(int (*f)(int), const int32_t size[3]);')
    with pytest.raises(ValueError, match=r'cannot read the parameter .int \(\*f\)\(int\)'):    # refused, not miscounted
        H.declarations(text)
    assert H.declarations(text.replace('int (*f)(int)', 'void *const *f')) == {
        'dfm_c': ('int', [('f', 'void', 2), ('size', 'int32_t', 1)])}


@pytest.mark.parametrize('header', H.HEADERS)
def test_table_matches_the_header(capi, header):
    """the parser missed no DFM_API; then names exactly, restypes, parameter counts, every parameter's type"""
    assert len(DECLS[header]) == len(re.findall(r'^[ \t]*DFM_API\b', CODE[header], flags=re.M)) > 0
    problems = signature_problems(header, DECLS[header], capi._BINDING[header], capi.STRUCTS)
    assert not problems, '\n'.join(problems)


def test_the_binding_is_whole(capi):
    names = collections.Counter(n for h in H.HEADERS for n in DECLS[h])
    assert [n for n, count in names.items() if count > 1] == []                # no name is declared in two headers
    assert sorted(capi._BINDING) == H.HEADERS and capi.EXPORTS == tuple(capi.SIGNATURES)
    assert sorted(capi.EXPORTS) == sorted(names)
    side = [h for h in H.HEADERS if h.startswith('dfm_hip_')]                  # dfm_hip.h is the one header to include
    assert sorted(re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', CODE['dfm_hip.h'], flags=re.M)) == side != []
    assert set(EXCEPTIONS) <= {(n, p[0]) for h in H.HEADERS for n, (_, params) in DECLS[h].items() for p in params}
    with pytest.raises(ValueError, match='dfm_b is bound twice in one header'):
        capi._table(('dfm_a', None, []), ('dfm_b', None, []), ('dfm_b', None, []))
    with pytest.raises(ValueError, match='dfm_a is bound twice: under a.h and under b.h'):
        capi._flatten({'a.h': {'dfm_a': (None, [])}, 'b.h': {'dfm_a': (None, [])}})


def test_structs_and_constants_match_the_headers(capi):
    parsed = {s: fields for h in H.HEADERS for s, fields in H.structs(CODE[h], KNOWN).items()}
    assert len(parsed) == sum(len(re.findall(r'\btypedef\s+struct\b', c)) for c in CODE.values()) >= 18    # none missed
    assert len(set(capi.STRUCTS.values())) == len(capi.STRUCTS)
    problems = struct_problems(parsed, capi.STRUCTS) + constant_problems(KNOWN, vars(capi))
    assert not problems, '\n'.join(problems)
    assert sorted(capi.SPARSE_STATUS) == sorted(v for n, v in KNOWN.items() if n.startswith('DFM_SPARSE_STATUS_'))


def test_library_exports_every_declaration_and_lib_applies_the_table(capi):
    fresh, lib = ctypes.CDLL(capi.LIB_PATH), capi.lib()
    for header in H.HEADERS:
        for name in DECLS[header]:
            assert hasattr(fresh, name), f'{name} declared in {header} but not exported'
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_a_swapped_parameter_pair_is_found(capi):
    table = dict(capi._BINDING['dfm_hip.h'])
    restype, argtypes = table['dfm_store_probe']        # (out, batch, int32_t planes, int64_t plane_bytes, ...)
    table['dfm_store_probe'] = (restype, argtypes[:2] + [argtypes[3], argtypes[2]] + argtypes[4:])
    assert signature_problems('dfm_hip.h', DECLS['dfm_hip.h'], table, capi.STRUCTS) == [
        'dfm_store_probe: parameter 2 (int32_t planes) is bound as c_long, the header asks for c_int',
        'dfm_store_probe: parameter 3 (int64_t plane_bytes) is bound as c_int, the header asks for c_long']
    table = dict(capi._BINDING['dfm_hip.h'], dfm_plane_sweep_tuning=(None, [ctypes.c_void_p, ctypes.c_int32]))
    assert signature_problems('dfm_hip.h', DECLS['dfm_hip.h'], table, capi.STRUCTS) == [
        'dfm_plane_sweep_tuning: restype None, the header returns int',
        'dfm_plane_sweep_tuning: parameter 0 (dfm_sweep_desc *desc) is bound as c_void_p, the header asks for '
        'LP_SweepDesc',
        'dfm_plane_sweep_tuning: parameter 1 (dfm_sweep_opts *opts) is bound as c_int, the header asks for '
        'LP_SweepOpts']
    more = H.declarations(CODE['dfm_hip.h'] + '\nDFM_API int dfm_unbound(void);\n')
    table = dict(capi._BINDING['dfm_hip.h'], dfm_undeclared=(None, []))
    assert signature_problems('dfm_hip.h', more, table, capi.STRUCTS, {('dfm_plane_sweep_tuning', 'desc'): ''}) == [
        'dfm_unbound: declared in dfm_hip.h, not bound under it',
        'dfm_undeclared: bound under dfm_hip.h, which does not declare it',
        'dfm_plane_sweep_tuning: parameter 0 (desc) is listed as an exception and needs none',
        'dfm_point_sample_mv_fwd_batched: parameter 0 (dfm_mv_desc *descs) is bound as c_void_p, the header asks for '
        'LP_MvDesc']


def test_a_moved_struct_field_is_found(capi):
    text = CODE['dfm_hip.h']                            # dfm_mv_desc: flip one place down; an array one shorter
    moved = text.replace('int32_t flip;\n    float pad_h, pad_w;', 'float pad_h;\n    int32_t flip;\n    float pad_w;')
    moved = moved.replace('float proj_inv[16];', 'float proj_inv[15];')
    parsed = {s: H.structs(moved, KNOWN)[s] for s in ('dfm_mv_desc', 'dfm_vs_desc', 'dfm_sweep_opts')}
    fields = capi.SweepOpts._fields_                    # and on the ctypes side: a field gone, a struct unknown
    classes = {'dfm_mv_desc': capi.MvDesc, 'dfm_vs_desc': capi.VsDesc, 'dfm_gone': capi.SppDesc,
               'dfm_sweep_opts': type('Short', (ctypes.Structure,), {'_fields_': fields[:10] + fields[11:]})}
    assert struct_problems(parsed, classes) == [
        'struct dfm_gone: in _capi.STRUCTS, defined in no header',
        'struct dfm_mv_desc: field 13 is c_float pad_h in the header, c_int flip in MvDesc',
        'struct dfm_mv_desc: field 14 is c_int flip in the header, c_float pad_h in MvDesc',
        'struct dfm_vs_desc: field 16 is c_float proj_inv[15] in the header, c_float proj_inv[16] in VsDesc',
        'struct dfm_sweep_opts: field 10 is c_int unpack in the header, c_int reserved[1] in Short',
        'struct dfm_sweep_opts: field 11 is c_int reserved[1] in the header, nothing in Short']
    assert struct_problems(H.structs(text, KNOWN), {}) == [
        f'struct {s}: defined in a header, not in _capi.STRUCTS' for s in H.structs(text, KNOWN)]


def test_a_changed_constant_is_found(capi):
    text = CODE['dfm_hip.h']
    for old, new, message in (
            ('#define DFM_VS_PAIR_FLOATS 24', '#define DFM_VS_PAIR_FLOATS 25',
             'DFM_VS_PAIR_FLOATS: 25 in the header, _capi.VS_PAIR_FLOATS is 24'),
            ('DFM_ERR_UNSUPPORTED = -2', 'DFM_ERR_UNSUPPORTED = -1',
             'DFM_ERR_UNSUPPORTED: -1 in the header, _capi.DFM_ERR_UNSUPPORTED is -2'),
            ('DFM_DL_HARD = 1', 'DFM_DL_HARD = 2', 'DFM_DL_HARD: 2 in the header, _capi.DL_HARD is 1')):
        assert old in text and constant_problems(H.constants(text.replace(old, new)), vars(capi)) == [message]
