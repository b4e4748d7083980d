"""CPU: the ctypes binding is read from include/infgen_hip.h (infgen_amd/_lib.py).  The layouts it builds are compared member by
member with what the host C compiler makes of the same header, the argument lists with the prototypes' text, and the reader
itself is tried on short snippets - one per construct the header uses, and some it must refuse."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO
from infgen_amd import _lib

HEADER_DIR = os.path.join(REPO, 'include')
PY_NAMES = {'InfgenLinearDesc': 'LinearDesc', 'InfgenEdgeBuf': 'EdgeBuf', 'InfgenRadiusEdges': 'RadiusEdges',
            'InfgenInsertion': 'Insertion', 'InfgenOptions': 'Options', 'InfgenSampling': 'Sampling', 'InfgenRollout': 'Rollout',
            'InfgenBatchIngest': 'BatchIngest'}


def test_header_is_found_next_to_the_package_and_a_missing_one_is_named():
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(HEADER_DIR, 'infgen_hip.h'))
    with pytest.raises(_lib.InfgenHipError, match='/nonexistent/infgen_hip.h'):
        _lib.read_header('/nonexistent/infgen_hip.h')


def test_every_struct_of_the_header_has_its_module_level_name():
    assert set(_lib.HEADER.structs) == set(PY_NAMES)
    for c_name, py_name in PY_NAMES.items():
        assert getattr(_lib, py_name) is _lib.HEADER.structs[c_name]


def test_struct_layouts_equal_the_host_compilers(tmp_path):
    """sizeof of every struct, offsetof and size of every member: a C program generated from the parsed header, compiled against
    the header itself and run, next to sizeof / .offset / .size of the ctypes classes"""
    cc = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc, 'no host C compiler found (CC, cc, gcc, clang)'
    lines, mine = [], {}
    for name, cls in _lib.HEADER.structs.items():
        lines.append(f'  printf("{name} %zu 0\\n", sizeof({name}));')
        mine[name] = (C.sizeof(cls), 0)
        for member, _ in cls._fields_:
            lines.append(f'  printf("{name}.{member} %zu %zu\\n", sizeof((({name}*)0)->{member}), offsetof({name}, {member}));')
            mine[f'{name}.{member}'] = (getattr(cls, member).size, getattr(cls, member).offset)
    src = tmp_path / 'abi_layout.c'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "infgen_hip.h"\nint main(void) {\n' + '\n'.join(lines) +
                   '\n  return 0;\n}\n')
    exe = tmp_path / 'abi_layout'
    subprocess.run([cc, '-std=c99', '-I', HEADER_DIR, '-o', str(exe), str(src)], check=True, capture_output=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    theirs = {k: (int(size), int(off)) for k, size, off in (line.split() for line in out.splitlines())}
    assert len(theirs) == len(lines) > 300
    assert {k: v for k, v in mine.items() if theirs[k] != v} == {}


_SCALAR_KINDS = {'int': C.c_int, 'float': C.c_float, 'double': C.c_double, 'unsigned': C.c_uint, 'long long': C.c_longlong,
                 'unsigned long long': C.c_ulonglong, 'uint8_t': C.c_ubyte, 'unsigned char': C.c_ubyte}


def _kind(param):
    """the ctypes type of one parameter's text, by the binding's rules, without the reader"""
    if re.fullmatch(r'\s*const\s+char\s*\*\s*\w+\s*', param):
        return C.c_char_p
    struct = re.search(r'\b(Infgen\w+)\s*\*', param)
    if struct:
        return C.POINTER(getattr(_lib, PY_NAMES[struct[1]]))
    if '*' in param:
        return C.c_void_p
    return _SCALAR_KINDS[' '.join(w for w in param.split()[:-1] if w != 'const')]


def _prototypes():
    """(return type, name, [parameter text]) of every prototype, by one regular expression of the test's own"""
    with open(_lib.HEADER_PATH) as f:
        txt = re.sub(r'/\*.*?\*/', ' ', f.read(), flags=re.S)
    protos = re.findall(r'\b(int|const char\*)\s+(infgen_\w+)\s*\(([^)]*)\)\s*;', txt)
    return [(ret, name, [] if params.strip() == 'void' else params.split(',')) for ret, name, params in protos]


# callers pass this entry the context's address as an integer (ctypes.addressof), so its struct pointer is not typed
UNTYPED = {('infgen_raw_feature_rows', 0): C.c_void_p}


def test_every_prototype_has_one_argtype_of_the_right_kind_per_parameter():
    protos = _prototypes()
    assert len(protos) >= 94 and {p[1] for p in protos} == set(_lib.SYMBOLS) and len(protos) == len(_lib.SYMBOLS)
    for ret, name, params in protos:
        res, argtypes = _lib.SYMBOLS[name]
        assert res is (C.c_int if ret == 'int' else C.c_char_p), name
        assert argtypes == [UNTYPED.get((name, k)) or _kind(p) for k, p in enumerate(params)], name
    # three of the entries that took void* for a struct the header names now take that struct's pointer
    assert _lib.SYMBOLS['infgen_linear_multi'][1][0] is C.POINTER(_lib.LinearDesc)
    assert _lib.SYMBOLS['infgen_rollout_validate'][1] == [C.POINTER(_lib.Rollout)]
    assert _lib.SYMBOLS['infgen_radius_edges'][1] == [C.POINTER(_lib.RadiusEdges), C.POINTER(_lib.EdgeBuf), C.c_void_p]


def test_library_exports_every_prototype_with_these_argtypes():
    lib = _lib.load()
    for _, name, _ in _prototypes():
        assert hasattr(lib, name), f'{name} is not exported'
        assert getattr(lib, name).argtypes == _lib.SYMBOLS[name][1] and getattr(lib, name).restype is _lib.SYMBOLS[name][0]
    ctx = _lib.Rollout()
    assert lib.infgen_raw_feature_rows(C.addressof(ctx), 0, None, None, 0, None) == \
        lib.infgen_raw_feature_rows(C.byref(ctx), 0, None, None, 0, None)           # both spellings reach the entry


def test_constants_keep_their_values():
    assert _lib.OPTIONS_VALUE_BYTES == 48 == C.sizeof(C.c_int) * 12
    assert [_lib.Q_ATTN_PACK_SIZE, _lib.Q_FOURIER_N2, _lib.Q_FOURIER_N3, _lib.Q_FOURIER_N4, _lib.Q_TILE_ROWS, _lib.Q_EDGE_ATTN_CAP,
            _lib.Q_MAX_AGENTS, _lib.Q_ABI_VERSION, _lib.Q_SIZEOF_ROLLOUT, _lib.Q_ATTN_SPLIT_ROWS, _lib.Q_HEADS_SAMPLE_K] == list(range(11))
    assert _lib.MAX_LAYERS == 8 and len(_lib.KERNEL_IDS) == 11 == _lib.HEADER.consts['INFGEN_KID_COUNT']
    assert _lib.VM_SCRATCH_DOUBLES == 3072 and _lib.GRID_OVERLAP_MAX_CELLS == 16384


def _fields(cls):
    return [(name, t, getattr(cls, name).offset) for name, t in cls._fields_]


def test_reader_several_declarators_per_statement():
    h = _lib.Header('typedef struct A {\n  int S, A_cap, T;   /* sizes */\n  float* pos; float* head;  // two on a line\n'
                    '  unsigned char* m; float r, q;\n} A;')
    assert _fields(h.structs['A']) == [('S', C.c_int, 0), ('A_cap', C.c_int, 4), ('T', C.c_int, 8), ('pos', C.c_void_p, 16),
                                       ('head', C.c_void_p, 24), ('m', C.c_void_p, 32), ('r', C.c_float, 40), ('q', C.c_float, 44)]


def test_reader_array_members():
    h = _lib.Header('#define N_W 3\ntypedef struct B { const float* w[N_W]; float k[2]; uint8_t b; } B;')
    assert h.consts == {'N_W': 3}
    assert _fields(h.structs['B']) == [('w', C.c_void_p * 3, 0), ('k', C.c_float * 2, 24), ('b', C.c_ubyte, 32)]
    assert C.sizeof(h.structs['B']) == 40


def test_reader_nested_structs_and_prototypes():
    h = _lib.Header('typedef struct In { int a; double d; } In;\ntypedef struct Out { In x, y; const In* p; long long n; } Out;\n'
                    'int f(const char* s, unsigned long long n, const Out* o, void* const* pp, int which /* bits */);\n'
                    'const char* g(void);')
    In, Out = h.structs['In'], h.structs['Out']
    assert _fields(Out) == [('x', In, 0), ('y', In, 16), ('p', C.POINTER(In), 32), ('n', C.c_longlong, 40)]
    assert h.protos == {'f': (C.c_int, [C.c_char_p, C.c_ulonglong, C.POINTER(Out), C.c_void_p, C.c_int]), 'g': (C.c_char_p, [])}


def test_reader_takes_the_extern_c_brackets_and_the_include_guard():
    h = _lib.Header('#ifndef X_H_\n#define X_H_\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n'
                    'int f(int a);\n#ifdef __cplusplus\n}\n#endif\n#endif  /* X_H_ */\n')
    assert h.protos == {'f': (C.c_int, [C.c_int])} and h.consts == {}


def test_reader_enum_with_implicit_values():
    h = _lib.Header('enum {\n  A = 0,\n  B,   /* 1 */\n  C = 7, D,\n};\nenum { E, F, G_COUNT };')
    assert h.consts == dict(A=0, B=1, C=7, D=8, E=0, F=1, G_COUNT=2)


@pytest.mark.parametrize('snippet,quoted', [
    ('typedef struct Z { int a; size_t n; } Z;', 'size_t n'),                       # an unknown type
    ('typedef struct Z { float* a, b; } Z;', 'float* a, b'),                        # which of them is a pointer
    ('typedef struct Z { int a : 3; } Z;', 'int a : 3'),
    ('typedef struct Z { int a[UNKNOWN]; } Z;', 'int a[UNKNOWN]'),
    ('typedef struct Z { union { int a; float b; } u; } Z;', 'typedef struct Z { union'),
    ('typedef struct Z { int a; } Y;', 'typedef struct Z'),
    ('int f(int a);\nlong h(int x);', 'long h(int x)'),
    ('int f(int);', 'int f(int)'),
    ('int f(Unknown* u);', 'Unknown* u'),
    ('int f(float x[3]);', 'int f(float x[3])'),                                    # an array parameter is a pointer in C
    ('#ifdef __cplusplus\nint g(int a);\n#endif', '#ifdef __cplusplus'),            # nothing is skipped unread
    ('#ifdef __cplusplus\nextern "C" {\nint g(int a);\n#endif', '#ifdef __cplusplus'),
    ('int f(int a);\nint f(int b);', 'int f(int b)'),
    ('#pragma once\nint f(int a);', '#pragma once'),
    ('int f(int a);\nstatic int x = 3;', 'static int x = 3'),
    ('enum { A = 1 << 2 };', 'A = 1 << 2'),
])
def test_reader_refuses_what_it_does_not_understand(snippet, quoted):
    with pytest.raises(_lib.InfgenHipError) as e:
        _lib.Header(snippet)
    assert quoted in str(e.value)
