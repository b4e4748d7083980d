"""ctypes binding of libinfgen_hip.so, derived at import from the C ABI's one source, include/infgen_hip.h.

The product path has NO fallback: if the header or the shared library is missing, or an entry point fails,
an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import threading
import os
import re
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libinfgen_hip.so')
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'infgen_hip.h')     # ../../include/infgen_hip.h of csrc/Makefile

_p = C.c_void_p
_i = C.c_int
_f = C.c_float


class InfgenHipError(RuntimeError):
    pass


# ---- a reader for the restricted C of infgen_hip.h (its style rules are in the header's own comment block), not a C parser:
# whatever it does not understand is an error that quotes the text, never a skipped declaration
_SCALARS = {'int': _i, 'float': _f, 'double': C.c_double, 'unsigned': C.c_uint, 'long long': C.c_longlong,
            'unsigned long long': C.c_ulonglong, 'uint8_t': C.c_ubyte, 'unsigned char': C.c_ubyte, 'uint32_t': C.c_uint32}
_TOP = re.compile(r'\s*(?:enum\s*\{(?P<enum>[^{};]*)\}\s*;'
                  r'|typedef\s+struct\s+(?P<tag>\w+)\s*\{(?P<body>[^{}]*)\}\s*(?P<name>\w+)\s*;'
                  r'|(?P<ret>[\w\s*]+?)\b(?P<fn>\w+)\s*\((?P<args>[^;{}()]*)\)\s*;)')
_DECLARATOR = re.compile(r'\s*(?P<type>[\w\s*]*?)\s*\b(?P<name>[A-Za-z_]\w*)\s*(?:\[\s*(?P<dim>\w+)\s*\])?\s*')


def _refuse(text: str):
    raise InfgenHipError(f'infgen_hip.h: cannot read {" ".join(text.split())[:160]!r}')


class Header:
    """consts: #define / enum name -> int; structs: C name -> ctypes.Structure class; protos: name -> (restype, [argtypes])"""

    def __init__(self, text: str):
        self.consts, self.structs, self.protos, self._types = {}, {}, {}, {}
        text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
        # the two extern "C" brackets and nothing else (any other #ifdef is refused below)
        text = re.sub(r'^#ifdef __cplusplus\n\s*(?:extern "C" \{|\})\s*\n#endif[ \t]*$', '', text, flags=re.M)
        for line in re.findall(r'^[ \t]*#.*$', text, flags=re.M):
            m = re.fullmatch(r'\s*#\s*define\s+(\w+)\s+(-?\d+)\s*', line)
            if m:
                self.consts[m[1]] = int(m[2])
            elif not re.fullmatch(r'\s*#\s*(ifndef\s+\w+|define\s+\w+|include\s*<[\w./]+>|endif)\s*', line):
                _refuse(line)
        text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
        pos, end = 0, len(text.rstrip())
        while pos < end:
            m = _TOP.match(text, pos)
            if not m:
                _refuse(text[pos:])
            pos = m.end()
            if m['enum'] is not None:
                self._enum(m['enum'])
            elif m['body'] is not None:
                if m['tag'] != m['name'] or m['name'] in self.structs:
                    _refuse(m[0])
                fields = [f for stmt in m['body'].split(';') if stmt.strip() for f in self._decl(stmt)]
                self.structs[m['name']] = type(m['name'], (C.Structure,), {'_fields_': fields})
            else:
                res = self._ctype(m['ret'], m[0])
                if res not in (_i, C.c_char_p) or m['fn'] in self.protos:
                    _refuse(m[0])
                args = [] if m['args'].strip() in ('', 'void') else m['args'].split(',')
                self.protos[m['fn']] = (res, [self._decl(a, m[0], array=False)[0][1] for a in args])

    def _enum(self, body: str):
        value = -1
        for item in body.split(','):
            m = re.fullmatch(r'\s*([A-Za-z_]\w*)\s*(?:=\s*(-?\d+)\s*)?', item)
            if m:
                value = int(m[2]) if m[2] else value + 1
                self.consts[m[1]] = value
            elif item.strip():
                _refuse(item)

    def _ctype(self, spec: str, where: str):
        if spec not in self._types:             # a few dozen spellings serve the header's thousand declarations
            self._types[spec] = self._lookup(spec, where)
        return self._types[spec]

    def _lookup(self, spec: str, where: str):
        words = re.findall(r'\w+', spec)
        base, stars = ' '.join(w for w in words if w != 'const'), spec.count('*')
        if stars == 0 and base in _SCALARS:
            return _SCALARS[base]
        if stars == 0 and base in self.structs:
            return self.structs[base]
        if stars == 1 and base == 'char' and 'const' in words:
            return C.c_char_p
        if stars == 1 and base in self.structs:
            return C.POINTER(self.structs[base])
        if stars and (base in _SCALARS or base == 'void'):
            return _p
        _refuse(where)

    def _decl(self, text: str, where: str = '', array: bool = True):
        """'const float* a[N]' -> [('a', c_void_p * N)]; 'int S, A_cap' -> [('S', c_int), ('A_cap', c_int)]; where: the text to quote;
        array = False (a parameter): a dimension is refused"""
        where = where or text
        out, parts = [], text.split(',')
        for k, part in enumerate(parts):
            m = _DECLARATOR.fullmatch(part)
            # the type stands in front of the first declarator only, and a pointer type declares one name ('float* a, b' is refused)
            if not m or bool(m['type']) != (k == 0) or (len(parts) > 1 and '*' in m['type']):
                _refuse(where)
            if k == 0:
                ctype = self._ctype(m['type'], where)
            dim = m['dim']
            if dim is not None and not (array and (dim.isdigit() or dim in self.consts)):
                _refuse(where)
            out.append((m['name'], ctype if dim is None else ctype * int(self.consts.get(dim, dim))))
        return out


def read_header(path: str) -> Header:
    if not os.path.exists(path):
        raise InfgenHipError(f'{path} not found: the binding is derived from the C header (in-tree use only)')
    with open(path) as f:
        return Header(f.read())


HEADER = read_header(HEADER_PATH)
LinearDesc, EdgeBuf, RadiusEdges, Insertion, Options, Sampling, Rollout, BatchIngest = (
    HEADER.structs['Infgen' + n] for n in ('LinearDesc', 'EdgeBuf', 'RadiusEdges', 'Insertion', 'Options', 'Sampling', 'Rollout',
                                           'BatchIngest'))
SYMBOLS = HEADER.protos                        # symbol -> (restype, argtypes)
# the one struct pointer that stays untyped: callers hand this entry the context's address as an integer (ctypes.addressof)
SYMBOLS['infgen_raw_feature_rows'][1][0] = _p
MAX_LAYERS, VM_SCRATCH_DOUBLES, GRID_OVERLAP_MAX_CELLS = (
    HEADER.consts['INFGEN_' + n] for n in ('MAX_LAYERS', 'VM_SCRATCH_DOUBLES', 'GRID_OVERLAP_MAX_CELLS'))
OPTIONS_VALUE_BYTES = Options.row_groups.offset       # the integer switches of Options (the two pointers follow)

Q_ATTN_PACK_SIZE, Q_FOURIER_N2, Q_FOURIER_N3, Q_FOURIER_N4, Q_TILE_ROWS, Q_EDGE_ATTN_CAP, Q_MAX_AGENTS, \
    Q_ABI_VERSION, Q_SIZEOF_ROLLOUT, Q_ATTN_SPLIT_ROWS, Q_HEADS_SAMPLE_K = (
        HEADER.consts['INFGEN_Q_' + n] for n in ('ATTN_PACK_SIZE', 'FOURIER_PACK_SIZE_N2', 'FOURIER_PACK_SIZE_N3',
                                                 'FOURIER_PACK_SIZE_N4', 'TILE_ROWS', 'EDGE_ATTN_CAP', 'MAX_AGENTS', 'ABI_VERSION',
                                                 'SIZEOF_ROLLOUT', 'ATTN_SPLIT_ROWS', 'HEADS_SAMPLE_K'))

# the profiler's names of the INFGEN_KID_* slots, in enum order (the C names do not map onto the kernels' names)
KERNEL_IDS = ['k_linear', 'k_fourier', 'k_attn_pre', 'k_edge_attn', 'k_attn_post', 'k_heads', 'k_build_edges',
              'k_integrate', 'k_rawfeat_prep', 'k_map_graph', 'k_map_head']
assert len(KERNEL_IDS) == HEADER.consts['INFGEN_KID_COUNT'], 'KERNEL_IDS and the INFGEN_KID_* enum of infgen_hip.h disagree'

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libinfgen_hip.so; raises if it is missing (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise InfgenHipError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            f'or `make -C infgen_amd/csrc` (there is no CPU fallback for the product path)')
    # torch first: its wheel bundles its own libamdhip64 (ROCm 7.0), libinfgen_hip.so is linked against the system's (/opt/rocm).
    # Whichever HIP runtime is mapped first serves both (same SONAME); with the library loaded BEFORE torch the process ends up with
    # two runtimes and the library's sees no device ("no ROCm-capable device is detected" from the first launch - found with
    # `python __graft_entry__.py smoke`, whose build() loads the library before smoke() imports torch)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.infgen_layout_query(Q_SIZEOF_ROLLOUT) != C.sizeof(Rollout):
        raise InfgenHipError('InfgenRollout layout mismatch between include/infgen_hip.h and the built library (rebuild it): '
                             f'{lib.infgen_layout_query(Q_SIZEOF_ROLLOUT)} != {C.sizeof(Rollout)}')
    _lib = lib
    return lib


def check(rc: int, what: str = '') -> None:
    if rc != 0:
        msg = load().infgen_last_error()
        raise InfgenHipError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')


def ptr(t) -> Optional[int]:
    """device pointer of a torch tensor (None -> NULL)"""
    if t is None:
        return None
    assert t.is_contiguous(), 'tensor must be contiguous'
    return t.data_ptr()


_tl = threading.local()


class thread_options:
    """context manager: the calling thread's option block for operator-level entries (infgen_thread_options, include/infgen_hip.h);
    nests (the outer block is restored on exit)"""

    def __init__(self, opts: 'Options'):
        self.opts, self.prev = opts, None

    def __enter__(self):
        lib = load()
        depth = getattr(_tl, 'depth', 0)
        if depth > 0:
            self.prev = Options()
            check(lib.infgen_get_effective_options(C.byref(self.prev)), 'infgen_get_effective_options')
        check(lib.infgen_thread_options(C.byref(self.opts)), 'infgen_thread_options')
        _tl.depth = depth + 1
        return self

    def __exit__(self, *exc):
        _tl.depth -= 1
        check(load().infgen_thread_options(C.byref(self.prev) if self.prev is not None else None), 'infgen_thread_options')
        return False


_prof_mask = 0


def prof_enable(mask: int, max_launches: int = 20000) -> None:
    global _prof_mask
    check(load().infgen_prof_enable(mask, max_launches), 'infgen_prof_enable')
    _prof_mask = int(mask)


def prof_set_stride(stride: int) -> None:
    """after prof_enable: only every stride-th launch inside decode steps carries an event pair (bench.py's timed region)"""
    check(load().infgen_prof_set_stride(int(stride)), 'infgen_prof_set_stride')


def prof_seen():
    """-> {kernel: dict(seen, seen_step)}: launches of the selected kernels since prof_enable, bracketed or not"""
    n = len(KERNEL_IDS)
    seen, seen_step = (_i * n)(), (_i * n)()
    check(load().infgen_prof_seen(seen, seen_step), 'infgen_prof_seen')
    return {k: dict(seen=seen[i], seen_step=seen_step[i]) for i, k in enumerate(KERNEL_IDS)}


def prof_active() -> bool:
    """per-kernel HIP-event profiling is on (bench.py's roofline legs): launches must be issued eagerly, not replayed"""
    return _prof_mask != 0


def prof_collect():
    """-> {kernel: dict(ms, calls, macs, step_ms, step_calls)} of the launches recorded since prof_enable; synchronises"""
    n = len(KERNEL_IDS)
    ms = (C.c_double * n)()
    calls = (_i * n)()
    macs = (C.c_double * n)()
    rows = (C.c_ulonglong * 16)()
    sms = (C.c_double * n)()
    scalls = (_i * n)()
    check(load().infgen_prof_collect_steps(ms, calls, macs, rows, sms, scalls), 'infgen_prof_collect_steps')
    # step_ms / step_calls: the launches issued inside decode steps (the rest: prologue and operator-level calls)
    out = {k: dict(ms=ms[i], calls=calls[i], macs=macs[i], step_ms=sms[i], step_calls=scalls[i]) for i, k in enumerate(KERNEL_IDS)}
    # edges built per set; every decode step's sets are consumed by one edge-attention launch per layer
    out['k_edge_attn']['edges_built'] = dict(temporal=int(rows[8]), map=int(rows[9]), agent=int(rows[10]))
    # FourierEmbedding: n x (129x128 + 128x128) + 128x128 MACs per row (reference layers.py:126-141)
    out['k_fourier']['macs'] = float(sum(rows[nd] * (nd * 32896 + 16384) for nd in range(8)))
    out['k_fourier']['rows'] = {nd: int(rows[nd]) for nd in range(8) if rows[nd]}
    return out
