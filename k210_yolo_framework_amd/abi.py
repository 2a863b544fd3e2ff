"""The ctypes signatures of libyolo_hip.so, read from include/yolo_hip.h: the header is the one statement of the ABI.

CPU only; imports neither torch nor the library.  engine.lib() sets what `signatures` returns on the loaded library, so a call passes plain
Python ints and floats, tensors and numpy arrays, and ctypes converts each to the width the header declares - or raises
ctypes.ArgumentError before the call is made."""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Tuple

import numpy as np


class DevPtr:
    """argtype of every pointer parameter: None (NULL), an int, a contiguous torch tensor (device or pinned host: data_ptr()), a
    C-contiguous numpy array, or whatever c_void_p takes (byref(...), ctypes arrays and pointers, c_void_p, create_string_buffer)."""

    @staticmethod
    def from_param(v):
        if type(v) in _AS_THEY_ARE:                # first, and without a try: handles and out-parameters
            return v
        if v is None or type(v) is int:            # (not bool, not a numpy scalar: c_void_p refuses those below)
            return C.c_void_p(v)
        try:
            ptr = v.data_ptr()
        except AttributeError:
            if not isinstance(v, np.ndarray):
                if isinstance(v, (bool, np.generic)):
                    raise TypeError(f'{type(v).__name__} {v!r} passed for a pointer')
                return C.c_void_p.from_param(v)
            if not v.flags['C_CONTIGUOUS']:
                raise TypeError(f'array of shape {v.shape}, strides {v.strides} is not C-contiguous')
            return C.c_void_p(v.ctypes.data)
        if not v.is_contiguous():
            raise TypeError(f'tensor of shape {tuple(v.shape)}, strides {tuple(v.stride())} is not contiguous')
        return C.c_void_p(ptr)


_AS_THEY_ARE = (C.c_void_p, type(C.byref(C.c_int())))

SCALARS = {'int': C.c_int, 'unsigned': C.c_uint, 'long long': C.c_longlong, 'unsigned long long': C.c_ulonglong,
           'size_t': C.c_size_t, 'float': C.c_float, 'double': C.c_double, 'callback_draw_box': DevPtr}
RETURNS = {'int': C.c_int, 'void': None, 'const char *': C.c_char_p, 'unsigned long long': C.c_ulonglong}

_NOT_PROTOTYPES = (r'/\*.*?\*/', r'//[^\n]*', r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*',                     # comments, preprocessor lines
                   r'\btypedef\b[^;{]*(?:\{(?:[^{}]|\{[^{}]*\})*\})?[^;]*;', r'\benum\s*\{[^}]*\}\s*;', r'extern\s*"C"\s*\{')
_PROTOTYPE = re.compile(r'([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)\s*;')


def signatures(header_text: str) -> Dict[str, Tuple[object, List[object]]]:
    """{function: (restype, [argtypes])} of every prototype in the header.  A type outside the tables above raises ValueError."""
    txt = header_text
    for pat in _NOT_PROTOTYPES:
        txt = re.sub(pat, ' ', txt, flags=re.S | re.M)
    sigs = {}
    for ret, name, params in _PROTOTYPE.findall(txt):
        ret = re.sub(r'\s*\*\s*', ' *', ' '.join(ret.split()))
        if ret not in RETURNS:
            raise ValueError(f'{name}: return type {ret!r} is not in abi.RETURNS')
        args = []
        for p in (' '.join(p.split()) for p in params.split(',')):
            if p in ('void', '') and ',' not in params:
                continue
            typ = p.rpartition(' ')[0]
            if '[' in p or ('*' not in p and typ not in SCALARS):
                raise ValueError(f'{name}: parameter {p!r} has a type that is not in abi.SCALARS')
            args.append(DevPtr if '*' in p else SCALARS[typ])
        sigs[name] = (RETURNS[ret], args)
    return sigs
