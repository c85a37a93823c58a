"""The window attention's 16-bit-row entries without a GPU: include/u2mkd_hip_sptr_rows16.h (included by u2mkd_hip.h), the library
and the binding table of u2mkd_amd/_lib.py name the same four entries, each typed with the arguments of its fp32 entry."""
import os
import re

from u2mkd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ['u2mkd_sptr_attention_%s_strided_%s' % (d, t) for d in ('forward', 'backward') for t in ('bf16', 'f16')]


def _code(name):
    text = open(os.path.join(ROOT, 'include', name)).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_header_library_and_table_hold_the_same_four_entries():
    assert re.search(r'^#include "u2mkd_hip_sptr_rows16.h"$', _code('u2mkd_hip.h'), flags=re.M)
    declared = sorted(set(re.findall(r'\b(u2mkd_[a-z0-9_]+)\s*\(', _code('u2mkd_hip_sptr_rows16.h'))))
    assert declared == sorted(ENTRIES) == sorted(_lib.SPTR_ROWS16_SIGNATURES)
    assert not set(ENTRIES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in ENTRIES:
        fn = getattr(lib, name)
        base = name.rsplit('_', 1)[0]
        assert (fn.restype, fn.argtypes) == _lib.SIGNATURES[base] == _lib.SPTR_ROWS16_SIGNATURES[name], name


def test_declarations_take_the_arguments_of_the_fp32_entries():
    """argument for argument: the fp32 declaration with `float` rows replaced by `void` is the 16-bit declaration"""
    def args(text, name):
        body = re.search(r'\b%s\s*\((.*?)\)\s*;' % name, text, flags=re.S).group(1)
        return [re.sub(r'\s+', ' ', a).strip() for a in body.split(',')]
    main, rows16 = _code('u2mkd_hip.h'), _code('u2mkd_hip_sptr_rows16.h')
    row_args = {'q', 'k', 'v', 'out', 'dout', 'dq', 'dk', 'dv'}
    for d in ('forward', 'backward'):
        want = []
        for a in args(main, 'u2mkd_sptr_attention_%s_strided' % d):
            m = re.match(r'(const )?float \*(\w+)$', a)
            want.append('%svoid *%s' % (m.group(1) or '', m.group(2)) if m and m.group(2) in row_args else a)
        for t in ('bf16', 'f16'):
            assert args(rows16, 'u2mkd_sptr_attention_%s_strided_%s' % (d, t)) == want, (d, t)
