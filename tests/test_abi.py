"""CPU: sfmlocalization_amd/_abi.py reads include/sfmloc.h -- the reader's rules on small header strings, the real header
read whole (no prototype and no struct dropped, every entry point bound as declared), and the layout of every derived
Structure and of RELPOSE_RESULT against what the C compiler gives the header's structs."""
import ctypes as C
import os
import re
import subprocess

import pytest

from sfmlocalization_amd import _abi, capi
from test_capi_load import HEADER, ROOT, declared_symbols

P = C.POINTER

SMALL = r'''
#ifndef T_H
#define T_H
#ifdef __cplusplus
extern "C" {
#endif
#define T_HEX 0xFFu
#define T_DEC 7   /* a comment; with ( and int fake_one(int a); inside */
#define T_U 64u
#define T_EXPR (1 << 3)
enum { T_A, T_B, T_C = -4, T_D, T_E = 0x10 };
/* int fake_two(void); */
typedef struct t_handle t_handle;
typedef struct t_rec {
  double R[9], s;          /* two declarators; the second a scalar */
  const float *p;
  uint8_t tag[T_DEC];
  t_handle *h;
} t_rec;
typedef struct t_outer { t_rec inner; uint64_t n; } t_outer;
const char *t_text(void);
void t_fill(t_rec *out,
            const uint8_t *const *rows,
            double R[9]);
int  t_open(const char *path, t_handle **out, size_t n, unsigned flags);
const void *t_dev(const t_handle *h, const char **name, const t_outer *o);
uint64_t t_count(t_handle *const *hs, float x, int16_t y);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_reader_on_a_small_header():
    h = _abi.Header(SMALL)
    assert h.constants == {"T_HEX": 255, "T_DEC": 7, "T_U": 64, "T_A": 0, "T_B": 1, "T_C": -4, "T_D": -3, "T_E": 16}
    assert h.opaque == {"t_handle"}
    assert list(h.prototypes) == ["t_text", "t_fill", "t_open", "t_dev", "t_count"]      # neither fake prototype
    rec, outer = h.structs["t_rec"], h.structs["t_outer"]
    assert h.fields["t_rec"] == [("R", "double", 0, 9), ("s", "double", 0, None), ("p", "float", 1, None),
                                 ("tag", "uint8_t", 0, 7), ("h", "t_handle", 1, None)]
    assert [(f, t) for f, t in rec._fields_] == [("R", C.c_double * 9), ("s", C.c_double), ("p", P(C.c_float)),
                                                 ("tag", C.c_uint8 * 7), ("h", C.c_void_p)]
    assert outer._fields_ == [("inner", rec), ("n", C.c_uint64)]
    assert h.prototypes["t_text"] == (C.c_char_p, [])                                     # a (void) list
    assert h.prototypes["t_fill"] == (None, [P(rec), P(P(C.c_uint8)), P(C.c_double)])     # three lines; T *const *; R[9]
    assert h.prototypes["t_open"] == (C.c_int, [C.c_char_p, P(C.c_void_p), C.c_size_t, C.c_uint])
    assert h.prototypes["t_dev"] == (C.c_void_p, [C.c_void_p, P(C.c_char_p), P(outer)])
    assert h.prototypes["t_count"] == (C.c_uint64, [P(C.c_void_p), C.c_float, C.c_int16])


@pytest.mark.parametrize("text,name", [
    ("int t_cb(void (*cb)(int), int n);", "t_cb"),                                        # a function pointer
    ("typedef struct t_b { int flag : 3; } t_b;", "t_b"),                                 # a bit-field
    ("typedef union t_u { int a; float b; } t_u;", "t_u"),                                # a union
    ("int t_long(long n);", "t_long"),
    ("int t_ull(unsigned long long n);", "t_ull"),                                        # not `unsigned` named `long`
    ("typedef struct t_l { unsigned long long n; } t_l;", "t_l.n"),
    ("int t_unknown(t_nobody *p);", "t_unknown"),
    ("typedef struct t_f { t_nobody x; } t_f;", "t_f.x"),
    ("int t_char(char *s);", "t_char"),                                                   # only `const char *` is a string
    ("int t_byvalue(void x);", "t_byvalue"),
    ("int t_noname(int);", "t_noname"),
    ("int t_empty();", "t_empty"),
    ("typedef struct t_a { double v[T_NOT_DEFINED]; } t_a;", "t_a"),
    ("enum { T_X = 1 + 2 };", "T_X"),
])
def test_reader_refuses_what_its_table_does_not_cover(text, name):
    with pytest.raises(_abi.AbiError) as e:
        _abi.Header(text)
    assert name in str(e.value)


def test_real_header_is_read_whole():
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert sorted(_abi.PROTOTYPES) == declared_symbols() and len(_abi.PROTOTYPES) >= 164
    assert capi.SYMBOLS == list(_abi.PROTOTYPES)
    assert sorted(_abi._header.structs) == sorted(re.findall(r"\}\s*(sfmloc_\w+)\s*;", hdr))
    assert len(_abi._header.structs) >= 19
    assert sorted(_abi._header.opaque) == sorted(re.findall(r"typedef\s+struct\s+(sfmloc_\w+)\s+\1\s*;", hdr))


def test_every_entry_point_is_bound_as_declared():
    L = capi._L()
    hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr).group(1).strip()
        f = getattr(L, name)
        assert f.argtypes is not None and list(f.argtypes) == argtypes, name
        assert len(f.argtypes) == (0 if params == "void" else len(params.split(","))), name
        assert f.restype is restype, name
    assert L.sfmloc_view_list_close.restype is None and L.sfmloc_last_error.restype is C.c_char_p
    assert L.sfmloc_imgbow_compute_batch.argtypes[1] is P(P(C.c_uint8))
    assert L.sfmloc_relpose_results.argtypes[1] is P(capi.RelposeResult)


def test_layout_of_every_struct_matches_the_compiler(tmp_path):
    """sizeof of every struct of the header, offsetof and size of every field, from a C program generated from the parsed
    structs: the derived Structures and RELPOSE_RESULT agree with all of it"""
    fields = _abi._header.fields
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "sfmloc.h"', "int main(void){"]
    for s, fs in fields.items():
        lines.append(f'  printf("{s} - %zu 0\\n", sizeof({s}));')
        lines += [f'  printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s} *)0)->{f}));' for f, _, _, _ in fs]
    (tmp_path / "t.c").write_text("\n".join(lines + ["  return 0; }", ""]))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")])
    got = [ln.split() for ln in subprocess.check_output([str(tmp_path / "t")]).decode().splitlines()]
    c = {(s, f): (int(a), int(b)) for s, f, a, b in got}
    assert len(c) == len(fields) + sum(len(fs) for fs in fields.values()) and len(c) > 190
    for s, fs in fields.items():
        cls = _abi.struct(s)
        assert C.sizeof(cls) == c[s, "-"][0], s
        assert [f for f, _ in cls._fields_] == [f for f, _, _, _ in fs]
        for f, _, _, _ in fs:
            d = getattr(cls, f)
            assert (d.offset, d.size) == c[s, f], (s, f)
    r = "sfmloc_relpose_result"
    assert capi.RELPOSE_RESULT.itemsize == c[r, "-"][0] == C.sizeof(capi.RelposeResult)
    assert list(capi.RELPOSE_RESULT.names) == [f for f, _, _, _ in fields[r]]
    for f in capi.RELPOSE_RESULT.names:
        dt, off = capi.RELPOSE_RESULT.fields[f][:2]
        assert (off, dt.itemsize) == c[r, f], f


def test_constants_come_from_the_header():
    k = _abi._header.constants
    assert (capi.NOMATCH, capi.COLOR_CHUNK, capi.K_COUNT, capi.ENOMEM) == (0xFFFFFFFF, 64, 8, -6)
    assert (k["SFMLOC_ABI_VERSION"], k["SFMLOC_DESC_BYTES"], k["SFMLOC_MAX_QUERY_ROWS"]) == (2, 64, 65535)
    assert (capi.OK, capi.EINVAL, capi.ENODEV, capi.EHIP, capi.EIO, capi.ECAP) == (0, -1, -2, -3, -4, -5)
    assert (capi.BA_ROTATION, capi.BA_TRANSLATION, capi.BA_INTRINSICS, capi.BA_STRUCTURE) == (1, 2, 4, 8)
    assert (capi.TRI_ROBUST, capi.TRI_BLIND, capi.MERGE_SIMILARITY, capi.MERGE_AFFINE) == (0, 1, 0, 1)
    assert (capi.K_HAMMING, capi.K_COMPACT, capi.K_FMATRIX, capi.K_MATCHSET, capi.K_P3P, capi.K_BOW) == (0, 1, 2, 3, 4, 5)
