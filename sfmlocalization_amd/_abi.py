"""include/sfmloc.h as ctypes: the header is the one statement of the C ABI, and capi.py binds what is read here.

This reads that header, not C.  After the comments are stripped it knows `#define NAME <integer>[u]`, `enum { ... };`,
`typedef struct X { fields } X;`, the opaque `typedef struct X X;` and prototypes, with the types of TYPES below and
these rules:
    const char *                            c_char_p
    void *, a pointer to an opaque handle   c_void_p
    one more * on any type                  POINTER(...)
    T name[N]                               POINTER(T) as a parameter, T * N as a field
    a struct of the header                  its Structure
    a return of void                        restype None
Anything else -- a function pointer, a bit-field, a union, `long`, an unknown identifier -- raises AbiError with the
prototype or field it stands in.  Nothing is guessed."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sfmloc.h")

TYPES = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
         **{f"{u}int{n}_t": getattr(C, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}


_INT = r"(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?"
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+%s[ \t]*$" % _INT, re.M)
_MEMBER = re.compile(r"(\w+)(?:\s*=\s*%s)?$" % _INT)
_PROTOTYPE = re.compile(r"([\w\s*]+?)(\w+)\s*\(([^()]*)\)$")
_BASE = re.compile(r"\s*((?:\w+\s+)+)(.*)$", re.S)
_CONST = re.compile(r"\bconst\b")
_DECLARATOR = re.compile(r"\s*((?:\*\s*)*)(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*$")


class AbiError(ImportError):
    pass


class Header:
    """constants: name -> int; opaque: handle names; fields: struct -> [(name, base type, pointer depth, array length)];
    structs: struct -> Structure; prototypes: name -> (restype, argtypes), all in the header's order"""

    def __init__(self, text):
        self.constants, self.opaque, self.fields, self.structs, self.prototypes = {}, set(), {}, {}, {}
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        self.constants.update((name, int(value, 0)) for name, value in _DEFINE.findall(text))
        text = re.sub(r"#\s*ifdef\s+__cplusplus.*?#\s*endif", " ", text, flags=re.S)   # extern "C" { and its }
        text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
        text = re.sub(r"\benum\s*\w*\s*\{([^{}]*)\}\s*;", self._enum, text)
        text = re.sub(r"\btypedef\s+struct\s+(\w+)\s+(\w+)\s*;", lambda m: self.opaque.add(m.group(2)) or " ", text)
        text = re.sub(r"\btypedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;", self._struct, text)
        for decl in filter(None, (" ".join(s.split()) for s in text.split(";"))):
            m = _PROTOTYPE.match(decl)
            if not m:
                raise AbiError(f"sfmloc.h: cannot read the declaration `{decl}`")
            ret, name, params = m.groups()
            where = f"prototype {name}"
            args = [] if params.strip() == "void" else [
                self._ctype(*self._declarators(p, where)[0][1:], True, f"{where}, parameter `{p.strip()}`")
                for p in params.split(",")]
            self.prototypes[name] = (None if ret.strip() == "void" else
                                     self._ctype(*self._declarators(ret + " _", where)[0][1:], True, where), args)

    def _enum(self, m):
        value = -1
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            mm = _MEMBER.match(item)
            if not mm:
                raise AbiError(f"sfmloc.h: cannot read the enum member `{item}`")
            value = self.constants[mm.group(1)] = value + 1 if mm.group(2) is None else int(mm.group(2), 0)
        return " "

    def _struct(self, m):
        body, name = m.groups()
        self.fields[name] = [d for s in body.split(";") if s.strip() for d in self._declarators(s, f"struct {name}")]
        self.structs[name] = type(name, (C.Structure,), {"_fields_": [
            (f, self._ctype(base, depth, n, False, f"field {name}.{f}")) for f, base, depth, n in self.fields[name]]})
        return " "

    def _declarators(self, text, where):
        """`const T *const *a, b[3]` -> [(a, T, 2, None), (b, T, 0, 3)]"""
        m = _BASE.match(text.replace("*", " * "))
        if not m:
            raise AbiError(f"sfmloc.h: {where}: cannot read `{text.strip()}`")
        base = " ".join(m.group(1).split())
        if base != "const char":
            base = " ".join(w for w in base.split() if w != "const")
        out = []
        for d in _CONST.sub(" ", m.group(2)).split(","):
            mm = _DECLARATOR.match(d)
            if not mm:
                raise AbiError(f"sfmloc.h: {where}: cannot read `{d.strip()}` of `{text.strip()}`")
            n = mm.group(3)
            if n is not None and not n.isdigit() and n not in self.constants:
                raise AbiError(f"sfmloc.h: {where}: the length of `{d.strip()}` is not a constant of the header")
            out.append((mm.group(2), base, mm.group(1).count("*"), n if n is None else int(self.constants.get(n, n))))
        return out

    def _ctype(self, base, depth, n, param, where):
        if base == "const char" or base == "void" or base in self.opaque:
            t, depth = (C.c_char_p if base == "const char" else C.c_void_p), depth - 1
        else:
            t = TYPES.get(base) or self.structs.get(base)
        if t is None or depth < 0:
            raise AbiError(f"sfmloc.h: {where}: `{base}` with {max(depth, 0)} `*` is not a type this reader knows")
        for _ in range(depth):
            t = C.POINTER(t)
        return t if n is None else C.POINTER(t) if param else t * n


try:
    with open(HEADER) as _f:
        _header = Header(_f.read())
except OSError as e:
    raise AbiError(f"{HEADER} cannot be read ({e}): the package binds libsfmloc_hip.so from this header") from e

PROTOTYPES = _header.prototypes


def struct(name):
    return _header.structs[name]


def constants(*names):
    """the integer constants SFMLOC_<name> of the header, in the order asked for"""
    return tuple(_header.constants["SFMLOC_" + n] for n in names)
