"""The ctypes signature of every C-ABI entry, read from include/ffp.h: the header is the one declaration, nothing is kept by hand.

A prototype is `<ret> ffp_name(<params>);`; each type maps by the fixed vocabulary below. Anything else in the header — a type
outside the vocabulary, a function-pointer or array parameter, a statement that is neither a typedef nor a prototype — raises
ValueError and names the statement: no entry is ever skipped."""
import ctypes as C
import re

_SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t, "long long": C.c_longlong, "int32_t": C.c_int32,
            "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
_BYTES = r"void|uint8_t|ffp_[a-z0-9_]+"            # pointees addressed as bytes: raw memory, pixels, handles, ffp_overlay_prim records
# Typed pointers that callers give as a bare address (an int), which POINTER(T) refuses: every device pointer — the header names them d_* —
# and the three host arrays below, which tests/test_gpu_sr_ops.py passes as `array.ctypes.data`.
_ADDRESSES = {("ffp_op_sr_pre", "flat"), ("ffp_op_sr_post", "net"), ("ffp_op_sr_post", "net_first")}
_PROTO = re.compile(r"([\w\s]+?[\s*]+)(ffp_[a-z0-9_]+)\s*\(([^()]*)\)")


def _ctype(decl: str, fn: str = None):
    """The ctypes type of one return type (fn None) or of one parameter of entry `fn`, whose last word is its name."""
    t = re.sub(r"\s*\*\s*", "* ", re.sub(r"\bconst\b", " ", decl)).split()      # e.g. ['uint8_t*', '*', 'imgs'] of `const uint8_t* const* imgs`
    name = t.pop() if fn and len(t) > 1 and "*" not in t[-1] else ""
    base, stars = " ".join(t).replace("*", "").strip(), "".join(t).count("*")
    if "[" in decl or not base:
        raise ValueError(decl)
    if stars == 0 and base == "void" and not fn:
        return None
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars in (1, 2) and re.fullmatch(_BYTES, base):
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    if stars == 1 and base in _SCALARS:
        return C.c_void_p if name.startswith("d_") or (fn, name) in _ADDRESSES else C.POINTER(_SCALARS[base])
    if stars == 2 and base in _SCALARS:
        return C.POINTER(C.POINTER(_SCALARS[base]))
    raise ValueError(decl)


def parse(header_text: str) -> dict:
    """{name: (restype, [argtypes])} of every prototype in the text of a header written like include/ffp.h, in the header's order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    text = re.sub(r"^\s*#.*$|extern\s+\"C\"\s*\{|^\s*\}\s*$", " ", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*(\{[^{}]*\}\s*)?\w+\s*;", " ", text)
    sigs = {}
    for stmt in filter(None, (" ".join(s.split()) for s in text.split(";"))):
        m = _PROTO.fullmatch(stmt)
        try:
            if not m:
                raise ValueError(stmt)
            fn = m.group(2)
            params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
            sigs[fn] = (_ctype(m.group(1)), [_ctype(p, fn) for p in params])
        except ValueError as e:
            raise ValueError(f"include/ffp.h: `{stmt};` is outside the binding's vocabulary (at `{e}`)") from None
    return sigs
