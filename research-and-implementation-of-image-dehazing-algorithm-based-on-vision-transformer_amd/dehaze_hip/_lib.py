"""ctypes binding of libdehaze_hip.so.  The C-ABI is stated ONCE, in include/dehaze_hip.h: the argument and return types of every
entry are read off that header when this module is imported (parse_header), not restated here.

There is NO fallback: if the shared object is missing the import of the product fails loudly with
the build instruction; nothing here routes to PyTorch eager or to the CPU oracle.  A missing header fails the same way.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DHZ_LIB_PATH") or os.path.join(_HERE, "libdehaze_hip.so")   # override: A/B of two builds

HEADER_PATH = os.path.join(_HERE, os.pardir, os.pardir, "include", "dehaze_hip.h")           # where csrc/build.sh finds it

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"(\w[\w\s*]*?)\b(dhz_\w+)\s*\(([^()]*)\)")


def parse_header(text):
    """The prototypes of a C header of this library's kind -> ({name: [ctypes type per parameter]}, {name: ctypes return type}).  Every
    parameter with a `*` is a c_void_p; the scalar and return types are the ones in the two tables above.  Comments, preprocessor lines
    and the `extern "C"` braces are dropped; whatever is left must be `ret dhz_name(params);` statements, each of which may span lines.
    Anything else - another type, a statement that names a dhz_ entry without being a whole prototype - raises ValueError with the
    statement in it: a binding that guessed would push garbage into a launch."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s*"C"\s*\{|\}', " ", text)
    args, rets = {}, {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = _PROTOTYPE.fullmatch(stmt)
        if m is None:
            raise ValueError(f"not a prototype `ret dhz_name(params);`: {stmt!r}")
        ret, name, params = re.sub(r"\s*\*\s*", "*", m.group(1)).strip(), m.group(2), m.group(3).strip()
        if ret not in _RETURNS:
            raise ValueError(f"return type {ret!r} outside {sorted(_RETURNS)}: {stmt!r}")
        if name in args:
            raise ValueError(f"declared twice: {stmt!r}")
        types = []
        for param in ([] if params in ("", "void") else params.split(",")):
            if "*" in param:
                types.append(ctypes.c_void_p)
                continue
            scalar = re.fullmatch(r"\s*(\w+)(\s+\w+)?\s*", param)               # `type name` or `type`, the type one word
            if scalar is None or scalar.group(1) not in _SCALARS:
                raise ValueError(f"parameter {param.strip()!r}: scalar type outside {sorted(_SCALARS)}: {stmt!r}")
            types.append(_SCALARS[scalar.group(1)])
        args[name], rets[name] = types, _RETURNS[ret]
    return args, rets


def _declared():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f"{HEADER_PATH} not found: the binding is derived from the header the library is built from "
                          "(include/dehaze_hip.h of this repository); there is no second statement of the C-ABI to fall back on.")
    with open(HEADER_PATH) as f:
        args, rets = parse_header(f.read())
    return args, {name: t for name, t in rets.items() if t is not ctypes.c_int}


# name -> argtypes, name -> return type where it is not int: read off the header at import (tests read SIGNATURES without load())
SIGNATURES, _RESTYPE = _declared()

_lib = None


class DehazeHipError(RuntimeError):
    pass


def load():
    """Load the shared object (once).  Raises ImportError with the build recipe if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension is mandatory (there is no PyTorch/CPU fallback). "
            "Build it with `python __graft_entry__.py build` or `csrc/build.sh` (hipcc --offload-arch=gfx950).")
    lib = ctypes.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header / library mismatch: fail loudly
        fn.argtypes = args
        fn.restype = _RESTYPE.get(name, ctypes.c_int)
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().dhz_last_error()
        raise DehazeHipError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def call(name, *args):
    check(getattr(load(), name)(*args), name)
