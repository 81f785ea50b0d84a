"""ctypes binding of libslu_hip.so (C ABI declared in include/slu_hip.h).

The library is built in-tree by csrc/build.sh (hipcc --offload-arch=gfx950).  There is no CPU or
PyTorch fallback: if the shared object is missing, or a call fails, this module raises.
"""
import ctypes
import os
import re

from . import knobs as _knobs

_HERE = os.path.dirname(os.path.abspath(__file__))
# SLU_HIP_LIB: another build of the same ABI (the probe build of tools/gru_probe.py); the product never sets it
LIB_PATH = _knobs.get("SLU_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libslu_hip.so")
# the header csrc/build.sh compiles every unit against, found the way build.sh finds it; SLU_HIP_LIB changes the .so only
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "include", "slu_hip.h"))

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}


class SluHipError(RuntimeError):
    pass


def _ctype(ctype, func, returned=False, header="slu_hip.h"):
    """The one mapping rule, by C type: any parameter with a `*` is c_void_p (device pointers, host arrays, out-parameters,
    hipStream_t as void*), a returned const char* is c_char_p, every scalar comes from _SCALARS.  Nothing has a default."""
    words = " ".join(w for w in ctype.replace("*", " * ").split() if w != "const")
    if returned and words == "char *":
        return ctypes.c_char_p
    if "*" in words and not returned:
        return ctypes.c_void_p
    if words not in _SCALARS:
        raise SluHipError("%s: %s: no ctypes mapping for the %s type '%s'"
                          % (header, func, "return" if returned else "parameter", " ".join(ctype.split())))
    return _SCALARS[words]


def parse_header(text, version_macro="SLU_ABI_VERSION", header="slu_hip.h"):
    """Header text -> ({name: (restype, [argtypes])}, SLU_ABI_VERSION).  Every statement of the header that is not a typedef
    must be a `RET slu_name(TYPE name, ...);` declaration; anything this cannot read raises SluHipError.  version_macro:
    the name of the header's version #define, header: the file name the errors carry (include/slu_decode.h has its own
    of both, slu_hip/decode.py)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(\d+)[ \t]*$" % re.escape(version_macro), text, flags=re.M)
    if not version:
        raise SluHipError("%s: no #define %s" % (header, version_macro))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\btypedef\s+(?:enum|struct)\b[^{};]*\{[^{}]*\}[^{};]*;", "", text)
    text = re.sub(r'\bextern\s+"C"\s*\{|\}\s*\Z', "", text)
    table = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\b(slu_\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise SluHipError("%s: not a function declaration: '%s'" % (header, " ".join(stmt.split())))
        ret, func, params = m.groups()
        if func in table:
            raise SluHipError("%s: %s is declared twice" % (header, func))
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            p = re.fullmatch(r"\s*(\w[\w\s*]*[\s*])(\w+)\s*", param)
            if not p:                  # function pointers and arrays have ( ) [ ]; an unnamed one has no trailing identifier
                raise SluHipError("%s: %s: parameter '%s' is not `TYPE name`" % (header, func, " ".join(param.split())))
            args.append(_ctype(p.group(1), func, header=header))
        table[func] = (_ctype(ret, func, returned=True, header=header), args)
    return table, int(version.group(1))


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return f.read()
    except OSError as e:
        raise SluHipError("the C ABI header %s cannot be read (%s); the binding table is derived from it"
                          % (HEADER_PATH, e)) from None


# name -> (restype, argtypes), and SLU_ABI_VERSION: both read from include/slu_hip.h at import
SIGNATURES, ABI_VERSION = parse_header(_read_header())

_lib = None


def load():
    """Loads libslu_hip.so (once).  Raises SluHipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime (libamdhip64); it must be the one already resident when
    # libslu_hip.so is mapped, or the process ends up with two runtimes and no visible device.
    import torch  # noqa: F401
    if not os.path.isfile(LIB_PATH):
        raise SluHipError(
            "libslu_hip.so not found at %s — build it with end-to-end-slu_amd/csrc/build.sh "
            "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the ABI and this table disagree
        fn.restype = res
        fn.argtypes = args
    if lib.slu_version() != ABI_VERSION:
        raise SluHipError("libslu_hip.so ABI version %d, expected %d (rebuild with csrc/build.sh)"
                          % (lib.slu_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().slu_last_error().decode("utf-8", "replace")
        raise SluHipError("%s failed (status %d): %s" % (what or "libslu_hip call", rc, msg))


def require_gfx950():
    lib = load()
    check(lib.slu_device_check(), "slu_device_check")
