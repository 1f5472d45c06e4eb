"""ctypes binding of the C-ABI in include/sympa_hip.h.

The header is READ, not mirrored: parse_header() takes every prototype and every integer #define from its text at import
(PROTOTYPES, SYMBOLS, DEFINES), and bind() sets the types of every declared entry on a library handle.  A
declaration the type table below cannot express is an error that names it, never a guess.

The product path has NO fallback: if libsympa_hip.so is missing or does not export a declared
symbol, importing/using the ops raises.  (Build it with `python -c "import __graft_entry__ as g; g.build()"`;
`make -C sympa_amd/csrc` runs the same function -- there is ONE build path, the one that scans every translation
unit's ISA for the DPP hazard and rebuilds the units that show it.)"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# SYMPA_HIP_LIB: another BUILD of the same library (tools/build_variant.sh: A/B timing, compiler-flag experiments); never a
# different implementation -- the symbol check of bind() applies to it as well
LIB_PATH = os.environ.get("SYMPA_HIP_LIB") or os.path.join(_HERE, "csrc", "libsympa_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sympa_hip.h")

_lib = None
_fast = None          # sympa_amd/_fast.<abi>.so (csrc/torch_binding.cpp) once bound; False when absent or switched off


class SympaHipError(RuntimeError):
    pass


# the C types of the header: by value these three, every pointer as an address, `const char*` only as a return
_BY_VALUE = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double}
_DECLARATION = re.compile(r"([\w\s*]+?)\b(sympa_\w+)\s*\(([^();]*)\)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(SYMPA_\w+)(.*)$", re.M)


def parse_header(text):
    """The prototypes of the header `text` in file order, name -> (return type, [parameter types]), and its integer
    defines, name -> int."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)       # the comments quote calls like sympa_model_forward(...)
    defines = {}
    for name, value in _DEFINE.findall(text):
        m = re.fullmatch(r"\s*(?:(\d+)|\((-?\d+)\))\s*", value)
        if m:
            defines[name] = int(m.group(1) or m.group(2))
        elif value.strip():                                  # no value at all: the include guard
            raise SympaHipError(f"sympa_hip.h: #define {name} is not an integer: {value.strip()!r}")
    code = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    prototypes = {}
    for m in _DECLARATION.finditer(code):
        ret, name, params = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
        if name in prototypes:
            raise SympaHipError(f"sympa_hip.h: {name} is declared twice")
        if ret == "const char*":
            restype = ctypes.c_char_p
        elif ret in _BY_VALUE:
            restype = _BY_VALUE[ret]
        else:
            raise SympaHipError(f"sympa_hip.h: {name}: no ctypes type for the return type {ret!r}")
        types = []
        for p in [] if params == "void" else params.split(","):
            by_value = re.fullmatch(r"\s*(\w+)\s+\w+\s*", p)     # `type name`
            if "*" in p:
                types.append(ctypes.c_void_p)
            elif by_value and by_value.group(1) in _BY_VALUE:
                types.append(_BY_VALUE[by_value.group(1)])
            else:
                raise SympaHipError(f"sympa_hip.h: {name}: no ctypes type for the parameter {p.strip()!r}")
        prototypes[name] = (restype, types)
    left = re.search(r"sympa_\w*\s*\(", _DECLARATION.sub(";", code))
    if left:
        raise SympaHipError(f"sympa_hip.h: cannot read the declaration at {left.group(0)!r}")
    return prototypes, defines


def read_header():
    if not os.path.exists(HEADER_PATH):
        raise SympaHipError(f"{HEADER_PATH} not found: the ctypes prototypes and the SYMPA_* constants are read from it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


PROTOTYPES, DEFINES = read_header()
SYMBOLS = tuple(PROTOTYPES)     # every symbol include/sympa_hip.h declares (the tests read the header with a regex of their own)


def fast():
    """The thin torch binding of sympa_model_forward (csrc/torch_binding.cpp: tensors in, one C call), bound to the SAME
    loaded libsympa_hip.so as the ctypes prototypes -- or None when it is not built (`__graft_entry__.build()` builds it) or
    SYMPA_NO_FAST_BINDING is set: callers then go through ctypes, which calls the same C-ABI entry of the same library."""
    global _fast
    if _fast is None:
        _fast = False
        if not os.environ.get("SYMPA_NO_FAST_BINDING"):
            try:
                import torch  # noqa: F401  (the extension links against libtorch)
                from sympa_amd import _fast as mod
                lib = load()
                mod.bind(ctypes.cast(lib.sympa_model_forward, ctypes.c_void_p).value,
                         ctypes.cast(lib.sympa_last_error, ctypes.c_void_p).value)
                _fast = mod
            except ImportError:
                _fast = False
    return _fast or None


def bind(cdll):
    """Sets the header's prototypes on a handle of (a build of) the library, which must export every declared symbol."""
    for s in SYMBOLS:
        if not hasattr(cdll, s):
            raise SympaHipError(f"{getattr(cdll, '_name', cdll)} does not export {s}")
    for s, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(cdll, s)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def load():
    """Loads libsympa_hip.so once and sets the prototypes.  Raises SympaHipError when absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SympaHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. There is no CPU fallback; "
            "run __graft_entry__.build() (hipcc --offload-arch=gfx950)."
        )
    _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc):
    if rc != 0:
        msg = load().sympa_last_error().decode()
        raise SympaHipError(f"sympa_hip call failed (code {rc}): {msg}")
