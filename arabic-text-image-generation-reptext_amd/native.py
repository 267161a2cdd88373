"""ctypes binding of librt_reptext_hip.so, derived from the C ABI declared in include/reptext_hip.h.

This is the only way compute leaves Python: there is NO CPU or eager-PyTorch fallback. If the shared
library has not been built (``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C csrc``)
importing a symbol raises ``NativeLibraryMissing``; if a call is rejected ``NativeCallError`` carries the
RT_E_* / hipError code.

Nothing of the header is repeated here. It is parsed once at import: every ``#define RT_<NAME> <integer>`` becomes a
module attribute (``RT_GEMM_MAX_GROUPS`` ...; ``ABI_VERSION`` is ``RT_ABI_VERSION``), every ``typedef struct`` a
``ctypes.Structure`` named after it (``rt_gemm_group`` -> ``GemmGroup``, ``SkinnyGroup``, ``LnSegment``, ``LoraTerm``), every
prototype an entry of ``SIGNATURES`` (name -> argtypes) and ``RESTYPES``. A new entry point is declared in the header only.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "librt_reptext_hip.so"
LIB_PATH = os.path.join(_HERE, LIB_NAME)
HEADER_PATH = os.path.join(_HERE, "..", "include", "reptext_hip.h")


class NativeLibraryMissing(RuntimeError):
    pass


class HeaderParseError(ValueError):
    pass


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
_POINTEES = set(_SCALARS) | {"void", "uint8_t", "uint32_t"}
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*((?:\w+\s*,\s*)*\w+)?")
_STATEMENT = re.compile(r"\s*(?:typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)|((?:const\s+)?\w+\s*\*?)\s*(rt_\w+)\s*\(([^()]*)\))\s*;")
_DEFINE = re.compile(r"#\s*define\s+(\w+)\s*(.*)")


def _declaration(text: str, structs: dict, named: bool):
    """(ctype, [names]) of ``const T* a`` / ``T a, b, c`` / (named=False) a bare return type. Anything else raises."""
    m = _DECL.fullmatch(text.strip())
    if not m or bool(m.group(3)) != named:
        raise HeaderParseError(f"unrecognised declaration: {text.strip()!r}")
    base, star, names = m.groups()
    if not star and base in _SCALARS:
        ctype = _SCALARS[base]
    elif star and base in structs:
        ctype = C.POINTER(structs[base])
    elif star and base in _POINTEES:
        ctype = C.c_void_p
    elif star and base == "char" and not named:
        ctype = C.c_char_p
    else:
        raise HeaderParseError(f"unrecognised type in: {text.strip()!r}")
    return ctype, re.split(r"\s*,\s*", names) if names else []


def parse_header(text: str):
    """(constants, structs, signatures, restypes) of a C header in the dialect of include/reptext_hip.h: integer ``#define RT_*``,
    ``typedef struct ... { ... } name;`` of scalar and pointer fields, and ``ret rt_name(args);`` prototypes. Strict: a type,
    declarator, define or statement outside that dialect raises HeaderParseError instead of being skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S)          # the extern "C" braces
    constants, structs, signatures, restypes = {}, {}, {}, {}
    for line in re.findall(r"^\s*(#.*)$", text, flags=re.M):
        m = _DEFINE.match(line)
        if m and m.group(2).strip():
            value = re.fullmatch(r"\(?\s*(-?\d+)\s*\)?", m.group(2).strip())
            if not m.group(1).startswith("RT_") or not value:
                raise HeaderParseError(f"unrecognised define: {line.strip()!r}")
            constants[m.group(1)] = int(value.group(1))
        elif not m and not re.match(r"#\s*(ifndef|ifdef|endif|include)\b", line):
            raise HeaderParseError(f"unrecognised preprocessor line: {line.strip()!r}")
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    pos = 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos)
        if not m:
            raise HeaderParseError(f"unrecognised statement near: {' '.join(text[pos:].split())[:80]!r}")
        pos = m.end()
        body, sname, ret, fname, args = m.groups()
        if sname:
            fields = []
            for decl in filter(str.strip, body.split(";")):
                ctype, names = _declaration(decl, structs, True)
                fields += [(n, ctype if ctype in _SCALARS.values() else C.c_void_p) for n in names]      # any pointer field: void*
            camel = "".join(w.capitalize() for w in sname.split("_")[1:])
            structs[sname] = type(camel, (C.Structure,), {"_fields_": fields, "__doc__": f"``{sname}`` of include/reptext_hip.h, generated from it."})
        else:
            restypes[fname] = _declaration(ret, {}, False)[0]
            signatures[fname] = [] if args.strip() == "void" else [_declaration(a, structs, True)[0] for a in args.split(",")]
    return constants, structs, signatures, restypes


def parse_header_file(path: str):
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as e:
        raise NativeLibraryMissing(f"{path} not found ({e}): the binding of {LIB_NAME} is read from this header") from e


CONSTANTS, STRUCTS, SIGNATURES, RESTYPES = parse_header_file(HEADER_PATH)
globals().update(CONSTANTS)                                           # RT_GEMM_MAX_GROUPS, RT_LORA_MAX_TERMS, RT_E_*, ...
globals().update({cls.__name__: cls for cls in STRUCTS.values()})     # GemmGroup, SkinnyGroup, LnSegment, LoraTerm
ABI_VERSION = CONSTANTS["RT_ABI_VERSION"]
_ERROR_NAMES = {v: k for k, v in CONSTANTS.items() if k.startswith("RT_E_")}


class NativeCallError(RuntimeError):
    def __init__(self, fn: str, code: int):
        super().__init__(f"{fn} failed: {_ERROR_NAMES.get(code, 'hipError ' + str(code))} ({code})")
        self.code = code


_lib = None


def library_present() -> bool:
    return os.path.isfile(LIB_PATH)


def bind(path: str):
    """dlopen a build of the library and type every entry point the header declares (also the ablation builds under tools/)."""
    lib = C.CDLL(path)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = RESTYPES[name]
    return lib


def load():
    """Load (once) and type the shared library. Raises NativeLibraryMissing when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not library_present():
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the HIP path."
        )
    lib = bind(LIB_PATH)
    if lib.rt_abi_version() != ABI_VERSION:
        raise NativeLibraryMissing(f"{LIB_NAME} ABI {lib.rt_abi_version()} != header ABI {ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def check(fn: str, code: int) -> None:
    if code != 0:
        raise NativeCallError(fn, code)


def call(name: str, *args) -> None:
    """Call the entry point ``name`` of the header (one that returns a status) and raise NativeCallError unless it returns 0."""
    if name not in SIGNATURES:
        raise KeyError(f"{name} is not declared in include/reptext_hip.h")
    code = getattr(_lib or load(), name)(*args)
    if code != 0:
        raise NativeCallError(name, code)
