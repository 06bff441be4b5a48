"""ctypes binding of ``libpyani_hip.so``, read from the header that declares it (``include/pyani_hip.h``).

This is the only route from Python into the compute path.  There is no CPU
fallback: if the shared library is missing, or no gfx950 device is usable,
the calls raise ``HipBackendError``.

The header is the one statement of the ABI.  ``parse_header`` turns its prototypes into ``SIGNATURES`` and
``TOOL_SIGNATURES`` (name -> (restype, argtypes)) and its integer ``#define PA_...`` and the ``pa_status`` enumerators into
attributes of this module; what it does not understand stops the import.
"""

from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "_lib" / "libpyani_hip.so"
# The same sources built with -DPA_TOOLS: the environment switches that force a rare path, cut a kernel short or select an
# ablation variant (PA_MAP_CUT, PA_FRAGANI_*, PA_KMER_*, PA_PAIRS_SYMMETRIC, ...) exist in this build only.  tools/ and
# the tests of those paths load it (``HipEngine(tools=True)``); nothing else does.
TOOLS_LIB_PATH = _PKG / "_lib" / "libpyani_hip_tools.so"
# The build copies the header next to the libraries it compiled from it, so a stale library is typed by the header it
# matches; before the first build the checkout's own header keeps the constants importable.
_BUILT_HEADER = _PKG / "_lib" / "pyani_hip.h"
HEADER_PATH = _BUILT_HEADER if _BUILT_HEADER.is_file() else _PKG.parent / "include" / "pyani_hip.h"


class HipBackendError(RuntimeError):
    """The HIP extension is missing, failed to load, or a call into it failed."""


# The whole typing policy.  By value (``const`` ignored); a return type is one of these, void or ``const char *``.
_BY_VALUE = {"int": C.c_int, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "double": C.c_double}
_RETURNS = {"void": None, "const char *": C.c_char_p, **_BY_VALUE}
# (base type, levels of * and []) of a parameter.  c_char_p, so that a str where bytes are meant raises (c_void_p would
# take it as a wide string); every other pointer or array parameter is a plain address, c_void_p.
_CHAR_POINTERS = {("char", 1): C.c_char_p, ("const char", 1): C.c_char_p, ("const char", 2): C.POINTER(C.c_char_p)}

_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_API_LINE = re.compile(r"^(?:PA_API|PA_TOOL_API) ", re.M)
_PROTOTYPE = re.compile(r"(PA_API|PA_TOOL_API)\s+([^;(]*?)\s*\b(\w+)\s*\(([^;]*)\)\s*;")
_PARAMETER = re.compile(r"((?:const\s+)?(?:struct\s+)?\w+)((?:\s*\*(?:\s*const\b)?)*)\s*(\w+)?\s*((?:\[\s*\w*\s*\]\s*)*)")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(PA_\w+)(.*)$", re.M)
_INTEGER = re.compile(r"(0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)[uUlL]*")
_STATUS_ENUM = re.compile(r"typedef\s+enum\s+pa_status\s*\{([^}]*)\}")
_ENUMERATOR = re.compile(r"\s*(\w+)\s*=\s*(-?[0-9]+)\s*")


def parse_header(text: str, where: str = "pyani_hip.h") -> tuple[dict, dict, dict]:
    """(SIGNATURES, TOOL_SIGNATURES, constants) of a header text.  Every line that starts with ``PA_API `` or
    ``PA_TOOL_API `` opens a prototype that ends at the first ``;`` and goes into the table of its macro; every
    ``#define PA_<NAME>`` but the two visibility macros must be an integer literal.  Anything else raises
    ``HipBackendError`` with the line."""
    text = _COMMENT.sub(lambda m: " " + "\n" * m.group().count("\n"), text)  # its line breaks stay, so a position still tells the line

    def fail(pos: int, message: str):
        raise HipBackendError(f"{where}:{text.count(chr(10), 0, pos) + 1}: {message}")

    def argtype(decl: str, pos: int, name: str):
        if decl == "...":
            fail(pos, f"{name} is variadic")
        m = _PARAMETER.fullmatch(decl)
        if "(" in decl or not m:
            fail(pos, f"{name}: cannot type the parameter `{decl}` (a function pointer, or a type the binding does not know)")
        base, stars, param, dims = m.groups()
        if param is None:
            fail(pos, f"{name}: the parameter `{decl}` has no name")
        base, levels = " ".join(base.split()), stars.count("*") + dims.count("[")
        if levels:
            return _CHAR_POINTERS.get((base, levels), C.c_void_p)
        if base.removeprefix("const ") not in _BY_VALUE:
            fail(pos, f"{name}: the by-value type of `{decl}` is not one of {', '.join(_BY_VALUE)}")
        return _BY_VALUE[base.removeprefix("const ")]

    tables: dict[str, dict] = {"PA_API": {}, "PA_TOOL_API": {}}
    starts = [m.start() for m in _API_LINE.finditer(text)]
    for pos, end in zip(starts, [*starts[1:], len(text)]):
        m = _PROTOTYPE.match(text, pos, end)  # one prototype per such line, and it ends before the next: none is skipped
        if not m:
            fail(pos, f"the line starts with {text[pos:].split()[0]} but is no prototype `<type> name(<parameters>);`")
        macro, ret, name, params = m.groups()
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in _RETURNS:
            fail(pos, f"{name}: the return type `{ret}` is not one of {', '.join(_RETURNS)}")
        if any(name in table for table in tables.values()):
            fail(pos, f"{name} is declared twice")
        decls = [" ".join(p.split()) for p in params.split(",")]
        tables[macro][name] = (_RETURNS[ret], [] if decls in ([""], ["void"]) else [argtype(d, pos, name) for d in decls])

    constants: dict[str, int] = {}

    def constant(name: str, value: int, pos: int):
        if name in constants:
            fail(pos, f"{name} is defined twice")
        constants[name] = value

    for m in _DEFINE.finditer(text):
        if m.group(1) not in tables:  # the two visibility macros
            literal = _INTEGER.fullmatch(m.group(2).strip())
            if not literal:
                fail(m.start(), f"#define {m.group(1)}{m.group(2)}: the value is not an integer literal")
            constant(m.group(1), int(literal.group(1), 0), m.start())
    enum = _STATUS_ENUM.search(text)
    for item in enum.group(1).split(",") if enum else ():
        m = _ENUMERATOR.fullmatch(item)
        if not m and item.strip():
            fail(enum.start(), f"enum pa_status: `{item.strip()}` is not `NAME = integer`")
        if m:
            constant(m.group(1), int(m.group(2)), enum.start())
    return tables["PA_API"], tables["PA_TOOL_API"], constants


# name -> (restype, argtypes).  TOOL_SIGNATURES: the probes of the internal radix sort and exclusive scan, which
# libpyani_hip_tools.so alone exports; load_library(tools=True) types them as well.
try:
    SIGNATURES, TOOL_SIGNATURES, _constants = parse_header(HEADER_PATH.read_text(), str(HEADER_PATH))
    globals().update(_constants)  # PA_OK, PA_E_INVALID, ..., PA_ALIGN_BASES, ...: every constant under the header's name
    PA_OK, ABI_VERSION = _constants["PA_OK"], _constants["PA_ABI_VERSION"]
    PROF_PHASES = {n.removeprefix("PA_PROF_").lower(): v for n, v in _constants.items() if n.startswith("PA_PROF_") and n != "PA_PROF_NPHASES"}
    if len(PROF_PHASES) != _constants["PA_PROF_NPHASES"]:
        raise HipBackendError(f"{HEADER_PATH}: {len(PROF_PHASES)} PA_PROF_ phases, but PA_PROF_NPHASES is {_constants['PA_PROF_NPHASES']}")
    PA_AGG = {name: _constants[f"PA_AGG_{name.upper()}"] for name in ("min", "max", "mean")}
    PA_DEREP_MODE = {name: _constants[f"PA_DEREP_{name.upper()}"] for name in ("greedy", "cover")}
    PA_HITS_RANK = {name: _constants[f"PA_HITS_RANK_{name.upper()}"] for name in ("identity", "containment")}
except (OSError, KeyError) as err:
    raise HipBackendError(f"cannot bind {HEADER_PATH}: {err!r} (a missing file or a missing constant)") from err

_libs: dict[bool, C.CDLL] = {}


def build_library(force: bool = False) -> Path:
    """Compile ``libpyani_hip.so`` and ``libpyani_hip_tools.so`` for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcdir = _PKG / "csrc"
    cmd = ["make", "-C", str(srcdir), "-j", str(min(8, os.cpu_count() or 1))]
    if force:
        cmd.append("-B")
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0 or not LIB_PATH.is_file() or not TOOLS_LIB_PATH.is_file():
        raise HipBackendError(f"building libpyani_hip.so failed:\n{proc.stdout}\n{proc.stderr}")
    return LIB_PATH


def load_library(tools: bool = False) -> C.CDLL:
    """Load the shared library (``tools``: the -DPA_TOOLS build, with its probes) and type every symbol of the header; raise loudly if absent."""
    if tools in _libs:
        return _libs[tools]
    path = TOOLS_LIB_PATH if tools else LIB_PATH
    if not path.is_file():
        raise HipBackendError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pyani_plus_amd/csrc`).  There is no CPU fallback for the compute path."
        )
    # PyTorch's ROCm wheel bundles its own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one
    # process cannot both own the GPU, so torch goes first and this library (same soname,
    # libamdhip64.so.7) binds to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover - plain ROCm install without torch
        pass
    try:
        lib = C.CDLL(str(path))
    except OSError as err:  # missing ROCm runtime, wrong arch, ...
        raise HipBackendError(f"cannot load {path}: {err}") from err
    for name, (restype, argtypes) in {**SIGNATURES, **(TOOL_SIGNATURES if tools else {})}.items():
        try:  # a prototype with parameter flags: unlike a bare `argtypes`, it refuses an argument too many as well as one too few
            setattr(lib, name, C.CFUNCTYPE(restype, *argtypes)((name, lib), ((1,),) * len(argtypes)))
        except AttributeError as err:
            raise HipBackendError(f"{path} does not export {name}") from err
    if lib.pa_abi_version() != ABI_VERSION:
        raise HipBackendError(f"ABI version mismatch: library reports {lib.pa_abi_version()}, binding expects {ABI_VERSION}")
    _libs[tools] = lib
    return lib


def last_error(lib: C.CDLL | None = None) -> str:
    return ((lib or load_library()).pa_last_error() or b"").decode(errors="replace")


def check(status: int, what: str, lib: C.CDLL | None = None) -> None:
    if status != PA_OK:
        err = HipBackendError(f"{what} failed with status {status}: {last_error(lib)}")
        err.status = status  # the library's code (PA_E_*), for callers that tell failures apart
        raise err
