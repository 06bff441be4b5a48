"""CPU tests of the binding's header reader (``_capi.parse_header``): the type mapping, what it must refuse, and what it
makes of the real ``include/pyani_hip.h``."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest

from pyani_plus_amd import _capi
from pyani_plus_amd._capi import HipBackendError, parse_header

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "pyani_hip.h"
CHAR_PP = C.POINTER(C.c_char_p)


def parse(text: str):
    return parse_header(text, "t.h")


# ------------------------------------------------------------------ the mapping
def test_every_row_of_the_type_mapping():
    sigs, tools, constants = parse(
        """
PA_API void pa_v(void);
PA_API const char *pa_s();
PA_API int pa_i(int a, uint32_t b, uint64_t c, int64_t d, double e, const int f, const uint64_t g);
PA_API uint32_t pa_u32(void);
PA_API uint64_t pa_u64(void);
PA_API int64_t pa_i64(void);
PA_API double pa_d(void);
PA_API int pa_c(char *a, const char *b, char c[33]);
PA_API int pa_cc(const char **a, const char *const *b);
PA_API int pa_p(pa_ctx *ctx, void *a, void **b, const uint8_t *c, const uint64_t **d, double e[4], char **f, uint32_t *const g, int *h);
"""
    )
    assert tools == {} and constants == {}
    assert sigs == {
        "pa_v": (None, []),
        "pa_s": (C.c_char_p, []),
        "pa_i": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_double, C.c_int, C.c_uint64]),
        "pa_u32": (C.c_uint32, []),
        "pa_u64": (C.c_uint64, []),
        "pa_i64": (C.c_int64, []),
        "pa_d": (C.c_double, []),
        "pa_c": (C.c_int, [C.c_char_p] * 3),
        "pa_cc": (C.c_int, [CHAR_PP, CHAR_PP]),
        "pa_p": (C.c_int, [C.c_void_p] * 9),
    }
    assert list(sigs) == ["pa_v", "pa_s", "pa_i", "pa_u32", "pa_u64", "pa_i64", "pa_d", "pa_c", "pa_cc", "pa_p"]


def test_prototypes_over_several_lines_and_odd_spacing():
    sigs, _tools, _constants = parse(
        "PA_API int pa_long(pa_ctx *ctx, const uint32_t *d_packed,\n"
        "                   uint64_t\n"
        "                       arena_bases,\n"
        "                   const char *const *paths, char md5hex33[ 33 ]\n"
        "                  )\n"
        ";\n"
        "PA_API const char*pa_tight(const char*a,const char*const*b,double*c,int d);\n"
        "PA_API   int64_t\n"
        "pa_next_line ( void ) ;\n"
    )
    assert sigs == {
        "pa_long": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, CHAR_PP, C.c_char_p]),
        "pa_tight": (C.c_char_p, [C.c_char_p, CHAR_PP, C.c_void_p, C.c_int]),
        "pa_next_line": (C.c_int64, []),
    }


def test_comments_are_no_code():
    sigs, tools, constants = parse(
        "/* PA_API int pa_fake(int a);\n"
        "PA_API int pa_fake_at_the_start_of_a_line(int a);\n"
        "#define PA_FAKE 1\n"
        " * text; with a ( paren and a ) and a ; */\n"
        "PA_API int pa_real(int a /* the count; (really), */, // PA_API int pa_no(void);\n"
        "                   uint64_t b);\n"
        "// PA_API int pa_line(void);\n"
        "#define PA_REAL 3 /* three; not (4) */\n"
        "#define PA_ALSO 4 // #define PA_NOT 5\n"
    )
    assert sigs == {"pa_real": (C.c_int, [C.c_int, C.c_uint64])} and tools == {}
    assert constants == {"PA_REAL": 3, "PA_ALSO": 4}
    # a refusal after a comment still names the line of the file
    with pytest.raises(HipBackendError, match=r"^t\.h:4: pa_x: the return type `float`"):
        parse("/* one\n * two\n */\nPA_API float pa_x(void);\n")


def test_the_tools_section_lands_in_the_tools_table_only():
    sigs, tools, constants = parse(
        '#define PA_API __attribute__((visibility("default")))\n'
        "PA_API int pa_a(void);\n"
        "#ifdef PA_TOOLS\n"
        '#define PA_TOOL_API __attribute__((visibility("default")))\n'
        "PA_TOOL_API int pa_tool_x(pa_ctx *ctx, uint64_t n, int *which);\n"
        "#endif\n"
        "PA_API void pa_b(pa_ctx *ctx);\n"
    )
    assert sigs == {"pa_a": (C.c_int, []), "pa_b": (None, [C.c_void_p])}
    assert tools == {"pa_tool_x": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p])}
    assert constants == {}  # the two visibility macros are the only PA_ macros that need not be integers


def test_constants_and_statuses():
    _sigs, _tools, constants = parse(
        "#define PA_A 5\n"
        "#define PA_B 64u\n"
        "#define PA_C 0xFFFFFFFFFFFFFFFFULL\n"
        "#define PA_D 0X10lU /* sixteen */\n"
        "#define PA_E 0\n"
        "  #  define PA_F 7L\n"
        "#define PA_G 0xFFFFFFFFu\n"
        "#define PYANI_HIP_H\n"
        "#define OTHER (1 << 3)\n"
        "typedef enum pa_status {\n"
        "  PA_OK = 0,\n"
        "  PA_E_ONE = -1, /* bad, very */\n"
        "  PA_E_SEVEN = -7 /* last */\n"
        "} pa_status;\n"
    )
    assert constants == {"PA_A": 5, "PA_B": 64, "PA_C": 2**64 - 1, "PA_D": 16, "PA_E": 0, "PA_F": 7, "PA_G": 2**32 - 1, "PA_OK": 0, "PA_E_ONE": -1, "PA_E_SEVEN": -7}


# ------------------------------------------------------------------ the refusals
@pytest.mark.parametrize(
    ("text", "message"),
    [
        # a return or by-value type outside the table
        ("\nPA_API float pa_x(int a);", r"t\.h:2: pa_x: the return type `float` is not one of"),
        ("\nPA_API char *pa_x(int a);", r"t\.h:2: pa_x: the return type `char \*` is not one of"),
        ("\nPA_API pa_status pa_x(int a);", r"t\.h:2: pa_x: the return type `pa_status`"),
        ("\nPA_API int pa_x(size_t n);", r"t\.h:2: pa_x: the by-value type of `size_t n` is not one of int, uint32_t, uint64_t, int64_t, double"),
        ("\nPA_API int pa_x(int a,\n unsigned b);", r"t\.h:2: pa_x: the by-value type of `unsigned b`"),
        ("\nPA_API int pa_x(unsigned int b);", r"t\.h:2: pa_x: cannot type the parameter `unsigned int b`"),
        ("\nPA_API int pa_x(char c);", r"t\.h:2: pa_x: the by-value type of `char c`"),
        ("\nPA_API int pa_x(void v);", r"t\.h:2: pa_x: the by-value type of `void v`"),
        # variadic, function pointer, by-value struct
        ("\nPA_API int pa_x(const char *fmt, ...);", r"t\.h:2: pa_x is variadic"),
        ("\nPA_API int pa_x(int a, int (*cb)(int, int));", r"t\.h:2: pa_x: cannot type the parameter `int \(\*cb\)\(int` \(a function pointer"),
        ("\nPA_API int pa_x(struct pa_opts opts);", r"t\.h:2: pa_x: the by-value type of `struct pa_opts opts`"),
        ("\nPA_API int pa_x(pa_opts opts);", r"t\.h:2: pa_x: the by-value type of `pa_opts opts`"),
        # a parameter without a name
        ("\nPA_API int pa_x(uint64_t);", r"t\.h:2: pa_x: the parameter `uint64_t` has no name"),
        ("\nPA_API int pa_x(int a, const char *);", r"t\.h:2: pa_x: the parameter `const char \*` has no name"),
        ("\nPA_API int pa_x(int a, uint32_t *const);", r"t\.h:2: pa_x: the parameter `uint32_t \*const` has no name"),
        ("\nPA_API int pa_x(int a, );", r"t\.h:2: pa_x: cannot type the parameter ``"),
        # a line that starts like a prototype and yields none
        ("\nPA_API int pa_x(int a)\nPA_API int pa_y(int b);", r"t\.h:2: the line starts with PA_API but is no prototype"),
        ("PA_API int pa_y(int b);\n\nPA_TOOL_API int pa_x;", r"t\.h:3: the line starts with PA_TOOL_API but is no prototype"),
        ("PA_API int pa_y(int b);\nPA_API int pa_x(int a)", r"t\.h:2: the line starts with PA_API but is no prototype"),
        ("PA_API typedef struct pa_ctx pa_ctx;", r"t\.h:1: the line starts with PA_API but is no prototype"),
        # a name twice, in one table or across the two
        ("PA_API int pa_x(void);\nPA_API int pa_x(int a);", r"t\.h:2: pa_x is declared twice"),
        ("PA_API int pa_x(void);\n\nPA_TOOL_API int pa_x(void);", r"t\.h:3: pa_x is declared twice"),
        # constants
        ("\n#define PA_X (1 << 3)", r"t\.h:2: #define PA_X \(1 << 3\): the value is not an integer literal"),
        ("#define PA_X 1.5", r"t\.h:1: #define PA_X 1\.5: the value is not an integer literal"),
        ("#define PA_X PA_Y", r"t\.h:1: #define PA_X PA_Y: the value is not an integer literal"),
        ("#define PA_X(a) 1", r"t\.h:1: #define PA_X\(a\) 1: the value is not an integer literal"),
        ("#define PA_X", r"t\.h:1: #define PA_X: the value is not an integer literal"),
        ("#define PA_X 010", r"t\.h:1: #define PA_X 010: the value is not an integer literal"),
        ("#define PA_X 8ull8", r"t\.h:1: #define PA_X 8ull8: the value is not an integer literal"),
        ("#define PA_X 1\n#define PA_X 2", r"t\.h:2: PA_X is defined twice"),
        ("#define PA_OK 0\ntypedef enum pa_status { PA_OK = 0 } pa_status;", r"t\.h:2: PA_OK is defined twice"),
        ("\ntypedef enum pa_status { PA_OK = 0, PA_E_X } pa_status;", r"t\.h:2: enum pa_status: `PA_E_X` is not `NAME = integer`"),
    ],
)
def test_what_the_reader_does_not_understand_stops_it(text, message):
    with pytest.raises(HipBackendError, match="^" + message):
        parse(text)


# ------------------------------------------------------------------ the real header
def test_the_real_header_types_every_prototype():
    header = HEADER.read_text()
    # the header that typed the binding is the checkout's: the copy the build leaves next to the libraries, when there is one
    assert _capi.HEADER_PATH.read_text() == header
    assert _capi.HEADER_PATH in (HEADER, _capi.LIB_PATH.with_name("pyani_hip.h"))
    # the lines that open a prototype, counted without the reader's own expressions
    n_api = sum(line.startswith("PA_API ") for line in header.splitlines())
    n_tool = sum(line.startswith("PA_TOOL_API ") for line in header.splitlines())
    assert len(_capi.SIGNATURES) == n_api >= 131 and len(_capi.TOOL_SIGNATURES) == n_tool == 2  # noqa: PLR2004
    allowed = {None, C.c_int, C.c_uint32, C.c_uint64, C.c_int64, C.c_double, C.c_char_p, C.c_void_p, CHAR_PP}
    for name, (restype, argtypes) in {**_capi.SIGNATURES, **_capi.TOOL_SIGNATURES}.items():
        assert restype in allowed - {C.c_void_p, CHAR_PP} and set(argtypes) <= allowed - {None}, name
        # as many argument types as the prototype has commas at the top level, plus one
        params = re.search(rf"^PA_(?:TOOL_)?API [^;(]*\b{name}\(([^;]*)\);", header, flags=re.M).group(1)
        assert len(argtypes) == (0 if params.strip() == "void" else params.count(",") + 1), name
    assert _capi.SIGNATURES["pa_fasta_batch_arena_bases"] == (C.c_uint64, [C.c_void_p])
    assert _capi.SIGNATURES["pa_fasta_batch_load"] == (C.c_int, [CHAR_PP, C.c_uint32, C.c_int, C.c_void_p])
    assert _capi.SIGNATURES["pa_msa_info"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p])
    assert _capi.SIGNATURES["pa_kde_gauss_f64_host"] == (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_double, C.c_void_p])
    assert _capi.SIGNATURES["pa_mask_runs"][0] is C.c_int64 and _capi.SIGNATURES["pa_fragani_identity"][0] is C.c_double
    assert _capi.SIGNATURES["pa_ctx_destroy"] == (None, [C.c_void_p]) and _capi.SIGNATURES["pa_last_error"] == (C.c_char_p, [])


def test_the_typed_library_refuses_a_wrong_call():
    lib = _capi.load_library()
    with pytest.raises(TypeError):
        lib.pa_max_hash()
    with pytest.raises(TypeError):
        lib.pa_max_hash(1, 2)
    assert lib.pa_max_hash(1000) == 18446744073709552  # noqa: PLR2004
    with pytest.raises(TypeError):
        lib.pa_fragani_window(16)
    # a str where the header says `const char *`: bytes are meant
    with pytest.raises(C.ArgumentError):
        lib.pa_msa_load("alignment.fasta", 1, None)
    with pytest.raises(C.ArgumentError):
        lib.pa_write_pairs_tsv(b"pairs.tsv", "x\ty", None, None, 0)
    # a by-value integer takes no float and no pointer
    with pytest.raises(C.ArgumentError):
        lib.pa_max_hash(1000.0)
    with pytest.raises(C.ArgumentError):
        lib.pa_fragani_identity(1, 2, None)


def test_the_statuses_and_the_abi_version_are_the_parents():
    header = HEADER.read_text()
    statuses = {"PA_OK": 0, "PA_E_INVALID": -1, "PA_E_HIP": -2, "PA_E_NOMEM": -3, "PA_E_CAPACITY": -4, "PA_E_NODEVICE": -5, "PA_E_IO": -6, "PA_E_NOCONVERGE": -7}
    body = re.search(r"typedef enum pa_status \{(.*?)\} pa_status;", header, flags=re.S).group(1)
    assert re.findall(r"^  (\w+) = (-?\d+)", body, flags=re.M) == [(name, str(value)) for name, value in statuses.items()]
    for name, value in statuses.items():
        assert getattr(_capi, name) == value, name
    assert "#define PA_ABI_VERSION 5\n" in header and _capi.ABI_VERSION == _capi.PA_ABI_VERSION == 5  # noqa: PLR2004
    # the names derived from the header's constants
    assert _capi.PA_AGG == {"min": 0, "max": 1, "mean": 2} and _capi.PA_DEREP_MODE == {"greedy": 0, "cover": 1}
    assert len(_capi.PROF_PHASES) == _capi.PA_PROF_NPHASES == 18 and list(_capi.PROF_PHASES.values()) == list(range(18))  # noqa: PLR2004
    assert list(_capi.PROF_PHASES)[:5] == ["kmer_hash", "sketch_sort", "pair_dict", "pair_count", "ani"] and _capi.PROF_PHASES["msa_boot_dist"] == 17  # noqa: PLR2004
