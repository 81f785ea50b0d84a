"""CPU: the C-ABI shared library loads and exports every symbol include/slu_hip.h declares; the
argument-validation paths that need no GPU behave as documented."""
import ctypes
import os
import re

import pytest

from abi_header import ROOT, abi_version, arg_counts, header_functions

c_int, i64, u64, f32, f64, vp, sz = (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double,
                                     ctypes.c_void_p, ctypes.c_size_t)


def test_header_and_binding_table_agree():
    """Two readers of include/slu_hip.h, the tests' (abi_header.py) and the binding's (lib.parse_header): the same names,
    and for EVERY entry point the same number of arguments."""
    from slu_hip import lib
    assert header_functions() == sorted(lib.SIGNATURES)
    counts = arg_counts()
    assert sorted(counts) == sorted(lib.SIGNATURES) and len(counts) >= 119
    for name, (_, argtypes) in lib.SIGNATURES.items():
        assert len(argtypes) == counts[name], name


def test_rows_of_every_scalar_and_return_type_are_pinned():
    """Literal rows, so that every C type the header uses is checked against a ctypes type written down here."""
    from slu_hip import lib
    S = lib.SIGNATURES
    assert S["slu_wconv_fwd"] == (c_int, [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, c_int, c_int, f32, i64, i64, vp,
                                          sz, vp])
    assert S["slu_adam_multi"] == (c_int, [vp, vp, vp, vp, vp, i64, c_int, vp, f64, f64, f64, f64, f64, vp, vp])
    assert S["slu_gru_cell_fwd"] == (c_int, [vp, vp, vp, i64, vp, i64, vp, vp, vp, f32, u64, u64, vp, u64, i64, i64, vp])
    assert S["slu_gemm_plan"] == (c_int, [i64, i64, i64, vp, vp, vp])            # three int* out-parameters
    assert S["slu_last_error"] == (ctypes.c_char_p, []) and S["slu_device_arch"] == (ctypes.c_char_p, [])
    assert S["slu_gru_reserve_bytes"] == (sz, [i64, i64, i64, i64])
    assert S["slu_comm_ipc_window_bytes"] == (i64, [i64])
    # every row is made of these types and no others: nothing fell through to a default
    for name, (res, args) in S.items():
        assert res in (c_int, i64, sz, ctypes.c_char_p), name
        assert set(args) <= {c_int, i64, u64, f32, f64, sz, vp}, name


SNIPPET = """
/* a block comment with a declaration in it: int slu_fake(int x); */
#ifndef X_H
#define X_H
#define SLU_ABI_VERSION 7   /* bumped */
extern "C" {
typedef enum { SLU_OK = 0, SLU_ERR = -1 } slu_status;
// int slu_fake2(int x);
int slu_none(void);
const char* slu_text(void);          /* trailing comment */
size_t
slu_four_lines(const float* const* A,
               void** out, int64_t n, double eps,
               uint64_t seed, float p, void* stream);
typedef struct slu_rec { double a; int64_t b; } slu_rec;
int64_t slu_rec_use(const slu_rec* r, int flag);
}
#endif
"""


def test_parser_on_small_headers():
    from slu_hip import lib
    table, version = lib.parse_header(SNIPPET)
    assert version == 7
    assert table == {"slu_none": (c_int, []),
                     "slu_text": (ctypes.c_char_p, []),
                     "slu_four_lines": (sz, [vp, vp, i64, f64, u64, f32, vp]),
                     "slu_rec_use": (i64, [vp, c_int])}
    assert arg_counts(SNIPPET) == {name: len(args) for name, (_, args) in table.items()}     # the test-side reader agrees


@pytest.mark.parametrize("decl, named", [
    ("int slu_bad(int64_t n, unsigned short flags, void* stream);", "unsigned short"),     # a scalar outside the dict
    ("int slu_bad(uint32_t word);", "uint32_t"),
    ("slu_status slu_bad(void);", "slu_status"),                                            # ... as a return type
    ("void* slu_bad(int64_t n);", "void*"),                                                 # a returned pointer that is no text
    ("int slu_bad(int64_t, void* stream);", "int64_t"),                                     # unnamed parameters
    ("int slu_bad(const float*, int64_t n);", "const float*"),
    ("int slu_bad(int);", "int"),
    ("int slu_bad(int (*callback)(int), void* stream);", "slu_bad"),                        # a function pointer
    ("int slu_bad(float taps[8], void* stream);", "float taps[8]"),                         # an array
    ("int slu_bad();", "slu_bad"),                                                          # not (void)
    ("int slu_bad(void) { return 0; }", "slu_bad"),                                         # not a declaration
    ("int slu_none(void);", "twice"),
])
def test_parser_refuses_what_it_cannot_map(decl, named):
    from slu_hip import lib
    with pytest.raises(lib.SluHipError) as e:
        lib.parse_header("#define SLU_ABI_VERSION 7\nint slu_none(void);\n" + decl + "\n")
    assert "slu_bad" in str(e.value) or named == "twice"
    assert named in str(e.value)


def test_parser_needs_the_version_and_the_header(monkeypatch, tmp_path):
    from slu_hip import lib
    with pytest.raises(lib.SluHipError, match="SLU_ABI_VERSION"):
        lib.parse_header("int slu_none(void);\n")
    missing = str(tmp_path / "include" / "slu_hip.h")
    monkeypatch.setattr(lib, "HEADER_PATH", missing)
    with pytest.raises(lib.SluHipError) as e:
        lib._read_header()
    assert missing in str(e.value)
    # found the way csrc/build.sh finds it, whatever SLU_HIP_LIB says
    monkeypatch.undo()
    assert os.path.samefile(lib.HEADER_PATH, os.path.join(ROOT, "include", "slu_hip.h"))
    assert "../../include/slu_hip.h" in open(os.path.join(ROOT, "end-to-end-slu_amd", "csrc", "build.sh")).read()


def test_integration_stub_agrees_with_the_binding_table():
    """INTEGRATION.md section 2 keeps a short hand-written stub for readers who bind the ABI without this package: each of
    its argtypes / restype lines must evaluate to the row lib.py derives, and a function it gives no restype (ctypes then
    assumes int) must return int."""
    from slu_hip import lib
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    stub = re.search(r"```python\n(# slu_ffi\.py.*?)```", doc, flags=re.S).group(1)
    names = {"ctypes": ctypes, "vp": vp, "i64": i64, "f32": f32}
    seen = {}
    for func, what, expr in re.findall(r"^_L\.(slu_\w+)\.(argtypes|restype) = (.*(?:\n[ \t]+.*)*)", stub, flags=re.M):
        seen.setdefault(func, {})[what] = eval(expr, dict(names))
    assert {"slu_last_error", "slu_sinc_filters_fwd", "slu_wconv_workspace_bytes", "slu_wconv_fwd"} <= set(seen)
    assert set(re.findall(r"_L\.(slu_\w+)", stub)) == set(seen)              # every function the stub calls is declared
    for func, row in seen.items():
        assert row.get("restype", c_int) == lib.SIGNATURES[func][0], func
        assert row.get("argtypes", []) == lib.SIGNATURES[func][1], func


def test_library_loads_at_abi_10_and_exports_every_symbol():
    from slu_hip import lib
    L = lib.load()
    for name in header_functions():
        assert hasattr(L, name), name
    assert L.slu_version() == lib.ABI_VERSION == abi_version() == 10
    assert isinstance(L.slu_last_error(), bytes)


def test_size_queries_and_argument_validation_without_gpu():
    from slu_hip import lib
    L = lib.load()
    # reserve: D*T*ceil(B/16)*(H/16)*5*256 floats
    assert L.slu_gru_reserve_bytes(300, 64, 128, 2) == 2 * 300 * 4 * 8 * 5 * 256 * 4
    assert L.slu_gru_reserve_bytes(7, 3, 16, 2) == 2 * 7 * 1 * 1 * 5 * 256 * 4
    assert L.slu_wconv_workspace_bytes(80, 1, 401) >= 101 * 5 * 64 * 4
    assert L.slu_gemm_workspace_bytes(19200, 768, 256) == 0          # enough tiles: no split-K
    assert L.slu_gemm_workspace_bytes(384, 128, 19200) > 0
    # null pointers / bad sizes are rejected before anything touches the device
    rc = L.slu_gru_seq_fwd(None, None, None, None, None, None, None, 10, 4, 128, 2, None)
    assert rc == -1 and b"null" in L.slu_last_error()
    rc = L.slu_sinc_filters_fwd(1, 1, 1, 80, 400, 16000.0, None)      # even filter length
    assert rc == -1 and b"odd" in L.slu_last_error()
    with pytest.raises(lib.SluHipError):
        lib.check(rc, "slu_sinc_filters_fwd")


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from slu_hip import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(lib.SluHipError, match="no CPU fallback"):
        lib.load()


def test_graft_entry_build_checks_the_current_abi_version():
    """__graft_entry__.build() is the driver's "does it build" check: it must accept whatever SLU_ABI_VERSION the header
    carries (a hard-coded number there went stale once), and the library on disk must be the one the binding expects."""
    from slu_hip import lib
    src = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "lib.ABI_VERSION" in src and not re.search(r"ABI_VERSION\s*==\s*\d", src)
    assert abi_version() == lib.ABI_VERSION
    # the binding reads the number from the header as well: no integer literal in lib.py to go stale
    assert not re.search(r"ABI_VERSION\s*=\s*\d", open(lib.__file__).read())
