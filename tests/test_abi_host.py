"""CPU-only tests of the header reader (afldm_amd/_abi.py) that the ctypes bindings are derived from: every declaration of the
two headers is understood, unknown C is refused by name, struct layouts agree with the C compiler, and the Python constants
keep their public values."""
import ctypes
import importlib.util
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("afldm_hip.h", "afldm_hip_experimental.h")


def _reader():
    """_abi.py loaded from its file, outside the package: it needs neither torch nor a library."""
    spec = importlib.util.spec_from_file_location("afldm_abi_alone", os.path.join(ROOT, "afldm_amd", "_abi.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def abis():
    rd = _reader()
    product = rd.read(HEADERS[0])
    return rd, {HEADERS[0]: product, HEADERS[1]: rd.read(HEADERS[1], product)}


def test_reader_needs_neither_torch_nor_the_library():
    code = ("import sys, importlib.util as u; s = u.spec_from_file_location('abi', %r); m = u.module_from_spec(s); "
            "s.loader.exec_module(m); a = m.read('afldm_hip.h'); e = m.read('afldm_hip_experimental.h', a); "
            "print(len(a.functions), len(e.functions), 'torch' in sys.modules, any('libafldm' in l for l in open('/proc/self/maps')))"
            % os.path.join(ROOT, "afldm_amd", "_abi.py"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    nprod, nexp, torch_loaded, lib_loaded = r.stdout.split()
    assert int(nprod) >= 100 and int(nexp) >= 8 and (torch_loaded, lib_loaded) == ("False", "False"), r.stdout


def test_every_declaration_is_understood_and_bound(abis):
    from afldm_amd import _exp, _lib
    _, by_header = abis
    loaded = {HEADERS[0]: _lib.lib, HEADERS[1]: _exp.lib()}
    for header, abi in by_header.items():
        text = open(os.path.join(ROOT, "include", header)).read()
        code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)            # the prose cites calls of the other header
        declared = set(re.findall(r"\b(afldm_[a-z0-9_]+)\s*\(", code))  # the regex of test_library_exports_every_symbol_...
        assert declared == set(abi.functions), (header, declared ^ set(abi.functions))
        for name, (argtypes, restype) in abi.functions.items():
            proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)\s*;", code).group(1).strip()
            nparams = 0 if proto == "void" else len(proto.split(","))
            fn = getattr(loaded[header], name)
            assert len(fn.argtypes) == len(argtypes) == nparams, name
            assert fn.restype is restype and restype in (ctypes.c_int, ctypes.c_size_t, ctypes.c_char_p), name
    assert _lib.EXPORTS == sorted(by_header[HEADERS[0]].functions) and _exp.exports() == sorted(by_header[HEADERS[1]].functions)
    assert len(by_header[HEADERS[0]].functions) >= 112 and len(by_header[HEADERS[1]].functions) >= 11
    # the type table, one declaration of each row
    vp, ip = ctypes.c_void_p, ctypes.c_int
    f = _lib.ABI.functions
    assert f["afldm_device_info"] == ([ctypes.c_char_p, ip], ip) and f["afldm_last_error"] == ([], ctypes.c_char_p)
    assert f["afldm_softmax_rows"][0] == [vp, vp, ctypes.c_longlong, ip, ctypes.c_float, ip, vp]
    assert f["afldm_cast"][0] == [vp, ip, vp, ip, ctypes.c_size_t, vp] and f["afldm_af_pack_bytes"][1] is ctypes.c_size_t
    assert f["afldm_conv2d"][0] == [ctypes.POINTER(_lib.ConvArgs), vp] and f["afldm_sep_pass"][0][0] is ctypes.POINTER(_lib.SepArgs)
    assert f["afldm_filter_matrix"][0] == [ip, ip, ip, vp] and f["afldm_af_resample_route"][0] == [ip, ip, ip, vp]
    assert f["afldm_flow_warp"][0][:4] == [vp] * 4                    # unsigned char* mask
    e = _lib.EXP_ABI.functions
    assert e["afldm_trunk_run"][0][8:10] == [vp, ctypes.c_size_t]     # unsigned int* sync, size_t sync_bytes
    assert e["afldm_act_conv_act_merged"][0] == [ctypes.POINTER(_lib.AfActArgs), ctypes.POINTER(_lib.ConvArgs),
                                                 ctypes.POINTER(_lib.AfActArgs)]
    assert dict(_lib.ConvArgs._fields_)["sync"] is vp and dict(_lib.ConvArgs._fields_)["w_batch_stride"] is ctypes.c_longlong


@pytest.mark.parametrize("text, names", [
    ("int afldm_x(const void* a, double scale, afldm_stream_t stream);", ("afldm_x", "double")),
    ("int afldm_x(const afldm_missing_args* args, afldm_stream_t stream);", ("afldm_x", "afldm_missing_args")),
    ("typedef struct { const void* x; short C1, C2; } afldm_bad_args;", ("afldm_bad_args", "short")),
    ("double afldm_x(int a);", ("afldm_x", "double")),
    ("enum { AFLDM_A = 0, AFLDM_B };", ("AFLDM_B",)),
    ("#define AFLDM_LIMIT (1 << 4)\nint afldm_x(void);", ("AFLDM_LIMIT",)),
    ("int afldm_x(int a) { return a; }", ("afldm_x",)),
])
def test_reader_refuses_what_it_does_not_know(abis, text, names):
    rd, _ = abis
    with pytest.raises(rd.HeaderError) as err:
        rd.Abi("typedef void* afldm_stream_t;\n" + text)
    for name in names:
        assert name in str(err.value), str(err.value)


def test_reader_reads_the_forms_the_headers_use(abis):
    rd, _ = abis
    abi = rd.Abi("""
        #ifndef GUARD_H
        #define GUARD_H
        #include <stddef.h>
        extern "C" {
        typedef void* afldm_stream_t; /* a stream */
        enum { AFLDM_P = 0, AFLDM_N = -3 };
        #define AFLDM_K_ONE 1   /* trailing prose */
        #define AFLDM_K_ZERO 0
        typedef struct {
          const void* x;   // a pointer; with punctuation
          int C1, C2;
          long long n;
          unsigned int* sync;
          float eps;
        } afldm_t_args;
        int afldm_f(const afldm_t_args* args, const float* w, size_t n,
                    afldm_stream_t stream);
        const char* afldm_g(void);
        }
        #endif
        """)
    t = abi.structs["afldm_t_args"]
    assert t.__name__ == "TArgs" and t._fields_ == [("x", ctypes.c_void_p), ("C1", ctypes.c_int), ("C2", ctypes.c_int),
                                                   ("n", ctypes.c_longlong), ("sync", ctypes.c_void_p), ("eps", ctypes.c_float)]
    assert abi.functions == {"afldm_f": ([ctypes.POINTER(t), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int),
                             "afldm_g": ([], ctypes.c_char_p)}
    assert abi.constants == {"AFLDM_P": 0, "AFLDM_N": -3, "AFLDM_K_ONE": 1, "AFLDM_K_ZERO": 0}
    assert abi.names("AFLDM_K_") == {"zero": 0, "one": 1} and list(abi.names("AFLDM_K_")) == ["zero", "one"]


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from afldm_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no host C compiler (cc / gcc / clang): the build needs one"
    structs = _lib.EXP_ABI.structs                                   # the product header's and the experimental one's
    assert set(structs.values()) == {_lib.ConvArgs, _lib.SepArgs, _lib.AfActArgs}
    assert set(structs) == {"afldm_conv_args", "afldm_sep_args", "afldm_af_act_args"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "afldm_hip_experimental.h"', 'int main(void) {']
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{cname} {field} %zu\\n", offsetof({cname}, {field}));')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {(c, f): int(v) for c, f, v in (l.split() for l in out.splitlines())}
    want = {}
    for cname, cls in structs.items():
        want[(cname, "sizeof")] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            want[(cname, field)] = getattr(cls, field).offset
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    if ctypes.sizeof(ctypes.c_void_p) == 8:                           # LP64: the figures every build so far has had
        assert got[("afldm_conv_args", "sizeof")] == 256 and got[("afldm_conv_args", "sc_C2")] == 252
        assert got[("afldm_sep_args", "sizeof")] == 120 and len(structs["afldm_conv_args"]._fields_) == 41


def test_python_constants_keep_their_public_values():
    from afldm_amd import _lib, ops
    assert (_lib.F32, _lib.BF16) == (0, 1)
    import torch
    assert _lib.DTYPE_CODE == {torch.float32: 0, torch.bfloat16: 1}
    assert (ops.MASK_MIN, ops.MASK_MEAN) == (0, 1) and (ops.FLOW_PICK, ops.FLOW_POOL) == (0, 1)
    assert ops.AF_KERNELS == ("plane", "kron", "p8", "small") and ops.RESAMPLE_KINDS == ("small", "reg", "generic")
    assert ops._AF_TUNE_FIELDS == {"ch": 1, "small_n": 2, "p8": 3, "stagger": 4, "no_resample_small": 5, "resample_split": 6,
                                   "max_grid": 7}
    assert ops._AF_TUNE_RESET == 0
    assert _lib.ABI.constants["AFLDM_OK"] == 0 and _lib.ABI.constants["AFLDM_ENULL"] == -5
    assert [_lib.ConvArgs.__name__, _lib.SepArgs.__name__, _lib.AfActArgs.__name__] == ["ConvArgs", "SepArgs", "AfActArgs"]


def test_a_missing_header_is_an_import_error(abis):
    rd, _ = abis
    with pytest.raises(ImportError, match="afldm_nope.h is missing"):
        rd.read("afldm_nope.h")
