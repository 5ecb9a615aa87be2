"""CPU: the C-ABI libraries build, load, and export every symbol their headers declare
(no compute calls -- there is no GPU in the build container)."""
import ctypes
import os
import shutil
import re
import subprocess

import pytest

from tests.conftest import ROOT


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nsh_\w+|nsr_\w+)\s*\(", txt)))


_INT = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
        "float": ctypes.c_float, "double": ctypes.c_double}
CTYPES = {**_INT, "void": None, "void*": ctypes.c_void_p, "const void*": ctypes.c_void_p,
          "void**": ctypes.POINTER(ctypes.c_void_p), "char*": ctypes.c_char_p, "const char*": ctypes.c_char_p,
          "float*": ctypes.POINTER(ctypes.c_float), "const float*": ctypes.POINTER(ctypes.c_float),
          "const float* const*": ctypes.POINTER(ctypes.POINTER(ctypes.c_float)),
          "int*": ctypes.POINTER(ctypes.c_int), "const int*": ctypes.POINTER(ctypes.c_int),
          "int64_t*": ctypes.POINTER(ctypes.c_int64), "uint64_t*": ctypes.POINTER(ctypes.c_uint64),
          "size_t*": ctypes.POINTER(ctypes.c_size_t)}


def spelling(decl):
    """('const float*', 'taps_host') of 'const float *taps_host': the type with one space between words
    and the stars attached, and the parameter's name ('' where the header gives none)."""
    words = re.sub(r"(\*+)", r"\1 ", re.sub(r"\s*\*\s*", "*", decl)).split()
    name = words.pop() if len(words) > 1 and re.fullmatch(r"\w+", words[-1]) else ""
    return " ".join(words), name


def prototypes(header):
    """{name: (restype, [argtypes], [parameter names])} in ctypes, of every `ret nsh_name(params);` the
    header declares. A spelling that CTYPES does not list raises, naming the entry."""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)                           # preprocessor lines
    protos = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(nsh_\w+)\s*\(([^()]*)\)\s*;", txt):
        parts = [spelling(p) for p in params.split(",") if p.strip() and p.strip() != "void"]
        for s in [spelling(ret + " _")[0]] + [p[0] for p in parts]:
            if s not in CTYPES:
                raise KeyError(f"{name}: no ctypes mapping for '{s}'")
        protos[name] = (CTYPES[spelling(ret + " _")[0]], [CTYPES[s] for s, _ in parts], [n for _, n in parts])
    return protos


def exported(so):
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


def test_hip_shim_exports_header():
    from newsched_amd import nsh

    syms = exported(nsh.HIP_LIB)
    missing = [s for s in declared("nsh_hip.h") if s not in syms]
    assert not missing, missing
    # the Python binding covers exactly the header
    assert sorted(nsh.SIGNATURES) == declared("nsh_hip.h")


def _binding_names():
    from newsched_amd import nsh

    return sorted(nsh.SIGNATURES)


@pytest.mark.parametrize("name", _binding_names())
def test_binding_matches_the_prototype(name):
    """nsh.SIGNATURES against include/nsh_hip.h: the restype and every argtype of every entry point, in
    the header's order. One latitude: a float* or const float* parameter may be bound as c_void_p (a
    device address) or as POINTER(c_float) (a host array); the binding uses both on purpose. The
    header's names do not tell the two apart: the host arrays are *_host, all but nsh_event_elapsed_ms's
    `float* ms`, a host out-parameter, so the rule "POINTER(c_float) iff *_host" fails on that one."""
    from newsched_amd import nsh

    restype, argtypes, names = prototypes("nsh_hip.h")[name]
    floats = ctypes.POINTER(ctypes.c_float)
    got_res, got_args = nsh.SIGNATURES[name]
    assert got_res is restype, (name, got_res, restype)
    assert len(got_args) == len(argtypes), (name, len(got_args), len(argtypes))
    for i, (g, w) in enumerate(zip(got_args, argtypes)):
        assert g is w or (w is floats and g is ctypes.c_void_p), (name, i, names[i], g, w)


PLAN_ATTRS = [("ArbPlan", ("close", "__call__", "span")), ("PfbPlan", ("close", "__call__")),
              ("PfbSynthPlan", ("close", "__call__")), ("ResampPlan", ("close", "__call__"))]


@pytest.mark.parametrize("cls,attrs", PLAN_ATTRS, ids=[c for c, _ in PLAN_ATTRS])
def test_plan_class_has_its_methods(cls, attrs):
    from newsched_amd import nsh

    for attr in attrs:
        assert hasattr(getattr(nsh, cls), attr), (cls, attr)


def test_hip_shim_loads_and_reports():
    from newsched_amd import nsh

    L = nsh.lib()
    assert L.nsh_abi_version() == 1
    assert L.nsh_last_error() == b""


def test_hip_shim_is_gfx950_code_object(tmp_path):
    from newsched_amd import nsh

    # --offloading extracts the bundled code objects next to its input: run it on a copy
    lib = tmp_path / os.path.basename(nsh.HIP_LIB)
    shutil.copyfile(nsh.HIP_LIB, lib)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(lib)],
                         capture_output=True, text=True, cwd=tmp_path)
    if out.returncode != 0:
        pytest.skip("llvm-objdump --offloading unavailable")
    assert "gfx950" in out.stdout + out.stderr


def test_hip_shim_rejects_null_arguments_before_launch():
    """Argument errors come back as codes with a message, before any HIP call (so they are
    checkable here, without a GPU): a NULL plan to the FIR entry points."""
    from newsched_amd import nsh

    L = nsh.lib()
    one = ctypes.c_void_p(1)
    assert L.nsh_fir_ccf(None, one, None, one, one, 16, None) != 0
    assert b"null plan" in L.nsh_last_error()
    assert L.nsh_fir_cascade_ccf(None, one, None, one, one, 16, None) != 0
    assert b"null plan" in L.nsh_last_error()
    assert L.nsh_fir_plan_algo(None) == 0
    assert L.nsh_fir_ccf(None, one, None, one, one, 0, None) != 0  # plan checked first


def test_stream_and_fft_entry_points_reject_null():
    from newsched_amd import nsh

    L = nsh.lib()
    one = ctypes.c_void_p(16)
    assert L.nsh_copy(None, one, 64, None) != 0 and b"null" in L.nsh_last_error()
    assert L.nsh_mul_const_cc(one, None, 8, 1.0, 0.0, None) != 0
    assert L.nsh_add_cc(one, None, one, 8, None) != 0
    assert L.nsh_fft1024_c2c(None, one, 1, 0, None) != 0
    assert L.nsh_channelizer1024(one, ctypes.c_void_p(32), None, 1, None) != 0
    assert L.nsh_synth_cf32(None, 8, 0, 1, None) != 0
    assert L.nsh_copy(None, None, 0, None) == 0  # nothing to move: no error
