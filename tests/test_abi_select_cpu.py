"""The scheme-level selection / compare-exchange entries of include/sc_amd.h at the C boundary, without a GPU:
declared in the header a maintainer binds (not in sc_amd_dev.h), exported by the built library, bound by _lib with the header's
argument counts, the ABI version unchanged, and reachable from a strict-C99 translation unit."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from protocols.secure_comparison_amd import _lib
from protocols.secure_comparison_amd.build import OUT, build_lib

ENTRIES = ["sc_initiator_select_d", "sc_paillier_one_minus", "sc_initiator_cx_differences", "sc_initiator_select_pack",
           "sc_keyholder_select_mult", "sc_initiator_select_finish", "sc_initiator_cx_finish"]


def _declarations(header):
    """{name: number of parameters} of every function a header declares (comments stripped)."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(sc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else params.count(",") + 1
    return out


def test_selection_entries_are_declared_in_the_public_header_only():
    public, dev = _declarations("sc_amd.h"), _declarations("sc_amd_dev.h")
    for name in ENTRIES:
        assert name in public, f"{name} is not declared in include/sc_amd.h"
        assert name not in dev, f"{name} belongs to include/sc_amd.h, not to the developer header"
    text = open(os.path.join(ROOT, "include", "sc_amd.h")).read()
    assert re.search(r"SC_ERR_LAYOUT\s*=\s*-5", text)                       # the key holder's layout verdict: an added status
    assert re.search(r"#define\s+SC_ABI_VERSION\s+5\b", text)               # additive: the version stays


def test_selection_entries_are_exported_and_bound_with_the_headers_argument_counts():
    lib = ctypes.CDLL(build_lib(verbose=False))
    public = _declarations("sc_amd.h")
    bound = _lib.load()
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} declared but not exported"
        assert name in _lib.SYMBOLS
        fn = getattr(bound, name)
        assert fn.restype is ctypes.c_int
        assert len(fn.argtypes) == public[name], f"{name}: the binding passes {len(fn.argtypes)} arguments, the header declares {public[name]}"
    assert bound.sc_abi_version() == _lib.ABI_VERSION == 5


def test_rho_p_is_documented_as_required():
    """The header says in words that P is never built without fresh randomness."""
    text = open(os.path.join(ROOT, "include", "sc_amd.h")).read()
    doc = text[:text.index("int sc_initiator_select_pack")]
    doc = doc[doc.rindex("/*"):]
    assert "rho_p is NOT nullable" in doc and "SC_ERR_ARG" in doc


def test_a_c99_host_takes_the_address_of_every_selection_entry(tmp_path):
    """Same compiler flags as test_header_is_plain_c_and_links: the new declarations are plain C and every entry links."""
    if shutil.which("gcc") is None:
        pytest.skip("no gcc here")
    build_lib(verbose=False)
    table = ",\n  ".join(f"(fn)&{n}" for n in ENTRIES)
    src = tmp_path / "host.c"
    src.write_text('#include "sc_amd.h"\n#include <stdio.h>\n'
                   "typedef void (*fn)(void);\n"
                   f"static fn const entries[] = {{\n  {table}\n}};\n"
                   "int main(void) {\n  unsigned i, n = 0;\n"
                   "  for (i = 0; i < sizeof entries / sizeof entries[0]; i++) n += entries[i] != 0;\n"
                   '  printf("%u %d %d\\n", n, sc_abi_version(), (int)SC_ERR_LAYOUT);\n  return 0;\n}\n')
    exe = tmp_path / "host"
    libdir = os.path.dirname(OUT)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-lsc_amd", "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [len(ENTRIES), _lib.ABI_VERSION, -5]
