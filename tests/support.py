"""What the ABI tests of more than one feature share: the compiler's view of include/*.h, the reference tree behind the pin drivers,
a process that never initialised the library, and the rule that keeps a Tier B export out of the RTCD bind table."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys
import tempfile

from svtav1_hip import abi

INCLUDE = os.path.join(abi.REPO_ROOT, "include")


def header_values(names, headers=None):
    """{expression: value} of C integer constant expressions over `headers` (every include/*.h by default) as gcc evaluates them:
    macros, enumerators, sizeof, offsetof.  Values come back as signed 64-bit."""
    headers = headers or sorted(os.path.basename(h) for h in glob.glob(os.path.join(INCLUDE, "*.h")))
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + [f'#include "{h}"' for h in headers] + ["int main(void) {"]
    lines += [f'    printf("%lld\\n", (long long)({n}));' for n in names] + ["    return 0;", "}"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "values")
        subprocess.run(["gcc", "-I", INCLUDE, "-x", "c", "-", "-o", exe], input="\n".join(lines), text=True, check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return dict(zip(names, map(int, out.split()), strict=True))


def reference_tree():
    """Where oracle/Makefile takes the reference from, and the defines and include paths a pin driver is compiled with."""
    with open(os.path.join(abi.REPO_ROOT, "oracle", "Makefile")) as f:
        mk = f.read()
    root = os.environ.get("REF") or re.search(r"^REF\s*\?=\s*(\S+)", mk, re.M).group(1)
    defs = re.search(r"^REF_DEFS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    incs = [f"-I{root}/{d}" for d in ("Source/API", "Source/Lib/Globals", "Source/Lib/Codec", "Source/Lib/C_DEFAULT", "third_party/fastfeat")]
    return root, defs + incs + ["-I" + INCLUDE]


def have_reference_tree():
    return os.path.isdir(os.path.join(reference_tree()[0], "Source", "Lib", "Codec"))


def build_pin(tmp_dir, driver_c):
    """The pin driver `driver_c` (it includes files of the reference for their static functions) built into tmp_dir against
    oracle/_ref/libsvtref.so, loaded."""
    import pyorc
    so = os.path.join(str(tmp_dir), os.path.splitext(os.path.basename(driver_c))[0] + ".so")
    subprocess.run(["gcc", "-O1", "-fPIC", "-shared", "-w", *reference_tree()[1], driver_c, "-o", so, pyorc.REF_SO], check=True)
    return C.CDLL(so)


def fresh_process(expr):
    """The integers of the tuple `expr`, evaluated in a new interpreter that has loaded the library and never called svt_hip_init.
    In scope: lib, abi, C and p, a c_void_p to 256 scratch bytes."""
    code = ("import sys; sys.path.insert(0, %r); import ctypes as C; from svtav1_hip import abi; lib = abi.load();"
            "b = C.create_string_buffer(256); p = C.cast(b, C.c_void_p); print(*map(int, (%s)))") % (abi.PKG_ROOT, expr)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
    return [int(v) for v in r.stdout.split()]


def assert_not_rtcd_leaf(name):
    """tools/e2e/gen_bind_table.py takes every exported name ending in _hip for an RTCD leaf: `name` is exported, is none, and
    the lookup does not resolve it."""
    lib = abi.load()
    assert hasattr(lib, name) and not name.endswith("_hip")
    assert lib.svt_hip_rtcd_lookup(name.encode()) is None
