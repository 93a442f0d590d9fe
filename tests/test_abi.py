"""CPU: the C-ABI shared library loads and exports every symbol the headers declare, every function carries the header's
prototype and every struct mirror the header's layout (no compute calls)."""
import ctypes as C
import functools
import glob
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from support import fresh_process, header_values
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES


def _generator(name):
    sys.path.insert(0, os.path.join(abi.REPO_ROOT, "tools", "e2e"))
    try:
        return importlib.import_module(name)
    finally:
        sys.path.pop(0)


def declared_symbols():
    """Every function the public headers declare (tools/e2e/gen_prototypes.py reads them)."""
    return list(_generator("gen_prototypes").scan_headers())


def test_library_exports_every_declared_symbol():
    lib = abi.load()
    names = declared_symbols()
    assert len(names) >= 150
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/*.h but not exported by libsvtav1_hip.so"


def test_prototype_table_is_what_the_generator_writes():
    """svtav1_hip/prototypes.py is the output of tools/e2e/gen_prototypes.py for the current headers: one entry per function."""
    gen = _generator("gen_prototypes")
    protos = gen.scan_headers()
    with open(gen.OUT) as f:
        assert f.read() == gen.render(protos)
    assert PROTOTYPES == protos and len(PROTOTYPES) >= 246
    assert sum(n.startswith("svt_hip_") for n in PROTOTYPES) + len(_generator("gen_bind_table").tier_a_names()) == len(PROTOTYPES)


def test_load_gives_every_declared_function_its_prototype():
    """No call goes through ctypes' defaults (every argument and the return value a C int): abi.load() has set the header's
    parameter list and return type on every function."""
    lib = abi.load()
    wide = 0
    for name, (restype, argtypes) in _generator("gen_prototypes").scan_headers().items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes), name
        assert list(fn.argtypes) == [getattr(C, t) for t in argtypes], name
        assert fn.restype is (restype and getattr(C, restype)), name
        wide += restype not in (None, "c_int32", "c_int")
    assert wide >= 37      # uint64_t sizes and distortions, int64_t, size_t, const char *, void *, ...


def test_64_bit_return_arrives_whole(monkeypatch):
    """svt_hip_tf_workspace_bytes is layout arithmetic (no device): 8K pictures with 32 references need more than 4 GiB, and a
    freshly loaded handle says so without any restype set by the caller."""
    monkeypatch.setattr(abi, "_lib", None)
    assert abi.load().svt_hip_tf_workspace_bytes(7680, 4320, abi.TF_MAX_REFS) > 2 ** 32


MIRRORS = [c for c in vars(abi).values() if isinstance(c, type) and issubclass(c, C.Structure) and c.__module__ == abi.__name__]


@functools.lru_cache(maxsize=None)
def c_layouts():
    """sizeof of SvtHip<mirror>, and offsetof and sizeof of each of its members, for every mirror, as the compiler has them."""
    exprs = []
    for m in MIRRORS:
        s = "SvtHip" + m.__name__
        exprs.append(f"sizeof({s})")
        for f, _ in m._fields_:
            exprs += [f"offsetof({s}, {f})", f"sizeof((({s} *)0)->{f})"]
    return header_values(exprs)


@pytest.mark.parametrize("mirror", MIRRORS, ids=lambda m: m.__name__)
def test_mirror_has_the_layout_of_its_header_struct(mirror):
    """Every ctypes.Structure of abi.py is SvtHip<its name> of include/*.h: size and every field's offset and size as the compiler
    has them, and abi.record_dtype(mirror), the numpy view of an array of them, is the same record."""
    fields = [f for f, _ in mirror._fields_]
    s, want, dt = "SvtHip" + mirror.__name__, c_layouts(), abi.record_dtype(mirror)
    assert C.sizeof(mirror) == dt.itemsize == want[f"sizeof({s})"] and list(dt.names) == fields
    for f in fields:
        offset, size = want[f"offsetof({s}, {f})"], want[f"sizeof((({s} *)0)->{f})"]
        assert (getattr(mirror, f).offset, getattr(mirror, f).size) == (offset, size), f
        assert (dt.fields[f][1], dt.fields[f][0].itemsize) == (offset, size), f


@pytest.mark.parametrize("mirror", [abi.WarpDesc, abi.CdefPickParams, abi.CdefPickResult], ids=lambda m: m.__name__)
def test_mirror_has_no_implicit_padding(mirror):
    end = 0
    for f, _ in mirror._fields_:
        assert getattr(mirror, f).offset == end, f"implicit padding before {mirror.__name__}.{f}"
        end += getattr(mirror, f).size
    assert end == C.sizeof(mirror)


def test_record_views_are_derived_from_their_mirrors():
    """The literal sizes pin the headers themselves, not only the agreement; the shapes are what the CDEF pick tests index."""
    assert [C.sizeof(m) for m in (abi.IntraPredDesc, abi.CflDesc, abi.LrUnit, abi.WarpDesc)] == [64, 56, 44, 104]
    assert abi.INTRA_PRED_DESC_DTYPE.itemsize == 64 and abi.CFL_DESC_DTYPE.itemsize == 56 and abi.LR_UNIT_DTYPE.itemsize == 44
    dt = abi.CDEF_PICK_RESULT_DTYPE
    assert abi.CDEF_MAX_STRENGTHS == 64
    assert (abi.CDEF_PICK_WIDTHS, abi.CDEF_PICK_MAX_LEVELS) == dt["lev0"].shape == dt["lev1"].shape == (4, 8)
    assert abi.RATE_TABLES_DTYPE["coeff"].shape == (5, 2) and abi.RATE_TABLES_DTYPE["coeff"].base == abi.COEFF_COST_DTYPE
    assert abi.COEFF_COST_DTYPE["lps"].shape == (21, 26) and abi.record_dtype(abi.MvCostParam)["ref_mv"] == np.dtype("<u8")


# what the per-feature constant tests of blend, warp and CDEF pick compared one by one before this test took them over
REQUIRED_CONSTANTS = {"SVT_HIP_BLEND_D16", "SVT_HIP_BLEND_D16_DIFFWTD", "SVT_HIP_BLEND_MASK", "SVT_HIP_BLEND_VMASK", "SVT_HIP_BLEND_HMASK",
                      "SVT_HIP_WEDGE_TYPES", "SVT_HIP_MASK_SEARCH_OK", "SVT_HIP_MASK_SEARCH_BAD_WEDGE_SIZE", "SVT_HIP_MASK_SEARCH_BAD_DESC",
                      "SVT_HIP_WARP_FILTER_ROWS", "SVT_HIP_WARP_FILTER_BYTES", "SVT_HIP_WARP_ERROR_BLOCK", "SVT_HIP_WARP_ERROR_OK",
                      "SVT_HIP_WARP_ERROR_BAD_SHEAR", "SVT_HIP_CDEF_MAX_STRENGTHS"}
CONSTANTS_FLOOR = 43   # how many of the headers' 59 constants abi.py states today; a count of what exists, it only grows


def header_constants():
    """Every object-like integer macro and every enumerator named SVT_HIP_* of include/*.h."""
    names = []
    for h in sorted(glob.glob(os.path.join(abi.REPO_ROOT, "include", "*.h"))):
        with open(h) as f:
            text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
        names += re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SVT_HIP_\w+)[ \t]+[-+~()\w \t*<|]+$", text, re.M)   # a value, no strings, no continuation
        for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
            names += re.findall(r"\bSVT_HIP_\w+(?=\s*(?:=|,|$))", body)
    return names


def test_constants_are_those_of_the_headers():
    """Every SVT_HIP_X of the headers that abi.py states (as X or as SVT_HIP_X) has the header's value there: the status codes as
    the signed 32-bit values a ctypes call returns, everything else as 64-bit."""
    names = header_constants()
    assert len(set(names)) == len(names)
    matched = set()
    for name, value in header_values(names).items():
        mine = getattr(abi, name, getattr(abi, name[len("SVT_HIP_"):], None))
        if type(mine) is int:
            assert (mine - value) % (1 << (32 if name.startswith("SVT_HIP_ERR_") else 64)) == 0, (name, mine, value)
            matched.add(name)
    assert matched >= REQUIRED_CONSTANTS, REQUIRED_CONSTANTS - matched
    assert len(matched) >= CONSTANTS_FLOOR, sorted(matched)


def test_every_mirror_is_covered():
    assert len(MIRRORS) >= 43 and len({m.__name__ for m in MIRRORS}) == len(MIRRORS)


def test_struct_sizes_match_header():
    """ctypes mirrors must have the C layout (checked against the compiler through the oracle library); the literal sizes pin the
    headers themselves, not only the agreement."""
    import pyorc
    orc = pyorc.oracle()
    assert orc.orc_sizeof_me_params() == C.sizeof(abi.MeParams)
    assert orc.orc_sizeof_me_job() == C.sizeof(abi.MeFrameJob)
    assert orc.orc_sizeof_plane() == C.sizeof(abi.Plane8)
    assert C.sizeof(abi.SadLoopDesc) == 48 and C.sizeof(abi.SadLoopResult) == 16
    assert C.sizeof(abi.MeSearchResult) == 16
    assert orc.orc_sizeof_lf_frame() == C.sizeof(abi.LfFrame)
    assert C.sizeof(abi.LfMi) == 8 and C.sizeof(abi.CdefList) == 2
    assert C.sizeof(abi.LrUnit) == 44


def test_rtcd_lookup_covers_every_tier_a_export():
    """svt_hip_rtcd_lookup(<reference pointer name>) resolves exactly the <name>_hip exports."""
    lib = abi.load()
    tier_a = [n[:-4] for n in declared_symbols() if n.endswith("_hip") and not n.startswith("svt_hip_")]
    assert len(tier_a) >= 120
    for n in tier_a:
        fn = lib.svt_hip_rtcd_lookup(n.encode())
        assert fn == C.cast(getattr(lib, n + "_hip"), C.c_void_p).value, n
    for n in ("svt_hip_init", "svt_no_such_kernel", "memcpy", ""):
        assert lib.svt_hip_rtcd_lookup(n.encode()) is None


def test_tier_a_exports_are_exactly_the_declared_leaves():
    """The dynamic symbol table holds one <pointer>_hip text symbol per Tier A prototype of include/*.h, no more and no fewer:
    the set the bind-table generator derives (one per line of tools/e2e/svt_hip_bind_table.inc after its header line)."""
    gen_bind_table = _generator("gen_bind_table")
    so = os.path.join(abi.REPO_ROOT, "svt-av1-mod-by-patman_amd", "csrc", "libsvtav1_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    exported = {f[2][:-4] for f in (ln.split() for ln in out.splitlines())
                if len(f) == 3 and f[1] == "T" and f[2].endswith("_hip") and not f[2].startswith("svt_hip_")}
    declared = set(gen_bind_table.tier_a_names())
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    with open(os.path.join(abi.REPO_ROOT, "tools", "e2e", "svt_hip_bind_table.inc")) as f:
        assert len(f.read().splitlines()) - 1 == len(declared)


def test_no_device_error_path():
    """Without a GPU the product path fails loudly instead of falling back to the CPU."""
    lib = abi.load()
    if lib.svt_hip_device_count() > 0:
        return
    assert lib.svt_hip_init(0) != 0
    assert b"no HIP device" in lib.svt_hip_last_error()


def test_no_stream_ordered_allocator_on_the_launch_paths():
    """The library neither allocates nor frees device memory stream-ordered (hipMallocAsync / hipFreeAsync): the round-1
    abort was confined to the one call path that did; descriptors travel through the event-guarded
    per-thread staging ring of runtime.cpp instead."""
    so = os.path.join(abi.REPO_ROOT, "svt-av1-mod-by-patman_amd", "csrc", "libsvtav1_hip.so")
    und = subprocess.run(["nm", "-D", "--undefined-only", so], check=True, capture_output=True, text=True).stdout
    for sym in ("hipMallocAsync", "hipFreeAsync", "hipMallocFromPoolAsync"):
        assert sym not in und, sym


def test_uninitialised_library_refuses_to_pick_a_device():
    """No silent fall-back to GPU 0 for a process that forgot svt_hip_init: without a successful init every entry
    point that needs the device reports SVT_HIP_ERR_NO_DEVICE."""
    rc, said_so = fresh_process('lib.svt_hip_malloc(C.byref(p), 64), "not initialised" in lib.svt_hip_last_error().decode()')
    assert rc == abi.SVT_HIP_ERR_NO_DEVICE and said_so
