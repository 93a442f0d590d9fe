"""Census of what every Tier B export answers before the library is initialised: tests/golden/tier_b_refusals.json holds, per export,
the (return code, svt_hip_last_error() text) of three probes made in one process that loaded the library and never called svt_hip_init.
It pins every refusal text (the names that aliases report and the formatted numbers included), which exports get as far as asking for
the device, and on which side of that question each one accepts an empty batch.  No device is needed, and none is touched.
The fixture is written by tests/golden/make_golden_refusals.py."""
import json
import os
import subprocess
import sys

from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tier_b_refusals.json")

# null: every pointer NULL, every integer 0; empty: every pointer one zero-filled 64 KiB buffer, every integer 0; one: that buffer, every integer 1
PROBES = ("null", "empty", "one")

# Exports the census leaves alone, each for what it would do in a process without svt_hip_init:
EXCLUDED = {
    "svt_hip_init": "would take a device on a GPU machine",
    "svt_hip_free": "reaches the HIP runtime without asking for a device",
    "svt_hip_host_free": "reaches the HIP runtime without asking for a device",
    "svt_hip_stream_destroy": "reaches the HIP runtime without asking for a device",
    "svt_hip_event_destroy": "reaches the HIP runtime without asking for a device",
    "svt_hip_comm_create": "reaches RCCL",
    "svt_hip_comm_destroy": "reaches RCCL",
    "svt_hip_comm_get_unique_id": "reaches RCCL",
    "svt_hip_device_count": "reaches the HIP runtime: its answer is the machine's",
}
# One probe of one export: it reads both arguments unchecked, so NULL ends the host process with a segmentation fault.
EXCLUDED_PROBES = {("svt_hip_warp_shear_params", "null")}


def census_names():
    """Every svt_hip_* prototype that returns int32_t and is not excluded."""
    return sorted(n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_int32" and n not in EXCLUDED)


# Runs in the child.  The error text is the thread's and a call that succeeds, or refuses without a text, leaves the previous one in
# place: a refusal of svt_hip_install_rtcd puts a known text there before every probe, and a probe that leaves it untouched records None.
_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from svtav1_hip import abi
from svtav1_hip.prototypes import PROTOTYPES
lib = abi.load()
buf = C.create_string_buffer(65536)
ptr = C.cast(buf, C.c_void_p)
out = {}
for name in json.loads(sys.argv[2]):
    fn, row = getattr(lib, name), []
    for probe in ("null", "empty", "one"):
        if [name, probe] in json.loads(sys.argv[3]):
            row.append(None)
            continue
        C.memset(buf, 0, len(buf))
        assert lib.svt_hip_install_rtcd(None, 1, None) == abi.SVT_HIP_ERR_BAD_PARAMETER
        mark = lib.svt_hip_last_error()
        args = [(None if probe == "null" else ptr) if t == "c_void_p" else int(probe == "one") for t in PROTOTYPES[name][1]]
        rc = int(fn(*args))
        text = lib.svt_hip_last_error()
        row.append([rc, None if text == mark else text.decode()])
    out[name] = row
json.dump(out, sys.stdout)
"""


def census():
    """{export: [[return code, error text or None], ... one per probe]} from one fresh interpreter."""
    for _, argtypes in (PROTOTYPES[n] for n in census_names()):
        assert all(t == "c_void_p" or t in ("c_int", "c_int32", "c_uint32", "c_int64", "c_uint64", "c_size_t") for t in argtypes), argtypes
    r = subprocess.run([sys.executable, "-c", _CHILD, abi.PKG_ROOT, json.dumps(census_names()), json.dumps(sorted(EXCLUDED_PROBES))],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout)


def test_census_covers_every_status_export():
    """Every int32_t svt_hip_* prototype is either probed or excluded with a reason, the exclusions exist and stay few, and the fixture
    has exactly the probed names: a new export cannot be forgotten."""
    status = {n for n, (restype, _) in PROTOTYPES.items() if n.startswith("svt_hip_") and restype == "c_int32"}
    assert set(EXCLUDED) <= status and len(EXCLUDED) <= 10 and all(EXCLUDED.values())
    assert {n for n, _ in EXCLUDED_PROBES} <= status - set(EXCLUDED) and len(EXCLUDED_PROBES) == 1
    with open(GOLD) as f:
        gold = json.load(f)
    assert sorted(gold) == census_names() and set(census_names()) | set(EXCLUDED) == status


def test_refusals_match_the_census():
    """All three probes of every export answer what the fixture recorded: the same return code and the same text, byte for byte."""
    with open(GOLD) as f:
        gold = json.load(f)
    got = census()
    diff = {n: (got.get(n), gold[n]) for n in gold if got.get(n) != gold[n]}
    assert not diff and sorted(got) == sorted(gold), diff
    # what the fixture itself must show: the empty-batch order on both sides of the device question, and the aliases' names
    ok, bad, none = abi.SVT_HIP_OK, abi.SVT_HIP_ERR_BAD_PARAMETER, abi.SVT_HIP_ERR_NO_DEVICE
    for n in ("svt_hip_subpel_search_batch", "svt_hip_obmc_search_batch", "svt_hip_obmc_target_batch"):
        assert gold[n][1][0] == ok, n
    assert gold["svt_hip_txfm_quant_batch"][1][0] == none
    assert gold["svt_hip_convolve_sr_batch"][0] == [bad, gold["svt_hip_convolve_batch"][0][1]]
    assert gold["svt_hip_convolve_sr_batch"][0][1].startswith("svt_hip_convolve_batch:")
    assert gold["svt_hip_me_validate_jobs"][0][1].startswith("svt_hip_me_frames:")
    for n in ("svt_hip_malloc", "svt_hip_host_alloc", "svt_hip_stream_create"):
        assert gold[n][0] == [bad, None], n
