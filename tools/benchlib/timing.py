"""What the tools/*_time.py measurements share: the library on device 0, HIP events around a launch, the median / min / max record,
and where a profile is written."""
import json
import os
import statistics

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def open_library():
    """libsvtav1_hip initialised on device 0, or None without a device.  torch comes first, as bench.py has it: both then share
    one HIP runtime."""
    import torch  # noqa: F401
    from svtav1_hip import abi
    lib = abi.load()
    return lib if lib.svt_hip_init(0) == 0 else None


def events(torch, stream, repeats, launch, warmup=3):
    """Milliseconds of each of `repeats` launches between two HIP events on `stream`, after `warmup` untimed ones."""
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(repeats)]
    for a, b in evs:
        a.record(stream)
        launch()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def write_profile(name, res):
    """One JSON line on stdout and the same record, indented, in profiles/<name> (or at `name` itself where it is absolute)."""
    print(json.dumps(res))
    path = os.path.join(ROOT, "profiles", name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
