"""The host side every Tier B entry point shares (csrc/runtime.cpp: the per-thread state, the event-guarded grow-only buffers, the
call scope TierBCall, svt_hip_init and the stream pool) is plain C++ over about twenty HIP runtime functions.
tests/runtime_driver.cpp links it against a fake runtime in host memory that defers every upload until something waits for its
stream, notices a source overwritten or memory freed while a copy is in flight, and whose n-th call can be made to fail: the failure
paths the GPU tests must never provoke run here, under the host's address, undefined-behaviour and thread sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# per-thread buffers and pooled streams are never handed back, by design: the leak check would report exactly that
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1 exitcode=66")
SVT_HIP_ERR_RUNTIME = -2147479551   # 0x80001001 (include/svt_hip.h)


def build(tmp_path_factory, sanitizer):
    exe = str(tmp_path_factory.mktemp("runtime_host") / "runtime_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-Wall", "-Werror", f"-fsanitize={sanitizer}", "-fno-sanitize-recover=undefined",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"), os.path.join(ROOT, "svt-av1-mod-by-patman_amd", "csrc", "runtime.cpp"),
                    os.path.join(ROOT, "tests", "runtime_driver.cpp"), "-ldl", "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory, "address,undefined")


@pytest.fixture(scope="module")
def tsan_driver(tmp_path_factory):
    return build(tmp_path_factory, "thread")


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, (args, r.stdout + r.stderr)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r


def test_scripted_call_succeeds_and_every_failure_point_unwinds(driver):
    """The driver itself asserts, for the failing call: SVT_HIP_ERR_RUNTIME, a message that names the call and the HIP function; and
    after it: a clean call on another stream succeeds, no source was overwritten in flight and nothing was freed early."""
    n_calls, rc = (int(x) for x in run(driver, "script", "-1").stdout.split()[1::2])
    assert rc == 0 and n_calls >= 12   # two slots reused, one slot and one buffer grown, two buffers taken, launch check, four events
    for n in range(n_calls):
        out = run(driver, "script", str(n)).stdout.split()
        assert int(out[3]) == SVT_HIP_ERR_RUNTIME, (n, out)


def test_nine_calls_through_four_slots_wait_once_per_reuse(driver):
    assert run(driver, "ring").stdout.split() == ["event_syncs", "5"]


def test_growth_waits_for_the_buffers_own_event_only(driver):
    assert run(driver, "grow").stdout.split() == ["device_syncs", "1"]   # svt_hip_init's, after the warm-up


def test_nested_scope_leaves_the_outer_slot_alone(driver):
    run(driver, "nested")


def test_failed_warm_up_is_repeated_by_the_next_init(driver):
    assert run(driver, "failed_init").stdout.split() == ["device_syncs", "2"]


def test_sixteen_threads_on_the_stream_pool(driver, tsan_driver):
    run(tsan_driver, "threads")
    run(driver, "threads")
