"""The layer every whole-picture hook of the patched encoder shares (tools/e2e/svt_hip_bind_dev.c: call scopes, the "first caller
computes the picture" table, device-resident mirrors, the pools) reaches the device only through the `sym` callback of its setup
function.  tests/bind_dev_driver.c hands it a fake device in host memory whose n-th call can be made to fail, so the failure paths
the GPU tests assert never run are exercised here, under the host's address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E = os.path.join(ROOT, "tools", "e2e")
# the pools never hand memory back to the driver, by design: the leak check would report exactly that
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
FAILURE = "bind_dev_driver: scripted call 7 stays on the CPU"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bind_dev") / "bind_dev_driver")
    subprocess.run(["gcc", "-std=gnu11", "-O1", "-g", "-pthread", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "include"), "-I", E2E, os.path.join(E2E, "svt_hip_bind_dev.c"),
                    os.path.join(ROOT, "tests", "bind_dev_driver.c"), "-o", exe], check=True)
    return exe


def run(driver, *args, env=ENV):
    r = subprocess.run([driver, *args], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_scripted_call_succeeds_and_every_failure_point_unwinds(driver):
    ok = run(driver, "script", "-1")
    n_calls, ret = (int(x) for x in ok.stdout.split()[1::2])
    assert ret == 0 and n_calls >= 10 and "stays on the CPU" not in ok.stderr
    assert "hook test_hook" in ok.stderr  # the scope added its timer
    for n in range(n_calls):
        r = run(driver, "script", str(n))
        assert r.stdout.split()[-1] == "1", (n, r.stdout)
        lines = [line for line in r.stderr.splitlines() if FAILURE in line]
        assert len(lines) == 1 and lines[0] == FAILURE + " (fake device error)", (n, r.stderr)


def test_one_acquisition_too_many_fails_the_call(driver):
    r = run(driver, "overflow")
    assert "no pin slot left" in r.stderr and "no block slot left" in r.stderr
    assert r.stderr.count("bind_dev_driver: too many") == 2


def test_once_run_computes_once_for_eight_threads(driver):
    run(driver, "once")


def test_mirrors_under_the_scope(driver):
    r = run(driver, "mirrors")
    assert "STALE" not in r.stderr.replace("0 STALE", "")
    run(driver, "mirrors", env=dict(ENV, SVTAV1_HIP_MIRROR_MB="0"))
