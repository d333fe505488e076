"""The C++ host mirror (csrc/rpt_host.cpp) on a CPU fake of the HIP runtime and of the C-ABI: no GPU needed.

tests/cpu_fake/ builds the unmodified tests/cpp/test_host_mirror.cpp against fake_hip.cpp (streams are lazy FIFOs
that run only what the host demands: the latest schedule HIP allows, so a missing hipStreamWaitEvent, a pinned
buffer refilled before its event or a result read before its synchronisation sees stale or poisoned bytes every
time) and fake_rpt_gpu.cpp (the C-ABI computed by the oracle, with strict workspaces), three times: plain,
ASan + UBSan and TSan. Every binary is a stand-alone program run directly; nothing is loaded into Python.

Wall times measured on an 8-core machine without a GPU (each subprocess timeout is four times its figure):
  host_mirror_fake        9 - 11 s (lazy, eager and the mixed schedules alike)
  host_mirror_fake_asan   38 s
  host_mirror_fake_tsan   259 s
"""
import os
import subprocess

import pytest

from conftest import REPO
from test_pushdown_plan import reference

FAKE = os.path.join(REPO, "tests", "cpu_fake")
BUILD = os.path.join(FAKE, "build")


def _build(target):
    subprocess.run(["make", "-s", "-C", FAKE, os.path.join("build", target)], check=True)
    return os.path.join(BUILD, target)


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k != "RPT_FAKE_EAGER"}
    env.update(extra)
    return env


def _run_ok(binary, env, timeout):
    r = subprocess.run([binary], capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-8000:]
    assert "ALL OK" in r.stdout, r.stdout[-4000:] + r.stderr[-8000:]
    return r


@pytest.mark.parametrize("mode", ["lazy", "eager", "mix:1", "mix:2", "mix:3"])
def test_host_mirror_on_fake(mode):
    """Every EXPECT of test_host_mirror.cpp under the latest (lazy) and the earliest (eager) legal schedule, and under
    three mixed ones (each stream eager or lazy by a hash of the seed): a write-after-read hazard between two streams
    shows only when the writer's stream runs early and the reader's late."""
    binary = _build("host_mirror_fake")
    env = _env() if mode == "lazy" else _env(RPT_FAKE_EAGER="1" if mode == "eager" else mode)
    _run_ok(binary, env, timeout=44)  # 4 x 11 s


def test_host_mirror_on_fake_asan():
    """The same run under AddressSanitizer + UndefinedBehaviorSanitizer with leak detection: any report fails it.
    The mirror's two intentionally leaked caches are suppressed (tests/cpu_fake/lsan.supp)."""
    binary = _build("host_mirror_fake_asan")
    _run_ok(binary, _env(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                         UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
                         LSAN_OPTIONS="suppressions=" + os.path.join(FAKE, "lsan.supp")), timeout=152)  # 4 x 38 s


def test_host_mirror_on_fake_tsan():
    """The same run under ThreadSanitizer (worker pool, parallel sinks, the shared caches): any report fails it."""
    binary = _build("host_mirror_fake_tsan")
    _run_ok(binary, _env(TSAN_OPTIONS="halt_on_error=1"), timeout=1036)  # 4 x 259 s


def test_pushdown_plan_on_fake():
    """tests/cpp/test_pushdown_plan.cpp linked against the fakes: the same table as with the product library."""
    binary = _build("pushdown_plan_fake")
    out = subprocess.run([binary], capture_output=True, text=True, check=True, timeout=60, env=_env()).stdout.split()
    assert len(out) == 2 * 3 * 2 * 2 * 2 * 2 * 2
    for line in out:  # the checks of test_pushdown_plan_every_combination
        dev, ft, fwd, tgt, rows, bfe, mm, passthrough, af, pbf, pmm, in_use = (int(x) for x in line.split(","))
        ref = reference(ft, fwd, tgt, rows, bfe, mm)
        if dev == 0:
            assert (passthrough, af, pbf, pmm) == ref, line
            assert in_use == int(not (fwd and tgt)), line
        else:
            assert pbf == 0, line
            assert (af, pmm) == ref[1:2] + ref[3:4], line
            forward_pushed = fwd and tgt
            assert passthrough == int(forward_pushed and ft == 2), line
            assert in_use == int(not forward_pushed or ft != 2), line


def test_fake_selftest():
    """The fake detects what it claims to (tests/cpu_fake/selftest.cpp): a read before the synchronisation, a
    pinned buffer refilled before its event, a missing cross-stream wait and a re-recorded event give poisoned or
    stale bytes in lazy mode, a buffer overwritten before another stream read it does with an eager writer and a
    lazy reader, and each gives the right bytes when done correctly; polling loops end; a short workspace is
    refused. Built with ASan + UBSan, so the fakes themselves are clean."""
    binary = _build("selftest")
    san = dict(ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = _run_ok(binary, _env(**san), timeout=60)
    assert "(lazy)" in r.stdout
    r = _run_ok(binary, _env(RPT_FAKE_EAGER="1", **san), timeout=60)
    assert "(eager)" in r.stdout
