"""The region / window geometry the two windowed MSDA kernels share (csrc/msda_window_geom.h), on the host: the item a lane
of the kernels computes (region_item) against the host forms the planning uses (q_bound, ext_lo, ext_hi), the partition of
an axis into regions, the window property the kernels' one-compare-per-axis test relies on, and the range of the
reciprocal division's dividends.  No GPU, nothing preloaded: a stand-alone program (tests/cabi_c/msda_window_host_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_region_geometry_host_check(tmp_path):
    """n in 1..96 and {1000, 4095, 4096}, every R in 1..min(n, 32) (64 takes 15 s under the sanitizers, 32 takes 3.5 s; the
    offset range is whole), every region, window offsets lo <= hi in -12..12:
    region_item's items 0 / 2 == ext_lo, 1 / 3 (raised to first + 1) == ext_hi, 4..7 == q_bound(r) / q_bound(r + 1);
    q_bound(0) == 0, q_bound(R) == n, non-decreasing; every corner of every query pixel at every offset in [lo, hi] lies
    inside [first, last]; every dividend is at most region_dividend_bound (the planning's 2^22 test).  On the host idiv is
    exact division: this pins the formulas, not the device's reciprocal.  Under -fsanitize=address,undefined where the
    compiler has the runtimes."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "msda_window_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(ROOT, "co-detr-tensorrt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cabi_c", "msda_window_host_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    built = subprocess.run(cmd + san, capture_output=True).returncode == 0
    probe = subprocess.run([exe, "1"], capture_output=True, text=True) if built else None
    if probe is not None and probe.returncode != 0:
        # a finding of the program or of a sanitizer is a failure; only a runtime that cannot start in this process
        # environment (it says so before main runs: no check has printed, no sanitizer report) sends us to the plain build
        assert ("FAILED" not in probe.stdout and "ERROR: AddressSanitizer: " not in probe.stderr
                and "ERROR: LeakSanitizer: " not in probe.stderr and "runtime error" not in probe.stderr), \
            probe.stdout[-2000:] + probe.stderr[-2000:]
    if probe is None or probe.returncode != 0:
        # a compiler without the sanitizer runtimes: the same program without them still holds the formulas together
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe, "32"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("clean"), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(r.stdout.split()[-2]) > 1000000   # (the sweep ran: (n, R, r, lo, hi) cases)
