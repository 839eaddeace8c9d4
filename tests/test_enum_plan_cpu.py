"""The trip plan of the forward's run-following enumeration (csrc/nlosgr_enum.hpp, trip_plan), on the host.

trip_plan decides, per lane, which groups of adjacent passing cells a trip of the enumeration appends to the
ray queue and how many cells it consumes; the kernel's enumeration loop ends only when every lane has consumed
its box, so a plan that consumed no cell would hang the forward.  This test compiles a stand-alone program
(tests/enum_plan_main.cpp, with the address and undefined-behaviour sanitizers) around the header and lets it walk
rows of 1 .. 12 cells for every pass mask and K = 2, 3.  It checks: every passing cell is emitted exactly once
and no failing cell ever; every trip consumes at least one cell, so trips per row <= the row's length; at most
2 entries per trip (the ray queue ring's bound); groups are contiguous and hold at most K cells; every run of
passing cells is cut into groups of K from its left end, so the rays left single are at most the runs whose
length is no multiple of K.
"""
import os
import shutil
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "nlos-gaussian-renderer_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "enum_plan_main.cpp")


def test_trip_plan_all_rows(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "enum_plan")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, MAIN, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("ok:")
