"""The workspace guard's host-only bookkeeping (aquery2_amd/csrc/ws_guard.hpp) under AddressSanitizer and UBSan: a stand-alone
program with its own main, built and run here.  No GPU, nothing loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ws_guard_selftest(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "ws_guard_selftest")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "ws_guard_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    # (the sanitizer runtimes are linked statically: the program needs nothing preloaded and does not care what is)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ws_guard selftest ok" in run.stdout


def test_ws_guard_header_is_host_only():
    """the bookkeeping header includes no HIP (it has to build with a plain host compiler)"""
    src = open(os.path.join(ROOT, "aquery2_amd", "csrc", "ws_guard.hpp")).read()
    assert "#include <hip" not in src and "aqg_internal" not in src
