"""The pair windows' host-only route and workspace arithmetic (aquery2_amd/csrc/pair_route.hpp) under AddressSanitizer and UBSan: a
stand-alone program with its own main, built and run here.  No GPU, nothing loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_route_selftest(tmp_path):
    cxx = shutil.which("g++")                        # (-static-libasan / -static-libubsan are GCC's spellings)
    if cxx is None:
        pytest.fail("no g++")
    exe = str(tmp_path / "pair_route_selftest")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "pair_route_selftest.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    # (the sanitizer runtimes are linked statically: the program needs nothing preloaded and does not care what is)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pair_route selftest ok" in run.stdout


def test_pair_route_header_is_host_only():
    """the header includes no HIP (it has to build with a plain host compiler), and its routes are those the test cases assume"""
    import pairwin_cases as pc
    src = open(os.path.join(ROOT, "aquery2_amd", "csrc", "pair_route.hpp")).read()
    assert "#include <hip" not in src and "aqg_internal" not in src
    assert "REG_MAX_W = %d;" % pc.REG_W in src and "LDS_MAX_W = %d;" % pc.LDS_W in src and "TILE_ROWS = %d;" % pc.TS in src
