"""The tile table of the grouped GEMM launch (csrc/gemm_group.h) on the host: tests/group_table_host.cpp, a stand-alone program
built with the address and undefined-behaviour sanitizers, deals the tiles of the benchmark's filters, of two- and one-problem
groups and of the edge cases (no rows, ragged last row tile, fewer tiles than workgroups) and checks that every tile is dealt
exactly once and none outside its problem."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


def test_every_tile_is_dealt_exactly_once(tmp_path):
    cxx = next((c for c in ("g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "group_table_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", os.path.join(PKG, "csrc"),
                            os.path.join(ROOT, "tests", "group_table_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-4000:], run.stderr[-4000:])
    assert "combsub 64x64" in run.stdout and "FAIL" not in run.stdout
