"""CPU test of the grouped product's tile map (cuda-l2_amd/csrc/hgemm_grouped.hpp, shared by the grouped kernels, the grouped reference kernel
and this program): tests/grouped_map_host.cpp restates the map's contract against a plain loop over rows, for BM = 64 and 128 over 400 offset
vectors each, malformed ones included.  A stand-alone program built by the host compiler with its address and undefined-behaviour sanitizers."""
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]


def test_the_map_covers_every_group_row_once_and_stays_in_bounds(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "grouped_map_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{REPO / 'cuda-l2_amd' / 'csrc'}", str(REPO / "tests" / "grouped_map_host.cpp"), "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "800 offset vectors checked" in res.stdout, res.stdout + res.stderr
