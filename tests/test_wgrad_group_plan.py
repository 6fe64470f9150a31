"""Planner of the grouped weight gradient on the CPU: builds
tools/wgrad_group_plan_check.cpp with the host compiler under the address and
undefined-behaviour sanitizers and runs it (coverage of every tile exactly
once, block indices inside the tables, disjoint partial regions inside the
workspace).  No GPU, no HIP: the planner header is plain C++."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_sweep_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "wgrad_group_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "dro-sfm_amd", "csrc"),
                           os.path.join(ROOT, "tools", "wgrad_group_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stderr
    assert "plans ok" in out.stdout
