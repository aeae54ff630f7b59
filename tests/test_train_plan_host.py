"""The training step's launch plan (csrc/train_plan.h) on the CPU: tests/train_plan_check.cpp, a stand-alone program, builds the
plan of the three nets under all 64 combinations of the six plan switches and checks that plan_train never refuses, that
every layer has one kernel of each kind, that virtual tensors and rebuilt dz are read only by kernels that rebuild them,
that every BatchNorm layer has one source of its backward sums, that every gradient tensor is stored or zeroed once and then
only added to, and that a switch leaves alone what it does not govern.  Compiled with the host compiler under
AddressSanitizer and UBSan and run as its own process; this file only compiles, runs and reports."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_launch_plans_of_the_three_nets_under_every_switch_combination(tmp_path):
    cxx = shutil.which(os.environ.get("CXX") or "g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "train_plan_check")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "train_plan_check.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    print("\n" + run.stdout[-4000:] + run.stderr[-4000:])
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "192 plans, 0 failures" in run.stdout
