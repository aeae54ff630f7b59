"""The one compile-and-run harness of the host tests: a stand-alone C++ program (its own main, no device, no HIP runtime) built
with the host compiler under AddressSanitizer and UBSan, run as its own process."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def build(tmp_path, name):
    """tests/<name>.cpp compiled into tmp_path; the path of the program."""
    cxx = shutil.which(os.environ.get("CXX") or "g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / name)
    cc = subprocess.run([cxx] + FLAGS + ["-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    return exe


def run(exe, args=(), tail=8000):
    """Runs the program, prints the end of what it wrote, asserts that it exited with 0; its stdout."""
    done = subprocess.run([exe] + [str(v) for v in args], capture_output=True, text=True)
    print("\n" + done.stdout[-tail:] + done.stderr[-4000:])
    assert done.returncode == 0, done.stdout[-4000:] + done.stderr[-4000:]
    return done.stdout
