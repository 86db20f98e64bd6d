"""Builds the stand-alone host programs of tests/host/: each includes one header of csrc/ that needs no GPU and has its own main."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def compiler():
    clang = os.path.join(ROCM, "llvm", "bin", "clang++")
    return clang if os.path.exists(clang) else shutil.which("g++")


def build(source, out_dir, flags=()):
    """tests/host/<source> -> an executable in out_dir; HIP's headers are found and read as on the AMD platform, no HIP runtime is linked."""
    exe = os.path.join(str(out_dir), os.path.splitext(source)[0])
    cmd = [compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"), *flags, "-o", exe, os.path.join(HERE, "host", source)]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, " ".join(cmd) + "\n" + done.stdout + done.stderr
    return exe
