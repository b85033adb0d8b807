"""The stripe mapping of the traversal launches (gravit_amd/csrc/xcd_stripes.h), host side (no GPU): tests/host/xcd_stripes_check.cpp -- a program of its own that
includes the header the kernels include -- is built with AddressSanitizer and UndefinedBehaviorSanitizer and run over every list length 0..4,200, unit size 64 / 128 / 320
and row length 0 / 64 / 576 / 1000 / 2048 / 8192."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gravit_amd", "csrc")


def compiler():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.fail("no host C++ compiler for the stand-alone mapping check")


def test_mapping_covers_every_list_exactly_once_under_sanitizers(tmp_path):
    exe = str(tmp_path / "xcd_stripes_check")
    cmd = [compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(ROOT, "tests", "host", "xcd_stripes_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert re.fullmatch(r"ok (\d+)\n", r.stdout), r.stdout
    assert int(r.stdout.split()[1]) == 4201 * 3 * 6 + 5

