"""The memo behind edgl_lds_limit (csrc/lds_limit.h: the dynamic-LDS limit of a kernel, remembered per (kernel, device)) is plain
C++ without HIP, so it is checked on the host: tests/host/lds_limit_main.cpp — a stand-alone program with a counting fake in place
of hipFuncSetAttribute — is built twice with the host compiler, under ThreadSanitizer and under Address + UndefinedBehavior
sanitizer, and run as an ordinary child process.  CPU only; nothing that is loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "lds_limit_main.cpp")
INC = os.path.join(ROOT, "easydgl_amd", "csrc")


def _host_compiler():
    # clang first: it links the sanitizer runtime statically, so the program does not depend on the order of preloaded libraries
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "clang++", "g++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_lds_limit_memo_under_sanitizer(tmp_path, sanitize):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lds_limit_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread",
           "-I", INC, SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.strip() == "ok", r.stdout[-1000:]
    for mark in ("Sanitizer", "runtime error"):
        assert mark not in r.stderr, r.stderr[-3000:]
