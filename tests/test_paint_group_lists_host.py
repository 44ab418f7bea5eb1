"""The slice arithmetic of the grouping kernel's wave-private lists (astrild_amd/csrc/paint_group_lists.h) in a
stand-alone host program under AddressSanitizer and UBSan: tests/host/paint_group_lists_test.cpp."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slice_arithmetic_under_sanitizers(tmp_path):
    rocm_clang = "/opt/rocm/lib/llvm/bin/clang++"              # the compiler the library itself is built with
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++") or (rocm_clang if os.path.exists(rocm_clang) else None)
    assert cxx is not None, "no host C++ compiler: neither g++ / clang++ / c++ on PATH nor " + rocm_clang
    exe = tmp_path / "paint_group_lists_test"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "astrild_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "paint_group_lists_test.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "fill combinations ok" in run.stdout
