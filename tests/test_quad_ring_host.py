"""CPU test of K1Q's ring and barrier schedule (deoss_amd/csrc/quad_ring.hpp, shared by the two
waves of leaf_kernel_quad): tests/cpp/test_quad_ring.cpp steps a producer and a consumer state
machine built from the header through every stage count and every pair of leaf lengths in a wave.
A stand-alone program, built plain with -Wall -Werror and with ASan/UBSan, run directly: no GPU.
Also the stream model (tools/quad_stream_model.py): one step stream across stage boundaries against
hashlib.sha256."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _builds():
    builds = [("plain", ["g++", "-O2", "-std=c++17", "-Wall", "-Werror"])]
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    san = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if os.path.exists(clang):
        builds.append(("asan", [clang] + san + ["-fno-omit-frame-pointer"]))
    elif shutil.which("g++"):
        builds.append(("asan", ["g++"] + san))
    return builds


def test_quad_ring_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_quad_ring.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_quad_ring_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "quad ring OK" in out.stdout


def test_stream_model_links_across_stage_boundaries():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "quad_stream_model.py")],
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    runs = dict(re.findall(r"^run\s+(\[[\d, ]+\])\s+\d+ instructions .*\s(ok|MISMATCH)$", out.stdout, re.M))
    assert runs == {"[8, 8]": "ok", "[8, 8, 8, 8]": "ok", "[8, 8, 3]": "ok"}, out.stdout
    assert "MISMATCH" not in out.stdout
