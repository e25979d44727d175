"""CPU tests of the FullProcessing host code shared by dm_process_*, dm_full_processing, the
processing stream, dm_fragment_lookup and the restore path: the layout (deoss_amd/csrc/fp_layout.hpp)
and the output files (deoss_amd/csrc/fp_files.hpp).  Stand-alone programs (tests/cpp/test_fp_layout.cpp,
tests/cpp/test_fp_files.cpp), built plain with -Wall -Werror and with ASan/UBSan, run directly: no GPU."""
import os
import shutil
import subprocess

import pytest

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


@pytest.mark.parametrize("prog, ok", [("test_fp_layout", "fp layout OK"), ("test_fp_files", "fp files OK")])
def test_fp_host_cpp_plain_and_asan(tmp_path, prog, ok):
    src = os.path.join(ROOT, "tests", "cpp", prog + ".cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"{prog}_{name}")
        subprocess.run(cc + [src, "-o", exe, "-pthread"], check=True)
        scratch = tmp_path / f"scratch_{name}"
        scratch.mkdir()
        out = subprocess.run([exe, str(scratch)], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert ok in out.stdout
