"""CPU test of the batched restore's host plan (deoss_amd/csrc/restore_batch_plan.hpp): what
dm_restore_batch decides before it touches the GPU.  Object counts {0, 1, 2, 17}, nseg {1, 2, 5},
parity fragments given {0, 1, 8} per segment, ciphers {none, 16, 24, 32 bytes, two objects sharing
one}, objects marked failed before the decrypt stage: offsets 16-byte aligned and disjoint, totals
match, the chain list holds exactly the surviving encrypted segments, keys deduplicated, every
argument error names the right object.  A stand-alone program
(tests/cpp/test_restore_batch_plan.cpp), built plain with -Wall -Werror and with ASan/UBSan, run
directly: no GPU."""
import os
import shutil
import subprocess

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


def test_restore_batch_plan_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_restore_batch_plan.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    builds = _builds()
    assert [name for name, _ in builds] == ["plain", "asan"], "no compiler for the sanitizer build"
    for name, cc in builds:
        exe = str(tmp_path / f"test_restore_batch_plan_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "restore batch plan OK (180 cases)" in out.stdout
