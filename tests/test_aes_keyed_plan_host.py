"""CPU test of the keyed AES-CBC launch's slot plan (deoss_amd/csrc/aes_keyed_plan.hpp): chains of
mixed key lengths are ordered so that every wave of aes_cbc_encrypt_keyed_kernel holds one round
count.  Group sizes {0, 1, 15, 16, 17, 33} in every combination over 10 / 12 / 14 rounds,
interleaved in the input: every chain once, one round count per wave, order kept within a group,
16 * sum ceil(n_g / 16) slots, nothing for no chains.  A stand-alone program
(tests/cpp/test_aes_keyed_plan.cpp), built plain with -Wall -Werror and with ASan/UBSan, run
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


def test_aes_keyed_plan_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_aes_keyed_plan.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_aes_keyed_plan_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "aes keyed plan OK (216 cases)" in out.stdout
