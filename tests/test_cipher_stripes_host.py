"""CPU test of the striped cipher file path's plan (dm_full_processing_cipher): the stripes of a
window (deoss_amd/csrc/fp_layout.hpp) and the plaintext span each one brings
(deoss_amd/csrc/cipher_scheme.hpp: stripe_span) at segment 256, 4,096 and 32 MiB over several slot
pitches: the spans tile [0, P) once and in order in whole AES blocks, no stripe crosses a fragment
boundary, exactly the last stripe carries the padding block.  A stand-alone program
(tests/cpp/test_cipher_stripes.cpp), built plain with -Wall -Werror and with ASan/UBSan, run
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


def test_cipher_stripes_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_cipher_stripes.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_cipher_stripes_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "cipher stripes OK" in out.stdout
