"""CPU test of the cipher branch's host code: the AES key schedule (deoss_amd/csrc/aes_host.hpp,
encrypt keys and equivalent-inverse-cipher keys, against the FIPS-197 Appendix A expansions) and the
scheme geometry (deoss_amd/csrc/cipher_scheme.hpp).  A stand-alone program
(tests/cpp/test_cipher_host.cpp), built plain with -Wall -Werror and with ASan/UBSan, run directly:
no GPU."""
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


def test_cipher_host_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_cipher_host.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_cipher_host_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "cipher host OK" in out.stdout
