"""CPU test of the range plan header (deoss_amd/csrc/range_plan.hpp) on its own: a stand-alone program
(tests/cpp/test_range_plan.cpp), built plain with -Wall -Werror and with ASan/UBSan, run directly: no
GPU.  tests/test_range_plan.py checks the same plans through the library (dm_range_plan)."""
import os
import subprocess

from test_fp_host import ROOT, _builds


def test_range_plan_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_range_plan.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_range_plan_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "range plan OK" in out.stdout
        counted = {ln.split()[1]: int(ln.split()[-1]) for ln in out.stdout.splitlines() if ln.startswith("cases")}
        # every (off, len) of every size, with and without a cipher, both settings of the padding flag
        assert counted["128"] == 2 * 2 * sum(s * (s + 1) // 2 for s in (1, 112, 113, 128, 129, 300, 384)), name
