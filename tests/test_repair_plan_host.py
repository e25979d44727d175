"""CPU test of the host side of a repair launch (deoss_amd/csrc/rs_plan.hpp: repair_plan, RepairBatch,
repair_add -- plans and their cache, table sharing, the flag that picks the kernel, a descriptor's
addresses).  A stand-alone program (tests/cpp/test_repair_plan.cpp), built plain with -Wall -Werror
and with ASan/UBSan, run directly: no GPU.  tests/test_repair_plan.py checks the same plans through
the library (dm_rs_repair_plan) against the Python oracle."""
import os
import subprocess

from test_fp_host import ROOT, _builds


def test_repair_plan_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_repair_plan.cpp")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_repair_plan_{name}")
        subprocess.run(cc + [src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "repair plan OK" in out.stdout
        counted = {tuple(ln.split()[1:3]): int(ln.split()[3]) for ln in out.stdout.splitlines() if ln.startswith("plans")}
        # every pattern with at least k present, with want = all and with a subset
        assert counted[("4", "8")] == 2 * sum(1 for p in range(1 << 12) if bin(p).count("1") >= 4), name
        assert counted[("3", "2")] == 2 * 16 and counted[("1", "8")] == 2 * 511, name
