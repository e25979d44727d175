"""CPU test of the host side of the Reed-Solomon entry points (deoss_amd/csrc/rs_plan.hpp: matrices,
input choice and inverse, restore plans, statuses, the descriptors and tables of a restore launch) and
of the restore path's file helpers in deoss_amd/csrc/fp_files.hpp.  A stand-alone program
(tests/cpp/test_rs_plan.cpp), built plain with -Wall -Werror and with ASan/UBSan, run directly: no
GPU.  tests/test_restore_plan.py checks the same code through the library (dm_rs_restore_plan)."""
import json
import os
import subprocess

from test_fp_host import ROOT, _builds


def test_rs_plan_cpp_plain_and_asan(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_rs_plan.cpp")
    with open(os.path.join(ROOT, "tests", "golden", "rs_golden.json")) as f:
        golden = {(m["data"], m["parity"]): m["rows"] for m in json.load(f)["matrices"]}
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    for name, cc in _builds():
        exe = str(tmp_path / f"test_rs_plan_{name}")
        subprocess.run(cc + [src, "-o", exe, "-pthread"], check=True)
        scratch = tmp_path / f"scratch_{name}"
        scratch.mkdir()
        out = subprocess.run([exe, str(scratch)], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (name, out.stdout, out.stderr)
        assert "rs plan OK" in out.stdout
        printed = {}
        for ln in out.stdout.splitlines():
            w = ln.split()
            if w and w[0] == "matrix":
                printed[(int(w[1]), int(w[2]))] = w[3:]
        assert set(printed) == {(4, 8), (8, 8)}, name
        for shape, rows in printed.items():
            assert rows == golden[shape], (name, shape)
