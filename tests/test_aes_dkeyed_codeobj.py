"""CPU test of the keyed AES-CBC decrypt kernel in the built library's gfx950 code object.  Its
metadata notes (llvm-readelf) must show one kernel (the round count is a branch inside, not a template
argument), no private segment and no spills -- the round keys of all three unrolled loops are
indexed at compile time; a run-time round index would send them to scratch -- a workgroup of 256
lanes, and exactly the 5,120 bytes of LDS that aes_fill_lds fills (4 rotations of the T-table + the
S-box): descriptor and key come by scalar loads, so a key copy adds nothing.  Metadata only; no GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "deoss_amd", "libdeoss_merkle.so")
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
LDS_BYTES = 5 * 256 * 4   # 5,120: aes_fill_lds's tables, and no key copy


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    from deoss_amd import build as b
    b.build(verbose=False)
    d = tmp_path_factory.mktemp("dkeyed_codeobj")
    fat, elf = d / "fat.bin", d / "gfx950.elf"
    # an explicit output file: objcopy without one rewrites the library in place
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", LIB, str(fat)], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    f"--targets={TARGET}", f"--output={elf}"], check=True)
    return subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(elf)], check=True, capture_output=True,
                          text=True).stdout


def _kernel_records(notes):
    """{kernel name: {field: value}} of the amdhsa.kernels metadata (one '  - ' item per kernel)."""
    out = {}
    for item in re.split(r"^  - (?=\.)", notes, flags=re.M)[1:]:
        fields = dict(re.findall(r"^\s+(\.\w+):\s+(\S+)\s*$", "    " + item, flags=re.M))
        if ".name" in fields:
            out[fields[".name"]] = fields
    return out


def test_keyed_decrypt_kernel_has_no_scratch_no_spills_and_5k_lds(notes):
    recs = _kernel_records(notes)
    keyed = [k for k in recs if "aes_cbc_decrypt_keyed_kernel" in k]
    assert len(keyed) == 1, sorted(recs)   # one kernel, not one per round count: the branch is inside
    r = recs[keyed[0]]
    assert int(r[".private_segment_fixed_size"]) == 0, r
    assert int(r[".vgpr_spill_count"]) == 0 and int(r[".sgpr_spill_count"]) == 0, r
    assert int(r[".group_segment_fixed_size"]) == LDS_BYTES, r
    assert int(r[".max_flat_workgroup_size"]) == 256 and int(r[".wavefront_size"]) == 64, r
    # the parser reads the existing single-key decrypt kernels the same way (three instantiations, same LDS)
    single = [k for k in recs if "aes_cbc_decrypt_kernel" in k]
    assert len(single) == 3 and all(int(recs[k][".group_segment_fixed_size"]) == LDS_BYTES for k in single)
