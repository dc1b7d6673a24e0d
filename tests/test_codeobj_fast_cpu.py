"""
The register budget of every k_fast instantiation in the gfx950 code object (no GPU needed).

k_fast is latency-bound: its launch bound asks for six waves per SIMD, i.e. at most 80 vector registers, and the host's choice
of resident blocks per CU (snpm_api_launch.hpp: fast_geom, fast_two_level) counts on it.  The two-level instantiations
(k_fast<..., TWO>: a tile sum and an epoch sum per accession of the lane) carry four more fp64 registers than the others; they
must stay inside the same budget without spilling, and the others must not grow because of them.
"""
import os
import re
import shutil
import subprocess

import pytest

from snpmatch_amd import _lib
from test_codeobj_cpu import READELF, gfx950_code_object

VGPR_BUDGET = 80                    # 512 registers per lane and SIMD / 6 waves, in allocation units of 8


def kernel_notes(tmp_path):
    co = tmp_path / "snpm_gfx950.elf"
    co.write_bytes(gfx950_code_object(_lib.LIB_PATH))
    tool = READELF if os.path.exists(READELF) else shutil.which("llvm-readelf")
    notes = subprocess.run([tool, "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    return re.split(r"\n(?=\s*- \.agpr_count)", notes)[1:]


def field(k, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, k).group(1))


@pytest.mark.skipif(not (os.path.exists(READELF) or shutil.which("llvm-readelf")), reason="llvm-readelf not available")
def test_every_k_fast_instantiation_fits_six_waves_per_simd(tmp_path):
    fast = {}
    for k in kernel_notes(tmp_path):
        name = re.search(r"\.name:\s+(\S+)", k).group(1)
        if "6k_fastI" in name:                  # snpm::k_fast<...> (not k_fast_bits / k_fast_packed_q4: other names, other budgets)
            fast[name] = (field(k, "vgpr_count"), field(k, "agpr_count"), field(k, "vgpr_spill_count"),
                          field(k, "private_segment_fixed_size"))
    for name, v in sorted(fast.items()):
        print(name, "vgpr %d agpr %d spills %d scratch %d" % v)
    # dense / gathered x skip_hets x pad line x {128-row, long tiles}, segmented ones, and the four two-level ones
    two_level = [n for n in fast if re.search(r"Lb0ELb0ELi\d+ELb[01]ELb1EE", n)]
    assert len(two_level) == 4, sorted(fast)
    assert len(fast) >= 20, sorted(fast)
    bad = {n: v for n, v in fast.items() if v[0] + v[1] > VGPR_BUDGET or v[2] or v[3]}
    assert not bad, bad
