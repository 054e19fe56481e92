"""SAM lines through the C++ mirror: journaled_sequence_tree::map_sam by the device route (spm_hip_jst_ref_loci_sam) equals
the host route (a plain std::string formatter over the host structs), tests/cpp/jst_sam_cases.cpp."""
import re
import subprocess

import pytest

from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_sam_cases.cpp", tmp_path).exists()


@gpu
def test_map_sam_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_sam_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 300, r.stdout[-2000:]
    assert len(re.findall(r"mode 2: \d+ lines", r.stdout)) == 2
