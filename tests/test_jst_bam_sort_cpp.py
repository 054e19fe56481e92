"""A coordinate-sorted BAM file and its BAI index through the C++ mirror: journaled_sequence_tree::map_bam with
jst_bam_options::sort and ::index by the device route (spm_hip_bam_sort, spm_hip_bam_index) returns the same file bytes, line
records and index bytes as the host route (std::stable_sort under the rule written again, spm_hip_bai_build_host), stored and
deflated, at two block sizes: tests/cpp/jst_bam_sort_cases.cpp."""
import re
import subprocess

import pytest

from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_bam_sort_cases.cpp", tmp_path).exists()


@gpu
def test_map_bam_sort_and_index_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_bam_sort_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 8 * 13 + 1, r.stdout[-2000:]
    assert len(re.findall(r"block_data \d+, mode \d, deflate \d: \d+ records", r.stdout)) == 8
