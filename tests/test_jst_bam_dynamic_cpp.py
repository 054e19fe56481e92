"""A BAM file with dynamic-Huffman blocks through the C++ mirror: journaled_sequence_tree::map_bam with jst_bam_options::deflate
and ::dynamic by the device route (spm_hip_bam_deflate with SPM_BGZF_DYNAMIC) returns the same file bytes and block offsets as the
host route (spm_hip_bgzf_deflate_host with the flag over its own header and records), and virtual_offset reaches every record:
tests/cpp/jst_bam_dynamic_cases.cpp."""
import re
import subprocess

import pytest

from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_bam_dynamic_cases.cpp", tmp_path).exists()


@gpu
def test_map_bam_dynamic_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_bam_dynamic_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 45, r.stdout[-2000:]
    assert len(re.findall(r"block_data \d+, mode \d: \d+ records", r.stdout)) == 4
