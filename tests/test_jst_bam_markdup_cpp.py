"""Duplicate marking through the C++ mirror: journaled_sequence_tree::map_bam with jst_bam_options::mark_duplicates by the device
route (spm_hip_bam_markdup behind the BAM call and the sort) returns the same file bytes, line records and index bytes as the
host route (spm_hip_bam_markdup_host over the host's own records), single-end and paired with rescues, in read order and
sorted, indexed and deflated; the flags of both equal the rule written again as an all-pairs comparison:
tests/cpp/jst_bam_markdup_cases.cpp."""
import re
import subprocess

import pytest

from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_bam_markdup_cases.cpp", tmp_path).exists()


@gpu
def test_map_bam_mark_duplicates_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_bam_markdup_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 4 * 9 + 1, r.stdout[-2000:]
    assert len(re.findall(r"mode \d, sorted \d: \d+ records, \d+ duplicates", r.stdout)) == 4
