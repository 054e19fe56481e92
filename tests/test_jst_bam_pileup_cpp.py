"""The pileup through the C++ mirror: journaled_sequence_tree::map_bam with jst_bam_options::pileup by the device route
(spm_hip_bam_pileup behind the BAM call, the sort and the duplicate marks) returns the counts of the host route, of
spm_hip_bam_pileup_host over the mirror's own file and of the rule written again as a walk over the record bytes, single-end
and paired with rescues, marked and not: tests/cpp/jst_bam_pileup_cases.cpp."""
import re
import subprocess

import pytest

from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_bam_pileup_cases.cpp", tmp_path).exists()


@gpu
def test_map_bam_pileup_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_bam_pileup_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 4 * 9 + 1, r.stdout[-2000:]
    assert len(re.findall(r"mode \d, marked \d: \d+ records, \d+ take part, \d+ duplicates", r.stdout)) == 4
