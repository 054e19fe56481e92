"""Variant calls through the C++ mirror: journaled_sequence_tree::map_bam with jst_bam_options::call_variants by the device
route (spm_hip_pileup_sites and spm_hip_pileup_sites_vcf behind the pileup) returns the text and the call records of the host
route and of the host twins over the mirror's own pileup, single-end and paired with rescues, marked and not; call_variants
without pileup ends the program: tests/cpp/jst_bam_vcf_cases.cpp."""
import re
import signal
import subprocess

import pytest

from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_call_variants_without_pileup_is_fatal(spm, tmp_path):
    """Asked of the host route's converter (bam_of_sam), which opens no device: the refusal is the same line in map_bam,
    map_bam_device and there."""
    exe = build_mirror("jst_bam_vcf_cases.cpp", tmp_path)
    r = subprocess.run([str(exe), "fatal"], capture_output=True, text=True, timeout=60)
    assert r.returncode == -signal.SIGABRT and "call_variants without pileup" in r.stderr and "was taken" not in r.stdout, (r.returncode, r.stderr[-500:])


@gpu
def test_map_bam_call_variants_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_bam_vcf_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 4 * 11 + 1, r.stdout[-2000:]
    assert len(re.findall(r"mode \d, marked \d: \d+ records, \d+ sites, \d+ lines, \d+ bytes", r.stdout)) == 4
