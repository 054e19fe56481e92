"""The host-only case program over libspm_amd/csrc/bam_pileup_core.hpp (tests/cpp/bam_pileup_core_cases.cpp), plain and as the
stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program: SEQ nibbles and quality bytes by dwords against by bytes at
every alignment, every CIGAR op in the worked table of spm_hip.h, what the serial builder refuses, the serial builder against a
host emulation of the device's tile scheme on a few thousand random small sorted record sets, and the sites of worked columns."""
import subprocess

import pytest

from cpp_programs import build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_bam_pileup_case_program(tmp_path, sanitize):
    exe = build_cases("bam_pileup_core_cases.cpp", tmp_path, sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 20000, r.stdout[-500:]
