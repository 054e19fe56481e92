"""The host-only case program over libspm_amd/csrc/pileup_vcf_core.hpp (tests/cpp/pileup_vcf_core_cases.cpp), plain and as the
stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program: the default cost literals against their formula, the decimal
writer at its edges, the worked table of spm_hip.h, where a run of lines splits into head bytes, dwords and tail bytes, and the
serial text builder against a host emulation of the device's write scheme on random site sets, at every alignment of the text
and with site counts around the group size."""
import subprocess

import pytest

from cpp_programs import build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_pileup_vcf_case_program(tmp_path, sanitize):
    exe = build_cases("pileup_vcf_core_cases.cpp", tmp_path, sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 5000, r.stdout[-500:]
