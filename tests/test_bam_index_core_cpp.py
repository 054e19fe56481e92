"""The host-only case program over libspm_amd/csrc/bam_index_core.hpp (tests/cpp/bam_index_core_cases.cpp), plain and as the
stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program: reading a record, its end, the order, virtual offsets, the
worked BAI cases of spm_hip.h and the serial builder at every bin-level border."""
import subprocess

import pytest

from cpp_programs import build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_bam_index_case_program(tmp_path, sanitize):
    exe = build_cases("bam_index_core_cases.cpp", tmp_path, sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 40000, r.stdout[-500:]
