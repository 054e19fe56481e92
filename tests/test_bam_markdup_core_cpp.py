"""The host-only case program over libspm_amd/csrc/bam_markdup_core.hpp (tests/cpp/bam_markdup_core_cases.cpp), plain and as the
stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program: 5' ends, keys and scores at every byte alignment of a record,
the worked cases of spm_hip.h, and the serial builder against a brute-force all-pairs comparison and against the device's
two-sort scheme on a few thousand random small record sets."""
import subprocess

import pytest

from cpp_programs import build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_bam_markdup_case_program(tmp_path, sanitize):
    exe = build_cases("bam_markdup_core_cases.cpp", tmp_path, sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 40000, r.stdout[-500:]
