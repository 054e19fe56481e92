"""CPU: the MD string and the base qualities as kinds of field of the SAM and BAM compositions, on the host
(tests/cpp/jst_sam_md_core_cases.cpp over libspm_amd/csrc/jst_sam_core.hpp and jst_bam_core.hpp): plain, and as a stand-alone
program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import os
import subprocess

import pytest

from cpp_programs import ROOT, build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_case_program(tmp_path, sanitize):
    exe = build_cases("jst_sam_md_core_cases.cpp", tmp_path, include=[os.path.join(ROOT, "include")], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 30000, r.stdout[-500:]
