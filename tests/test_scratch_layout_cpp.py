"""The scratch layout of the sort-and-compact drivers (scratch_layout, libspm_amd/csrc/scratch_layout.hpp) through
tests/cpp/scratch_layout_cases -- plain asserts, no device, also under AddressSanitizer + UndefinedBehaviorSanitizer.  The
program is compiled here, into the test's own directory."""
import re
import subprocess

import pytest

from cpp_programs import build_cases


def _exe(out_dir, sanitize):
    return build_cases("scratch_layout_cases.cpp", out_dir, std="c++17", sanitize=sanitize)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_scratch_layout_cases(tmp_path, sanitize):
    r = subprocess.run([str(_exe(tmp_path, sanitize))], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 200, r.stdout
