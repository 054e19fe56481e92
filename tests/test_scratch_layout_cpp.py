"""The scratch layout of the sort-and-compact drivers (scratch_layout, libspm_amd/csrc/scratch_layout.hpp) through
tests/cpp/scratch_layout_cases -- plain asserts, no device, also under AddressSanitizer + UndefinedBehaviorSanitizer.  The
program is compiled here, into the test's own directory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _exe(out_dir, sanitize):
    exe = out_dir / ("scratch_layout_cases" + ("_asan" if sanitize else ""))
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-std=c++17", "-O2", "-pedantic"]
    subprocess.check_call(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe),
                                             os.path.join(CPP, "scratch_layout_cases.cpp")])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_scratch_layout_cases(tmp_path, sanitize):
    r = subprocess.run([str(_exe(tmp_path, sanitize))], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 200, r.stdout
