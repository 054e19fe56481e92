"""CPU: the scan driver's host-side decisions (libspm_amd/csrc/scan_plan.hpp) -- tile tables and the span-local fallback's
ranges on generated inputs, the retry policy row by row, the clean predicate against the device kernel's status
expression, the filter's buffer layout -- through tests/cpp/scan_plan_cases (plain asserts; includes that header only)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_scan_plan_cases():
    subprocess.check_call(["make", "-C", CPP, "-s", "scan_plan_cases"])
    r = subprocess.run([os.path.join(CPP, "scan_plan_cases")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 10000, r.stdout
