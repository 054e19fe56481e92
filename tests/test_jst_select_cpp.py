"""The C++ side of pan-genome hit selection: the host-side plan (plan_jst_select, libspm_amd/csrc/select_plan.hpp) through
tests/cpp/jst_select_plan_cases -- plain asserts, no device, also under AddressSanitizer + UndefinedBehaviorSanitizer -- and
the mirror's journaled_sequence_tree::search(..., hit_selection) through tests/cpp/jst_select_cases on the VCF fixtures,
compiled with the reference's warning flags and run on the GPU.  The programs are compiled here, into the test's own
directory."""
import re
import subprocess

import pytest

from cpp_programs import build_cases, build_mirror


def _plan_exe(out_dir, sanitize):
    return build_cases("jst_select_plan_cases.cpp", out_dir, std="c++17" if sanitize else "c++20", sanitize=sanitize)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_select_plan_cases(tmp_path, sanitize):
    r = subprocess.run([str(_plan_exe(tmp_path, sanitize))], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 3000, r.stdout


def _mirror_exe(out_dir):
    return build_mirror("jst_select_cases.cpp", out_dir)


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert _mirror_exe(tmp_path).exists()


@pytest.mark.gpu
def test_mirror_selected_search_on_the_fixtures(spm, tmp_path):
    """device route == host route (search_host + the rule in C++) == batch_matcher with the same hit_selection on every
    fixture haplotype"""
    r = subprocess.run([str(_mirror_exe(tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 100, r.stdout[-2000:]
    kept = [(int(a), int(b)) for a, b in re.findall(r": (\d+) of (\d+) hits", r.stdout)]
    assert len(kept) == 36 and sum(a < b for a, b in kept) >= 20
