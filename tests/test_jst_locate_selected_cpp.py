"""The C++ side of aligning the selected hits of a pan-genome search: the host-side plan (plan_jst_locate,
libspm_amd/csrc/select_plan.hpp) through tests/cpp/jst_locate_plan_cases -- plain asserts, no device, also under
AddressSanitizer + UndefinedBehaviorSanitizer -- and the mirror's journaled_sequence_tree::locate(..., hit_selection) through
tests/cpp/jst_locate_selected_cases on the VCF fixtures, compiled with the reference's warning flags and run on the GPU.  The
programs are compiled here, into the test's own directory."""
import re
import subprocess

import pytest

from cpp_programs import build_cases, build_mirror


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_locate_plan_cases(tmp_path, sanitize):
    exe = build_cases("jst_locate_plan_cases.cpp", tmp_path, std="c++17" if sanitize else "c++20", sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 4000, r.stdout


def _mirror_exe(out_dir):
    return build_mirror("jst_locate_selected_cases.cpp", out_dir)


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert _mirror_exe(tmp_path).exists()


@pytest.mark.gpu
def test_mirror_selected_locate_on_the_fixtures(spm, tmp_path):
    """device route == host route (locate_host filtered by select_host) == batch_matcher::locate with the same hit_selection
    on every fixture haplotype"""
    r = subprocess.run([str(_mirror_exe(tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 100, r.stdout[-2000:]
    kept = [(int(a), int(b)) for a, b in re.findall(r": (\d+) of (\d+) alignments", r.stdout)]
    assert len(kept) == 24 and sum(a < b for a, b in kept) >= 12
