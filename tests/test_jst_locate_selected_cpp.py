"""The C++ side of aligning the selected hits of a pan-genome search: the host-side plan (plan_jst_locate,
libspm_amd/csrc/select_plan.hpp) through tests/cpp/jst_locate_plan_cases -- plain asserts, no device, also under
AddressSanitizer + UndefinedBehaviorSanitizer -- and the mirror's journaled_sequence_tree::locate(..., hit_selection) through
tests/cpp/jst_locate_selected_cases on the VCF fixtures, compiled with the reference's warning flags and run on the GPU.  The
programs are compiled here, into the test's own directory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "libspm_amd")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_locate_plan_cases(tmp_path, sanitize):
    exe = tmp_path / ("jst_locate_plan_cases" + ("_asan" if sanitize else ""))
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-std=c++20", "-O2", "-pedantic"]
    subprocess.check_call(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe),
                                             os.path.join(CPP, "jst_locate_plan_cases.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 4000, r.stdout


def _mirror_exe(out_dir):
    exe = out_dir / "jst_locate_selected_cases"
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pedantic", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "include"),
                           '-DSPM_TEST_DATA="' + os.path.join(ROOT, "tests", "golden", "jst") + '"',
                           "-o", str(exe), os.path.join(CPP, "jst_locate_selected_cases.cpp"),
                           "-L" + LIB, "-l:libspm_hip.so", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-lz"])
    return exe


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
