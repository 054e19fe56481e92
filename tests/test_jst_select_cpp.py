"""The C++ side of pan-genome hit selection: the host-side plan (plan_jst_select, libspm_amd/csrc/select_plan.hpp) through
tests/cpp/jst_select_plan_cases -- plain asserts, no device, also under AddressSanitizer + UndefinedBehaviorSanitizer -- and
the mirror's journaled_sequence_tree::search(..., hit_selection) through tests/cpp/jst_select_cases on the VCF fixtures,
compiled with the reference's warning flags and run on the GPU.  The programs are compiled here, into the test's own
directory."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIB = os.path.join(ROOT, "libspm_amd")


def _plan_exe(out_dir, sanitize):
    exe = out_dir / ("jst_select_plan_cases" + ("_asan" if sanitize else ""))
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-std=c++20", "-O2", "-pedantic"]
    subprocess.check_call(["g++"] + flags + ["-Wall", "-Wextra", "-Werror", "-o", str(exe),
                                             os.path.join(CPP, "jst_select_plan_cases.cpp")])
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_select_plan_cases(tmp_path, sanitize):
    r = subprocess.run([str(_plan_exe(tmp_path, sanitize))], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 3000, r.stdout


def _mirror_exe(out_dir):
    exe = out_dir / "jst_select_cases"
    subprocess.check_call(["g++", "-std=c++20", "-O2", "-pedantic", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(ROOT, "include"),
                           '-DSPM_TEST_DATA="' + os.path.join(ROOT, "tests", "golden", "jst") + '"',
                           "-o", str(exe), os.path.join(CPP, "jst_select_cases.cpp"),
                           "-L" + LIB, "-l:libspm_hip.so", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib",
                           "-Wl,-rpath-link,/opt/rocm/lib", "-lz"])
    return exe


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
