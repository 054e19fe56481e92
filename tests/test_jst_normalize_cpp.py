"""The C++ side of left-normalising projected pan-genome alignments: the rule of libspm_amd/csrc/jst_normalize_core.hpp -- the
code the normalise kernel instantiates -- through tests/cpp/jst_normalize_core_cases: the header alone, no device, as a
stand-alone program, also under AddressSanitizer + UndefinedBehaviorSanitizer; and the mirror's
journaled_sequence_tree::locate_reference_normalized / locate_reference_loci_normalized through tests/cpp/jst_normalize_cases on
the VCF fixtures, compiled with the reference's warning flags and run on the GPU.  The programs are compiled here, into the
test's own directory."""
import re
import subprocess

import pytest

from cpp_programs import LIB, build_cases, build_mirror


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_normalize_core_cases(tmp_path, sanitize):
    exe = build_cases("jst_normalize_core_cases.cpp", tmp_path, include=[LIB + "/csrc"], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 100_000, r.stdout
    m = re.search(r"stepped (\d+), grew (\d+), shrank (\d+), joined (\d+), pinned (\d+)", r.stdout)
    assert m and all(int(x) > 0 for x in m.groups()), r.stdout


def _mirror_exe(out_dir):
    return build_mirror("jst_normalize_cases.cpp", out_dir)


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert _mirror_exe(tmp_path).exists()


@pytest.mark.gpu
def test_mirror_locate_reference_normalized_on_the_fixtures(spm, tmp_path):
    """locate_reference_normalized and locate_reference_loci_normalized through the device route == the host route, with and
    without a hit_selection, on the VCF fixtures; every alignment replays against the fixture reference; the fixtures show
    transcripts that normalisation changes and loci that it merges"""
    r = subprocess.run([str(_mirror_exe(tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 80, r.stdout[-2000:]
    shown = [(int(a), int(b)) for a, b in re.findall(r"fixture: (\d+) transcripts changed, (\d+) loci merged", r.stdout)]
    assert len(shown) == 2 and any(c > 0 for c, _m in shown) and any(m > 0 for _c, m in shown), shown
