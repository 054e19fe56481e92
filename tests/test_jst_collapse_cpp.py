"""The C++ side of collapsing projected pan-genome alignments: the order and equality rule of
libspm_amd/csrc/jst_collapse_core.hpp -- the code the walk kernels instantiate -- through tests/cpp/jst_collapse_core_cases:
the header alone, no device, as a stand-alone program, also under AddressSanitizer + UndefinedBehaviorSanitizer; and the
mirror's journaled_sequence_tree::locate_reference_loci through tests/cpp/jst_collapse_cases on the VCF fixtures, compiled with
the reference's warning flags and run on the GPU.  The programs are compiled here, into the test's own directory."""
import re
import subprocess

import pytest

from cpp_programs import LIB, build_cases, build_mirror


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_collapse_core_cases(tmp_path, sanitize):
    exe = build_cases("jst_collapse_core_cases.cpp", tmp_path, include=[LIB + "/csrc"], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 4000, r.stdout


def _mirror_exe(out_dir):
    return build_mirror("jst_collapse_cases.cpp", out_dir)


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert _mirror_exe(tmp_path).exists()


@pytest.mark.gpu
def test_mirror_locate_reference_loci_on_the_fixtures(spm, tmp_path):
    """locate_reference_loci through the device route == the host route, with and without a hit_selection, on the VCF
    fixtures; every locus replays against the fixture reference and covers the alignments of locate_reference"""
    r = subprocess.run([str(_mirror_exe(tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 60, r.stdout[-2000:]
    merged = [int(x) for x in re.findall(r"(\d+) of them on several haplotypes", r.stdout)]
    assert len(merged) == 6 and all(c > 0 for c in merged)
