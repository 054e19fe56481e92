"""The C++ side of projecting pan-genome alignments onto the reference: the composition template of
libspm_amd/csrc/jst_project_core.hpp -- the code both kernels instantiate -- through tests/cpp/jst_project_core_cases: the
header alone, plain asserts, no device, as a stand-alone program, also under AddressSanitizer + UndefinedBehaviorSanitizer;
and the mirror's journaled_sequence_tree::locate_reference through tests/cpp/jst_project_cases on the VCF fixtures, compiled
with the reference's warning flags and run on the GPU.  The programs are compiled here, into the test's own directory."""
import re
import subprocess

import pytest

from cpp_programs import build_cases, build_mirror


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_jst_project_core_cases(tmp_path, sanitize):
    exe = build_cases("jst_project_core_cases.cpp", tmp_path, sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 4000, r.stdout
    kinds = re.search(r"inside an insertion (\d+), D words (\d+), changed (\d+), insertion behind deletion (\d+), alleles at "
                      r"the ends (\d+)", r.stdout)
    assert kinds and all(int(x) > 0 for x in kinds.groups()), r.stdout


def _mirror_exe(out_dir):
    return build_mirror("jst_project_cases.cpp", out_dir)


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert _mirror_exe(tmp_path).exists()


@pytest.mark.gpu
def test_mirror_locate_reference_on_the_fixtures(spm, tmp_path):
    """locate_reference through the device route == the host route, with and without a hit_selection, on the VCF fixtures;
    every alignment replays against the fixture reference; projected transcripts differ from the haplotype ones"""
    r = subprocess.run([str(_mirror_exe(tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 40, r.stdout[-2000:]
    changed = [int(x) for x in re.findall(r"(\d+) projected transcripts differ", r.stdout)]
    assert len(changed) == 6 and sum(c > 0 for c in changed) >= 1
