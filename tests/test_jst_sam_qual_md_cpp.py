"""Base qualities and the MD tag through the C++ mirror: journaled_sequence_tree::map_sam and map_bam with
jst_sam_options::qualities and ::md return the same by the device route (spm_hip_jst_ref_loci_sam_ex / _bam_ex) and by the host
route (a plain formatter with an MD writer of its own, a plain SAM-to-BAM converter), tests/cpp/jst_sam_qual_md_cases.cpp."""
import re
import subprocess

import pytest

from cpp_programs import build_mirror
from test_gpu_sam_qual_md import decode_bam

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_sam_qual_md_cases.cpp", tmp_path).exists()


def test_host_converter_takes_qualities_and_a_z_tag(spm, tmp_path):
    """CPU: SAM lines with QUAL and MD:Z: written by hand -> bam_of_sam -> the decoder -> the same lines"""
    exe = build_mirror("bam_of_sam_qual_md_cases.cpp", tmp_path, fixtures=False)
    r = subprocess.run([str(exe), str(tmp_path / "out.bam"), str(tmp_path / "in.sam")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    raw, want = (tmp_path / "out.bam").read_bytes(), (tmp_path / "in.sam").read_bytes()
    text, stream, records, _blocks = decode_bam(raw)
    assert text == spm.sam_header("chr", 20000) and b"".join(line for _o, _n, line in records) == want
    assert stream.count(b"MDZ20G11\0") == 1 and stream.count(b"MDZ5A0C3^GT0A4\0") == 1 and stream.count(b"MDZ0\0") == 1
    assert bytes(range(32)) in stream and b"\x5d" * 5 + b"\x5c" * 5 + b"\x5b" * 5 in stream       # the values, not the characters


@gpu
def test_map_sam_and_map_bam_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_sam_qual_md_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 400, r.stdout[-2000:]
    assert len(re.findall(r"mode 1, fields 3: \d+ lines", r.stdout)) == 2
