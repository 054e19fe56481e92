"""A BAM file through the C++ mirror: journaled_sequence_tree::map_bam by the device route (spm_hip_jst_ref_loci_bam) returns the
same file bytes as the host route (a plain SAM-to-BAM converter over the host route's SAM lines, framed by
spm_hip_bgzf_frame_host), tests/cpp/jst_bam_cases.cpp."""
import re
import struct
import subprocess

import pytest

from bam_decode import at_voffset, bam_to_sam
from cpp_programs import build_mirror

gpu = pytest.mark.gpu


def test_mirror_program_compiles_with_reference_flags(spm, tmp_path):
    assert build_mirror("jst_bam_cases.cpp", tmp_path).exists()


@pytest.mark.parametrize("block_data", [0, 7, 64])
def test_host_converter_against_the_decoder(spm, tmp_path, block_data):
    """CPU: SAM lines written by hand -> bam_of_sam -> the decoder of tests/bam_decode.py -> the same lines"""
    exe = build_mirror("bam_of_sam_cases.cpp", tmp_path, fixtures=False)
    r = subprocess.run([str(exe), str(tmp_path / "out.bam"), str(tmp_path / "in.sam"), str(block_data)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    raw, want = (tmp_path / "out.bam").read_bytes(), (tmp_path / "in.sam").read_bytes()
    text, stream, records, blocks = bam_to_sam(raw, block_data or 65280)
    assert text == spm.sam_header("chr", 20000) + want
    assert raw.startswith(spm.bam_header("chr", 20000, block_data))
    voffsets = [int(x) for x in r.stdout.split()]
    assert len(voffsets) == len(records) == 8
    for v, (_o, n, _l) in zip(voffsets, records):
        assert struct.unpack("<i", at_voffset(blocks, v, 4))[0] == n - 4


@gpu
def test_map_bam_routes_agree(spm, tmp_path):
    r = subprocess.run([str(build_mirror("jst_bam_cases.cpp", tmp_path))], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 400, r.stdout[-2000:]
    assert len(re.findall(r"mode 2: \d+ records", r.stdout)) == 2
