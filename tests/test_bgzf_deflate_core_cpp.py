"""The host-only case program over libspm_amd/csrc/bgzf_deflate_core.hpp (tests/cpp/bgzf_deflate_core_cases.cpp), plain and as
the stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program; the files it writes are inflated here, block by block, by
tests/bgzf_inflate.py and by gzip."""
import gzip
import subprocess

import pytest

import bgzf_inflate
from cpp_programs import build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_deflate_case_program(tmp_path, sanitize):
    exe = build_cases("bgzf_deflate_core_cases.cpp", tmp_path, sanitize=sanitize)
    out = tmp_path / "files"
    out.mkdir()
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 35000, r.stdout[-500:]
    files = sorted(out.glob("*.bgzf"))
    assert len(files) == 18
    types = set()
    for f in files:
        kind, D = f.name.split(".")[:2]
        raw, want = f.read_bytes(), f.with_suffix(".raw").read_bytes()
        blocks = bgzf_inflate.parse(raw, int(D))
        assert bgzf_inflate.payload_of(blocks) == want == gzip.decompress(raw), f.name
        types |= {(kind, t) for _o, _p, t in blocks}
    assert ("random", 0) in types and ("equal", 1) in types and ("records", 1) in types
    assert {t for k, t in types if k == "mixed"} == {0, 1}
