"""The host-only case program over libspm_amd/csrc/bgzf_huffman_core.hpp (tests/cpp/bgzf_huffman_core_cases.cpp), plain and as
the stand-alone AddressSanitizer + UndefinedBehaviorSanitizer program; the files it writes with SPM_BGZF_DYNAMIC's rule are
taken apart here, block by block and header by header, by tests/deflate_dynamic.py and by gzip."""
import gzip
import subprocess

import pytest

import deflate_dynamic
from cpp_programs import build_cases


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_huffman_case_program(tmp_path, sanitize):
    exe = build_cases("bgzf_huffman_core_cases.cpp", tmp_path, sanitize=sanitize)
    out = tmp_path / "files"
    out.mkdir()
    r = subprocess.run([str(exe), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 400_000, r.stdout[-500:]
    files = sorted(out.glob("*.bgzf"))
    assert len(files) == 18
    types = set()
    for f in files:
        kind, D = f.name.split(".")[:2]
        raw, want = f.read_bytes(), f.with_suffix(".raw").read_bytes()
        blocks = deflate_dynamic.parse(raw, int(D))
        assert deflate_dynamic.payload_of(blocks) == want == gzip.decompress(raw), f.name
        types |= {(kind, D, blk[2]) for blk in blocks}
    assert {t for k, D, t in types if k == "random" and D != "64"} == {0}
    assert {t for k, D, t in types if k in ("uniform40", "skewed") and D != "64"} == {2}
    assert ("equal", "65280", 2) in types and ("records", "65280", 2) in types
    assert {0, 2} <= {t for k, _D, t in types if k == "mixed"} and {t for _k, _D, t in types} == {0, 1, 2}
