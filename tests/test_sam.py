"""SAM lines and MAPQ, the part that needs no device: the case program over the rule (jst_sam_core.hpp), the layouts of the
three structs of spm_hip.h against ctypes and the numpy dtype, the Python signature, spm_hip_sam_header and spm_hip_sam_mapq."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from cpp_programs import ROOT, build_cases, c_layout

LINE = np.dtype([("offset", "<u8"), ("len", "<u4"), ("read", "<u4"), ("source", "<u4"), ("flag", "<u2"), ("mapq", "u1"), ("kind", "u1")])
OK, INVALID, OVERFLOW = 0, -1, -5


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_case_program(tmp_path, sanitize):
    exe = build_cases("jst_sam_core_cases.cpp", tmp_path, include=[os.path.join(ROOT, "include")], sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 3000, r.stdout[-500:]


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_sam_opts, f))
#define F(f) printf("line.%s %zu\n", #f, offsetof(spm_sam_line, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_sam_stats, f))
int main(void)
{
    O(rname); O(symbols); O(names); O(name_off); O(n_names); O(mapq_unique); O(mapq_multi); O(mapq_defaults); O(flags); O(reserved);
    F(offset); F(len); F(read); F(source); F(flag); F(mapq); F(kind);
    S(ms_total); S(ms_lines); S(ms_measure); S(ms_write); S(ms_stats); S(ms_host); S(n_lines); S(n_bytes); S(n_reported);
    S(n_secondary); S(n_unmapped); S(n_rescue_lines);
    printf("sizeof.opts %zu\nsizeof.line %zu\nsizeof.stats %zu\n", sizeof(spm_sam_opts), sizeof(spm_sam_line), sizeof(spm_sam_stats));
    printf("kind.values %d\n", SPM_SAM_UNMAPPED + 10 * SPM_SAM_LOCUS + 100 * SPM_SAM_RESCUE + 1000 * SPM_SAM_SECONDARY_LINE);
    printf("flag.values %u\n", SPM_SAM_CIGAR_M + 10 * SPM_SAM_SECONDARY);
    return 0;
}
"""
CALLS = ("spm_hip_jst_ref_loci_sam", "spm_hip_sam_view", "spm_hip_sam_device", "spm_hip_sam_stats", "spm_hip_sam_destroy",
         "spm_hip_sam_header", "spm_hip_sam_mapq")


def test_layouts_and_names(spm, tmp_path):
    capi = spm.capi
    assert ctypes.sizeof(capi.SamOpts) == 64 and ctypes.sizeof(capi.SamStats) == 72
    assert ctypes.sizeof(capi.SamLine) == 24 == spm.SAM_LINE_DTYPE.itemsize and spm.SAM_LINE_DTYPE == LINE
    assert np.dtype(capi.SamLine) == LINE
    want = c_layout(tmp_path, LAYOUT_C)
    assert (int(want.pop("sizeof.opts")), int(want.pop("sizeof.line")), int(want.pop("sizeof.stats"))) == (64, 24, 72)
    assert int(want.pop("kind.values")) == 3210
    assert (capi.SAM_UNMAPPED, capi.SAM_LOCUS, capi.SAM_RESCUE, capi.SAM_SECONDARY_LINE) == (0, 1, 2, 3)
    assert int(want.pop("flag.values")) == 21 == capi.SAM_CIGAR_M + 10 * capi.SAM_SECONDARY
    seen = {"opts": 0, "line": 0, "stats": 0}
    for name, off in want.items():
        kind, field = name.split(".")
        ctype = {"opts": capi.SamOpts, "line": capi.SamLine, "stats": capi.SamStats}[kind]
        assert getattr(ctype, field).offset == int(off), name
        if kind == "line":
            assert LINE.fields[field][1] == int(off) and LINE.fields[field][0].itemsize == getattr(ctype, field).size, name
        seen[kind] += 1
    assert seen == {"opts": len(capi.SamOpts._fields_), "line": len(capi.SamLine._fields_),
                    "stats": len(capi.SamStats._fields_)} == {"opts": 10, "line": 7, "stats": 12}
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    for f in (spm.JstRefLoci.sam, spm.Sam.text, spm.Sam.lines, spm.Sam.device, spm.Sam.stats, spm.Sam.header, spm.Sam.close):
        assert callable(f)
    sig = inspect.signature(spm.JstRefLoci.sam)
    assert list(sig.parameters)[1:] == ["reads", "patterns", "rname", "pairs", "rescues", "names", "symbols", "cigar_m", "secondary",
                                       "mapq_unique", "mapq_multi"]
    keyword_only = [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert keyword_only == ["pairs", "rescues", "names", "symbols", "cigar_m", "secondary", "mapq_unique", "mapq_multi"]
    assert (sig.parameters["symbols"].default, sig.parameters["cigar_m"].default, sig.parameters["secondary"].default) == ("ACGT", False, False)


def np_mapq(n_best, n_next, unique=(60, 40, 30, 20), multi=(3, 1, 1, 0)):
    """the policy of spm_hip.h, written again"""
    if n_best == 0:
        return 0
    return unique[min(n_next, 3)] if n_best == 1 else multi[min(n_best, 5) - 2]


def test_mapq_tables(spm):
    lib = spm.capi.lib()
    counts = (0, 1, 2, 3, 4, 5, 6, 7, 1000, 0xFFFFFFFE, 0xFFFFFFFF)
    # the defaults: multi is floor(-10 log10(1 - 1/n)) for n = 2, 3, 4, >= 5
    assert [int(np.floor(-10 * np.log10(1 - 1 / n) + 1e-9)) for n in (2, 3, 4, 5, 50)] == [3, 1, 1, 0, 0]
    defaults = spm.sam_opts("chr")
    assert defaults.mapq_defaults == 1
    for nb in counts:
        for nn in counts:
            assert lib.spm_hip_sam_mapq(ctypes.byref(defaults), nb, nn) == np_mapq(nb, nn) == spm.sam_mapq(nb, nn)
    assert [spm.sam_mapq(1, i) for i in range(5)] == [60, 40, 30, 20, 20] and [spm.sam_mapq(i, 9) for i in range(7)] == [0, 20, 3, 1, 1, 0, 0]
    # an overridden table, at every index; the marker decides, not the content
    unique, multi = (9, 8, 7, 6), (5, 4, 255, 2)
    own = spm.sam_opts("chr", mapq_unique=unique, mapq_multi=multi)
    assert own.mapq_defaults == 0 and list(own.mapq_unique) == list(unique) and list(own.mapq_multi) == list(multi)
    for nb in counts:
        for nn in counts:
            assert lib.spm_hip_sam_mapq(ctypes.byref(own), nb, nn) == np_mapq(nb, nn, unique, multi)
    own.mapq_defaults = 1
    assert lib.spm_hip_sam_mapq(ctypes.byref(own), 1, 0) == 60
    own.mapq_defaults = 2
    assert lib.spm_hip_sam_mapq(ctypes.byref(own), 1, 0) == -1 and lib.spm_hip_sam_mapq(None, 1, 0) == -1
    with pytest.raises(ValueError):
        spm.sam_opts("chr", mapq_unique=unique)


def test_header(spm):
    lib = spm.capi.lib()
    want = b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:chr1\tLN:12000\n"
    assert spm.sam_header("chr1", 12000) == want
    need = ctypes.c_uint64(0)
    buf = ctypes.create_string_buffer(b"#" * 64, 64)
    # cap too small: SPM_E_OVERFLOW, len reports the need, nothing is written
    for cap in (0, 1, len(want) - 1):
        need.value = 0
        assert lib.spm_hip_sam_header(b"chr1", 12000, buf, cap, ctypes.byref(need)) == OVERFLOW
        assert need.value == len(want) and buf.raw == b"#" * 64
    assert lib.spm_hip_sam_header(b"chr1", 12000, None, 0, ctypes.byref(need)) == OVERFLOW and need.value == len(want)
    assert lib.spm_hip_sam_header(b"chr1", 12000, buf, len(want), ctypes.byref(need)) == OK
    assert buf.raw[:len(want)] == want and buf.raw[len(want):] == b"#" * (64 - len(want))      # not NUL-terminated
    big = 2 ** 64 - 1
    assert spm.sam_header("a@b|c", big) == b"@HD\tVN:1.6\tSO:unknown\n@SQ\tSN:a@b|c\tLN:%d\n" % big
    assert spm.sam_header("x" * 254, 0).count(b"x") == 254
    # a bad rname, NULL arguments
    for bad in (b"", b"*", b"a b", b"a\tb", b"a\nb", b"\x7f", "ä".encode(), b"x" * 255):
        need.value = 7
        assert lib.spm_hip_sam_header(bad, 5, buf, 64, ctypes.byref(need)) == INVALID and need.value == 7
        with pytest.raises(spm.SpmError, match="-1"):
            spm.sam_header(bad, 5)
    assert lib.spm_hip_sam_header(None, 5, buf, 64, ctypes.byref(need)) == INVALID
    assert lib.spm_hip_sam_header(b"chr1", 5, buf, 64, None) == INVALID
    assert lib.spm_hip_sam_header(b"chr1", 5, None, 64, ctypes.byref(need)) == INVALID
    assert spm.sam_header("**", 1).endswith(b"SN:**\tLN:1\n")         # "*" alone is refused, not a name that holds one
