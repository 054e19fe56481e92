"""BAM records and BGZF framing, the part that needs no device: the case programs over the container's core (bgzf_core.hpp)
and the composition of a record (jst_bam_core.hpp), the layouts of the structs of spm_hip.h against ctypes, the host framer's
output parsed block by block and through gzip, the header section decoded, and every refusal of the host-only calls."""
import ctypes
import gzip
import inspect
import os
import subprocess

import numpy as np
import pytest

from bam_decode import EOF_BLOCK, bam_to_sam, parse_bam_header, parse_bgzf, payload_of, reg2bin
from cpp_programs import ROOT, build_cases, c_layout

OK, INVALID, UNSUPPORTED, OVERFLOW = 0, -1, -4, -5


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_bgzf_case_program(tmp_path, sanitize):
    exe = build_cases("bgzf_core_cases.cpp", tmp_path, sanitize=sanitize)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    tail = r.stdout.strip().splitlines()[-1].split()
    assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 30000, r.stdout[-500:]


def test_bam_case_program(tmp_path):
    for sanitize in (False, True):
        exe = build_cases("jst_bam_core_cases.cpp", tmp_path, include=[os.path.join(ROOT, "include")], sanitize=sanitize)
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        tail = r.stdout.strip().splitlines()[-1].split()
        assert tail[1:] == ["checks,", "0", "failures"] and int(tail[0]) >= 550, r.stdout[-500:]


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_bgzf_opts, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_bgzf_stats, f))
#define BO(f) printf("bamopts.%s %zu\n", #f, offsetof(spm_bam_opts, f))
#define BS(f) printf("bamstats.%s %zu\n", #f, offsetof(spm_bam_stats, f))
int main(void)
{
    O(block_data); O(flags); O(reserved);
    S(ms_frame); S(ms_host); S(n_in); S(n_out); S(n_blocks);
    BO(sam); BO(ref_len); BO(block_data); BO(reserved);
    BS(ms_total); BS(ms_lines); BS(ms_measure); BS(ms_write); BS(ms_frame); BS(ms_stats); BS(ms_host); BS(reserved); BS(n_records);
    BS(n_record_bytes); BS(n_file_bytes); BS(header_file_bytes); BS(n_record_blocks); BS(n_reported); BS(n_secondary); BS(n_unmapped);
    BS(n_rescue_lines);
    printf("sizeof.bamopts %zu\nsizeof.bamstats %zu\n", sizeof(spm_bam_opts), sizeof(spm_bam_stats));
    printf("sizeof.opts %zu\nsizeof.stats %zu\n", sizeof(spm_bgzf_opts), sizeof(spm_bgzf_stats));
    printf("flag.values %u\n", SPM_BGZF_EOF + 10 * SPM_BGZF_BLOCK_DATA);
    return 0;
}
"""
CALLS = ("spm_hip_bgzf_frame", "spm_hip_bgzf_view", "spm_hip_bgzf_device", "spm_hip_bgzf_stats", "spm_hip_bgzf_destroy",
         "spm_hip_bgzf_frame_host", "spm_hip_bgzf_framed_size", "spm_hip_jst_ref_loci_bam", "spm_hip_bam_view", "spm_hip_bam_device",
         "spm_hip_bam_stats", "spm_hip_bam_destroy", "spm_hip_bam_header")


def test_layouts_and_names(spm, tmp_path):
    capi = spm.capi
    assert ctypes.sizeof(capi.BgzfOpts) == 16 and ctypes.sizeof(capi.BgzfStats) == 32
    assert ctypes.sizeof(capi.BamOpts) == 80 and ctypes.sizeof(capi.BamStats) == 104
    want = c_layout(tmp_path, LAYOUT_C)
    assert (int(want.pop("sizeof.opts")), int(want.pop("sizeof.stats"))) == (16, 32)
    assert (int(want.pop("sizeof.bamopts")), int(want.pop("sizeof.bamstats"))) == (80, 104)
    assert int(want.pop("flag.values")) == 652801 == capi.BGZF_EOF + 10 * capi.BGZF_BLOCK_DATA
    types = {"opts": capi.BgzfOpts, "stats": capi.BgzfStats, "bamopts": capi.BamOpts, "bamstats": capi.BamStats}
    seen = dict.fromkeys(types, 0)
    for name, off in want.items():
        kind, field = name.split(".")
        assert getattr(types[kind], field).offset == int(off), name
        seen[kind] += 1
    assert seen == {k: len(t._fields_) for k, t in types.items()} == {"opts": 3, "stats": 5, "bamopts": 4, "bamstats": 17}
    for name in CALLS:
        assert name in capi.EXPORTS and hasattr(capi.lib(), name)
    for f in (spm.JstRefLoci.bam, spm.Bam.bytes, spm.Bam.records, spm.Bam.lines, spm.Bam.voffsets, spm.Bam.device, spm.Bam.stats,
              spm.Bam.close, spm.bam_header, spm.Context.bgzf, spm.Sam.bgzf, spm.Bgzf.bytes, spm.Bgzf.device, spm.Bgzf.stats, spm.Bgzf.close, spm.bgzf_frame_host):
        assert callable(f)
    sig = inspect.signature(spm.Context.bgzf)
    assert list(sig.parameters)[1:] == ["device_ptr", "n", "block_data", "eof"]
    assert (sig.parameters["block_data"].default, sig.parameters["eof"].default) == (0, True)
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == ["block_data", "eof"]
    sig = inspect.signature(spm.JstRefLoci.bam)
    assert list(sig.parameters)[1:] == ["reads", "patterns", "rname", "ref_len", "pairs", "rescues", "names", "symbols", "cigar_m",
                                       "secondary", "mapq_unique", "mapq_multi", "block_data"]
    assert [n for n, p in sig.parameters.items() if p.kind is inspect.Parameter.KEYWORD_ONLY] == list(sig.parameters)[5:]
    assert sig.parameters["block_data"].default == 0
    sig = inspect.signature(spm.Sam.bgzf)
    assert list(sig.parameters)[1:] == ["ref_len", "block_data", "eof"] and sig.parameters["ref_len"].default is None


def _bytes(n, seed=77):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("D", [1, 7, 65280])
def test_host_framer_block_by_block(spm, D):
    for n in (0, 1, D, D + 1):
        data = _bytes(n, seed=D + n)
        for eof in (False, True):
            raw = spm.bgzf_frame_host(data, D, eof)
            n_blocks = (n + D - 1) // D
            assert len(raw) == n + 31 * n_blocks + (28 if eof else 0)
            blocks = parse_bgzf(raw, D, eof)                       # every header byte, BSIZE, LEN, NLEN, CRC32, ISIZE
            assert len(blocks) == n_blocks and payload_of(blocks) == data
            assert [o for o, _p in blocks] == [b * (D + 31) for b in range(n_blocks)]
            assert [len(p) for _o, p in blocks] == [min(D, n - b * D) for b in range(n_blocks)]
            if raw:
                assert gzip.decompress(raw) == data                # (verifies CRC and ISIZE of every member itself)
            else:
                assert n == 0 and not eof
            if n == 0 and eof:
                assert raw == EOF_BLOCK
            # the default block size is 65280, given as 0
            if D == 65280:
                assert spm.bgzf_frame_host(data, 0, eof) == raw == spm.bgzf_frame_host(data, block_data=65280, eof=eof)
    assert spm.bgzf_frame_host(b"abcdef", 4) == bytes.fromhex(
        "1f8b08040000000000ff0600424302002200" "01" "0400" "fbff" "61626364" "11cd82ed" "04000000"
        "1f8b08040000000000ff0600424302002000" "01" "0200" "fdff" "6566" "704982fd" "02000000") + EOF_BLOCK


def test_host_calls_and_their_refusals(spm):
    lib, capi = spm.capi.lib(), spm.capi
    err = lambda: lib.spm_hip_last_error(None)
    need = ctypes.c_uint64(0)
    opts = spm.bgzf_opts(4, True)
    src = ctypes.create_string_buffer(b"abcdef", 6)
    want = spm.bgzf_frame_host(b"abcdef", 4)
    assert lib.spm_hip_bgzf_framed_size(6, ctypes.byref(opts), ctypes.byref(need)) == OK and need.value == 96 == len(want)
    assert lib.spm_hip_bgzf_framed_size(0, ctypes.byref(spm.bgzf_opts(0, False)), ctypes.byref(need)) == OK and need.value == 0
    assert lib.spm_hip_bgzf_framed_size(200000, ctypes.byref(spm.bgzf_opts(0, True)), ctypes.byref(need)) == OK
    assert need.value == 200000 + 4 * 31 + 28
    # cap too small: SPM_E_OVERFLOW, len reports the need, nothing is written
    buf = ctypes.create_string_buffer(b"#" * 128, 128)
    for cap in (0, 1, 95):
        need.value = 0
        assert lib.spm_hip_bgzf_frame_host(src, 6, ctypes.byref(opts), buf, cap, ctypes.byref(need)) == OVERFLOW
        assert need.value == 96 and buf.raw == b"#" * 128
    assert lib.spm_hip_bgzf_frame_host(src, 6, ctypes.byref(opts), None, 0, ctypes.byref(need)) == OVERFLOW and need.value == 96
    assert lib.spm_hip_bgzf_frame_host(src, 6, ctypes.byref(opts), buf, 96, ctypes.byref(need)) == OK
    assert buf.raw[:96] == want and buf.raw[96:] == b"#" * 32
    assert lib.spm_hip_bgzf_frame_host(None, 0, ctypes.byref(opts), buf, 128, ctypes.byref(need)) == OK and need.value == 28

    def refused(word, rc, code=INVALID):
        assert rc == code and word in err(), (rc, err())

    for word, o in ((b"block_data", capi.BgzfOpts(65281, 1, 0)), (b"block_data", capi.BgzfOpts(0xFFFFFFFF, 0, 0)),
                    (b"flag", capi.BgzfOpts(0, 2, 0)), (b"flag", capi.BgzfOpts(0, 0x80000001, 0)), (b"reserved", capi.BgzfOpts(0, 1, 1))):
        need.value = 7
        refused(word, lib.spm_hip_bgzf_framed_size(6, ctypes.byref(o), ctypes.byref(need)))
        refused(word, lib.spm_hip_bgzf_frame_host(src, 6, ctypes.byref(o), buf, 128, ctypes.byref(need)))
        assert need.value == 7
    refused(b"NULL opts", lib.spm_hip_bgzf_framed_size(6, None, ctypes.byref(need)))
    refused(b"NULL len", lib.spm_hip_bgzf_framed_size(6, ctypes.byref(opts), None))
    refused(b"NULL opts", lib.spm_hip_bgzf_frame_host(src, 6, None, buf, 128, ctypes.byref(need)))
    refused(b"NULL len", lib.spm_hip_bgzf_frame_host(src, 6, ctypes.byref(opts), buf, 128, None))
    refused(b"NULL src", lib.spm_hip_bgzf_frame_host(None, 6, ctypes.byref(opts), buf, 128, ctypes.byref(need)))
    refused(b"NULL dst", lib.spm_hip_bgzf_frame_host(src, 6, ctypes.byref(opts), None, 128, ctypes.byref(need)))
    refused(b"64 bits", lib.spm_hip_bgzf_framed_size(2 ** 64 - 1, ctypes.byref(opts), ctypes.byref(need)), UNSUPPORTED)
    with pytest.raises(spm.SpmError, match="-1.*block_data"):
        spm.bgzf_frame_host(b"abc", 65281)
    # the device call, without a device: its host-side refusals come first
    out = ctypes.c_void_p(1)
    assert lib.spm_hip_bgzf_frame(None, None, 0, ctypes.byref(opts), ctypes.byref(out)) == INVALID and b"NULL ctx" in err()
    assert lib.spm_hip_bgzf_view(None, None, None) == INVALID and lib.spm_hip_bgzf_device(None, None, None) == INVALID
    assert lib.spm_hip_bgzf_stats(None, None) == INVALID
    lib.spm_hip_bgzf_destroy(None)


def test_bam_header(spm):
    lib = spm.capi.lib()
    err = lambda: lib.spm_hip_last_error(None)
    for rname, ref_len in (("chr1", 12000), ("a@b|c", 2 ** 31 - 1), ("x" * 254, 1)):
        text = spm.sam_header(rname, ref_len)
        plain = b"BAM\x01" + len(text).to_bytes(4, "little") + text + (1).to_bytes(4, "little") + \
            (len(rname) + 1).to_bytes(4, "little") + rname.encode() + b"\0" + ref_len.to_bytes(4, "little")
        for D in (0, 1, 7, 64, 65280):
            raw = spm.bam_header(rname, ref_len, D)
            blocks = parse_bgzf(raw, D or 65280, eof=False)         # blocks of its own, no EOF block
            assert payload_of(blocks) == plain == gzip.decompress(raw)
            assert raw == spm.bgzf_frame_host(plain, D, eof=False)
            got_text, refs, first = parse_bam_header(plain)
            assert got_text == text and refs == [(rname, ref_len)] and first == len(plain)
            sam, stream, records, _b = bam_to_sam(raw + EOF_BLOCK, D or 65280)   # header plus EOF: a valid empty BAM
            assert sam == text and stream == b"" and records == []
    need = ctypes.c_uint64(0)
    buf = ctypes.create_string_buffer(b"#" * 256, 256)
    want = spm.bam_header("chr1", 12000)
    for cap in (0, 1, len(want) - 1):                               # cap too small: SPM_E_OVERFLOW, nothing is written
        assert lib.spm_hip_bam_header(b"chr1", 12000, 0, buf, cap, ctypes.byref(need)) == OVERFLOW
        assert need.value == len(want) and buf.raw == b"#" * 256
    assert lib.spm_hip_bam_header(b"chr1", 12000, 0, buf, 256, ctypes.byref(need)) == OK and buf.raw[:len(want)] == want
    for word, code, args in ((b"ref_len is 0", INVALID, (b"chr1", 0, 0)), (b"2^31 - 1", UNSUPPORTED, (b"chr1", 2 ** 31, 0)),
                             (b"block_data", INVALID, (b"chr1", 5, 65281)), (b"rname", INVALID, (b"*", 5, 0)),
                             (b"rname", INVALID, (b"a b", 5, 0)), (b"NULL rname", INVALID, (None, 5, 0))):
        need.value = 7
        assert lib.spm_hip_bam_header(*args, buf, 256, ctypes.byref(need)) == code and word in err() and need.value == 7, (args, err())
    assert lib.spm_hip_bam_header(b"chr1", 5, 0, buf, 256, None) == INVALID and lib.spm_hip_bam_header(b"chr1", 5, 0, None, 256, ctypes.byref(need)) == INVALID
    with pytest.raises(spm.SpmError, match="-4"):
        spm.bam_header("chr1", 2 ** 31)
    # the device call's refusals that need no device
    assert lib.spm_hip_jst_ref_loci_bam(None, None, None, None, None, None, ctypes.byref(ctypes.c_void_p())) == INVALID
    assert lib.spm_hip_bam_view(None, None, None, None, None, None, None) == INVALID and lib.spm_hip_bam_stats(None, None) == INVALID
    lib.spm_hip_bam_destroy(None)


def test_decoder_bins_follow_the_specification():
    assert [reg2bin(*x) for x in ((-1, 0), (0, 1), (0, 16384), (0, 16385), (16383, 16385), (2 ** 23 - 1, 2 ** 23 + 1),
                                  (2 ** 26 - 1, 2 ** 26 + 1), (2 ** 29 - 1, 2 ** 29 + 1))] == [4680, 4681, 4681, 585, 585, 1, 0, 0]
