"""GPU: genotype calls for pileup sites and the VCF text (spm_hip_pileup_sites_vcf, spm_hip_pileup_sites_vcf_records), byte for
byte against the serial host twins and the rule written again in tests/vcf_rule.py: site counts around the write stage's group
size as its stats report it, the first line at every alignment, the shortest line beside the longest, sets without a line and
with nothing but lines, saturating counts; the refusals counted on the device; and the chain behind sort, markdup, pileup and
sites on the mapped set with planted substitutions, its text deflated and inflated again."""
import ctypes

import numpy as np
import pytest

import bgzf_inflate
import vcf_rule
from cpp_programs import download
from test_gpu_bai import _Device
from test_gpu_markdup import RNAME, _single_reads
from test_pairs import _free_stretches
from test_rescue import _chain_of
from vcf_rule import make_sites

gpu = pytest.mark.gpu
INVALID, UNSUPPORTED = -1, -4
U32 = (1 << 32) - 1
_group = {}


def _raw(spm, ctx, rows, rname="chr1", sample="S", ref_len=None, **opts):
    """Context.pileup_sites_vcf over uploaded site records == the host twins == the Python rule -> (text, calls, stats)"""
    ref_len = ref_len if ref_len is not None else (max(r[0] for r in rows) + 1 if rows else 0)
    sites = make_sites(spm.PILEUP_SITE_DTYPE, rows)
    dev = _Device(sites.tobytes())
    try:
        v = ctx.pileup_sites_vcf(dev.ptr.value if rows else 0, len(rows), rname, sample, ref_len, **opts)
        text, calls, st = v.text(), v.calls(), v.stats()
        d_text, n_bytes, d_calls, n_calls = v.device()
        assert (n_bytes, n_calls) == (len(text), len(rows)) and len(v) == len(rows)
        assert download(ctx, d_text, n_bytes, np.uint8).tobytes() == text
        assert download(ctx, d_calls, n_calls, spm.VARIANT_CALL_DTYPE).tobytes() == calls.tobytes()
        v.close()
    finally:
        ctx.synchronize()
        dev.close()
    host = spm.pileup_sites_vcf_host(sites, rname, sample, ref_len, **opts)
    assert text == host, next(((i, a, b) for i, (a, b) in enumerate(zip(text.split(b"\n"), host.split(b"\n"))) if a != b), (len(text), len(host)))
    assert text == vcf_rule.text(rows, rname, sample, ref_len, **opts)
    # the call records: the host twin's but for offset and len, which name the site's line in the text
    want = spm.pileup_sites_calls_host(sites, **opts)
    head = len(spm.vcf_header(rname, sample, ref_len))
    at = head
    for c, row in zip(calls, rows):
        line = vcf_rule.line(row, rname, **opts)
        assert (int(c["offset"]), int(c["len"])) == (at, len(line)) and text[at:at + len(line)] == line
        at += len(line)
    assert at == len(text)
    got = calls.copy()
    got["offset"], got["len"] = 0, 0
    assert got.tobytes() == want.tobytes()
    status = calls["status"].tolist()
    low = sum(1 for c in calls if c["status"] == 1 and c["qual"] < vcf_rule.resolve(**opts)["min_qual"])
    assert (st.n_sites, st.n_variant, st.n_ref, st.n_ref_n, st.n_low_qual) == (len(rows), status.count(1), status.count(0), status.count(2), low)
    assert (st.n_header_bytes, st.n_text_bytes) == (head, len(text)) and st.group_sites >= 1 and st.ms_host > 0 and st.ms_total >= 0
    return text, calls, st


def _group_sites(spm, ctx):
    if not _group:
        _group["G"] = int(_raw(spm, ctx, [(3, 3, 0, (0, 0, 3, 0), 0)])[2].group_sites)
    return _group["G"]


def _rows(rng, n, kind="mixed", top=6, step=40):
    pos = np.cumsum(rng.integers(1, step, n)) if n else []
    rows = []
    for p in (pos.tolist() if n else []):
        ref = int(rng.integers(0, 5 if kind == "mixed" else 4))
        if kind == "none":
            counts = tuple(9 if x == ref else 0 for x in range(4))
        elif kind == "all":
            counts = tuple(0 if x == ref else int(rng.integers(5, 30)) * int(x == (ref + 1) % 4 or rng.random() < 0.3) for x in range(4))
        else:
            counts = tuple(int(v) for v in rng.integers(0, top + 1, 4) * (rng.random(4) < 0.6))
        rows.append((int(p), sum(counts) + int(rng.integers(0, 2)), 0, counts, ref))
    return rows


@gpu
def test_device_text_and_calls_against_the_host_twins(spm, ctx):
    G = _group_sites(spm, ctx)
    rng = np.random.default_rng(41)
    for i, n in enumerate((0, 1, 63, 64, 65, G - 1, G, G + 1, 2 * G + 1)):
        _text, _calls, st = _raw(spm, ctx, _rows(rng, n), sample="samp"[:1 + i % 4], ploidy=1 + i % 2)
        assert st.group_sites == G
    starts = set()
    for sample in ("s", "sa", "sam", "samp"):                      # every alignment mod 4 of the first line
        _text, calls, st = _raw(spm, ctx, _rows(rng, G + 3, "all"), sample=sample)
        starts.add(st.n_header_bytes % 4)
        assert st.n_variant == G + 3
    assert starts == {0, 1, 2, 3}
    for rname in ("c", "c" * 254):                                  # the longest name a line can carry
        _raw(spm, ctx, _rows(rng, G + 1), rname=rname)
    # no site yields a line; every site yields one
    text, _calls, st = _raw(spm, ctx, _rows(rng, 2 * G + 1, "none"))
    assert st.n_variant == 0 and st.n_ref == 2 * G + 1 and len(text) == st.n_header_bytes
    text, _calls, st = _raw(spm, ctx, _rows(rng, 2 * G + 1, "all"), min_qual=300)
    assert st.n_variant == 2 * G + 1 and text.count(b"\n") == 9 + 2 * G + 1 and 0 < st.n_low_qual < st.n_variant
    # custom costs and priors reach the device as they reach the host
    _raw(spm, ctx, _rows(rng, G + 1), cost_match=5, cost_het=700, cost_miss=9000, prior_het=2, prior_hom_alt=3, min_qual=0)


@gpu
def test_shortest_beside_longest_and_saturating_counts(spm, ctx):
    G = _group_sites(spm, ctx)
    # a one-digit POS and one ALT against a ten-digit POS, two ALTs and ten-digit AD, DP and PL, alternating, across a group border
    short = lambda pos: (pos, 3, 0, (0, 0, 3, 0), 0)
    long_ = lambda pos: (pos, U32, 0, (0, U32, 0, U32 - 1), 0)
    rows = [short(i) for i in range(9)] + [(long_ if i % 2 else short)(4294967000 + i) for i in range(G + 5)] + [long_(U32 - 1)]
    text, calls, st = _raw(spm, ctx, rows, rname="c", ref_len=U32)
    lines = text[st.n_header_bytes:].splitlines()
    assert len(lines) == len(rows) and min(map(len, lines)) < 60 and max(map(len, lines)) > 140
    assert lines[-1].split(b"\t")[1] == b"4294967295" and b"2147483647" in lines[-1] and lines[-1].split(b"\t")[4] == b"C,T"
    assert int(calls["len"].max()) > 140 and int(calls["len"].min()) < 60
    # counts of 2^32 - 1 in all four planes: no overflow, PLs saturating at 2^31 - 1
    big = [(5, U32, U32, (U32,) * 4, 0), (6, U32, 0, (0, U32, 0, 0), 3), (7, U32, 0, (U32, U32, U32, 0), 2)]
    for ploidy in (1, 2):
        text, calls, _st = _raw(spm, ctx, big, ploidy=ploidy)
        assert b"2147483647" in text and calls["qual"][1] == (1 << 31) - 1
    _raw(spm, ctx, big, cost_match=1000000, cost_het=1000000, cost_miss=1000000, prior_het=1000000, prior_hom_alt=1000000)


@gpu
def test_refusals_counted_on_the_device(spm, ctx):
    G = _group_sites(spm, ctx)
    lib = spm.capi.lib()
    rng = np.random.default_rng(43)
    rows = _rows(rng, 2 * G + 7, "all")
    ref_len = rows[-1][0] + 1

    def refused(bad_rows, ref_len=ref_len):
        sites = make_sites(spm.PILEUP_SITE_DTYPE, bad_rows)
        dev = _Device(sites.tobytes())
        h = ctypes.c_void_p(0x7777)
        rc = lib.spm_hip_pileup_sites_vcf_records(ctx._h, dev.ptr, len(bad_rows), b"chr1", b"S", ref_len, None, ctypes.byref(h))
        assert rc == INVALID and not h.value and b"ascend" in lib.spm_hip_last_error(ctx._h)
        ctx.synchronize()
        assert download(ctx, dev.ptr.value, len(sites), spm.PILEUP_SITE_DTYPE).tobytes() == sites.tobytes()   # the caller's buffer is untouched
        dev.close()
        with pytest.raises(spm.SpmError, match="-1.*ascend"):
            spm.pileup_sites_vcf_host(sites, "chr1", "S", ref_len)  # the host twin refuses the same inputs

    def with_pos(i, pos):
        out = list(rows)
        out[i] = (pos,) + rows[i][1:]
        return out

    refused(with_pos(G, rows[G - 1][0]))                            # not ascending at a group border: equal to the left neighbour's
    refused(with_pos(G, rows[G - 1][0] - 1))                        # and descending
    refused(with_pos(G + 5, rows[G + 4][0]))                        # inside a group
    refused(with_pos(1, rows[0][0]))
    refused(rows, ref_len=rows[-1][0])                              # the last pos == ref_len
    refused(rows[:1], ref_len=rows[0][0])
    refused(with_pos(len(rows) - 1, ref_len))
    _raw(spm, ctx, rows, ref_len=ref_len)                           # the context works on, and pos == ref_len - 1 is taken
    # what the host decides before any launch
    sites = make_sites(spm.PILEUP_SITE_DTYPE, rows)
    dev = _Device(sites.tobytes())
    for rc, kw in ((INVALID, dict(ploidy=3)), (INVALID, dict(cost_miss=1000001)), (INVALID, dict(rname="a b")), (INVALID, dict(rname="*")),
                   (INVALID, dict(sample="")), (INVALID, dict(sample="a\tb")), (UNSUPPORTED, dict(ref_len=1 << 32)), (UNSUPPORTED, dict(n=1 << 32))):
        kw = dict(dict(rname="chr1", sample="S", ref_len=ref_len, n=len(rows)), **kw)
        n, rname, sample, rl = kw.pop("n"), kw.pop("rname"), kw.pop("sample"), kw.pop("ref_len")
        with pytest.raises(spm.SpmError, match=str(rc)):
            ctx.pileup_sites_vcf(dev.ptr.value, n, rname, sample, rl, **kw)
    h = ctypes.c_void_p(0x7777)
    assert lib.spm_hip_pileup_sites_vcf_records(ctx._h, None, 3, b"chr1", b"S", ref_len, None, ctypes.byref(h)) == INVALID and not h.value
    assert lib.spm_hip_pileup_sites_vcf_records(ctx._h, dev.ptr, 3, None, b"S", ref_len, None, ctypes.byref(h)) == INVALID
    assert lib.spm_hip_pileup_sites_vcf_records(ctx._h, dev.ptr, 3, b"chr1", None, ref_len, None, ctypes.byref(h)) == INVALID
    assert lib.spm_hip_pileup_sites_vcf_records(ctx._h, dev.ptr, 3, b"chr1", b"S", ref_len, None, None) == INVALID
    assert lib.spm_hip_pileup_sites_vcf_records(None, dev.ptr, 3, b"chr1", b"S", ref_len, None, ctypes.byref(h)) == INVALID
    assert lib.spm_hip_pileup_sites_vcf(None, b"chr1", b"S", ref_len, None, ctypes.byref(h)) == INVALID
    ctx.synchronize()
    dev.close()


@gpu
def test_the_chain_behind_sort_markdup_pileup_and_sites(spm, ctx):
    t = _single_reads()[0]
    ref = t["ref"]
    ref_len = len(ref)
    spots = _free_stretches(t, 300, 40, first=1000)
    reads, planted = [], []
    for spot, m_len, col, carriers in ((spots[-1], 50, 20, 3), (spots[-2], 64, 31, 6), (spots[-3], 37, 5, 2)):   # het, hom, too few
        x = spot + 40
        base = (int(ref[x + col]) + 1 + len(planted)) % 4
        for j in range(6):
            r = np.array(ref[x:x + m_len], np.uint8)
            if j < carriers:
                r[col] = base
            reads.append(r)
        planted.append((x + col, base, carriers))
    lc, rd, ref_text, ps, rest = _chain_of(spm, ctx, t, reads)
    b = lc.bam_ex(rd, ps, RNAME, ref_len)
    s = b.sort()
    m = s.markdup()
    p = m.pileup(exclude_flags=0x4)                                 # the six copies of a read are duplicates of each other: keep them
    sr = p.site_records(ref_text)
    sites = sr.view()
    assert sites.tobytes() == p.sites(ref_text).tobytes() and len(sr) == len(sites) == len(planted)
    v = sr.vcf(RNAME, "sample_1", ref_len)
    sr.close()                                                      # the result outlives its source
    text, calls = v.text(), v.calls()
    assert text == spm.pileup_sites_vcf_host(sites, RNAME, "sample_1", ref_len)
    assert text == vcf_rule.text([(int(x["pos"]), int(x["depth"]), int(x["alt"]), tuple(int(c) for c in x["counts"]), int(x["ref"])) for x in sites],
                                 RNAME, "sample_1", ref_len)
    want = spm.pileup_sites_calls_host(sites)
    got = calls.copy()
    got["offset"], got["len"] = 0, 0
    assert got.tobytes() == want.tobytes()
    by_pos = {int(c["pos"]): c for c in calls}
    for pos, base, carriers in planted:
        c = by_pos[pos]
        r = int(ref[pos])
        want_gt = {3: sorted((r, base)), 6: [base, base], 2: sorted((r, base))}[carriers]   # 2 of 6: 2 * 24771 + 4 * 44 against 6 * 3039 + 30000
        assert c["status"] == 1 and c["gt"].tolist() == want_gt and c["depth"] == 6, (pos, carriers)
        assert text[int(c["offset"]):int(c["offset"]) + int(c["len"])].split(b"\t")[:2] == [RNAME.encode(), str(pos + 1).encode()]
    st = v.stats()
    assert (st.n_sites, st.n_variant, st.n_text_bytes) == (len(sites), len(planted), len(text))
    z = v.bgzf_deflate()
    assert bgzf_inflate.payload_of(bgzf_inflate.parse(z.bytes())) == text
    z2 = v.bgzf()
    assert bgzf_inflate.payload_of(bgzf_inflate.parse(z2.bytes())) == text
    assert v.text() == text                                         # two runs give identical bytes
    again = p.site_records(ref_text).vcf(RNAME, "sample_1", ref_len, ploidy=1)
    assert again.text() == spm.pileup_sites_vcf_host(sites, RNAME, "sample_1", ref_len, ploidy=1)
    for x in (again, z2, z, v, p, m, s, b, rd, lc, ps, ref_text) + rest:
        x.close()
