"""CPU: genotype calls for pileup sites and the VCF text by the serial host twins (spm_hip_pileup_sites_calls_host,
spm_hip_pileup_sites_vcf_host, spm_hip_vcf_header): the worked table of spm_hip.h byte for byte; the twins against the rule
written again in tests/vcf_rule.py on random sites with small counts, every reference rank, both ploidies, custom costs and
priors; min_qual at its edge; a tie at every adjacent pair of the genotype order; reference ranks above 3; counts of 2^32 - 1;
every refusal; the overflow path; layouts, names and the header's bytes; and a truth test over the haplotype fixtures."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import vcf_rule
from cpp_programs import ROOT, c_layout
from pileup_rule import make_stream
from vcf_rule import make_sites

INVALID, UNSUPPORTED, OVERFLOW = -1, -4, -5
A, C, G, T = range(4)
U32 = (1 << 32) - 1

WORKED = [  # counts, depth, the tail of the line (None: no line) -- the table of spm_hip.h and pileup_vcf_core.hpp
    ((10, 10, 0, 0), 20, "A C 157 PASS DP=20 GT:AD:GQ:PL 0/1:10,10:99:157,0,190"),
    ((0, 0, 3, 0), 3, "A G 41 PASS DP=3 GT:AD:GQ:PL 1/1:0,3:6:41,6,0"),
    ((0, 8, 0, 8), 16, "A C,T 288 PASS DP=16 GT:AD:GQ:PL 1/2:0,8,8:99:288,144,123,144,0,123"),
    ((19, 1, 0, 0), 20, None),
]


def both(spm, rows, rname="chr1", sample="S", ref_len=None, **opts):
    """host twins == the Python rule -> (text, calls)"""
    ref_len = ref_len if ref_len is not None else (max(r[0] for r in rows) + 1 if rows else 0)
    sites = make_sites(spm.PILEUP_SITE_DTYPE, rows)
    text = spm.pileup_sites_vcf_host(sites, rname, sample, ref_len, **opts)
    want = vcf_rule.text(rows, rname, sample, ref_len, **opts)
    assert text == want, next((a, b) for a, b in zip(text.split(b"\n"), want.split(b"\n")) if a != b)
    calls = spm.pileup_sites_calls_host(sites, **opts)
    assert calls.dtype == spm.VARIANT_CALL_DTYPE and len(calls) == len(rows)
    assert vcf_rule.calls_as_dicts(calls) == [vcf_rule.call_as_record(vcf_rule.call(r, **opts)) for r in rows]
    assert calls["pos"].tolist() == [r[0] for r in rows] and calls["depth"].tolist() == [r[1] for r in rows]
    assert not calls["len"].any() and not calls["offset"].any() and not calls["reserved"].any()
    return text, calls


def test_worked_table_of_the_header(spm):
    rows = [(7 + 3 * i, depth, 0, counts, A) for i, (counts, depth, _t) in enumerate(WORKED)]
    text, calls = both(spm, rows, ref_len=100)
    head = spm.vcf_header("chr1", "S", 100)
    assert text.startswith(head)
    want = [("chr1 %d . " % (r[0] + 1) + tail).replace(" ", "\t").encode() + b"\n" for r, (_c, _d, tail) in zip(rows, WORKED) if tail]
    assert text[len(head):] == b"".join(want)
    assert calls["status"].tolist() == [1, 1, 1, 0] and calls["qual"].tolist() == [157, 41, 288, 0] and calls["gq"].tolist() == [99, 6, 99, 0]
    assert calls["gt"].tolist() == [[A, C], [G, G], [C, T], [A, A]] and calls["n_alt"].tolist() == [1, 1, 2, 0]
    # the costs the table quotes
    o = vcf_rule.resolve()
    assert vcf_rule.cost((10, 10, 0, 0), (A, A), A, o) == 248150 and vcf_rule.cost((10, 10, 0, 0), (A, C), A, o) == 90780
    assert vcf_rule.cost((10, 10, 0, 0), (C, C), A, o) == 281160
    assert vcf_rule.cost((19, 1, 0, 0), (A, A), A, o) == 25607 and vcf_rule.cost((19, 1, 0, 0), (A, C), A, o) == 90780
    assert vcf_rule.cost((20, 20, 0, 0), (A, C), A, o) == 151560 and vcf_rule.cost((20, 20, 0, 0), (A, A), A, o) == 496300


def random_rows(rng, n, top):
    pos = np.sort(rng.choice(50 * n, n, replace=False))
    rows = []
    for p in pos.tolist():
        counts = tuple(int(v) for v in rng.integers(0, top + 1, 4) * (rng.random(4) < 0.6))
        extra = int(rng.integers(0, 3))                             # N and DEL evidence: in depth, not in the counts
        rows.append((p, sum(counts) + extra, int(rng.integers(0, 9)), counts, int(rng.integers(0, 4))))
    return rows


@pytest.mark.parametrize("ploidy", [1, 2])
def test_host_twins_against_the_python_rule(spm, ploidy):
    rng = np.random.default_rng(11 + ploidy)
    rows = random_rows(rng, 3000, 4) + []                           # small counts: ties occur
    text, calls = both(spm, rows, ploidy=ploidy)
    status = calls["status"].tolist()
    assert status.count(1) > 500 and status.count(0) > 100 and {int(r[4]) for r in rows} == {0, 1, 2, 3}
    ties = sum(1 for r in rows if len({vcf_rule.cost(r[3], g, r[4], vcf_rule.resolve(ploidy=ploidy))
                                      for g in (((a, a) for a in range(4)) if ploidy == 1 else ((a, b) for a in range(4) for b in range(a, 4)))}) < (4 if ploidy == 1 else 10))
    assert ties > 1000
    assert text.count(b"\n") == 9 + status.count(1)
    both(spm, random_rows(rng, 500, 40), ploidy=ploidy, rname="c", sample="sample_name")
    # custom costs and priors; the three costs and the two priors are each taken as a group
    for kw in (dict(cost_match=100, cost_het=3100, cost_miss=20000), dict(prior_het=1000, prior_hom_alt=1), dict(cost_match=0, cost_het=1, cost_miss=0),
               dict(prior_het=0, prior_hom_alt=7), dict(cost_match=1000000, cost_het=1000000, cost_miss=1000000, prior_het=1000000, prior_hom_alt=1000000),
               dict(cost_match=5, cost_het=700, cost_miss=9000, prior_het=2, prior_hom_alt=3, min_qual=0)):
        both(spm, random_rows(rng, 300, 6), ploidy=ploidy, **kw)
    both(spm, [])                                                   # zero sites: the header alone
    assert spm.pileup_sites_vcf_host(make_sites(spm.PILEUP_SITE_DTYPE, []), "r", "s", 0) == spm.vcf_header("r", "s", 0)


def test_min_qual_at_its_edge(spm):
    rows = [(5, 3, 0, (0, 0, 3, 0), A)]                             # QUAL 41
    for min_qual, want in ((0, b"PASS"), (40, b"PASS"), (41, b"PASS"), (42, b"LowQual"), (U32, b"LowQual")):
        text, _ = both(spm, rows, min_qual=min_qual)
        assert text.splitlines()[-1].split(b"\t")[5:7] == [b"41", want], min_qual
    lib, sites = spm.capi.lib(), make_sites(spm.PILEUP_SITE_DTYPE, rows)   # NULL opts: 20
    buf, n = ctypes.create_string_buffer(4096), ctypes.c_uint64()
    assert lib.spm_hip_pileup_sites_vcf_host(sites.ctypes.data, 1, b"chr1", b"S", 10, None, buf, 4096, ctypes.byref(n)) == 0
    assert buf.raw[:n.value] == vcf_rule.text(rows, "chr1", "S", 10)


def test_a_tie_at_every_adjacent_pair_of_the_genotype_order(spm):
    """For each reference rank and each adjacent pair (g, h) of the order (0,0) (0,1) (1,1) (0,2) ... over (ref, the other
    ranks ascending) a site -- found by a search over counts 0..3 and small costs and priors, odd ones included -- where g and h
    tie for the least cost: the first genotype of the order with that cost must win, and that is g wherever no earlier one ties
    too (for some pairs the symmetry of the costs always lets an earlier one in)."""
    rng = np.random.default_rng(3)
    option_sets = [dict(zip(("cost_match", "cost_het", "cost_miss", "prior_het", "prior_hom_alt"), (int(v) for v in rng.integers(0, 5, 5)))) for _ in range(300)]
    option_sets = [kw for kw in option_sets if (kw["cost_match"] or kw["cost_het"] or kw["cost_miss"]) and (kw["prior_het"] or kw["prior_hom_alt"])]
    seen = strict = 0
    for ref in range(4):
        order = [ref] + [x for x in range(4) if x != ref]
        pairs = [(j, k) for k in range(4) for j in range(k + 1)]
        for at, (g, h) in enumerate(zip(pairs, pairs[1:])):
            found = None
            for kw in option_sets:
                o = vcf_rule.resolve(**kw)
                for code in range(256):
                    counts = tuple((code >> (2 * x)) & 3 for x in range(4))
                    costs = [vcf_rule.cost(counts, tuple(order[i] for i in p), ref, o) for p in pairs]
                    if costs[at] == costs[at + 1] == min(costs):
                        first = costs.index(min(costs))
                        if found is None or first == at:
                            found = (counts, kw, first)
                        if first == at:
                            break
                if found and found[2] == at:
                    break
            assert found, (ref, g, h)
            counts, kw, first = found
            _text, calls = both(spm, [(9, sum(counts), 0, counts, ref)], **kw)
            assert calls["gt"][0].tolist() == sorted(order[i] for i in pairs[first]), (ref, g, h, counts, kw)
            seen += 1
            strict += first == at
    assert seen == 4 * 9 and strict >= 4 * 6, strict
    # the same with the defaults, where the table's tie is real: 0,8,0,8 at ploidy 1 ties C with T, and C wins
    _text, calls = both(spm, [(1, 16, 0, (0, 8, 0, 8), A)], ploidy=1)
    assert calls["gt"][0].tolist() == [C, C]
    _text, calls = both(spm, [(1, 0, 0, (0, 0, 0, 0), G)])         # no evidence at all: ref/ref by its prior
    assert calls["status"][0] == 0 and calls["gt"][0].tolist() == [G, G]


def test_ref_above_3_and_saturating_counts(spm):
    rows = [(3, 9, 9, (0, 9, 0, 0), 4), (4, 9, 9, (0, 9, 0, 0), 255), (5, 9, 9, (0, 9, 0, 0), 3)]
    text, calls = both(spm, rows)
    assert calls["status"].tolist() == [2, 2, 1] and text.count(b"\n") == 10 and calls["qual"].tolist()[:2] == [0, 0]
    big = [(0, U32, U32, (U32,) * 4, A), (U32 - 1, U32, 0, (0, U32, 0, 0), T)]
    for ploidy in (1, 2):
        text, calls = both(spm, big, ref_len=U32, ploidy=ploidy)
        line = text.splitlines()[-1].split(b"\t")
        assert line[1] == b"4294967295" and line[7] == b"DP=4294967295"   # a ten-digit POS
        pls = [int(v) for v in line[9].split(b":")[3].split(b",")]
        assert max(pls) == (1 << 31) - 1 and min(pls) == 0         # 2^32 * 21000 / 1000 lies far above 2^31: saturated
        assert calls["status"].tolist() == [1 if ploidy == 2 else 0, 1] and calls["qual"][1] == (1 << 31) - 1
        assert max(vcf_rule.cost((U32,) * 4, (a, b), A, vcf_rule.resolve(ploidy=ploidy)) for a in range(4) for b in range(a, 4)) < 1 << 64
    for kw in (dict(cost_match=1000000, cost_het=1000000, cost_miss=1000000, prior_het=1000000, prior_hom_alt=1000000),
               dict(cost_match=1, cost_het=1000000, cost_miss=999999)):
        both(spm, big, ref_len=U32, **kw)                           # the largest costs the options take: still below 2^64


def test_refusals_and_the_overflow_path(spm):
    lib, Opts = spm.capi.lib(), spm.capi.VcfOpts
    rows = [(7 + 3 * i, depth, 0, counts, A) for i, (counts, depth, _t) in enumerate(WORKED)]
    sites = make_sites(spm.PILEUP_SITE_DTYPE, rows)
    want = vcf_rule.text(rows, "chr1", "S", 100)
    buf, n = ctypes.create_string_buffer(b"\x07" * 4096, 4096), ctypes.c_uint64(77)
    calls = np.frombuffer(bytearray(b"\x07" * (32 * len(rows))), spm.VARIANT_CALL_DTYPE)

    def text_call(s=sites.ctypes.data, k=len(rows), rname=b"chr1", sample=b"S", ref_len=100, opts=None, dst=buf, cap=4096, length=ctypes.byref(n)):
        return lib.spm_hip_pileup_sites_vcf_host(s, k, rname, sample, ref_len, ctypes.byref(opts) if opts is not None else None, dst, cap, length)

    def calls_call(s=sites.ctypes.data, k=len(rows), opts=None, dst=calls.ctypes.data):
        return lib.spm_hip_pileup_sites_calls_host(s, k, ctypes.byref(opts) if opts is not None else None, dst)

    bad_opts = [Opts(ploidy=3), Opts(ploidy=0xFFFFFFFF), Opts(flags=1), Opts(reserved0=1), Opts(reserved1=1), Opts(cost_match=1000001),
                Opts(cost_het=1000001), Opts(cost_miss=1000001), Opts(prior_het=1000001), Opts(prior_hom_alt=1000001)]
    descending = make_sites(spm.PILEUP_SITE_DTYPE, [rows[1], rows[0]] + rows[2:])
    equal = make_sites(spm.PILEUP_SITE_DTYPE, [rows[0], (rows[0][0],) + rows[1][1:]] + rows[2:])
    for rc, kw in ([(INVALID, dict(s=None)), (INVALID, dict(rname=None)), (INVALID, dict(sample=None)), (INVALID, dict(length=None)),
                    (INVALID, dict(dst=None)), (INVALID, dict(rname=b"")), (INVALID, dict(rname=b"*")), (INVALID, dict(rname=b"a b")),
                    (INVALID, dict(rname=b"c" * 255)), (INVALID, dict(rname=b"a\tb")), (INVALID, dict(sample=b"")), (INVALID, dict(sample=b"a b")),
                    (INVALID, dict(sample=b"a\nb")), (INVALID, dict(sample=b"s" * 255)), (INVALID, dict(sample=b"\x7f")),
                    (INVALID, dict(s=descending.ctypes.data)), (INVALID, dict(s=equal.ctypes.data)), (INVALID, dict(ref_len=rows[-1][0])),
                    (INVALID, dict(ref_len=0)), (UNSUPPORTED, dict(k=1 << 32)), (UNSUPPORTED, dict(ref_len=1 << 32))] +
                   [(INVALID, dict(opts=o)) for o in bad_opts]):
        n.value = 77
        assert text_call(**kw) == rc, kw
        assert buf.raw == b"\x07" * 4096 and n.value == 77, kw      # nothing written
    assert text_call(ref_len=rows[-1][0] + 1) == 0                  # the last pos is ref_len - 1
    assert text_call(rname=b"c" * 254, sample=b"s" * 254) == 0 and text_call(sample=b"*") == 0
    assert text_call() == 0 and n.value == len(want) and buf.raw[:n.value] == want
    for rc, kw in ([(INVALID, dict(s=None)), (INVALID, dict(dst=None)), (INVALID, dict(s=descending.ctypes.data)), (INVALID, dict(s=equal.ctypes.data))] +
                   [(INVALID, dict(opts=o)) for o in bad_opts]):
        assert calls_call(**kw) == rc, kw
        assert calls.tobytes() == b"\x07" * calls.nbytes, kw
    assert calls_call(s=None, k=0, dst=None) == 0 and calls_call() == 0 and calls["status"].tolist() == [1, 1, 1, 0]
    for good in (Opts(ploidy=1), Opts(ploidy=2), Opts(cost_miss=1000000), Opts(min_qual=0xFFFFFFFF)):
        assert calls_call(opts=good) == 0
    # the overflow path: the length comes back, nothing is written
    buf2 = ctypes.create_string_buffer(b"\x07" * 4096, 4096)
    for cap in (0, 1, len(want) - 1):
        n.value = 0
        assert text_call(dst=buf2, cap=cap) == OVERFLOW and n.value == len(want) and buf2.raw == b"\x07" * 4096
    assert text_call(dst=None, cap=0) == OVERFLOW and n.value == len(want)
    assert text_call(dst=buf2, cap=len(want)) == 0 and buf2.raw[:len(want)] == want and buf2.raw[len(want)] == 7
    with pytest.raises(spm.SpmError, match="-1.*ploidy"):
        spm.pileup_sites_vcf_host(sites, "chr1", "S", 100, ploidy=3)
    with pytest.raises(spm.SpmError, match="-1.*ascend"):
        spm.pileup_sites_vcf_host(descending, "chr1", "S", 100)
    with pytest.raises(spm.SpmError, match="-1.*sample"):
        spm.pileup_sites_vcf_host(sites, "chr1", "a b", 100)
    with pytest.raises(spm.SpmError, match="-1.*rname"):
        spm.pileup_sites_vcf_host(sites, "*", "S", 100)
    # the header call: *len / SPM_E_OVERFLOW as spm_hip_sam_header has them
    head = vcf_rule.header("chr1", "S", 100)
    assert spm.vcf_header("chr1", "S", 100) == head and spm.vcf_header(b"x", b"*", (1 << 64) - 1) == vcf_rule.header("x", "*", (1 << 64) - 1)
    assert lib.spm_hip_vcf_header(b"chr1", b"S", 100, None, 0, ctypes.byref(n)) == OVERFLOW and n.value == len(head)
    assert lib.spm_hip_vcf_header(b"chr1", b"S", 100, buf2, len(head) - 1, ctypes.byref(n)) == OVERFLOW
    for rname, sample, length in ((None, b"S", ctypes.byref(n)), (b"chr1", None, ctypes.byref(n)), (b"chr1", b"S", None), (b"*", b"S", ctypes.byref(n)),
                                  (b"chr1", b"", ctypes.byref(n)), (b"chr1", b"a b", ctypes.byref(n))):
        assert lib.spm_hip_vcf_header(rname, sample, 100, buf2, 4096, length) == INVALID
    assert lib.spm_hip_vcf_header(b"chr1", b"S", 100, None, 8, ctypes.byref(n)) == INVALID


LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "spm_hip.h"
#define O(f) printf("opts.%s %zu\n", #f, offsetof(spm_vcf_opts, f))
#define C(f) printf("call.%s %zu\n", #f, offsetof(spm_variant_call, f))
#define S(f) printf("stats.%s %zu\n", #f, offsetof(spm_vcf_stats, f))
int main(void)
{
    O(ploidy); O(cost_match); O(cost_het); O(cost_miss); O(prior_het); O(prior_hom_alt); O(min_qual); O(flags); O(reserved0); O(reserved1);
    C(pos); C(depth); C(qual); C(len); C(offset); C(status); C(gq); C(gt); C(n_alt); C(alt); C(reserved);
    S(ms_total); S(ms_call); S(ms_scan); S(ms_write); S(ms_host); S(group_sites); S(n_sites); S(n_variant); S(n_ref); S(n_ref_n);
    S(n_low_qual); S(n_header_bytes); S(n_text_bytes);
    printf("sizeof.opts %zu\nsizeof.call %zu\nsizeof.stats %zu\n", sizeof(spm_vcf_opts), sizeof(spm_variant_call), sizeof(spm_vcf_stats));
    printf("status.ref %d\nstatus.variant %d\nstatus.ref_n %d\n", SPM_CALL_REF, SPM_CALL_VARIANT, SPM_CALL_REF_N);
    return 0;
}
"""
CALLS = ("spm_hip_pileup_sites_vcf", "spm_hip_pileup_sites_vcf_records", "spm_hip_vcf_view", "spm_hip_vcf_device", "spm_hip_vcf_stats",
         "spm_hip_vcf_destroy", "spm_hip_pileup_sites_calls_host", "spm_hip_pileup_sites_vcf_host", "spm_hip_vcf_header")


def test_layouts_and_names(spm, tmp_path):
    kinds = {"opts": spm.capi.VcfOpts, "call": spm.capi.VariantCall, "stats": spm.capi.VcfStats}
    want = c_layout(tmp_path, LAYOUT_C)
    assert (want.pop("status.ref"), want.pop("status.variant"), want.pop("status.ref_n")) == ("0", "1", "2")
    assert (spm.capi.CALL_REF, spm.capi.CALL_VARIANT, spm.capi.CALL_REF_N) == (0, 1, 2)
    sizes = {k: int(want.pop("sizeof." + k)) for k in kinds}
    assert sizes == {"opts": 40, "call": 32, "stats": 80} == {k: ctypes.sizeof(t) for k, t in kinds.items()}
    seen = dict.fromkeys(kinds, 0)
    for name, off in want.items():
        kind, field = name.split(".")
        assert getattr(kinds[kind], field).offset == int(off), name
        seen[kind] += 1
    assert seen == {k: len(t._fields_) for k, t in kinds.items()} == {"opts": 10, "call": 11, "stats": 13}
    assert spm.VARIANT_CALL_DTYPE.itemsize == 32 and spm.VARIANT_CALL_DTYPE["gt"].shape == (2,)
    for name in CALLS:
        assert name in spm.capi.EXPORTS and hasattr(spm.capi.lib(), name)
    for f in (spm.engine.PileupSites.vcf, spm.engine.Pileup.site_records, spm.Context.pileup_sites_vcf, spm.pileup_sites_calls_host,
              spm.pileup_sites_vcf_host, spm.vcf_header, spm.engine.Vcf.text, spm.engine.Vcf.calls, spm.engine.Vcf.stats, spm.engine.Vcf.device, spm.engine.Vcf.bgzf, spm.engine.Vcf.bgzf_deflate):
        assert callable(f)
    opts = spm.vcf_opts()
    assert (opts.ploidy, opts.min_qual, opts.cost_match, opts.prior_het, opts.flags) == (2, 20, 0, 0, 0)


# ---- the truth test ----
def read_fasta_gz(path):
    names, seqs = [], []
    with gzip.open(path, "rt") as f:
        for ln in f:
            if ln.startswith(">"):
                names.append(ln[1:].strip())
                seqs.append([])
            else:
                seqs[-1].append(ln.strip())
    return names, ["".join(s) for s in seqs]


def test_truth_over_the_haplotype_fixtures(spm):
    """Records 0 and 1 of sim_ref_10Kb_SNPs_haplotypes.fasta.gz are named "1/sample_1 haplotype_1" and "1/sample_1 haplotype_2":
    the two haplotypes of the first sample, which is column simulated_0 of sim_ref_10Kb_SNPs.vcf (the reference's reader,
    libjst's VCF loader, numbers the haplotypes 2 * sample + phase in column order; the test checks the mapping itself: the
    letters the two records carry at every row's POS are the alleles simulated_0's a|b names).  Each haplotype is tiled with
    error-free 100-base forward reads every 5 bases, depth 20 per haplotype away from the ends; pileup, sites and calls by the
    host builders.  Over positions 100..9900 the variant lines are exactly the rows where simulated_0 is not 0|0, each with the
    right REF, ALT set and unphased genotype, each PASS."""
    data = os.path.join(ROOT, "tests", "golden", "jst")
    _, (ref,) = read_fasta_gz(os.path.join(data, "sim_ref_10Kb.fasta.gz"))
    names, haps = read_fasta_gz(os.path.join(data, "sim_ref_10Kb_SNPs_haplotypes.fasta.gz"))
    assert names[0].endswith("sample_1 haplotype_1") and names[1].endswith("sample_1 haplotype_2")
    h0, h1 = haps[0].upper(), haps[1].upper()
    ref = ref.upper()
    n = len(ref)
    assert n == 10000 and len(h0) == len(h1) == n and set(ref + h0 + h1) <= set("ACGT")
    last = -1
    truth = {}                                                      # 0-based pos -> (REF, {alt letters}, sorted genotype letters)
    with open(os.path.join(data, "sim_ref_10Kb_SNPs.vcf")) as f:
        for ln in f:
            if ln.startswith("#"):
                if ln.startswith("#CHROM"):
                    assert ln.rstrip("\n").split("\t")[9] == "simulated_0"
                continue
            c = ln.rstrip("\n").split("\t")
            pos, alleles = int(c[1]) - 1, [c[3]] + c[4].split(",")
            if pos == last:                                         # (POS 9987 stands twice, the second row with every sample 0|0)
                assert pos > 9900
                continue
            last = pos
            assert all(len(a) == 1 for a in alleles) and ref[pos] == c[3]
            a, b = (int(v) for v in c[9].split("|"))
            assert (h0[pos], h1[pos]) == (alleles[a], alleles[b]), pos   # the mapping: record 0 is the left allele, record 1 the right
            if (a, b) != (0, 0) and 100 <= pos <= 9900:
                truth[pos] = (c[3], {alleles[v] for v in (a, b) if v}, sorted((alleles[a], alleles[b])))
    assert len(truth) > 100 and any(len(t[1]) == 2 for t in truth.values()) and any(t[2][0] == t[2][1] for t in truth.values())
    assert sum(1 for p in range(n) if (h0[p], h1[p]) != (ref[p], ref[p]) and 100 <= p <= 9900) == len(truth)
    recs = [dict(pos=s, cigar="100M", seq=h[s:s + 100]) for s in range(0, n - 99, 5) for h in (h0, h1)]
    stream, lines = make_stream(recs)
    counts = spm.bam_pileup_host(stream, lines, n)
    assert (counts[:6].sum(axis=0)[100:9901] == 40).all()
    ranks = np.array(["ACGT".index(ch) for ch in ref], np.uint8)
    sites = spm.pileup_sites_host(counts, 0, ranks)
    text = spm.pileup_sites_vcf_host(sites, "1", "simulated_0", n)
    calls = spm.pileup_sites_calls_host(sites)
    assert text == vcf_rule.text([(int(s["pos"]), int(s["depth"]), int(s["alt"]), tuple(int(v) for v in s["counts"]), int(s["ref"])) for s in sites],
                                 "1", "simulated_0", n)
    got = {}
    for ln in text[len(spm.vcf_header("1", "simulated_0", n)):].decode().splitlines():
        c = ln.split("\t")
        pos = int(c[1]) - 1
        if 100 <= pos <= 9900:
            alleles = [c[3]] + c[4].split(",")
            gt = [int(v) for v in c[9].split(":")[0].split("/")]
            assert c[0] == "1" and c[6] == "PASS" and c[7] == "DP=40", ln
            got[pos] = (c[3], set(c[4].split(",")), sorted(alleles[v] for v in gt))
    assert sorted(got) == sorted(truth)
    assert got == truth
    inside = calls[(calls["pos"] >= 100) & (calls["pos"] <= 9900)]
    assert (inside["status"] == 1).all() and len(inside) == len(truth) and (inside["qual"] >= 20).all()
