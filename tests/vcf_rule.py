"""The genotyping rule and the VCF text of spm_hip.h (spm_hip_pileup_sites_vcf) written again in plain Python over site
tuples: the cost of every genotype with Python integers, the tie order, the kept alleles, the PLs in VCF genotype order, the
line and the header.  Independent of pileup_vcf_core.hpp.  A plain module, imported by the test files that need it."""
from itertools import combinations_with_replacement

LETTERS = "ACGT"
DEFAULTS = dict(ploidy=2, cost_match=44, cost_het=3039, cost_miss=24771, prior_het=30000, prior_hom_alt=33010, min_qual=20)
PL_CAP = (1 << 31) - 1
REF, VARIANT, REF_N = 0, 1, 2


def resolve(ploidy=2, cost_match=0, cost_het=0, cost_miss=0, prior_het=0, prior_hom_alt=0, min_qual=20):
    """the options as the header resolves them: the three costs all 0, or the two priors both 0, select the defaults"""
    o = dict(DEFAULTS, ploidy=ploidy or 2, min_qual=min_qual)
    if cost_match or cost_het or cost_miss:
        o.update(cost_match=cost_match, cost_het=cost_het, cost_miss=cost_miss)
    if prior_het or prior_hom_alt:
        o.update(prior_het=prior_het, prior_hom_alt=prior_hom_alt)
    return o


def cost(counts, g, ref, o):
    """g: a tuple of allele ranks, one per chromosome copy"""
    total = 0
    for x in range(4):
        if x not in g:
            per = o["cost_miss"]
        else:
            per = o["cost_match"] if len(set(g)) == 1 else o["cost_het"]
        total += counts[x] * per
    non_ref = [a for a in g if a != ref]
    if o["ploidy"] == 1:
        return total + (o["prior_hom_alt"] if non_ref else 0)
    if not non_ref:
        return total
    if len(non_ref) == 1:
        return total + o["prior_het"]
    return total + (o["prior_hom_alt"] if non_ref[0] == non_ref[1] else 2 * o["prior_het"])


def vcf_order(alleles, ploidy):
    """the genotypes over `alleles` (a list, REF first) in VCF order, as tuples of indices into it: F(j, k) = k (k + 1) / 2 + j"""
    if ploidy == 1:
        return [(k,) for k in range(len(alleles))]
    return sorted(combinations_with_replacement(range(len(alleles)), 2), key=lambda jk: jk[1] * (jk[1] + 1) // 2 + jk[0])


def call(site, **opts):
    """site: (pos, depth, alt, (A, C, G, T), ref rank) -> dict(status, ...) with, for a variant, kept (ranks, REF first), gt
    (indices into kept), pl, qual, gq, low_qual"""
    o = resolve(**opts)
    _pos, _depth, _alt, counts, ref = site
    if ref > 3:
        return dict(status=REF_N)
    order = [ref] + [x for x in range(4) if x != ref]
    best, best_g = None, None
    for g in vcf_order(order, o["ploidy"]):
        c = cost(counts, tuple(order[i] for i in g), ref, o)
        if best is None or c < best:
            best, best_g = c, g
    ranks = tuple(order[i] for i in best_g)
    kept = [ref] + sorted({a for a in ranks if a != ref})
    if len(kept) == 1:
        return dict(status=REF, gt_ranks=tuple(sorted(ranks)))
    pl = [min((cost(counts, tuple(kept[i] for i in g), ref, o) - best + 500) // 1000, PL_CAP) for g in vcf_order(kept, o["ploidy"])]
    qual = pl[0]
    return dict(status=VARIANT, kept=kept, gt=tuple(sorted(kept.index(a) for a in ranks)), gt_ranks=tuple(sorted(ranks)), pl=pl, qual=qual,
                gq=min(99, sorted(pl)[1]), low_qual=qual < o["min_qual"])


def line(site, rname, **opts):
    """-> the line of a site (bytes), or b'' where it has none"""
    c = call(site, **opts)
    if c["status"] != VARIANT:
        return b""
    pos, depth, _alt, counts, _ref = site
    kept = c["kept"]
    sample = ":".join(["/".join(str(i) for i in c["gt"]), ",".join(str(counts[a]) for a in kept), str(c["gq"]), ",".join(str(v) for v in c["pl"])])
    fields = [rname, str(pos + 1), ".", LETTERS[kept[0]], ",".join(LETTERS[a] for a in kept[1:]), str(c["qual"]),
              "LowQual" if c["low_qual"] else "PASS", f"DP={depth}", "GT:AD:GQ:PL", sample]
    return ("\t".join(fields) + "\n").encode()


def header(rname, sample, ref_len):
    return (f"##fileformat=VCFv4.2\n##contig=<ID={rname},length={ref_len}>\n"
            '##FILTER=<ID=LowQual,Description="QUAL below the threshold">\n'
            '##INFO=<ID=DP,Number=1,Type=Integer,Description="Depth: A + C + G + T + N + DEL">\n'
            '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
            '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Base counts of the REF and ALT alleles">\n'
            '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype quality">\n'
            '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype costs">\n'
            f"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t{sample}\n").encode()


def text(sites, rname, sample, ref_len, **opts):
    return header(rname, sample, ref_len) + b"".join(line(s, rname, **opts) for s in sites)


def calls_as_dicts(calls):
    """VARIANT_CALL_DTYPE records -> what call() gives, as far as a record keeps it"""
    out = []
    for c in calls:
        d = dict(status=int(c["status"]))
        if d["status"] != REF_N:
            d["gt_ranks"] = tuple(int(v) for v in c["gt"])
        if d["status"] == VARIANT:
            d.update(kept_alt=[int(v) for v in c["alt"][:int(c["n_alt"])]], qual=int(c["qual"]), gq=int(c["gq"]))
        out.append(d)
    return out


def call_as_record(c, ploidy=2):
    """call()'s dict cut down to the fields calls_as_dicts reads"""
    d = dict(status=c["status"])
    if c["status"] != REF_N:
        g = c["gt_ranks"]
        d["gt_ranks"] = g if len(g) == 2 else (g[0], g[0])
    if c["status"] == VARIANT:
        d.update(kept_alt=c["kept"][1:], qual=c["qual"], gq=c["gq"])
    return d


def make_sites(dtype, rows):
    """rows: (pos, depth, alt, (A, C, G, T), ref rank) -> records of dtype (PILEUP_SITE_DTYPE)"""
    import numpy as np
    s = np.zeros(len(rows), dtype)
    for i, (pos, depth, alt, counts, ref) in enumerate(rows):
        s[i]["pos"], s[i]["depth"], s[i]["alt"], s[i]["counts"], s[i]["ref"] = pos, depth, alt, counts, ref
    return s
