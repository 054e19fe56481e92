"""The duplicate-marking rule of spm_hip.h (spm_hip_bam_markdup) written again in Python, from the SAM text of the records
(FLAG, POS, CIGAR, QUAL) and the read index of every line, with dictionaries and no sort: independent of the C record parser
and of the device's two sorts.  A plain module, imported by the test files that need it."""
import re

MAX_SCORE = (1 << 24) - 1
DEFAULT_MIN_QUAL = 15
_ITEM = re.compile(r"([0-9]+)([MIDNSHP=X])")


def fields_of(line):
    """a SAM line (bytes or str) -> (flag, 0-based pos, CIGAR, QUAL)"""
    f = (line.decode("latin-1") if isinstance(line, bytes) else line).rstrip("\n").split("\t")
    return int(f[1]), int(f[3]) - 1, f[5], f[10]


def five_prime(flag, pos, cigar):
    """(u, s) of a placed record"""
    span = sum(int(n) for n, op in _ITEM.findall(cigar) if op in "MDN=X") if cigar != "*" else 0
    end = pos + max(span, 1)
    return (end - 1, 1) if flag & 0x10 else (pos, 0)


def score_of(qual, min_qual):
    if qual == "*":
        return 0
    return min(sum(v for v in (ord(c) - 33 for c in qual) if min_qual <= v <= 93), MAX_SCORE)


def py_markdup(sam_lines, reads, min_qual=0):
    """sam_lines: the record lines in record order; reads: the read of every line -> (dup per line as a list of 0 / 1, the counts
    of spm_bam_markdup_stats as a dict)"""
    min_qual = min_qual or DEFAULT_MIN_QUAL
    reads = [int(r) for r in reads]
    assert len(sam_lines) == len(reads)
    primary, end, score, paired = {}, {}, {}, {}
    for i, (line, r) in enumerate(zip(sam_lines, reads)):
        flag, pos, cigar, qual = fields_of(line)
        if flag & 0x900:
            continue
        assert r not in primary, ("two primary records", r)
        primary[r] = i
        if flag & 0x4:
            continue
        assert "S" not in cigar and "H" not in cigar
        end[r], score[r], paired[r] = five_prime(flag, pos, cigar), score_of(qual, min_qual), bool(flag & 1)
    is_pair_end = lambda r: r in end and paired[r] and (r ^ 1) in end and paired[r ^ 1]
    dup_read = set()
    # pairs: the best of every key is the one with the highest score, then the lowest p
    best, pair_ends, pairs = {}, set(), []
    for r in sorted(end):
        if r & 1 or not is_pair_end(r):
            continue
        p = r >> 1
        key = tuple(sorted((end[r], end[r + 1])))
        pairs.append((p, key))
        pair_ends |= set(key)
        rank = (-(score[r] + score[r + 1]), p)
        if key not in best or rank < best[key]:
            best[key] = rank
    for p, key in pairs:
        if best[key][1] != p:
            dup_read |= {2 * p, 2 * p + 1}
    n_dup_pairs = len(dup_read) // 2
    # fragments
    fragments = [r for r in sorted(end) if not is_pair_end(r)]
    beside = [r for r in fragments if end[r] in pair_ends]
    dup_read |= set(beside)
    best = {}
    for r in fragments:
        if end[r] not in pair_ends:
            rank = (-score[r], r)
            if end[r] not in best or rank < best[end[r]]:
                best[end[r]] = rank
    dup_read |= {r for r in fragments if end[r] not in pair_ends and best[end[r]][1] != r}
    dup = [int(primary.get(r) == i and r in dup_read) for i, r in enumerate(reads)]
    n_dup_fragments = sum(1 for r in fragments if r in dup_read)
    counts = dict(n_records=len(reads), n_pairs=len(pairs), n_fragments=len(fragments), n_dup_pairs=n_dup_pairs,
                  n_dup_fragments=n_dup_fragments, n_dup_records=sum(dup), n_fragments_beside_pairs=len(beside))
    assert counts["n_dup_records"] == 2 * n_dup_pairs + n_dup_fragments
    return dup, counts
