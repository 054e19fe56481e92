// jst_bam_cases.cpp -- a BAM file through the C++ mirror, on the committed fixtures (tests/golden/jst):
// journaled_sequence_tree::map_bam by the device route (spm_hip_jst_ref_loci_bam behind the chain) returns the same file bytes,
// record stream and line records as the host route (map_sam_host's lines, each converted to a record from its text fields by
// a plain SAM-to-BAM converter, framed by spm_hip_bgzf_frame_host), single-end, paired and paired with rescues, under both
// flag combinations, with and without names and an own MAPQ table, at the default block size and at small ones.
// The pairs are cut as jst_sam_cases.cpp cuts them: exact, diverged and noise mates.
#include <algorithm>
#include <cstdio>
#include <string>

#include <libspm/jst/journaled_sequence_tree.hpp>

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
        }                                                                                                              \
    } while (0)

static std::string const DATA = std::string(SPM_TEST_DATA) + "/";

static std::uint64_t mix64(std::uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::vector<std::uint8_t> revcomp4(std::vector<std::uint8_t> const & r)
{
    std::vector<std::uint8_t> out;
    for (std::size_t i = r.size(); i-- > 0;)
        out.push_back(static_cast<std::uint8_t>(3 - r[i]));
    return out;
}

static constexpr std::size_t L = 60;
static constexpr std::uint32_t MIN_TLEN = 150, MAX_TLEN = 400, K = 8;

// pair i: a fragment of 200 .. 350 haplotype symbols; i % 4: 0 both mates exact, 1 the right mate diverged, 2 the left mate
// diverged, 3 the right mate is noise; every other pair has mate 1 on the reverse strand
static std::vector<std::vector<std::uint8_t>> cut_pairs(std::vector<spm::io::fasta_record> const & haps, std::size_t n_pairs)
{
    std::vector<std::vector<std::uint8_t>> out;
    std::uint64_t r = 0x5A3C0Eull;
    for (std::size_t i = 0; i < n_pairs; ++i) {
        r = mix64(r + i);
        std::vector<std::uint8_t> const & hap = haps[r % haps.size()].ranks;
        std::size_t const frag = 200 + (r >> 44) % 151, at = (r >> 20) % (hap.size() - 800);
        auto const cut = [&](std::size_t from) {
            return std::vector<std::uint8_t>(hap.begin() + static_cast<std::ptrdiff_t>(from), hap.begin() + static_cast<std::ptrdiff_t>(from + L));
        };
        std::vector<std::uint8_t> left = cut(at), right = cut(at + frag - L);
        auto const diverge = [](std::vector<std::uint8_t> & x) {
            for (std::size_t j = 5; j < L; j += 11)
                x[j] = static_cast<std::uint8_t>((x[j] + 1) & 3);
        };
        if (i % 4 == 1)
            diverge(right);
        if (i % 4 == 2)
            diverge(left);
        if (i % 4 == 3)
            for (std::size_t j = 0; j < L; ++j)
                right[j] = static_cast<std::uint8_t>(mix64(r + 77 * j) & 3);
        if (i % 2) {
            out.push_back(revcomp4(right));
            out.push_back(left);
        } else {
            out.push_back(left);
            out.push_back(revcomp4(right));
        }
    }
    return out;
}

static std::size_t count_kind(spm::jst_bam const & s, std::uint8_t kind)
{
    return static_cast<std::size_t>(std::count_if(s.lines.begin(), s.lines.end(), [&](spm::jst_sam_line const & x) { return x.kind == kind; }));
}

static std::uint32_t le32(std::string const & s, std::size_t at)
{
    std::uint32_t v = 0;
    for (int i = 0; i < 4; ++i)
        v |= static_cast<std::uint32_t>(static_cast<unsigned char>(s[at + static_cast<std::size_t>(i)])) << (8 * i);
    return v;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps, std::size_t block)
{
    std::size_t const n_pairs = 32, n_reads = 2 * n_pairs;
    unsigned const k = 2;
    auto const reads = cut_pairs(haps, n_pairs);
    std::vector<std::uint8_t> cat;
    std::vector<std::uint32_t> off{0};
    std::vector<std::uint16_t> ks(n_reads, static_cast<std::uint16_t>(k));
    std::vector<std::vector<std::uint8_t>> needles;
    for (auto const & rd : reads) {
        cat.insert(cat.end(), rd.begin(), rd.end());
        off.push_back(static_cast<std::uint32_t>(cat.size()));
        needles.push_back(rd);
        needles.push_back(revcomp4(rd));
    }
    spm_ctx * ctx = spm::hip::default_context();
    spm_patterns * ps = nullptr;
    if (spm_hip_patterns_create_stranded(ctx, SPM_ALGO_MYERS, cat.data(), off.data(), static_cast<std::uint32_t>(n_reads), ks.data(), 4,
                                         &ps) != SPM_OK)
        spm::hip::fatal("spm_hip_patterns_create_stranded", ctx);
    spm::hip::patterns_ptr compiled{ps, spm::hip::patterns_deleter{}};
    std::size_t const window = L + k;
    EXPECT_TRUE(jst.device_ready());
    spm::hip::hit_selection const sel{true, {}, 1u, true, true};
    auto const nr = static_cast<std::uint32_t>(n_reads);
    spm::jst_sam_pairing const single{}, paired{true, MIN_TLEN, MAX_TLEN, false, 0}, rescued{true, MIN_TLEN, MAX_TLEN, true, K};
    std::vector<std::string> read_names, pair_names;
    for (std::size_t r = 0; r < n_reads; ++r)
        read_names.push_back("read:" + std::string(r % 7, '#') + std::to_string(r * 977));
    for (std::size_t p = 0; p < n_pairs; ++p)
        pair_names.push_back(std::string(1 + p % 3, static_cast<char>('A' + p % 26)));
    std::string const eof("\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00\x42\x43\x02\x00\x1b\x00\x03\x00\x00\x00\x00\x00\x00\x00\x00\x00", 28);
    std::size_t records_seen = 0;
    for (int flags = 0; flags < 4; ++flags)
        for (int mode = 0; mode < 3; ++mode)
            for (int named = 0; named < 2; ++named) {
                spm::jst_bam_options o;
                o.sam.rname = "sim_ref";
                o.sam.cigar_m = (flags & 1) != 0;
                o.sam.secondary = (flags & 2) != 0;
                o.ref_len = jst.reference().size();
                std::uint32_t const sizes[4] = {0, 1000, 257, 7};
                o.block_data = sizes[(flags + mode + named) % 4];
                if (named) { // names and an own table
                    o.sam.names = mode == 0 ? read_names : pair_names;
                    o.sam.default_tables = false;
                    o.sam.mapq_unique = {50, 41, 32, 23};
                    o.sam.mapq_multi = {9, 8, 7, 6};
                }
                spm::jst_sam_pairing const & pairing = mode == 0 ? single : mode == 1 ? paired : rescued;
                spm::jst_bam const dev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, block, nullptr);
                spm::jst_bam const host = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, block, nullptr);
                EXPECT_TRUE(dev.file == host.file);
                EXPECT_TRUE(dev.records == host.records);
                EXPECT_TRUE(dev.lines == host.lines);
                EXPECT_TRUE(dev.header_file_bytes == host.header_file_bytes);
                EXPECT_TRUE(dev == jst.map_bam(ps, window, needles, false, 2, nr, pairing, o, sel, block, nullptr));
                if (dev.records != host.records) { // the first record that differs
                    for (std::size_t i = 0; i < dev.lines.size() && i < host.lines.size(); ++i) {
                        std::string const a = dev.records.substr(dev.lines[i].offset, dev.lines[i].len);
                        std::string const b = host.records.substr(host.lines[i].offset, host.lines[i].len);
                        if (a != b) {
                            std::printf("  record %zu differs: device %zu bytes, host %zu bytes\n", i, a.size(), b.size());
                            break;
                        }
                    }
                }
                // records tile the stream, each block_size is its length less 4, and the line records are map_sam's but for
                // offset / len
                spm::jst_sam const sam = jst.map_sam_device(ps, window, 2, nr, pairing, o.sam, sel, block, nullptr);
                EXPECT_TRUE(sam.lines.size() == dev.lines.size());
                std::uint64_t end = 0;
                bool tiled = true, same = sam.lines.size() == dev.lines.size();
                for (std::size_t i = 0; i < dev.lines.size(); ++i) {
                    spm::jst_sam_line const & x = dev.lines[i];
                    tiled = tiled && x.offset == end && x.len >= 38 && x.offset + x.len <= dev.records.size() &&
                            le32(dev.records, x.offset) + 4 == x.len;
                    end = x.offset + x.len;
                    if (same)
                        same = x.read == sam.lines[i].read && x.source == sam.lines[i].source && x.flag == sam.lines[i].flag &&
                               x.mapq == sam.lines[i].mapq && x.kind == sam.lines[i].kind;
                }
                EXPECT_TRUE(tiled && same && end == dev.records.size());
                std::uint64_t const D = o.block_data ? o.block_data : 65280, n_blocks = (dev.records.size() + D - 1) / D;
                EXPECT_TRUE(dev.file.size() == dev.header_file_bytes + dev.records.size() + 31 * n_blocks + 28);
                EXPECT_TRUE(dev.file.substr(0, 4) == std::string("\x1f\x8b\x08\x04", 4) && dev.file.substr(dev.file.size() - 28) == eof);
                if (!dev.lines.empty())
                    EXPECT_TRUE(dev.virtual_offset(0, o.block_data) == dev.header_file_bytes << 16);
                EXPECT_TRUE((count_kind(dev, SPM_SAM_RESCUE) > 0) == (mode == 2) && count_kind(dev, SPM_SAM_UNMAPPED) >= 4);
                records_seen += dev.lines.size();
                if (flags == 3 && named == 0)
                    std::printf("  block %zu, mode %d: %zu records, %zu bytes, file %zu bytes, %zu rescue records\n", block, mode,
                                dev.lines.size(), dev.records.size(), dev.file.size(), count_kind(dev, SPM_SAM_RESCUE));
            }
    EXPECT_TRUE(records_seen >= 24 * n_reads);
}

int main()
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + "sim_ref_10Kb_SNP_INDELs.vcf");
    auto haps = spm::io::read_fasta(DATA + "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(ref.size() == 1 && haps.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    tree_cases(jst, haps, 0);
    tree_cases(jst, haps, 64);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
