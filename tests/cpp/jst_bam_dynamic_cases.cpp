// jst_bam_dynamic_cases.cpp -- a BAM file whose deflated blocks may take a Huffman code of their own, through the C++ mirror, on
// the committed fixtures (tests/golden/jst): journaled_sequence_tree::map_bam with jst_bam_options::deflate and ::dynamic by the
// device route (spm_hip_bam_deflate with SPM_BGZF_DYNAMIC) and by the host route (the mirror's own header and records through
// spm_hip_bgzf_deflate_host with the flag), at two block sizes: the same file bytes and block offsets, no longer than without the
// flag, dynamic blocks among them; zlib inflates the file to what the stored file holds, and every record's virtual offset leads
// to its block_size.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include <zlib.h>

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

// one gzip member at `at` of file, inflated by zlib; *size: the member's bytes
static std::string inflate_member(std::string const & file, std::size_t at, std::size_t * size)
{
    z_stream z{};
    std::string out(70000, '\0');
    if (inflateInit2(&z, 16 + 15) != Z_OK)
        return {};
    z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(file.data() + at));
    z.avail_in = static_cast<uInt>(file.size() - at);
    z.next_out = reinterpret_cast<Bytef *>(out.data());
    z.avail_out = static_cast<uInt>(out.size());
    int const rc = inflate(&z, Z_FINISH);
    *size = z.total_in;
    out.resize(rc == Z_STREAM_END ? z.total_out : 0);
    inflateEnd(&z);
    return rc == Z_STREAM_END ? out : std::string("\xff not a member");
}

static std::string inflate_file(std::string const & file)
{
    std::string out;
    for (std::size_t at = 0, size = 0; at < file.size(); at += size) {
        out += inflate_member(file, at, &size);
        if (size == 0)
            return "\xff stuck";
    }
    return out;
}

static std::uint32_t le32(std::string const & s, std::size_t at)
{
    std::uint32_t v = 0;
    for (int i = 0; i < 4; ++i)
        v |= static_cast<std::uint32_t>(static_cast<unsigned char>(s[at + static_cast<std::size_t>(i)])) << (8 * i);
    return v;
}

static void tree_cases(spm::journaled_sequence_tree const & jst, std::vector<spm::io::fasta_record> const & haps)
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
    spm::hip::hit_selection const sel{true, {}, 1u, true, true};
    auto const nr = static_cast<std::uint32_t>(n_reads);
    spm::jst_sam_pairing const single{}, rescued{true, MIN_TLEN, MAX_TLEN, true, K};
    for (std::uint32_t block_data : {0u, 1000u})
        for (int mode = 0; mode < 2; ++mode) {
            spm::jst_bam_options o;
            o.sam.rname = "sim_ref";
            o.sam.secondary = true;
            o.ref_len = jst.reference().size();
            o.block_data = block_data;
            spm::jst_sam_pairing const & pairing = mode == 0 ? single : rescued;
            spm::jst_bam const stored = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            EXPECT_TRUE(stored.block_offsets.empty());
            o.deflate = true;
            spm::jst_bam const fixed = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            o.dynamic = true;
            spm::jst_bam const dev = jst.map_bam_device(ps, window, 2, nr, pairing, o, sel, 0, nullptr);
            spm::jst_bam const host = jst.map_bam_host(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr);
            EXPECT_TRUE(dev.file == host.file);
            EXPECT_TRUE(dev.block_offsets == host.block_offsets);
            EXPECT_TRUE(dev.header_file_bytes == host.header_file_bytes);
            EXPECT_TRUE(dev.records == host.records && dev.records == stored.records && dev.lines == host.lines && dev.lines == stored.lines);
            EXPECT_TRUE(dev == jst.map_bam(ps, window, needles, false, 2, nr, pairing, o, sel, 0, nullptr));
            EXPECT_TRUE(dev.file.size() < stored.file.size() && inflate_file(dev.file) == inflate_file(stored.file));
            EXPECT_TRUE(dev.file.size() < fixed.file.size() && dev.records == fixed.records && dev.block_offsets.size() == fixed.block_offsets.size());
            std::size_t n_dynamic = 0; // BTYPE of a block's one deflate block: bits 1 and 2 of the first payload byte
            for (std::size_t b = 0; b + 1 < dev.block_offsets.size(); ++b)
                n_dynamic += ((static_cast<unsigned char>(dev.file[dev.block_offsets[b] + 18]) >> 1) & 3) == 2;
            EXPECT_TRUE(n_dynamic >= 1);
            std::uint64_t const D = block_data ? block_data : 65280, n_blocks = (dev.records.size() + D - 1) / D;
            EXPECT_TRUE(dev.block_offsets.size() == n_blocks + 1 && dev.block_offsets.front() == dev.header_file_bytes &&
                        dev.block_offsets.back() + 28 == dev.file.size());
            // a record's virtual offset names a block and a byte in it: its block_size, read across the border if need be
            bool reached = !dev.lines.empty();
            for (std::size_t i = 0; i < dev.lines.size() && reached; ++i) {
                std::uint64_t const v = dev.virtual_offset(i, block_data);
                std::size_t at = v >> 16, size = 0;
                std::string bytes = inflate_member(dev.file, at, &size).substr(v & 0xFFFF);
                while (bytes.size() < 4 && size) {
                    at += size;
                    bytes += inflate_member(dev.file, at, &size);
                }
                reached = std::find(dev.block_offsets.begin(), dev.block_offsets.end(), v >> 16) != dev.block_offsets.end() &&
                          bytes.size() >= 4 && le32(bytes, 0) + 4 == dev.lines[i].len;
            }
            EXPECT_TRUE(reached);
            std::printf("  block_data %u, mode %d: %zu records, %zu bytes, stored file %zu bytes, fixed %zu, dynamic %zu bytes in %zu blocks\n", block_data,
                        mode, dev.lines.size(), dev.records.size(), stored.file.size(), fixed.file.size(), dev.file.size(), dev.block_offsets.size() - 1);
        }
}

int main()
{
    auto ref = spm::io::read_fasta(DATA + "sim_ref_10Kb.fasta.gz");
    auto variants = spm::io::read_vcf(DATA + "sim_ref_10Kb_SNP_INDELs.vcf");
    auto haps = spm::io::read_fasta(DATA + "sim_ref_10Kb_SNP_INDELs_haplotypes.fasta.gz");
    EXPECT_TRUE(ref.size() == 1 && haps.size() == 100 && variants.n_haplotypes == 100);
    spm::journaled_sequence_tree jst{ref[0].ranks, variants};
    tree_cases(jst, haps);
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures;
}
