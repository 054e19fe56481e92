// bench_bam_host.cpp -- the clock of the C++ mirror's host route of map_bam (journaled_sequence_tree::sam_host, a plain
// std::string formatter, then bam_of_sam, a plain SAM-to-BAM converter framed by spm_hip_bgzf_frame_host) on views that
// scripts/bench_bam.py downloaded and wrote to a directory: loci, pools, reads, pairs, rescues, needles (one length), optionally
// names.  Prints one JSON object: the medians of `runs` calls behind a warm-up (the formatter, the converter with its framing,
// both), the time to rebuild the host structs from the views, and whether the file equals the device's.
//     bench_bam_host DIR needle_len runs cigar_m secondary named ref_len
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

#include <libspm/jst/journaled_sequence_tree.hpp>

template <class T> static std::vector<T> slurp(std::string const & path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) {
        std::fprintf(stderr, "cannot read %s\n", path.c_str());
        std::exit(2);
    }
    auto const bytes = static_cast<std::size_t>(f.tellg());
    std::vector<T> out(bytes / sizeof(T));
    f.seekg(0);
    f.read(reinterpret_cast<char *>(out.data()), static_cast<std::streamsize>(out.size() * sizeof(T)));
    return out;
}

int main(int argc, char ** argv)
{
    if (argc != 8)
        return 2;
    std::string const dir = std::string(argv[1]) + "/";
    std::size_t const L = std::strtoul(argv[2], nullptr, 10);
    int const runs = std::atoi(argv[3]);
    using clk = std::chrono::steady_clock;
    auto const ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    auto const loci = slurp<spm_jst_ref_locus>(dir + "loci.bin");
    auto const ops = slurp<std::uint32_t>(dir + "ops.bin"), members = slurp<std::uint32_t>(dir + "members.bin");
    auto const scores = slurp<std::int32_t>(dir + "member_scores.bin");
    auto const reads = slurp<spm_jst_read>(dir + "reads.bin");
    auto const pairs = slurp<spm_jst_pair>(dir + "pairs.bin");
    auto const rescues = slurp<spm_jst_rescue>(dir + "rescues.bin");
    auto const rops = slurp<std::uint32_t>(dir + "rescue_ops.bin");
    auto const ranks = slurp<std::uint8_t>(dir + "needles.bin");
    auto const want = slurp<char>(dir + (std::string("bam_") + argv[4] + argv[5] + argv[6] + ".bin"));
    auto const t0 = clk::now();
    spm::jst_read_loci mapped;
    for (auto const & x : loci) {
        spm::jst_ref_locus y{x.pattern,
                             spm::alignment{static_cast<std::size_t>(x.ref_begin), static_cast<std::size_t>(x.ref_end), x.ref_score,
                                            ops.data() + x.cigar_off, x.cigar_len},
                             x.score, x.n_records, {}};
        for (std::uint32_t m = 0; m < x.n_haplotypes; ++m)
            y.members.emplace_back(members[x.member_off + m], scores[x.member_off + m]);
        mapped.loci.push_back(std::move(y));
    }
    for (auto const & r : reads)
        mapped.reads.push_back({r.first_locus, r.n_loci, r.n_forward, r.primary, r.best, r.best_ref_score, r.n_best, r.n_next});
    std::vector<spm::jst_pair> pp;
    for (auto const & p : pairs)
        pp.push_back({p.locus1, p.locus2, p.tlen, p.best, p.n_pairs, p.n_best, p.n_next, p.flag1, p.flag2});
    std::vector<spm::jst_rescue> rr;
    for (auto const & r : rescues)
        rr.push_back({r.pair, r.pattern, r.anchor,
                      spm::alignment{static_cast<std::size_t>(r.ref_begin), static_cast<std::size_t>(r.ref_end), r.score,
                                     rops.data() + r.cigar_off, r.cigar_len},
                      r.tlen, r.flag, r.status});
    std::vector<std::vector<std::uint8_t>> needles;
    for (std::size_t at = 0; at + L <= ranks.size(); at += L)
        needles.emplace_back(ranks.begin() + static_cast<std::ptrdiff_t>(at), ranks.begin() + static_cast<std::ptrdiff_t>(at + L));
    double const ms_structs = ms(t0, clk::now());
    spm::jst_bam_options b;
    b.ref_len = std::strtoull(argv[7], nullptr, 10);
    spm::jst_sam_options & o = b.sam;
    o.rname = "pan_ref";
    o.cigar_m = argv[4][0] == '1';
    o.secondary = argv[5][0] == '1';
    if (argv[6][0] == '1')
        for (std::size_t p = 0; p < pp.size(); ++p)
            o.names.push_back("pair." + std::to_string(p) + "/frag");
    std::vector<double> t_sam, t_bam, t_all;
    bool equal = true;
    for (int i = 0; i <= runs; ++i) {
        auto const a = clk::now();
        spm::jst_sam const s = spm::journaled_sequence_tree::sam_host(mapped, &pp, &rr, needles, 2, o);
        auto const m = clk::now();
        spm::jst_bam const f = spm::journaled_sequence_tree::bam_of_sam(s, b);
        auto const e = clk::now();
        t_sam.push_back(ms(a, m));
        t_bam.push_back(ms(m, e));
        t_all.push_back(ms(a, e));
        equal = equal && f.file.size() == want.size() && std::equal(want.begin(), want.end(), f.file.begin());
    }
    auto const median = [](std::vector<double> & t) {
        std::sort(t.begin() + 1, t.end());
        return t[1 + (t.size() - 1) / 2];
    };
    double const first = t_all[0];
    std::printf("{\"ms_host_route\": %.3f, \"ms_sam_host\": %.3f, \"ms_bam_of_sam\": %.3f, \"ms_first\": %.3f, \"ms_host_structs\": %.3f, "
                "\"equal_to_device\": %s}\n",
                median(t_all), median(t_sam), median(t_bam), first, ms_structs, equal ? "true" : "false");
    return equal ? 0 : 1;
}
