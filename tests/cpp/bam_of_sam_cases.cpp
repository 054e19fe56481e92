// bam_of_sam_cases.cpp -- the host route's SAM-to-BAM converter (journaled_sequence_tree::bam_of_sam) without a device: SAM
// lines written out by hand here go in, the file goes to argv[1] and the lines to argv[2]; tests/test_jst_bam_cpp.py decodes the
// file with tests/bam_decode.py and wants the lines back.
#include <cstdio>
#include <fstream>
#include <string>

#include <libspm/jst/journaled_sequence_tree.hpp>

int main(int argc, char ** argv)
{
    if (argc != 4)
        return 2;
    char const * const lines[] = {
        "7\t16\tchr\t100\t40\t20=1X11=\t*\t0\t0\tACGTACGTACGTACGTACGTACGTACGTACGT\t*\tNM:i:1\tXH:i:0\tXN:i:2\tX0:i:1\tX1:i:1\n",
        "p0\t99\tchr\t1001\t60\t30M\t=\t1171\t200\tACGTACGTACGTACGTACGTACGTACGTAC\t*\tNM:i:0\tXH:i:0\tXN:i:1\tX0:i:1\tX1:i:0\n",
        "p0\t147\tchr\t1171\t3\t10=4X16=\t=\t1001\t-200\tGGGGGGGGGGGGGGGGGGGGGGGGGGGGGG\t*\tNM:i:4\tXR:i:1\tX0:i:2\tX1:i:0\n",
        "p1\t73\tchr\t501\t60\t5=1I2=1D3=\t=\t501\t0\tACGTNACGTAC\t*\tNM:i:2\tXH:i:-1\tXN:i:4294967295\tX0:i:4294967295\tX1:i:0\n",
        "p1\t133\tchr\t501\t0\t*\t=\t501\t0\tACG\t*\n",
        "p1\t393\tchr\t16384\t255\t3I\t=\t501\t0\t*\t*\tNM:i:3\tXH:i:3\tXN:i:1\n",
        "9\t4\t*\t0\t0\t*\t*\t0\t0\tT\t*\n",
        "10\t0\tchr\t16383\t60\t2=\t*\t0\t0\tAC\t*\tNM:i:0\tXH:i:0\tXN:i:1\tX0:i:1\tX1:i:0\n",
    };
    spm::jst_sam sam;
    for (char const * l : lines) {
        std::string const s = l;
        sam.lines.push_back({sam.text.size(), static_cast<std::uint32_t>(s.size()), static_cast<std::uint32_t>(sam.lines.size()), 0, 0, 0, 0});
        sam.text += s;
    }
    spm::jst_bam_options o;
    o.sam.rname = "chr";
    o.ref_len = 20000;
    o.block_data = static_cast<std::uint32_t>(std::stoul(argv[3]));
    spm::jst_bam const bam = spm::journaled_sequence_tree::bam_of_sam(sam, o);
    std::ofstream(argv[1], std::ios::binary).write(bam.file.data(), static_cast<std::streamsize>(bam.file.size()));
    std::ofstream(argv[2], std::ios::binary).write(sam.text.data(), static_cast<std::streamsize>(sam.text.size()));
    std::uint64_t end = 0;
    for (std::size_t i = 0; i < bam.lines.size(); ++i) {
        if (bam.lines[i].offset != end)
            return 1;
        end += bam.lines[i].len;
        std::printf("%llu\n", static_cast<unsigned long long>(bam.virtual_offset(i, o.block_data)));
    }
    return end == bam.records.size() && bam.lines.size() == sam.lines.size() ? 0 : 1;
}
