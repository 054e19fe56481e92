// bam_of_sam_qual_md_cases.cpp -- the host route's SAM-to-BAM converter (journaled_sequence_tree::bam_of_sam) on lines that
// carry a QUAL field and an MD:Z: tag, without a device: lines written out by hand here go in, the file goes to argv[1] and the
// lines to argv[2]; tests/test_jst_sam_qual_md_cpp.py decodes the file and wants the lines back.
#include <fstream>
#include <string>

#include <libspm/jst/journaled_sequence_tree.hpp>

int main(int argc, char ** argv)
{
    if (argc != 3)
        return 2;
    char const * const lines[] = {
        "7\t16\tchr\t100\t40\t20=1X11=\t*\t0\t0\tTTTTTTTTTTTTTTTTTTTTATTTTTTTTTTT\t!\"#$%&'()*+,-./0123456789:;<=>?@\tNM:i:1\tMD:Z:20G11\tXH:i:0\tXN:i:2\tX0:i:1\tX1:i:1\n",
        "p0\t147\tchr\t1171\t3\t5=2X3=2D1X4=\t=\t1001\t-200\tGGGGGGGGGGGGGGG\t~~~~~}}}}}|||||\tNM:i:5\tMD:Z:5A0C3^GT0A4\tXR:i:1\tX0:i:2\tX1:i:0\n",
        "p1\t133\tchr\t501\t0\t*\t=\t501\t0\tACG\tIJK\n",
        "p1\t393\tchr\t16384\t255\t3I\t=\t501\t0\t*\t*\tNM:i:3\tMD:Z:0\tXH:i:3\tXN:i:1\n",
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
    spm::jst_bam const bam = spm::journaled_sequence_tree::bam_of_sam(sam, o);
    std::ofstream(argv[1], std::ios::binary).write(bam.file.data(), static_cast<std::streamsize>(bam.file.size()));
    std::ofstream(argv[2], std::ios::binary).write(sam.text.data(), static_cast<std::streamsize>(sam.text.size()));
    return bam.lines.size() == sam.lines.size() ? 0 : 1;
}
