// scratch_layout_cases.cpp -- how a call carves its arrays out of one scratch buffer (scratch_layout,
// libspm_amd/csrc/scratch_layout.hpp) without a device: every slice on a 256-byte boundary, no two slices overlapping,
// zero-size takes that cost nothing, bytes() as the end of the last slice, and the offsets of one real driver
// (select_run, select.hip) for 257 records, written out by hand -- as byte takes and as the typed takes the drivers state
// (take(pointer, count), then bind(base)): a typed take is the byte take of count * sizeof(element), for every element size.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../libspm_amd/csrc/scratch_layout.hpp"

using namespace spm_hip;

static int failures = 0, checks = 0;
#define EXPECT_TRUE(cond)                                                                                              \
    do {                                                                                                               \
        ++checks;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            ++failures;                                                                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                                              \
        }                                                                                                              \
    } while (0)

static void empty_layout()
{
    scratch_layout L;
    EXPECT_TRUE(L.bytes() == 0);
    EXPECT_TRUE(L.take(0) == 0);
    EXPECT_TRUE(L.bytes() == 0);
}

// sizes around the boundary, zero-size takes in between: alignment, no overlap, bytes()
static void slices_cases()
{
    const size_t sizes[] = {1, 0, 255, 256, 257, 0, 0, 511, 512, 513, 16, 0, 4096, 100000, 1};
    scratch_layout L;
    std::vector<size_t> at, len;
    for (size_t s : sizes) {
        const size_t before = L.bytes();
        const size_t o = L.take(s);
        at.push_back(o);
        len.push_back(s);
        EXPECT_TRUE(o % 256 == 0);
        EXPECT_TRUE(o == before);              // a slice begins where the layout ended
        EXPECT_TRUE(L.bytes() % 256 == 0);
        EXPECT_TRUE(L.bytes() >= o + s);       // ... and lies inside it
        EXPECT_TRUE(L.bytes() - (o + s) < 256); // ... with less than one boundary of padding
        if (s == 0)
            EXPECT_TRUE(L.bytes() == before);  // a zero-size take adds nothing
    }
    for (size_t i = 0; i < at.size(); ++i)
        for (size_t j = i + 1; j < at.size(); ++j) {
            EXPECT_TRUE(at[i] <= at[j]);
            if (len[i] && len[j])
                EXPECT_TRUE(at[i] + len[i] <= at[j]); // no two slices share a byte
            if (len[i] == 0 && j == i + 1)
                EXPECT_TRUE(at[i] == at[j]);          // a zero-size take shares its offset with its successor
        }
    // bytes() is the end of the last slice, rounded up to the boundary
    const size_t last = at.size() - 1;
    EXPECT_TRUE(L.bytes() == ((at[last] + len[last] + 255) & ~size_t(255)));
    EXPECT_TRUE(L.bytes() == 256 + 256 + 256 + 512 + 512 + 512 + 768 + 256 + 4096 + 100096 + 256);
}

// at(): base + offset as a typed pointer
static void pointer_cases()
{
    alignas(256) static unsigned char buf[1024];
    scratch_layout L;
    const size_t a = L.take(8), b = L.take(300), c = L.take(4);
    EXPECT_TRUE((void *)scratch_layout::at<uint64_t>(buf, a) == (void *)buf);
    EXPECT_TRUE((void *)scratch_layout::at<uint32_t>(buf, b) == (void *)(buf + 256));
    EXPECT_TRUE((void *)L.at<int32_t>(buf, c) == (void *)(buf + 768));
    *L.at<int32_t>(buf, c) = -7;
    EXPECT_TRUE(*reinterpret_cast<int32_t *>(buf + 768) == -7);
    EXPECT_TRUE(L.bytes() == 1024);
}

// select_run's takes for n = 257 records: keys twice (8 bytes each), indices twice (4), keep flags (1), scores (4), offsets
// (4), the per-pattern minima (BEST only), the segment table (segmented sources only), 16 bytes of counts, hipcub's temporary.
// 257 * 8 = 2056 -> 2304; 257 * 4 = 1028 -> 1280; 257 -> 512.
static void select_run_cases()
{
    const size_t n = 257;
    for (int variant = 0; variant < 3; ++variant) {
        const bool best = variant >= 1;
        const size_t n_patterns = 3, n_segs = variant == 2 ? 70 : 0, tmp_bytes = 1000;
        scratch_layout L;
        const size_t o_keys0 = L.take(n * 8), o_keys1 = L.take(n * 8), o_idx0 = L.take(n * 4), o_idx1 = L.take(n * 4),
                     o_keep = L.take(n), o_score = L.take(n * 4), o_offs = L.take(n * 4), o_min = L.take(best ? n_patterns * 4 : 0),
                     o_segs = L.take(n_segs ? (n_segs + 1) * 8 : 0), o_counts = L.take(16), o_tmp = L.take(tmp_bytes);
        EXPECT_TRUE(o_keys0 == 0);
        EXPECT_TRUE(o_keys1 == 2304);
        EXPECT_TRUE(o_idx0 == 4608);
        EXPECT_TRUE(o_idx1 == 5888);
        EXPECT_TRUE(o_keep == 7168);
        EXPECT_TRUE(o_score == 7680);
        EXPECT_TRUE(o_offs == 8960);
        EXPECT_TRUE(o_min == 10240);
        if (variant == 0) { // neither minima nor segments: three takes share an offset
            EXPECT_TRUE(o_segs == 10240 && o_counts == 10240 && o_tmp == 10496 && L.bytes() == 11520);
        } else if (variant == 1) { // 12 bytes of minima -> 256
            EXPECT_TRUE(o_segs == 10496 && o_counts == 10496 && o_tmp == 10752 && L.bytes() == 11776);
        } else { // ... and 71 * 8 = 568 bytes of segment table -> 768
            EXPECT_TRUE(o_segs == 10496 && o_counts == 11264 && o_tmp == 11520 && L.bytes() == 12544);
        }
    }
}

// the typed take: n elements of T are n * sizeof(T) bytes, whatever T and n
struct rec16
{
    uint64_t a, b;
};
template <class T> static void typed_sizes_cases()
{
    const size_t counts[] = {0, 1, 63, 64, 65, 257};
    scratch_layout typed, bytes;
    T *p[6] = {};
    for (int i = 0; i < 6; ++i) {
        EXPECT_TRUE(typed.take(p[i], counts[i]) == bytes.take(counts[i] * sizeof(T)));
        EXPECT_TRUE(typed.bytes() == bytes.bytes());
    }
}

// zero-count typed takes share their offset, and after bind() their pointer, with the take that follows; bind() points every
// pointer at base + its offset, in the pointer's own type (const element types too)
static void typed_bind_cases()
{
    alignas(256) static unsigned char buf[2048];
    uint64_t *keys = nullptr;
    const uint32_t *none = nullptr;
    uint8_t *flags = nullptr, *none8 = nullptr;
    rec16 *recs = nullptr;
    int32_t *last = nullptr;
    scratch_layout L;
    const size_t o_keys = L.take(keys, 3), o_none = L.take(none, 0), o_flags = L.take(flags, 257), o_none8 = L.take(none8, 0),
                 o_recs = L.take(recs, 17), o_last = L.take(last, 1);
    EXPECT_TRUE(o_keys == 0 && o_none == 256 && o_flags == 256 && o_none8 == 768 && o_recs == 768 && o_last == 1280);
    EXPECT_TRUE(L.bytes() == 1536);
    EXPECT_TRUE(keys == nullptr && last == nullptr); // nothing is bound before bind()
    L.bind(buf);
    EXPECT_TRUE((void *)keys == (void *)(buf + o_keys));
    EXPECT_TRUE((const void *)none == (const void *)(buf + o_none) && (const void *)none == (const void *)flags);
    EXPECT_TRUE((void *)flags == (void *)(buf + o_flags));
    EXPECT_TRUE((void *)none8 == (void *)recs && (void *)recs == (void *)(buf + o_recs));
    EXPECT_TRUE((void *)last == (void *)(buf + o_last));
    // the pointers are usable as what they are: the first and the last element of every slice
    keys[0] = keys[2] = ~0ull;
    flags[0] = flags[256] = 0xAB;
    recs[0] = recs[16] = rec16{1, 2};
    *last = -7;
    EXPECT_TRUE(*reinterpret_cast<int32_t *>(buf + 1280) == -7 && buf[256 + 256] == 0xAB && recs[16].b == 2);
    // a second bind moves them all
    L.bind(buf + 256);
    EXPECT_TRUE((void *)keys == (void *)(buf + 256) && (void *)last == (void *)(buf + 256 + o_last));
}

// select_run's takes as the driver states them now: the same offsets as the byte takes above
static void select_run_typed_cases()
{
    const size_t n = 257;
    for (int variant = 0; variant < 3; ++variant) {
        const bool best = variant >= 1;
        const size_t n_patterns = 3, n_segs = variant == 2 ? 70 : 0, tmp_bytes = 1000;
        unsigned long long *keys_in = nullptr, *keys = nullptr, *segs = nullptr, *counts = nullptr;
        uint32_t *idx_in = nullptr, *idx = nullptr, *offs = nullptr;
        uint8_t *keep = nullptr, *tmp = nullptr;
        int32_t *score = nullptr, *minima = nullptr;
        scratch_layout L;
        EXPECT_TRUE(L.take(keys_in, n) == 0);
        EXPECT_TRUE(L.take(keys, n) == 2304);
        EXPECT_TRUE(L.take(idx_in, n) == 4608);
        EXPECT_TRUE(L.take(idx, n) == 5888);
        EXPECT_TRUE(L.take(keep, n) == 7168);
        EXPECT_TRUE(L.take(score, n) == 7680);
        EXPECT_TRUE(L.take(offs, n) == 8960);
        EXPECT_TRUE(L.take(minima, best ? n_patterns : 0) == 10240);
        const size_t o_segs = L.take(segs, n_segs ? n_segs + 1 : 0), o_counts = L.take(counts, 2), o_tmp = L.take(tmp, tmp_bytes);
        if (variant == 0) {
            EXPECT_TRUE(o_segs == 10240 && o_counts == 10240 && o_tmp == 10496 && L.bytes() == 11520);
        } else if (variant == 1) {
            EXPECT_TRUE(o_segs == 10496 && o_counts == 10496 && o_tmp == 10752 && L.bytes() == 11776);
        } else {
            EXPECT_TRUE(o_segs == 10496 && o_counts == 11264 && o_tmp == 11520 && L.bytes() == 12544);
        }
        std::vector<unsigned char> buf(L.bytes());
        L.bind(buf.data());
        EXPECT_TRUE((void *)keys_in == (void *)buf.data() && (void *)tmp == (void *)(buf.data() + o_tmp));
        EXPECT_TRUE((void *)counts == (void *)(buf.data() + o_counts) && (void *)minima == (void *)(buf.data() + 10240));
        tmp[tmp_bytes - 1] = 1; // (the last byte of the last slice lies inside bytes(): the sanitised build checks it)
    }
}

int main()
{
    empty_layout();
    slices_cases();
    pointer_cases();
    select_run_cases();
    typed_sizes_cases<uint8_t>();
    typed_sizes_cases<uint32_t>();
    typed_sizes_cases<uint64_t>();
    typed_sizes_cases<rec16>();
    typed_bind_cases();
    select_run_typed_cases();
    std::printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
