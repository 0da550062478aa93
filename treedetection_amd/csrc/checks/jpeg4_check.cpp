// The four-component path of the JPEG core (jpeg_core.h mode 4, jpegcodec.cpp: td_jpeg_decode and td_tiff_jpeg_plan) in a program of its
// own, built with AddressSanitizer + UBSan (`make jpeg4-check`): every buffer is a heap block of exactly the size the ABI states, so a
// read or write one byte outside it ends the run. Input: the streams of tests/golden/jpeg4 (*.jpg, Pillow's CMYK encoder) and, beside
// each, the bytes it stores (*.raw, [h][w][4], Pillow's libjpeg).
//   1. td_jpeg_decode gives exactly those bytes; one byte of capacity less is TD_ERR_CAPACITY and writes nothing;
//   2. the plan takes the stream as one block of a four-band raster (mode 4, no transform, 4 * 64 coefficients per MCU), reports the
//      sizes it needs when given none, and refuses the block for one and three bands;
//   3. every prefix of the stream and 4 000 seeded single-bit flips anywhere in it (headers included) return a status or decode —
//      the sanitizers are the judge of what the decoder touched on the way.
// Exit status 0 and a final "ok" line on success; the first mismatch prints what differed and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../../../include/treedet.h"

namespace {

[[noreturn]] void fail(const std::string& file, const char* what, long long a = 0, long long b = 0) {
    std::printf("jpeg4_check: %s: %s (%lld, %lld)\n", file.c_str(), what, a, b);
    std::exit(1);
}

std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    if (FILE* f = std::fopen(path.c_str(), "rb")) {
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + n);
        std::fclose(f);
    }
    return v;
}

std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {       // a heap block of exactly n bytes
    std::unique_ptr<uint8_t[]> q(new uint8_t[n]);
    std::memcpy(q.get(), p, n);
    return q;
}

int64_t decode(const uint8_t* src, size_t n, uint8_t* dst, int64_t cap, int32_t* shape) {
    const auto s = exact(src, n);
    return td_jpeg_decode(s.get(), (int64_t)n, dst, cap, shape);
}

td_status plan(const uint8_t* src, size_t n, int bands, int width, int rows, int64_t* info, int64_t* segs, int64_t seg_cap, void* sets,
               int64_t set_cap, int64_t* totals) {
    const auto s = exact(src, n);
    const int64_t off = 0, len = (int64_t)n;
    const int32_t r = rows;
    return td_tiff_jpeg_plan(nullptr, 0, s.get(), &off, &len, 1, 2, bands, width, &r, info, segs, seg_cap, sets, set_cap, totals);
}

void check_file(const std::string& jpg) {
    const std::vector<uint8_t> stream = slurp(jpg), want = slurp(jpg.substr(0, jpg.size() - 4) + ".raw");
    if (stream.size() < 4 || want.empty()) fail(jpg, "cannot read the stream or its .raw");
    // 1. the bytes
    int32_t shape[3] = {};
    std::unique_ptr<uint8_t[]> out(new uint8_t[want.size()]);
    const int64_t n = decode(stream.data(), stream.size(), out.get(), (int64_t)want.size(), shape);
    if (n != (int64_t)want.size() || shape[2] != 4 || (int64_t)shape[0] * shape[1] * 4 != n) fail(jpg, "td_jpeg_decode", n, (long long)want.size());
    if (std::memcmp(out.get(), want.data(), want.size())) fail(jpg, "decoded bytes differ from the .raw");
    std::unique_ptr<uint8_t[]> small(new uint8_t[want.size() - 1]);
    std::memset(small.get(), 0x5a, want.size() - 1);
    if (decode(stream.data(), stream.size(), small.get(), (int64_t)want.size() - 1, shape) != TD_ERR_CAPACITY) fail(jpg, "capacity - 1 accepted");
    for (size_t i = 0; i + 1 < want.size(); ++i)
        if (small[i] != 0x5a) fail(jpg, "TD_ERR_CAPACITY wrote output", (long long)i);
    // 2. the plan
    const int h = shape[0], w = shape[1];
    const int64_t mcus = (int64_t)((w + 7) / 8) * ((h + 7) / 8);
    int64_t info[8], totals[4];
    if (plan(stream.data(), stream.size(), 4, w, h, info, nullptr, 0, nullptr, 0, totals) != TD_ERR_CAPACITY || totals[0] < 1 || totals[1] != 1)
        fail(jpg, "plan without room", totals[0], totals[1]);
    std::unique_ptr<int64_t[]> segs(new int64_t[(size_t)totals[0] * 4]);
    std::unique_ptr<uint8_t[]> sets(new uint8_t[TD_JPEG_TABSET_BYTES]);
    const int64_t nseg = totals[0];
    if (plan(stream.data(), stream.size(), 4, w, h, info, segs.get(), nseg, sets.get(), 1, totals) != TD_OK) fail(jpg, "plan");
    if (info[0] != 0 || info[2] != 4 || info[3] != 0 || info[4] != w || info[5] != h || totals[2] != mcus * 256 || totals[3] != 0)
        fail(jpg, "plan: block info", info[2], totals[2]);
    int64_t covered = 0;
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t* sg = segs.get() + s * 4;
        if (sg[0] < 0 || sg[1] < 0 || sg[0] + sg[1] > (int64_t)stream.size() || sg[2] != 0 || (sg[3] & 0xffffffff) != covered) fail(jpg, "plan: segment", s);
        covered += sg[3] >> 32;
    }
    if (covered != mcus) fail(jpg, "plan: the segments do not cover the MCUs", covered, mcus);
    for (int bands : {1, 3}) {
        if (plan(stream.data(), stream.size(), bands, w, h, info, segs.get(), nseg, sets.get(), 1, totals) != TD_OK || info[0] != 1 || totals[3] != 1)
            fail(jpg, "a four-component block planned for other bands", bands);
    }
    if (plan(stream.data(), stream.size(), 4, w + 1, h, info, segs.get(), nseg, sets.get(), 1, totals) != TD_OK || info[0] != 1) fail(jpg, "plan: block width");
    // 3. prefixes and bit flips
    long long errors = 0, decoded = 0;
    for (size_t cut = 0; cut < stream.size(); ++cut) {
        const int64_t r = decode(stream.data(), cut, out.get(), (int64_t)want.size(), shape);
        if (r >= 0 && cut + 2 < stream.size()) fail(jpg, "a truncated stream decoded", (long long)cut);
        plan(stream.data(), cut, 4, w, h, info, segs.get(), nseg, sets.get(), 1, totals);
    }
    std::mt19937 rng(20251018u + (unsigned)stream.size());
    std::vector<uint8_t> bad(stream);
    for (int k = 0; k < 4000; ++k) {
        const size_t pos = rng() % stream.size();
        bad[pos] ^= (uint8_t)(1u << (rng() % 8));
        const int64_t r = decode(bad.data(), bad.size(), out.get(), (int64_t)want.size(), shape);
        if (r >= 0 && (int64_t)shape[0] * shape[1] * shape[2] != r) fail(jpg, "shape and size disagree after a bit flip", (long long)pos);
        (r < 0 ? errors : decoded)++;
        for (int bands : {3, 4}) plan(bad.data(), bad.size(), bands, w, h, info, segs.get(), nseg, sets.get(), 1, totals);
        bad[pos] = stream[pos];
    }
    std::printf("jpeg4_check: %s: %d x %d, %lld segments; 4000 bit flips: %lld refused, %lld decoded\n", jpg.c_str(), w, h, (long long)nseg, errors,
                decoded);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: jpeg4_check stream.jpg ... (each with its .raw beside it)\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    std::printf("jpeg4_check: ok\n");
    return 0;
}
