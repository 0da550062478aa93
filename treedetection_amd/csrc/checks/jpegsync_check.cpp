// The many-lane JPEG entropy decoder (jpeg_core.h: jpeg_sync_walk / jpeg_sync_segment / jpeg_sync_dc, through jpegcodec.cpp:
// td_jpeg_decode_sync — the procedure one wave runs on the GPU, on emulated lanes) in a program of its own, built with AddressSanitizer +
// UBSan (`make jpegsync-check`): every buffer is a heap block of exactly the size the ABI states, so a read or write one byte outside
// it ends the run. Input: the streams of tests/golden/jpegsync and tests/golden/jpeg4 (*.jpg, Pillow's encoder). For each stream, with
// subsequences of 8, 32 and 128 bytes and 1, 3 and 64 lanes, td_jpeg_decode_sync must return what the sequential td_jpeg_decode returns
// — the same bytes, or the same error code —
//   1. for the stream itself (which must decode, in at most 64 rounds a window);
//   2. for every prefix of it (the settings taken in turn);
//   3. for 3 000 seeded single-bit flips anywhere in it, headers included (the settings taken in turn).
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

constexpr int SUBSEQ[3] = {8, 32, 128}, LANES[3] = {1, 3, 64};

[[noreturn]] void fail(const std::string& file, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    std::printf("jpegsync_check: %s: %s (%lld, %lld, %lld)\n", file.c_str(), what, a, b, c);
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

struct Result {
    int64_t n = 0;
    int32_t shape[3] = {};
};

// Both decoders on a heap copy of exactly n bytes, into heap blocks of exactly cap bytes. → true when they agree.
bool same(const uint8_t* src, size_t n, size_t cap, int subseq, int lanes, Result& seq, int64_t* stats) {
    std::unique_ptr<uint8_t[]> s(new uint8_t[n ? n : 1]), a(new uint8_t[cap]), b(new uint8_t[cap]);
    std::memcpy(s.get(), src, n);
    Result syn;
    seq.n = td_jpeg_decode(s.get(), (int64_t)n, a.get(), (int64_t)cap, seq.shape);
    syn.n = td_jpeg_decode_sync(s.get(), (int64_t)n, b.get(), (int64_t)cap, syn.shape, subseq, lanes, stats);
    if (seq.n != syn.n) return false;
    if (seq.n < 0) return true;
    return !std::memcmp(seq.shape, syn.shape, sizeof seq.shape) && !std::memcmp(a.get(), b.get(), (size_t)seq.n);
}

void check_file(const std::string& jpg) {
    const std::vector<uint8_t> stream = slurp(jpg);
    if (stream.size() < 4) fail(jpg, "cannot read the stream");
    // 1. the stream itself, every setting
    Result r;
    int64_t stats[4];
    size_t cap = 1 << 20;
    long long most = 0;
    for (int subseq : SUBSEQ)
        for (int lanes : LANES) {
            if (!same(stream.data(), stream.size(), cap, subseq, lanes, r, stats)) fail(jpg, "the decoders disagree on the stream", subseq, lanes, r.n);
            if (r.n <= 0) fail(jpg, "the stream does not decode", r.n);
            if (stats[1] < 1 || stats[0] < stats[1] || stats[2] > 64 || stats[2] > lanes || stats[3] > stats[1]) fail(jpg, "stats", stats[0], stats[1], stats[2]);
            if (stats[2] > most) most = stats[2];
            cap = (size_t)r.n;                             // from here on the output blocks have exactly the size of the image
        }
    if (td_jpeg_decode_sync(stream.data(), (int64_t)stream.size(), nullptr, 0, r.shape, 3, 64, nullptr) != TD_ERR_INVALID ||
        td_jpeg_decode_sync(stream.data(), (int64_t)stream.size(), nullptr, 0, r.shape, 32, 65, nullptr) != TD_ERR_INVALID)
        fail(jpg, "bad arguments accepted");
    // 2. every prefix
    int turn = 0;
    for (size_t cut = 0; cut < stream.size(); ++cut, ++turn) {
        if (!same(stream.data(), cut, cap, SUBSEQ[turn % 3], LANES[(turn / 3) % 3], r, nullptr)) fail(jpg, "the decoders disagree on a prefix", (long long)cut, r.n);
        if (r.n >= 0 && cut + 2 < stream.size()) fail(jpg, "a truncated stream decoded", (long long)cut);
    }
    // 3. bit flips
    std::mt19937 rng(20261018u + (unsigned)stream.size());
    std::vector<uint8_t> bad(stream);
    long long errors = 0, decoded = 0;
    for (int k = 0; k < 3000; ++k, ++turn) {
        const size_t pos = rng() % stream.size();
        bad[pos] ^= (uint8_t)(1u << (rng() % 8));
        if (!same(bad.data(), bad.size(), 1 << 20, SUBSEQ[turn % 3], LANES[(turn / 3) % 3], r, nullptr))
            fail(jpg, "the decoders disagree after a bit flip", (long long)pos, bad[pos], r.n);
        (r.n < 0 ? errors : decoded)++;
        bad[pos] = stream[pos];
    }
    if (errors == 0 || decoded == 0) fail(jpg, "the bit flips gave one outcome only", errors, decoded);
    std::printf("jpegsync_check: %s: %d x %d x %d, %zu bytes, at most %lld rounds a window; 3000 bit flips: %lld refused, %lld decoded\n", jpg.c_str(),
                r.shape[1], r.shape[0], r.shape[2], stream.size(), most, errors, decoded);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: jpegsync_check stream.jpg ...\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) check_file(argv[i]);
    std::printf("jpegsync_check: ok\n");
    return 0;
}
