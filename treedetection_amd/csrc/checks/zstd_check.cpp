// The host instantiation of zstd_core.h (td_tiff_zstd_decode, and zstd_single_frame<1>: the rules the kernel applies to a block) under
// AddressSanitizer + UBSan in a program of its own: `make -C treedetection_amd/csrc zstd-check`. Arguments: manifest.json, then every
// .zst file of tests/golden/zstd — the streams libzstd wrote and the hand-built frames (hand_*.zst). Per file: the undamaged stream
// reproduces its recorded length and SHA-256 (a frame recorded as refused is refused); EVERY prefix of it and ZSTD_CHECK_FLIPS (4 000)
// single-bit flips return, with no report from the sanitizers — streams and outputs lie in heap buffers of their exact size, so a
// byte read or written outside src[0, n) or dst[0, cap) is a report — and the block rules agree with the host wrapper case by case
// (0 ↔ the same bytes, 1 ↔ TD_ERR_INVALID, 2 ↔ TD_ERR_CAPACITY; 4 = declined, the wrapper decides). The flipped bits come from the
// generator tests/zstd_cases.py:flip_bits restates, so the damaged streams the GPU tests feed to the kernel are among these; the
// capacities are the GPU tests' too: the stream's own length, ZSTD_CHECK_SMALL_CAP as well for the streams of up to that many bytes (some decode to more), and
// ZSTD_CHECK_HAND_CAP for the hand-built frames. The work is spread over the machine's threads (16 at the most).
#include "../common.h"
#include "../zstd_core.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr int ZSTD_CHECK_FLIPS = 4000;
constexpr int64_t ZSTD_CHECK_SMALL_CAP = 20000, ZSTD_CHECK_HAND_CAP = 300000;
std::atomic<long> g_calls{0}, g_accepted{0}, g_declined{0};

[[noreturn]] void fail(const std::string& file, const char* what, long long a = 0, long long b = 0) {
    std::fprintf(stderr, "zstd_check: %s: %s (%lld, %lld)\n", file.c_str(), what, a, b);
    std::exit(1);
}

// SHA-256 (FIPS 180-4)
std::string sha256(const uint8_t* data, size_t n) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
        0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
        0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
        0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
        0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
        0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    std::vector<uint8_t> m(data, data + n);
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int i = 7; i >= 0; --i) m.push_back((uint8_t)(((uint64_t)n * 8) >> (8 * i)));
    auto rotr = [](uint32_t v, int r) { return (v >> r) | (v << (32 - r)); };
    for (size_t off = 0; off < m.size(); off += 64) {
        uint32_t w[64];
        for (int i = 0; i < 16; ++i)
            w[i] = (uint32_t)m[off + 4 * i] << 24 | (uint32_t)m[off + 4 * i + 1] << 16 | (uint32_t)m[off + 4 * i + 2] << 8 | (uint32_t)m[off + 4 * i + 3];
        for (int i = 16; i < 64; ++i)
            w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
            const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    char out[65];
    for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
}

std::vector<uint8_t> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) fail(path, "cannot open");
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// the manifest's "length" and "sha256" of the entry whose "file" is `base` (they follow it in the entry)
void recorded(const std::string& manifest, const std::string& base, long long* length, std::string* sha) {
    const size_t at = manifest.find("\"file\": \"" + base + "\"");
    if (at == std::string::npos) fail(base, "not in the manifest");
    const size_t l = manifest.find("\"length\": ", at), s = manifest.find("\"sha256\": \"", at);
    if (l == std::string::npos || s == std::string::npos) fail(base, "manifest entry without length / sha256");
    *length = std::atoll(manifest.c_str() + l + 10);             // -1: a frame that must be refused
    *sha = *length < 0 ? std::string() : manifest.substr(s + 11, 64);
}

// one stream (damaged or not) through both entry points, in exact-size heap buffers
int64_t run(const std::string& file, const uint8_t* bytes, size_t n, int64_t cap, std::vector<uint8_t>* keep = nullptr) {
    std::unique_ptr<uint8_t[]> src(new uint8_t[n ? n : 1]), dst(new uint8_t[cap ? cap : 1]), dst2(new uint8_t[cap ? cap : 1]);
    std::memcpy(src.get(), bytes, n);
    const int64_t r = td_tiff_zstd_decode(src.get(), (int64_t)n, dst.get(), cap);
    ++g_calls;
    if (r > cap || (r < 0 && r != TD_ERR_INVALID && r != TD_ERR_CAPACITY)) fail(file, "td_tiff_zstd_decode returns", r, cap);
    static thread_local ZstdScratch S;
    static thread_local std::unique_ptr<uint8_t[]> lit(new uint8_t[ZSTD_BLOCK_MAX + ZSTD_LIT_PAD]);
    const ZstdResult b = zstd_single_frame<1>(S, src.get(), (int64_t)n, dst2.get(), (uint32_t)cap, lit.get(), 0);
    if (b.status == 4) ++g_declined;
    else if (b.status == 0) {
        if (r != (int64_t)b.produced || std::memcmp(dst.get(), dst2.get(), (size_t)r) != 0) fail(file, "block rules: status 0, the wrapper disagrees", r, b.produced);
    } else if (b.status == 1) {
        if (n != 0 && r != TD_ERR_INVALID) fail(file, "block rules: status 1, the wrapper says", r);
    } else if (b.status == 2) {
        if (r != TD_ERR_CAPACITY || b.produced <= (uint32_t)cap) fail(file, "block rules: status 2, the wrapper says", r, b.produced);
    } else {
        fail(file, "block rules: status", b.status);
    }
    if (r >= 0) ++g_accepted;
    if (keep && r >= 0) keep->assign(dst.get(), dst.get() + r);
    return r;
}

struct File {
    std::string base;
    std::vector<uint8_t> stream;
    long long length;                     // what it decodes to; -1: refused
    int64_t cap, small_cap;               // the capacities every damaged form of it is run with (small_cap 0: none)
    std::vector<size_t> flips;            // bit positions
};

// the undamaged stream, and what its damaged forms will be run with
File open_file(const std::string& manifest, const std::string& path) {
    File f;
    f.base = path.substr(path.find_last_of('/') + 1);
    std::string sha;
    recorded(manifest, f.base, &f.length, &sha);
    f.stream = read_file(path);
    const bool hand = f.base.compare(0, 5, "hand_") == 0;
    f.cap = hand ? ZSTD_CHECK_HAND_CAP : f.length;
    const size_t n = f.stream.size();
    f.small_cap = !hand && f.length != ZSTD_CHECK_SMALL_CAP && n <= (size_t)ZSTD_CHECK_SMALL_CAP ? ZSTD_CHECK_SMALL_CAP : 0;
    std::vector<uint8_t> out;
    const int64_t r = run(f.base, f.stream.data(), n, f.cap, &out);
    if (f.length < 0) {
        if (r != TD_ERR_INVALID) fail(f.base, "a frame recorded as refused returns", r);
    } else {
        if (r != f.length) fail(f.base, "undamaged stream: length", f.length, r);
        if (sha256(out.data(), out.size()) != sha) fail(f.base, "undamaged stream: SHA-256 differs");
        if (f.length > 0 && run(f.base, f.stream.data(), n, f.length - 1) != TD_ERR_CAPACITY) fail(f.base, "capacity - 1 accepted");
    }
    uint64_t seed = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;          // tests/zstd_cases.py:flip_bits is this sequence
    for (int k = 0; k < ZSTD_CHECK_FLIPS; ++k) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        f.flips.push_back((size_t)((seed >> 24) % (n * 8)));
    }
    return f;
}

void run_caps(const File& f, const uint8_t* bytes, size_t n) {
    run(f.base, bytes, n, f.cap);
    if (f.small_cap) run(f.base, bytes, n, f.small_cap);
}

struct Task { const File* f; bool flips; size_t lo, hi; };        // prefixes [lo, hi) or flips [lo, hi)

void work(const std::vector<Task>& tasks, std::atomic<size_t>& next) {
    for (size_t t = next.fetch_add(1); t < tasks.size(); t = next.fetch_add(1)) {
        const Task& k = tasks[t];
        if (!k.flips) {
            for (size_t cut = k.lo; cut < k.hi; ++cut) run_caps(*k.f, k.f->stream.data(), cut);
        } else {
            std::vector<uint8_t> bad(k.f->stream);
            for (size_t i = k.lo; i < k.hi; ++i) {
                const size_t bit = k.f->flips[i];
                bad[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
                run_caps(*k.f, bad.data(), bad.size());
                bad[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
            }
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: zstd_check manifest.json stream.zst ...\n");
        return 2;
    }
    const std::vector<uint8_t> m = read_file(argv[1]);
    const std::string manifest(m.begin(), m.end());
    std::vector<File> files;
    for (int i = 2; i < argc; ++i) files.push_back(open_file(manifest, argv[i]));
    std::sort(files.begin(), files.end(), [](const File& a, const File& b) { return a.stream.size() > b.stream.size(); });      // the long ones first
    std::vector<Task> tasks;
    long prefixes = 0;
    for (const File& f : files) {
        const size_t n = f.stream.size();
        for (size_t lo = 0; lo < n; lo += 256) tasks.push_back({&f, false, lo, std::min(n, lo + 256)});      // every prefix: cuts 0 .. n - 1
        for (size_t lo = 0; lo < f.flips.size(); lo += 100) tasks.push_back({&f, true, lo, std::min(f.flips.size(), lo + 100)});
        prefixes += (long)n;
    }
    std::atomic<size_t> next{0};
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = hw < 1 ? 1 : (hw > 16 ? 16 : hw);
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work, std::cref(tasks), std::ref(next));
    work(tasks, next);
    for (auto& t : pool) t.join();
    std::printf("zstd_check: %d files, %ld prefixes (every one) and %d flips each, %ld calls (%ld accepted, %ld declined by the block rules), no sanitizer report\n",
                argc - 2, prefixes, ZSTD_CHECK_FLIPS, g_calls.load(), g_accepted.load(), g_declined.load());
    return 0;
}
