// Zstandard on a host thread (TIFF compression 50000): the decoder the GPU runs (zstd_core.h, one wave per block), instantiated for ONE
// lane — the tile reader's block decoder, and the same source as the kernel, so that its parity with libzstd is tested without a GPU
// (tests/test_zstd_decode.py). What only the host does: walking concatenated frames, skipping skippable frames, and verifying a content
// checksum (the low 32 bits of XXH64, seed 0, over the frame's output). libtiff writes none of these; the device declines them.
// Pure host code; called from the reader's decode threads with the GIL released.
#include "common.h"
#include "zstd_core.h"

#include <cstring>
#include <vector>

namespace {

uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }
uint64_t read64(const uint8_t* p) {
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
    return v;
}
uint32_t read32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// XXH64 (the xxHash specification, 64-bit variant), seed 0
uint64_t xxh64(const uint8_t* p, uint64_t len) {
    constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull,
                       P5 = 0x27D4EB2F165667C5ull;
    auto round = [&](uint64_t acc, uint64_t in) { return rotl64(acc + in * P2, 31) * P1; };
    auto merge = [&](uint64_t h, uint64_t v) { return (h ^ round(0, v)) * P1 + P4; };
    const uint8_t* end = p + len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = P1 + P2, v2 = P2, v3 = 0, v4 = 0 - P1;
        for (; end - p >= 32; p += 32) {
            v1 = round(v1, read64(p));
            v2 = round(v2, read64(p + 8));
            v3 = round(v3, read64(p + 16));
            v4 = round(v4, read64(p + 24));
        }
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = merge(merge(merge(merge(h, v1), v2), v3), v4);
    } else {
        h = P5;
    }
    h += len;
    for (; end - p >= 8; p += 8) h = rotl64(h ^ round(0, read64(p)), 27) * P1 + P4;
    if (end - p >= 4) {
        h = rotl64(h ^ (read32(p) * P1), 23) * P2 + P3;
        p += 4;
    }
    for (; p < end; ++p) h = rotl64(h ^ (*p * P5), 11) * P1;
    h ^= h >> 33;
    h *= P2;
    h ^= h >> 29;
    h *= P3;
    h ^= h >> 32;
    return h;
}

// every frame of src[0, n) → dst[0, cap): bytes produced or a negative status
int64_t zstd_host(const char* what, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int64_t* stats) {
    if (!src || !dst || n < 0 || cap < 0 || cap >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) {
        td_set_error("%s: bad argument", what);
        return TD_ERR_INVALID;
    }
    static thread_local ZstdScratch scratch;
    static thread_local std::vector<uint8_t> lit(ZSTD_BLOCK_MAX + ZSTD_LIT_PAD);
    int64_t pos = 0, total = 0;
    while (pos < n) {
        if (n - pos < 4) {
            td_set_error("%s: corrupt stream (%lld bytes after the last frame)", what, (long long)(n - pos));
            return TD_ERR_INVALID;
        }
        const uint32_t magic = read32(src + pos);
        if ((magic & 0xFFFFFFF0u) == ZSTD_SKIP_MAGIC) {
            if (n - pos < 8 || (int64_t)read32(src + pos + 4) > n - pos - 8) {
                td_set_error("%s: corrupt stream (skippable frame longer than the stream)", what);
                return TD_ERR_INVALID;
            }
            if (stats) ++stats[ZS_SKIPPABLE];
            pos += 8 + (int64_t)read32(src + pos + 4);
            continue;
        }
        const ZstdResult r = zstd_frame<1>(scratch, src + pos, n - pos, dst + total, (uint32_t)(cap - total), lit.data(), 0, true, stats);
        if (r.status == 2) {
            td_set_error("%s: more than %lld bytes decoded, capacity %lld", what, (long long)(total + r.produced - 1), (long long)cap);
            return TD_ERR_CAPACITY;
        }
        if (r.status != 0) {
            td_set_error("%s: corrupt stream", what);
            return TD_ERR_INVALID;
        }
        if (r.has_checksum && (uint32_t)xxh64(dst + total, r.produced) != r.checksum) {
            td_set_error("%s: content checksum mismatch", what);
            return TD_ERR_INVALID;
        }
        total += r.produced;
        pos += r.end;
    }
    return total;
}

}  // namespace

extern "C" int64_t td_tiff_zstd_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap) {
    return zstd_host("td_tiff_zstd_decode", src, n, dst, cap, nullptr);
}

// What a stream is made of (the fixture generator and the coverage test): counters[TD_ZSTD_STATS] in the order of ZstdStat (zstd_core.h).
// → bytes the stream decodes to, or a negative status (the counters then cover what was read before the error).
extern "C" int64_t td_zstd_stream_stats(const uint8_t* src, int64_t n, int64_t* counters) {
    if (!src || !counters || n < 0) {
        td_set_error("td_zstd_stream_stats: bad argument");
        return TD_ERR_INVALID;
    }
    static_assert(ZS_COUNT == TD_ZSTD_STATS, "counter list and header out of sync");
    for (int64_t cap = 1 << 20;; cap *= 4) {                       // (the output is not kept: grow until it fits)
        std::vector<uint8_t> out((size_t)cap);
        std::memset(counters, 0, sizeof(int64_t) * ZS_COUNT);
        const int64_t r = zstd_host("td_zstd_stream_stats", src, n, out.data(), cap, counters);
        if (r != TD_ERR_CAPACITY || cap >= ((int64_t)1 << 30)) return r;
    }
}
