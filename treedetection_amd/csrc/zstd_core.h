// Zstandard (RFC 8878) frames — the stream of TIFF compression 50000 strips and tiles (GDAL's COMPRESS=ZSTD) — decoded by ONE
// 64-lane wave per block on the GPU (zstddecode.hip) and, from the same source, by one host thread (zstdcodec.cpp: td_tiff_zstd_decode,
// NL = 1). Written from the format description; libzstd is the judge in the tests only (tests/test_zstd_decode.py).
// What runs how on the wave: the frame, block and section headers, the FSE table descriptions and the sequences are decoded by every
// lane alike (the stream is sequential; values that come out of memory or LDS at a wave-uniform address are declared uniform, as in
// inflate_core.h); tables are built by lane 0; the (up to) four Huffman streams of a literals section are decoded by four lanes into a
// literal buffer in memory (up to 128 KB: it does not fit LDS beside other waves); literal runs and matches are copied by the whole
// wave, 64 bytes per step, a match out of the block's own earlier output in memory, behind a wait for this wave's stores.
// One frame per call. A content checksum is only parsed here (the host wrapper verifies it; the device declines such a block), and so
// are further frames and skippable frames (the host wrapper walks them).
#pragma once
#include <cstdint>
#include "inflate_core.h"                 // TD_INF_SYNC / TD_INF_STORES_DONE / TD_INF_LOAD_OUT / TD_INF_UNIFORM / TD_INF_HD

constexpr uint32_t ZSTD_MAGIC = 0xFD2FB528u, ZSTD_SKIP_MAGIC = 0x184D2A50u;        // (skippable: the low four bits are free)
constexpr uint32_t ZSTD_BLOCK_MAX = 128u << 10;
constexpr int ZSTD_HUF_LOG = 11;          // Huffman codes of at most 11 bits (RFC 8878 4.2.1)
constexpr int ZSTD_LL_LOG = 9, ZSTD_OF_LOG = 8, ZSTD_ML_LOG = 9, ZSTD_W_LOG = 6;     // most accuracy of each FSE table
constexpr int ZSTD_LL_MAX = 35, ZSTD_OF_MAX = 31, ZSTD_ML_MAX = 52;                // highest code of each kind
constexpr int ZSTD_LIT_PAD = 8;           // the literal buffer holds ZSTD_BLOCK_MAX + ZSTD_LIT_PAD bytes

// counters of td_zstd_stream_stats (host only; a null pointer everywhere else)
enum ZstdStat {
    ZS_FRAMES, ZS_BLOCK_RAW, ZS_BLOCK_RLE, ZS_BLOCK_COMP, ZS_MAX_BLOCKS_PER_FRAME, ZS_LIT_RAW, ZS_LIT_RLE, ZS_LIT_HUFF, ZS_LIT_TREELESS,
    ZS_LIT_STREAMS_1, ZS_LIT_STREAMS_4, ZS_HUFW_DIRECT, ZS_HUFW_FSE, ZS_SEQ0, ZS_LL_PREDEF, ZS_LL_RLE, ZS_LL_FSE, ZS_LL_REPEAT,
    ZS_OF_PREDEF, ZS_OF_RLE, ZS_OF_FSE, ZS_OF_REPEAT, ZS_ML_PREDEF, ZS_ML_RLE, ZS_ML_FSE, ZS_ML_REPEAT, ZS_WINDOW_DESC,
    ZS_SINGLE_SEGMENT, ZS_CHECKSUM, ZS_SEQ_LONG, ZS_SEQ_2BYTE, ZS_SKIPPABLE, ZS_COUNT
};

struct ZstdScratch {                      // LDS on the device (11.3 KB per wave), a plain struct on the host
    uint16_t huf[1 << ZSTD_HUF_LOG];      // Huffman lookup by the next bits of a stream: code length << 8 | symbol
    uint32_t fse[3][1 << ZSTD_LL_LOG];    // LL / OF / ML decoding tables by state: baseline << 16 | bits << 8 | symbol
    uint32_t wfse[1 << ZSTD_W_LOG];       // the table of FSE-compressed Huffman weights
    int16_t norm[256];                    // normalised counts of the table being built, then its per-symbol state counters
    uint8_t weights[256];                 // Huffman weights of the tree being built
};

// status: 0 ok, 1 corrupt, 2 more bytes than the block holds, 4 declined (a content checksum where the caller takes none).
// end: offset of the first byte after the frame (after its checksum, if it has one). checksum: the four bytes stored there.
struct ZstdResult {
    uint32_t produced;
    int status;
    uint32_t end;
    uint32_t has_checksum, checksum;
};
#define TD_ZSTD_CORRUPT return res       /* status 1: every rule that refuses a stream leaves through here */

#ifdef __HIPCC__
#define TD_ZSTD_MEMBER __host__ __device__ inline
#else
#define TD_ZSTD_MEMBER inline
#endif

namespace zstd_detail {

TD_INF_HD int highbit(uint32_t v) { return 31 - __builtin_clz(v); }           // (v != 0)

// byte i of the stream, 0 outside it
TD_INF_HD uint32_t byte_at(const uint8_t* p, int64_t n, int64_t i) { return i >= 0 && i < n ? (uint32_t)p[i] : 0u; }
template <bool UNI>
TD_INF_HD uint32_t le_bytes(const uint8_t* p, int64_t n, int64_t i, int count) {     // count <= 4 bytes from i, little-endian
    uint32_t v = 0;
    for (int k = 0; k < count; ++k) v |= byte_at(p, n, i + k) << (8 * k);
    return UNI ? TD_INF_UNIFORM(v) : v;
}

// A backward bit stream (RFC 8878 4.1): n bytes read from the last one down; `pos` = bits not yet consumed, counted from the stream's
// first byte. Bits below the first byte read as zeros and leave pos negative: every caller checks that. UNI: all lanes read the same
// stream (the container becomes a scalar); otherwise each lane has a stream of its own.
template <bool UNI>
struct BackBits {
    const uint8_t* p;
    int64_t n, pos;
    uint64_t acc;                         // the next bits, from bit 63 down
    int avail;                            // how many of them are there
    TD_ZSTD_MEMBER void refill() {
        const int64_t b = pos > 0 ? (pos + 7) >> 3 : 0;          // bytes [b - 8, b) end at or behind bit `pos`
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) v |= (uint64_t)byte_at(p, n, b - 8 + k) << (8 * k);
        v = pos > 0 ? v << (b * 8 - pos) : 0;
        if (UNI) v = ((uint64_t)TD_INF_UNIFORM(v >> 32) << 32) | TD_INF_UNIFORM((uint32_t)v);
        acc = v;
        avail = 57;
    }
    // false: no end mark (the last byte is zero) or no bytes
    TD_ZSTD_MEMBER bool init(const uint8_t* src, int64_t len) {
        p = src;
        n = len;
        pos = 0;
        acc = 0;
        avail = 0;
        if (len < 1) return false;
        const uint32_t last = UNI ? TD_INF_UNIFORM(src[len - 1]) : src[len - 1];
        if (!last) return false;
        pos = (len - 1) * 8 + highbit(last);
        refill();
        return true;
    }
    TD_ZSTD_MEMBER uint32_t peek(int nb) {      // nb <= 32
        if (nb > avail) refill();
        return nb ? (uint32_t)(acc >> (64 - nb)) : 0u;
    }
    TD_ZSTD_MEMBER void skip(int nb) {          // after a peek of at least nb bits
        acc <<= nb;
        avail -= nb;
        pos -= nb;
    }
    TD_ZSTD_MEMBER uint32_t read(int nb) {
        const uint32_t v = peek(nb);
        skip(nb);
        return v;
    }
};

// An FSE table description (RFC 8878 4.1.1) at src[0, n): normalised counts into S.norm (lane 0 writes; every lane decodes), → bytes
// used, 0 = corrupt. *log_out: the accuracy, *nsym_out: symbols described.
template <int NL>
TD_INF_HD int read_ncount(ZstdScratch& S, const uint8_t* src, int64_t n, int max_log, int max_sym, int* log_out, int* nsym_out, int lane) {
    uint32_t bit = 0;
    auto bits = [&](int nb) { return (le_bytes<true>(src, n, bit >> 3, 4) >> (bit & 7)) & ((1u << nb) - 1u); };     // nb <= 16: (bit & 7) + nb <= 23
    const int log = (int)bits(4) + 5;
    bit += 4;
    if (log > max_log) return 0;
    int remaining = (1 << log) + 1, threshold = 1 << log, nb = log + 1, sym = 0;
    bool prev0 = false;
    while (remaining > 1 && sym <= max_sym) {                     // ends: every turn adds a symbol, at most max_sym + 1 of them
        if (prev0) {
            for (;;) {                                            // ends: each turn of three zeros moves sym towards max_sym
                const int r = (int)bits(2);
                bit += 2;
                for (int k = 0; k < r && sym <= max_sym; ++k, ++sym)
                    if (lane == 0) S.norm[sym] = 0;
                if (r != 3 || sym > max_sym) break;
            }
            if (sym > max_sym) return 0;
        }
        const int max = 2 * threshold - 1 - remaining;
        const int v = (int)bits(nb);
        int count;
        if ((v & (threshold - 1)) < max) {
            count = v & (threshold - 1);
            bit += nb - 1;
        } else {
            count = v & (2 * threshold - 1);
            if (count >= threshold) count -= max;
            bit += nb;
        }
        --count;                                                  // -1: "less than one"
        remaining -= count < 0 ? 1 : count;
        if (remaining < 1) return 0;
        if (lane == 0) S.norm[sym] = (int16_t)count;
        ++sym;
        prev0 = count == 0;
        while (remaining < threshold && threshold > 1) {
            --nb;
            threshold >>= 1;
        }
    }
    if (remaining != 1 || sym > max_sym + 1) return 0;
    const int used = (int)((bit + 7) >> 3);
    if (used > n) return 0;
    *log_out = log;
    *nsym_out = sym;
    return used;
}

// The decoding table of S.norm[0, nsym) at accuracy `log` (RFC 8878 4.1.1; lane 0 only). false: the spread does not close.
TD_INF_HD bool build_fse(ZstdScratch& S, uint32_t* tab, int log, int nsym) {
    const int size = 1 << log;
    int high = size - 1;
    for (int s = 0; s < nsym; ++s)
        if (S.norm[s] == -1) {
            tab[high--] = (uint32_t)s;
            S.norm[s] = (int16_t)(1 | 0x4000);                    // its state counter starts at 1; marked: placed here, not by the spread
        }
    const int step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    int pos = 0;
    for (int s = 0; s < nsym; ++s) {
        const int c = S.norm[s];
        if (c & 0x4000) continue;
        for (int i = 0; i < c; ++i) {                             // the counts sum to `size` (read_ncount: remaining == 1)
            tab[pos] = (uint32_t)s;
            do pos = (pos + step) & mask; while (pos > high);
        }
    }
    if (pos != 0) return false;
    for (int s = 0; s < nsym; ++s) S.norm[s] &= 0x3fff;
    for (int u = 0; u < size; ++u) {
        const uint32_t s = tab[u];
        const uint32_t nx = (uint32_t)S.norm[s]++;
        const int nbits = log - highbit(nx);
        tab[u] = s | (uint32_t)nbits << 8 | ((nx << nbits) - (uint32_t)size) << 16;
    }
    return true;
}

// The Huffman lookup table of S.weights[0, nw) plus the implied last weight (RFC 8878 4.2.1; lane 0 only) → its log, 0 = corrupt
TD_INF_HD int build_huf(ZstdScratch& S, int nw) {
    uint32_t total = 0;
    for (int i = 0; i < nw; ++i) {
        const int w = S.weights[i];
        if (w > ZSTD_HUF_LOG) return 0;
        total += w ? 1u << (w - 1) : 0u;
    }
    if (total == 0) return 0;
    const int log = highbit(total) + 1;
    if (log > ZSTD_HUF_LOG) return 0;
    const uint32_t rest = (1u << log) - total;
    if (rest & (rest - 1)) return 0;                              // the last weight completes a power of two
    S.weights[nw] = (uint8_t)(highbit(rest) + 1);
    const int nsym = nw + 1;
    uint32_t start[ZSTD_HUF_LOG + 2], run = 0;
    for (int w = 1; w <= log; ++w) {                               // cells of weight w: after all those of lower weights
        start[w] = run;
        for (int i = 0; i < nsym; ++i)
            if (S.weights[i] == w) run += 1u << (w - 1);
    }
    for (int i = 0; i < nsym; ++i) {
        const int w = S.weights[i];
        if (!w) continue;
        const uint32_t len = 1u << (w - 1);
        const uint16_t e = (uint16_t)((log + 1 - w) << 8 | i);
        for (uint32_t k = 0; k < len; ++k) S.huf[start[w] + k] = e;         // start[w] + len <= 2^log: the weights sum to it
        start[w] += len;
    }
    return log;
}

// one Huffman stream of `count` symbols (a lane's own on the device) → false: corrupt (no end mark, bits left over or missing)
TD_INF_HD bool huf_stream(const ZstdScratch& S, int log, const uint8_t* src, int64_t len, uint8_t* out, uint32_t count) {
    BackBits<false> b;
    if (!b.init(src, len)) return false;
    for (uint32_t i = 0; i < count; ++i) {                        // ends at count (<= 128 KB); every symbol takes at least one bit
        const uint32_t e = S.huf[b.peek(log)];
        b.skip((int)(e >> 8));
        if (b.pos < 0) return false;                              // past the stream's first bit
        out[i] = (uint8_t)e;
    }
    return b.pos == 0;
}

#ifdef __HIP_DEVICE_COMPILE__
#define TD_ZSTD_ALL(ok) (TD_INF_UNIFORM(__all((int)(ok))) != 0)    // the lanes agree on what one (or four) of them found
#define TD_ZSTD_FROM0(v) (TD_INF_UNIFORM(__shfl((int)(v), 0)))
#else
#define TD_ZSTD_ALL(ok) (ok)
#define TD_ZSTD_FROM0(v) ((uint32_t)(v))
#endif
#define TD_ZSTD_STAT(i) do { if (NL == 1 && stats) ++stats[i]; } while (0)

}  // namespace zstd_detail

// One frame at src[0, n) (which begins with the magic number) → dst[0, cap). lit: ZSTD_BLOCK_MAX + ZSTD_LIT_PAD bytes for the literals
// of a block (memory of this wave's own on the device). Every lane of the wave calls this with its lane id (host: NL = 1, lane 0); the
// result is the same on every lane. take_checksum = false: a frame with a content checksum is declined (status 4) unread.
template <int NL>
TD_INF_HD TD_INF_INLINE ZstdResult zstd_frame(ZstdScratch& S, const uint8_t* src, int64_t n, uint8_t* dst, uint32_t cap, uint8_t* lit, int lane,
                                               bool take_checksum, int64_t* stats) {
    using namespace zstd_detail;
    // code → baseline | extra bits << 24 (RFC 8878 3.1.1.3.2.1.1)
    constexpr uint32_t LL_CODE[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 | 1 << 24, 18 | 1 << 24, 20 | 1 << 24, 22 | 1 << 24,
                                      24 | 2 << 24, 28 | 2 << 24, 32 | 3 << 24, 40 | 3 << 24, 48 | 4 << 24, 64 | 6 << 24, 128 | 7 << 24, 256 | 8 << 24,
                                      512 | 9 << 24, 1024 | 10 << 24, 2048 | 11 << 24, 4096 | 12 << 24, 8192 | 13 << 24, 16384 | 14 << 24,
                                      32768 | 15 << 24, 65536 | 16 << 24};
    constexpr uint32_t ML_CODE[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34,
                                      35 | 1 << 24, 37 | 1 << 24, 39 | 1 << 24, 41 | 1 << 24, 43 | 2 << 24, 47 | 2 << 24, 51 | 3 << 24, 59 | 3 << 24,
                                      67 | 4 << 24, 83 | 4 << 24, 99 | 5 << 24, 131 | 7 << 24, 259 | 8 << 24, 515 | 9 << 24, 1027 | 10 << 24,
                                      2051 | 11 << 24, 4099 | 12 << 24, 8195 | 13 << 24, 16387 | 14 << 24, 32771 | 15 << 24, 65539 | 16 << 24};
    // predefined distributions (RFC 8878 3.1.1.3.2.2): accuracy 6 / 5 / 6
    constexpr int8_t LL_DEF[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    constexpr int8_t OF_DEF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    constexpr int8_t ML_DEF[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                   1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    ZstdResult res{0, 1, 0, 0, 0};
    auto u8 = [&](int64_t i) { return TD_INF_UNIFORM(byte_at(src, n, i)); };

    // ---- frame header (RFC 8878 3.1.1.1)
    if (n < 6 || le_bytes<true>(src, n, 0, 4) != ZSTD_MAGIC) TD_ZSTD_CORRUPT;
    const uint32_t fhd = u8(4);
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1u, did_flag = fhd & 3u;
    if (fhd & 0x08u) TD_ZSTD_CORRUPT;                                   // the reserved bit
    const bool has_sum = (fhd & 0x04u) != 0;
    int64_t ip = 5;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wd = u8(ip++);
        const uint32_t wlog = 10 + (wd >> 3);
        if (wlog > 41) TD_ZSTD_CORRUPT;
        window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wd & 7u);
        TD_ZSTD_STAT(ZS_WINDOW_DESC);
    } else {
        TD_ZSTD_STAT(ZS_SINGLE_SEGMENT);
    }
    const int did_bytes = did_flag == 3 ? 4 : (int)did_flag;
    if (ip + did_bytes > n) TD_ZSTD_CORRUPT;
    if (did_bytes && le_bytes<true>(src, n, ip, did_bytes) != 0) TD_ZSTD_CORRUPT;      // a dictionary: unsupported
    ip += did_bytes;
    const int fcs_bytes = fcs_flag == 0 ? (int)single : (1 << fcs_flag);
    bool has_fcs = fcs_bytes != 0;
    uint64_t fcs = 0;
    if (ip + fcs_bytes > n) TD_ZSTD_CORRUPT;
    if (has_fcs) {
        fcs = le_bytes<true>(src, n, ip, fcs_bytes > 4 ? 4 : fcs_bytes);
        if (fcs_bytes == 8) fcs |= (uint64_t)le_bytes<true>(src, n, ip + 4, 4) << 32;
        if (fcs_bytes == 2) fcs += 256;
    }
    ip += fcs_bytes;
    if (single) window = fcs;
    if (has_sum) {
        TD_ZSTD_STAT(ZS_CHECKSUM);
        if (!take_checksum) {
            res.status = 4;
            return res;
        }
    }
    TD_ZSTD_STAT(ZS_FRAMES);
    const uint32_t block_max = window < ZSTD_BLOCK_MAX ? (uint32_t)window : ZSTD_BLOCK_MAX;

    // ---- the frame's state
    uint32_t rep0 = 1, rep1 = 4, rep2 = 8;
    int huf_log = 0;                                               // 0: no Huffman table yet
    int fse_log[3] = {-1, -1, -1};                                 // -1: no table yet (LL, OF, ML)
    uint32_t op = 0, flushed = 0;                                  // bytes produced; how many of them have surely reached memory
    int64_t frame_blocks = 0;

    for (;;) {                                                     // blocks. Ends: each takes three bytes of the stream at least
        if (ip + 3 > n) TD_ZSTD_CORRUPT;
        const uint32_t bh = le_bytes<true>(src, n, ip, 3);
        ip += 3;
        const uint32_t last = bh & 1u, btype = (bh >> 1) & 3u, bsize = bh >> 3;
        if (btype == 3 || bsize > block_max) TD_ZSTD_CORRUPT;
        ++frame_blocks;
        if (btype == 0) {                                          // Raw
            TD_ZSTD_STAT(ZS_BLOCK_RAW);
            if (ip + bsize > n) TD_ZSTD_CORRUPT;
            for (uint32_t k = (uint32_t)lane; k < bsize; k += NL)
                if (op + k < cap) dst[op + k] = src[ip + k];
            ip += bsize;
            op += bsize;
        } else if (btype == 1) {                                   // RLE
            TD_ZSTD_STAT(ZS_BLOCK_RLE);
            if (ip + 1 > n) TD_ZSTD_CORRUPT;
            const uint8_t v = (uint8_t)u8(ip);
            for (uint32_t k = (uint32_t)lane; k < bsize; k += NL)
                if (op + k < cap) dst[op + k] = v;
            ip += 1;
            op += bsize;
        } else {                                                   // Compressed
            TD_ZSTD_STAT(ZS_BLOCK_COMP);
            if (ip + bsize > n || bsize < 2) TD_ZSTD_CORRUPT;
            const uint8_t* bs = src + ip;                          // the block's content: bs[0, bn)
            const int64_t bn = bsize;
            auto b8 = [&](int64_t i) { return TD_INF_UNIFORM(byte_at(bs, bn, i)); };
            const uint32_t op0 = op;
            // -- literals section (RFC 8878 3.1.1.3.1)
            const uint32_t b0 = b8(0), ltype = b0 & 3u, sf = (b0 >> 2) & 3u;
            uint32_t lit_n = 0, lit_c = 0;
            int lh = 0, streams = 1;
            if (ltype < 2) {
                if (sf == 1) {
                    lh = 2;
                    lit_n = le_bytes<true>(bs, bn, 0, 2) >> 4;
                } else if (sf == 3) {
                    lh = 3;
                    lit_n = le_bytes<true>(bs, bn, 0, 3) >> 4;
                } else {
                    lh = 1;
                    lit_n = b0 >> 3;
                }
            } else {
                const int bits = sf < 2 ? 10 : (sf == 2 ? 14 : 18);
                lh = sf < 2 ? 3 : (sf == 2 ? 4 : 5);
                const uint64_t h = (uint64_t)le_bytes<true>(bs, bn, 0, 4) | (uint64_t)b8(4) << 32;
                lit_n = (uint32_t)(h >> 4) & ((1u << bits) - 1u);
                lit_c = (uint32_t)(h >> (4 + bits)) & ((1u << bits) - 1u);
                streams = sf == 0 ? 1 : 4;
            }
            if (lit_n > ZSTD_BLOCK_MAX || lh > bn) TD_ZSTD_CORRUPT;
            const uint8_t* lit_src = lit;                          // where the sequences take their literals from
            bool lit_rle = false, lit_mem = false;                 // one byte repeated / the literal buffer (read behind a store wait)
            uint32_t lit_byte = 0;
            int64_t sp = lh;                                       // position in the block's content
            if (ltype == 0) {
                TD_ZSTD_STAT(ZS_LIT_RAW);
                if (sp + lit_n > bn) TD_ZSTD_CORRUPT;
                lit_src = bs + sp;
                sp += lit_n;
            } else if (ltype == 1) {
                TD_ZSTD_STAT(ZS_LIT_RLE);
                if (sp + 1 > bn) TD_ZSTD_CORRUPT;
                lit_rle = true;
                lit_byte = b8(sp);
                sp += 1;
            } else {
                if (sp + lit_c > bn) TD_ZSTD_CORRUPT;
                const uint8_t* hs = bs + sp;                       // tree description (if any) + streams: hs[0, lit_c)
                int64_t hn = lit_c, hp = 0;
                if (ltype == 2) {                                  // a new tree (RFC 8878 4.2.1)
                    TD_ZSTD_STAT(ZS_LIT_HUFF);
                    if (hn < 1) TD_ZSTD_CORRUPT;
                    const uint32_t hb = TD_INF_UNIFORM(hs[0]);
                    hp = 1;
                    int nw = 0;
                    if (hb >= 128) {                               // weights as they are: four bits each
                        TD_ZSTD_STAT(ZS_HUFW_DIRECT);
                        nw = (int)hb - 127;
                        const int nbytes = (nw + 1) >> 1;
                        if (hp + nbytes > hn) TD_ZSTD_CORRUPT;
                        TD_INF_SYNC();
                        for (int i = lane; i < nw; i += NL) {
                            const uint32_t v = hs[hp + (i >> 1)];
                            S.weights[i] = (uint8_t)((i & 1) ? v & 15u : v >> 4);
                        }
                        hp += nbytes;
                    } else {                                       // FSE-compressed weights: two states in turn (RFC 8878 4.2.1.2)
                        TD_ZSTD_STAT(ZS_HUFW_FSE);
                        if (hb == 0 || hp + hb > hn) TD_ZSTD_CORRUPT;
                        int wlog = 0, wsym = 0;
                        TD_INF_SYNC();
                        const int used = read_ncount<NL>(S, hs + hp, hb, ZSTD_W_LOG, 255, &wlog, &wsym, lane);
                        if (!used) TD_ZSTD_CORRUPT;
                        TD_INF_SYNC();
                        bool ok = true;
                        if (lane == 0) ok = build_fse(S, S.wfse, wlog, wsym);
                        TD_INF_SYNC();
                        if (!TD_ZSTD_ALL(ok)) TD_ZSTD_CORRUPT;
                        BackBits<true> wb;
                        if (!wb.init(hs + hp + used, (int64_t)hb - used)) TD_ZSTD_CORRUPT;
                        uint32_t s1 = wb.read(wlog), s2 = wb.read(wlog);
                        if (wb.pos < 0) TD_ZSTD_CORRUPT;
                        // the states emit in turn; when updating one runs past the stream's first bit, the other emits once more
                        for (;;) {                                 // ends at 255 weights: every turn stores one
                            if (nw >= 254) TD_ZSTD_CORRUPT;             // (this one and the closing one: 255 at the most)
                            const uint32_t e = TD_INF_UNIFORM(S.wfse[s1]);
                            if (lane == 0) S.weights[nw] = (uint8_t)e;
                            ++nw;
                            s1 = s2;
                            s2 = (e >> 16) + wb.read((int)((e >> 8) & 255u));       // (the states swap roles each turn)
                            if (wb.pos < 0) {
                                if (lane == 0) S.weights[nw] = (uint8_t)TD_INF_UNIFORM(S.wfse[s1]);
                                ++nw;
                                break;
                            }
                        }
                        hp += hb;
                    }
                    TD_INF_SYNC();
                    int lg = 0;
                    if (lane == 0) lg = build_huf(S, nw);
                    TD_INF_SYNC();
                    huf_log = (int)TD_ZSTD_FROM0(lg);
                    if (!huf_log) TD_ZSTD_CORRUPT;
                } else {
                    TD_ZSTD_STAT(ZS_LIT_TREELESS);
                    if (!huf_log) TD_ZSTD_CORRUPT;                      // no tree to repeat
                }
                // the streams: one lane each, into the literal buffer
                if (streams == 1) TD_ZSTD_STAT(ZS_LIT_STREAMS_1);
                else TD_ZSTD_STAT(ZS_LIT_STREAMS_4);
                const int64_t left = hn - hp;
                if (left < 0) TD_ZSTD_CORRUPT;
                uint32_t l0 = (uint32_t)left, l1 = 0, l2 = 0, l3 = 0, seg = lit_n;      // stream lengths; symbols per stream (the last: the rest)
                if (streams == 4) {
                    if (left < 6) TD_ZSTD_CORRUPT;
                    seg = (lit_n + 3) >> 2;
                    if (3 * seg > lit_n) TD_ZSTD_CORRUPT;
                    l0 = le_bytes<true>(hs, hn, hp, 2);
                    l1 = le_bytes<true>(hs, hn, hp + 2, 2);
                    l2 = le_bytes<true>(hs, hn, hp + 4, 2);
                    if ((int64_t)6 + l0 + l1 + l2 > left) TD_ZSTD_CORRUPT;
                    l3 = (uint32_t)left - 6u - l0 - l1 - l2;
                }
                bool ok = true;
                // stream k: its bytes, its length, its first symbol's place, its symbols (selected, not indexed: no array for the lanes to index)
                auto run = [&](int k) {
                    const uint32_t at = streams == 1 ? 0u : 6u + (k > 0 ? l0 : 0u) + (k > 1 ? l1 : 0u) + (k > 2 ? l2 : 0u);
                    const uint32_t ln = k == 0 ? l0 : (k == 1 ? l1 : (k == 2 ? l2 : l3));
                    const uint32_t cn = k == 3 ? lit_n - 3 * seg : seg;
                    return huf_stream(S, huf_log, hs + hp + at, ln, lit + seg * (uint32_t)k, cn);
                };
#ifdef __HIP_DEVICE_COMPILE__
                if (lane < streams) ok = run(lane);
#else
                for (int k = 0; k < streams && ok; ++k) ok = run(k);
#endif
                if (!TD_ZSTD_ALL(ok)) TD_ZSTD_CORRUPT;
                TD_INF_STORES_DONE();
                lit_mem = true;
                sp += lit_c;
            }
            // -- sequences section (RFC 8878 3.1.1.3.2)
            if (sp + 1 > bn) TD_ZSTD_CORRUPT;
            uint32_t nseq = b8(sp++);
            if (nseq >= 128) {
                if (nseq == 255) {
                    if (sp + 2 > bn) TD_ZSTD_CORRUPT;
                    nseq = le_bytes<true>(bs, bn, sp, 2) + 0x7F00u;
                    sp += 2;
                    TD_ZSTD_STAT(ZS_SEQ_LONG);
                } else {
                    if (sp + 1 > bn) TD_ZSTD_CORRUPT;
                    nseq = ((nseq - 128u) << 8) + b8(sp++);
                    TD_ZSTD_STAT(ZS_SEQ_2BYTE);
                }
            }
            uint32_t lp = 0;                                       // literals used
            auto copy_literals = [&](uint32_t count) {             // → dst[op ..], by the whole wave
                for (uint32_t k = (uint32_t)lane; k < count; k += NL) {
                    if (op + k < cap) dst[op + k] = lit_rle ? (uint8_t)lit_byte : (lit_mem ? TD_INF_LOAD_OUT(lit + lp + k) : lit_src[lp + k]);
                }
                lp += count;
                op += count;
            };
            if (nseq == 0) {
                TD_ZSTD_STAT(ZS_SEQ0);
                if (sp != bn) TD_ZSTD_CORRUPT;
            } else {
                if (sp + 1 > bn) TD_ZSTD_CORRUPT;
                const uint32_t modes = b8(sp++);
                if (modes & 3u) TD_ZSTD_CORRUPT;
                TD_INF_SYNC();
                for (int t = 0; t < 3; ++t) {                      // LL, OF, ML
                    const uint32_t mode = (modes >> (6 - 2 * t)) & 3u;
                    const int max_log = t == 0 ? ZSTD_LL_LOG : (t == 1 ? ZSTD_OF_LOG : ZSTD_ML_LOG);
                    const int max_sym = t == 0 ? ZSTD_LL_MAX : (t == 1 ? ZSTD_OF_MAX : ZSTD_ML_MAX);
                    if (NL == 1 && stats) ++stats[ZS_LL_PREDEF + 4 * t + (int)mode];
                    if (mode == 3) {
                        if (fse_log[t] < 0) TD_ZSTD_CORRUPT;
                        continue;
                    }
                    bool ok = true;
                    if (mode == 1) {
                        if (sp + 1 > bn) TD_ZSTD_CORRUPT;
                        const uint32_t s = b8(sp++);
                        if ((int)s > max_sym) TD_ZSTD_CORRUPT;
                        if (lane == 0) S.fse[t][0] = s;
                        fse_log[t] = 0;
                    } else {
                        int lg = t == 1 ? 5 : 6, ns = t == 0 ? 36 : (t == 1 ? 29 : 53);
                        if (mode == 0) {
                            const int8_t* def = t == 0 ? LL_DEF : (t == 1 ? OF_DEF : ML_DEF);
                            for (int i = lane; i < ns; i += NL) S.norm[i] = def[i];
                        } else {
                            const int used = read_ncount<NL>(S, bs + sp, bn - sp, max_log, max_sym, &lg, &ns, lane);
                            if (!used) TD_ZSTD_CORRUPT;
                            sp += used;
                        }
                        TD_INF_SYNC();
                        if (lane == 0) ok = build_fse(S, S.fse[t], lg, ns);
                        fse_log[t] = lg;
                    }
                    TD_INF_SYNC();
                    if (!TD_ZSTD_ALL(ok)) TD_ZSTD_CORRUPT;
                }
                BackBits<true> sb;
                if (!sb.init(bs + sp, bn - sp)) TD_ZSTD_CORRUPT;
                uint32_t st_ll = sb.read(fse_log[0]), st_of = sb.read(fse_log[1]), st_ml = sb.read(fse_log[2]);
                if (sb.pos < 0) TD_ZSTD_CORRUPT;
                for (uint32_t q = 0; q < nseq; ++q) {              // ends at nseq (< 2^17)
                    const uint32_t e_ll = TD_INF_UNIFORM(S.fse[0][st_ll]), e_of = TD_INF_UNIFORM(S.fse[1][st_of]), e_ml = TD_INF_UNIFORM(S.fse[2][st_ml]);
                    const uint32_t c_ll = e_ll & 255u, c_of = e_of & 255u, c_ml = e_ml & 255u;
                    if (c_ll > (uint32_t)ZSTD_LL_MAX || c_of > (uint32_t)ZSTD_OF_MAX || c_ml > (uint32_t)ZSTD_ML_MAX) TD_ZSTD_CORRUPT;
                    const uint64_t ofv = (1ull << c_of) + sb.read((int)c_of);
                    const uint32_t mc = TD_INF_UNIFORM(ML_CODE[c_ml]), lc = TD_INF_UNIFORM(LL_CODE[c_ll]);
                    const uint32_t mlen = (mc & 0xffffffu) + sb.read((int)(mc >> 24));
                    const uint32_t llen = (lc & 0xffffffu) + sb.read((int)(lc >> 24));
                    if (q + 1 < nseq) {
                        st_ll = (e_ll >> 16) + sb.read((int)((e_ll >> 8) & 255u));
                        st_ml = (e_ml >> 16) + sb.read((int)((e_ml >> 8) & 255u));
                        st_of = (e_of >> 16) + sb.read((int)((e_of >> 8) & 255u));
                    }
                    if (sb.pos < 0) TD_ZSTD_CORRUPT;
                    uint64_t off;
                    if (ofv > 3) {
                        off = ofv - 3;
                        rep2 = rep1;
                        rep1 = rep0;
                        rep0 = (uint32_t)off;
                    } else {                                       // a repeat offset; shifted by one when no literals precede
                        const uint32_t idx = (uint32_t)ofv - 1u + (llen == 0 ? 1u : 0u);
                        if (idx == 0) {
                            off = rep0;
                        } else {
                            uint32_t v = idx == 1 ? rep1 : (idx == 2 ? rep2 : rep0 - 1u);
                            if (!v) v = 1;
                            if (idx != 1) rep2 = rep1;
                            rep1 = rep0;
                            rep0 = v;
                            off = v;
                        }
                    }
                    if (llen > lit_n - lp) TD_ZSTD_CORRUPT;
                    copy_literals(llen);
                    if (off > op || off >= (1ull << 31)) TD_ZSTD_CORRUPT;     // beyond the frame's first byte
                    if ((uint64_t)(op - op0) + mlen > ZSTD_BLOCK_MAX) TD_ZSTD_CORRUPT;
                    const uint32_t o32 = (uint32_t)off, from0 = op - o32;
                    // out[op + k] = out[op - off + (k mod off)]: every source byte was written before this match began. Only a match longer
                    // than its offset (a periodic copy) pays the integer modulo, once per byte copied: a known slow spot
                    if (from0 + (mlen < o32 ? mlen : o32) > flushed) {
                        TD_INF_STORES_DONE();
                        flushed = op;
                    }
                    const bool wraps = o32 < mlen;
                    for (uint32_t k = (uint32_t)lane; k < mlen; k += NL) {
                        const uint32_t from = from0 + (wraps ? k % o32 : k);
                        const uint8_t v = from < cap ? TD_INF_LOAD_OUT(dst + from) : (uint8_t)0;      // (past cap: status 2 anyway)
                        if (op + k < cap) dst[op + k] = v;
                    }
                    op += mlen;
                }
                if (sb.pos != 0) TD_ZSTD_CORRUPT;                       // the stream is used up exactly
            }
            copy_literals(lit_n - lp);                             // what is left follows the last match
            if (op - op0 > block_max) TD_ZSTD_CORRUPT;
            ip += bsize;
        }
        if (op > cap) {                                            // more than the block holds: no need to go on
            res.produced = op;
            res.status = 2;
            return res;
        }
        if (last) break;
    }
    if (NL == 1 && stats && frame_blocks > stats[ZS_MAX_BLOCKS_PER_FRAME]) stats[ZS_MAX_BLOCKS_PER_FRAME] = frame_blocks;
    if (has_fcs && fcs != op) TD_ZSTD_CORRUPT;
    if (has_sum) {
        if (ip + 4 > n) TD_ZSTD_CORRUPT;
        res.has_checksum = 1;
        res.checksum = le_bytes<true>(src, n, ip, 4);
        ip += 4;
    }
    res.produced = op;
    res.status = 0;
    res.end = (uint32_t)ip;
    return res;
}

// One TIFF block as the device takes it: exactly one frame, no content checksum. status 4 (declined: the host reader's business) for a
// checksum, for a skippable frame in front, and for bytes behind the frame that begin another frame of either kind; other bytes behind
// the frame are corrupt (as for the host wrapper, which finds no frame there).
template <int NL>
TD_INF_HD TD_INF_INLINE ZstdResult zstd_single_frame(ZstdScratch& S, const uint8_t* src, int64_t n, uint8_t* dst, uint32_t cap, uint8_t* lit, int lane) {
    using namespace zstd_detail;
    if (n >= 4 && (le_bytes<true>(src, n, 0, 4) & 0xFFFFFFF0u) == ZSTD_SKIP_MAGIC) return ZstdResult{0, 4, 0, 0, 0};
    ZstdResult r = zstd_frame<NL>(S, src, n, dst, cap, lit, lane, false, nullptr);
    if (r.status == 0 && (int64_t)r.end != n) {
        const uint32_t next = n - r.end >= 4 ? le_bytes<true>(src, n, r.end, 4) : 0u;
        r.status = next == ZSTD_MAGIC || (next & 0xFFFFFFF0u) == ZSTD_SKIP_MAGIC ? 4 : 1;
    }
    return r;
}
