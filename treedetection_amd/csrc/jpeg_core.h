// JPEG-in-TIFF (compression 7) decoded on the GPU (jpegdecode.hip) and, from the same source, by one host thread (jpegcodec.cpp:
// td_jpeg_decode), so that the CPU suite pins the decoder byte for byte against Pillow's libjpeg without a GPU. Written from ITU-T T.81
// (sequential Huffman decoding, F.2.2) and the output arithmetic of the IJG decoder that the host reader runs through Pillow:
//   - dequantisation + the accurate integer IDCT (13-bit constants, 2 extra bits between the passes, "islow") with the decoder's
//     range-limit table: a result x of the second pass becomes table[x & 1023] — 0..255 for -384 <= x < 512 (clamped), and the
//     table's wrap-around beyond that;
//   - "fancy" upsampling of chroma (triangular filter, 3/4 - 1/4 weights, edge samples replicated at the component's real size
//     ceil(W * h / hmax) x ceil(H * v / vmax); components at most 2 samples wide are replicated instead, as libjpeg does);
//   - YCbCr → RGB in 16-bit fixed point.
// What this core decodes: baseline / extended sequential Huffman, 8-bit samples, one component, three with Y sampled 1x1, 2x1 or
// 2x2 and chroma 1x1, or four that are all sampled 1x1 and come out as stored (libjpeg's JCS_CMYK / JCS_UNKNOWN: what libtiff writes for
// a four-band RGB + extra sample or separated raster), one interleaved scan, restart intervals. The host plan (jpegcodec.cpp) parses the headers, builds the Huffman
// lookup tables and cuts a block's entropy-coded data into segments (one per restart interval); everything else is unsupported.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define TD_JPG_HD __host__ __device__ inline
#define TD_JPG_INLINE __attribute__((always_inline))
#else
#define TD_JPG_HD static inline
#define TD_JPG_INLINE
#endif

constexpr int JPG_LOOK = 9;              // Huffman codes up to this length are decoded by one table lookup

// One Huffman table, built on the host (jpegcodec.cpp: jpeg_build_huff).
struct JpegHuff {
    uint16_t look[1 << JPG_LOOK];        // next JPG_LOOK bits → (code length << 8) | symbol; 0 = a longer code (or none)
    int32_t maxcode[18];                 // largest code of length l, -1 when there is none (T.81 F.2.2.3 MAXCODE)
    int32_t valoff[18];                  // index in vals of the first code of length l, minus that code
    uint8_t vals[256];                   // symbols in code order (HUFFVAL)
};

// The tables a block's components use, resolved per component (Y, Cb, Cr; or the four bands). Blocks that use the same tables share
// one set.
constexpr int JPG_MAXC = 4;
struct JpegTables {
    uint16_t q[JPG_MAXC][64];            // quantisation tables in natural (row-major) order
    JpegHuff dc[JPG_MAXC], ac[JPG_MAXC];
};

// Sampling modes: 0 grey, 1 4:4:4, 2 4:2:2 (Y 2x1), 3 4:2:0 (Y 2x2), chroma always 1x1; 4 four components, all 1x1, no colour step.
struct JpegGeom {
    int ncomp, hmax, vmax, mcus_x, mcus_y;
    int bw[JPG_MAXC], bh[JPG_MAXC];      // 8x8 blocks across / down per component (the MCU grid's, padding included)
    int cw[JPG_MAXC], ch[JPG_MAXC];      // real size of each component in samples
    int64_t off[JPG_MAXC];               // where the component's coefficients / samples start, in elements from the block's base
    int64_t total;                       // elements of one block (coefficients, or samples of the component planes)
};

TD_JPG_HD JpegGeom jpeg_geom(int mode, int w, int h) {
    JpegGeom g;
    g.ncomp = mode == 0 ? 1 : (mode == 4 ? 4 : 3);
    g.hmax = mode == 2 || mode == 3 ? 2 : 1;
    g.vmax = mode == 3 ? 2 : 1;
    g.mcus_x = (w + 8 * g.hmax - 1) / (8 * g.hmax);
    g.mcus_y = (h + 8 * g.vmax - 1) / (8 * g.vmax);
    int64_t o = 0;
    for (int c = 0; c < JPG_MAXC; ++c) {
        const bool y = c == 0;
        g.bw[c] = c < g.ncomp ? g.mcus_x * (y ? g.hmax : 1) : 0;
        g.bh[c] = c < g.ncomp ? g.mcus_y * (y ? g.vmax : 1) : 0;
        g.cw[c] = c < g.ncomp ? (y ? w : (w + g.hmax - 1) / g.hmax) : 0;
        g.ch[c] = c < g.ncomp ? (y ? h : (h + g.vmax - 1) / g.vmax) : 0;
        g.off[c] = o;
        o += (int64_t)g.bw[c] * g.bh[c] * 64;
    }
    g.total = o;
    return g;
}

TD_JPG_HD int jpeg_zigzag(int k) {       // position k of the zig-zag sequence → natural-order index (T.81 figure A.6)
    constexpr uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return ZZ[k];
}

// ---- entropy-coded segment → coefficients ----------------------------------------------------------------------------------------
// Bit reader over [p, p + n): 0xFF00 is a stuffed 0xFF, any other 0xFF xx (or the end of the bytes) ends the data; zeros are fed
// past it and counted, and a segment that CONSUMES any of them is corrupt (a marker or the end of data before its last MCU).
struct JpegBits {
    const uint8_t* p;
    uint32_t pos, n;
    uint64_t acc;                        // MSB-first
    int have, pad;                       // bits in acc / how many of them are padding
};

TD_JPG_HD TD_JPG_INLINE void jpeg_fill(JpegBits& b) {
    while (b.have <= 56) {
        uint32_t v = 0;
        if (b.pad == 0 && b.pos < b.n) {
            v = b.p[b.pos];
            if (v != 0xFF) {
                ++b.pos;
            } else if (b.pos + 1 < b.n && b.p[b.pos + 1] == 0) {
                b.pos += 2;
            } else {
                v = 0;                   // a marker: the data ends here
                b.pad = 8;
            }
        } else {
            b.pad += 8;
        }
        b.acc |= (uint64_t)v << (56 - b.have);
        b.have += 8;
    }
}

TD_JPG_HD uint32_t jpeg_bits(JpegBits& b, int s) {         // s in 1..16
    if (b.have < s) jpeg_fill(b);
    const uint32_t v = (uint32_t)(b.acc >> (64 - s));
    b.acc <<= s;
    b.have -= s;
    return v;
}

TD_JPG_HD int jpeg_extend(uint32_t v, int s) {             // T.81 F.2.2.1 EXTEND
    return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v;
}

TD_JPG_HD TD_JPG_INLINE int jpeg_huff(const JpegHuff& H, JpegBits& b) {
    if (b.have < 16) jpeg_fill(b);
    const uint32_t e = H.look[b.acc >> (64 - JPG_LOOK)];
    if (e) {
        const int l = (int)(e >> 8);
        b.acc <<= l;
        b.have -= l;
        return (int)(e & 255);
    }
    for (int l = JPG_LOOK + 1; l <= 16; ++l) {
        const int32_t code = (int32_t)(b.acc >> (64 - l));
        if (code <= H.maxcode[l]) {
            b.acc <<= l;
            b.have -= l;
            return H.vals[(H.valoff[l] + code) & 255];
        }
    }
    return -1;                                             // not a code of the table
}

// One 8x8 block: DC difference + AC run / size pairs, coefficients written (natural order) into a zeroed blk. → 0 or 1 (corrupt).
// A dequantised coefficient of 8-bit samples lies within 1024 + q / 2 of zero (the DCT of [-128, 127] is at most 1024, and rounding
// to a multiple of q adds at most q / 2). Larger ones only come out of corrupt data (a flipped bit that still parses): libjpeg's vector
// IDCT then wraps 16-bit intermediates that this IDCT keeps whole, so such a block is reported instead of decoded differently.
TD_JPG_HD bool jpeg_coef_ok(int32_t v, uint16_t q) {
    const int64_t qq = (int16_t)q, d = (int64_t)v * qq;
    return (d < 0 ? -d : d) <= 1024 + 16 + ((qq < 0 ? -qq : qq) >> 1);
}

TD_JPG_HD TD_JPG_INLINE int jpeg_block(const JpegHuff& dc, const JpegHuff& ac, const uint16_t* q, JpegBits& b, int32_t& pred, int16_t* blk) {
    // 8-bit samples: DC differences of at most 11 bits, AC values of at most 10 (T.81 tables F.1, F.2). Larger ones only come out of
    // corrupt data, where libjpeg's vector IDCT wraps 16-bit products that this one keeps whole: reported instead of decoded differently
    const int t = jpeg_huff(dc, b);
    if (t < 0 || t > 11) return 1;
    const int diff = t ? jpeg_extend(jpeg_bits(b, t), t) : 0;
    pred = (int32_t)((uint32_t)pred + (uint32_t)diff);       // libjpeg's int predictor, stored as a 16-bit coefficient
    if (!jpeg_coef_ok(pred, q[0])) return 1;
    blk[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = jpeg_huff(ac, b);
        if (rs < 0) return 1;
        const int r = rs >> 4, s = rs & 15;
        if (s) {
            if (s > 10) return 1;
            k += r;
            if (k > 63) return 1;                          // a run past coefficient 63
            const int z = jpeg_zigzag(k), v = jpeg_extend(jpeg_bits(b, s), s);
            if (!jpeg_coef_ok(v, q[z])) return 1;
            blk[z] = (int16_t)v;
            ++k;
        } else if (r == 15) {
            k += 16;
            if (k > 64) return 1;
        } else {
            break;                                         // end of block
        }
    }
    return 0;
}

// MCUs [mcu0, mcu0 + nmcu) of one block from its segment [src, src + nbytes) (one restart interval, or the whole scan) into the
// block's zeroed coefficient area coef (layout: JpegGeom::off / bw). → 0 ok, 1 corrupt. FOUR: the block is of mode 4 (four DC
// predictors, an MCU of four blocks) — a parameter of the instantiation, so that the one- and three-component decoder carries nothing
// of it (the entropy kernel is bound by its registers).
template <bool FOUR = false>
TD_JPG_HD TD_JPG_INLINE int jpeg_decode_segment(const JpegTables& T, const JpegGeom& g, const uint8_t* src, uint32_t nbytes, uint32_t mcu0,
                                                uint32_t nmcu, int16_t* coef) {
    JpegBits b;
    b.p = src;
    b.pos = 0;
    b.n = nbytes;
    b.acc = 0;
    b.have = 0;
    b.pad = 0;
    int32_t pred[FOUR ? 4 : 3] = {};
    for (uint32_t m = mcu0; m < mcu0 + nmcu; ++m) {
        const int mx = (int)(m % (uint32_t)g.mcus_x), my = (int)(m / (uint32_t)g.mcus_x);
        if constexpr (FOUR) {
            const int64_t at = ((int64_t)my * g.mcus_x + mx) * 64, plane = (int64_t)g.mcus_x * g.mcus_y * 64;
            for (int c = 0; c < 4; ++c)
                if (jpeg_block(T.dc[c], T.ac[c], T.q[c], b, pred[c], coef + c * plane + at)) return 1;
        } else if (g.ncomp == 1) {
            if (jpeg_block(T.dc[0], T.ac[0], T.q[0], b, pred[0], coef + ((int64_t)my * g.bw[0] + mx) * 64)) return 1;
        } else {
            for (int v = 0; v < g.vmax; ++v)
                for (int h = 0; h < g.hmax; ++h)
                    if (jpeg_block(T.dc[0], T.ac[0], T.q[0], b, pred[0], coef + ((int64_t)(my * g.vmax + v) * g.bw[0] + mx * g.hmax + h) * 64)) return 1;
            for (int c = 1; c < 3; ++c)
                if (jpeg_block(T.dc[c], T.ac[c], T.q[c], b, pred[c], coef + g.off[c] + ((int64_t)my * g.bw[c] + mx) * 64)) return 1;
        }
        if (b.have < b.pad) return 1;                      // consumed bits past the end of the data
    }
    // and the data ends here: at most 7 bits are left before the marker (or the end), all ones (the encoder's padding). A stream
    // that decodes its MCUs with bytes to spare was misread (a flipped bit) — libjpeg warns about "extraneous bytes" and goes on
    jpeg_fill(b);
    const int left = b.have - b.pad;
    if (b.pad == 0 || left >= 8) return 1;
    return left > 0 && (uint32_t)(b.acc >> (64 - left)) != (1u << left) - 1u;
}

// ---- one long segment decoded by many lanes: self-synchronising Huffman decoding ------------------------------------------------
// A segment's bytes are cut into subsequences of S raw bytes; 64 consecutive ones form a window, one per lane. The state of a decoder
// between two symbols (a Huffman code + its extra bits) is (bit position, zig-zag index k in the current 8x8 block with k == 0 = "a DC
// code comes next", index j of that block in its MCU): two decoders in the same state have the same future. Lane 0 of a window enters
// with the true state; every other lane guesses (its first byte, k = 0, j = 0), walks its subsequence WITHOUT writing and records the
// state at the first symbol boundary at or past the subsequence's end and the blocks it completed. Then rounds: lane i takes lane
// i - 1's exit and walks again when it differs from the entry it last walked from. A lane is validated when its predecessor is and its
// entry equals the predecessor's exit; the validated lanes are a growing prefix (at least one more per round), so at most 64 rounds,
// and a few when the stream synchronises. An exclusive prefix sum of the validated counts gives each lane the ordinal of its first
// block; a last walk from the validated entries writes the coefficients (DC: the DIFFERENCE — jpeg_sync_dc / jpeg_dc_scan_kernel sums them).
//
// The bit position is (raw byte index, bit 0..7 from the MSB) of the next unconsumed bit, canonical: the byte index never names the
// 00 of a stuffed FF 00 (inside the data a 00 after an FF is always the stuffed one, an FF followed by anything else ends the data),
// and a guess that would start on such a 00 starts one byte later. A position at the end of the data is (index of the marker, 0).
// "Lost" (an invalid code, a size beyond the 8-bit limits, a run past coefficient 63, bits consumed past the end of the data) equals
// no state: the successor of a lost guess keeps its own guess; the successors of a lost VALIDATED lane have nothing left to decode.
typedef uint64_t JpegSyncState;                            // byte | bit << 32 | k << 35 | j << 41
constexpr JpegSyncState JPG_SYNC_LOST = ~(uint64_t)0;
constexpr uint32_t JPG_SYNC_NO_END = 0xFFFFFFFFu;          // the segment's last subsequence ends with the blocks, not at a byte
constexpr int JPG_SYNC_MIN_SUBSEQ = 4, JPG_SYNC_MAX_SUBSEQ = 1 << 20;      // a symbol is at most 27 bits

TD_JPG_HD JpegSyncState jpeg_sync_state(uint32_t byte, int bit, int k, int j) {
    return (uint64_t)byte | (uint64_t)bit << 32 | (uint64_t)k << 35 | (uint64_t)j << 41;
}

// JpegBits + what it takes to name the position of the next bit: which of the bytes in acc were an FF with its stuffed 00.
struct JpegSyncBits {
    JpegBits b;
    uint32_t stuff;                      // bit i: the (i + 1)-th most recently fetched data byte took two raw bytes
#ifdef __HIP_DEVICE_COMPILE__
    uint32_t word, wat;                  // the compressed bytes come a dword at a time: the aligned dword last loaded, and which
#endif
};

TD_JPG_HD TD_JPG_INLINE uint32_t jpeg_sync_byte(JpegSyncBits& r, uint32_t i) {       // byte i < n of the segment
#ifdef __HIP_DEVICE_COMPILE__
    const uintptr_t lo = (uintptr_t)r.b.p, a = lo + i, q = a & ~(uintptr_t)3;
    const uint32_t at = (uint32_t)((q - (lo & ~(uintptr_t)3)) >> 2);
    if (at != r.wat) {
        r.wat = at;
        if (q >= lo && q + 4 <= lo + r.b.n) {
            r.word = *reinterpret_cast<const uint32_t*>(q);
        } else {                                           // the dwords that hold the segment's first and last bytes: those bytes only
            r.word = 0;
            for (int t = 0; t < 4; ++t)
                if (q + t >= lo && q + t < lo + r.b.n) r.word |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + t) << (8 * t);
        }
    }
    return (r.word >> (8 * (int)(a & 3))) & 255u;
#else
    return r.b.p[i];
#endif
}

TD_JPG_HD TD_JPG_INLINE void jpeg_sync_fill(JpegSyncBits& r) {       // jpeg_fill, keeping r.stuff
    JpegBits& b = r.b;
    while (b.have <= 56) {
        uint32_t v = 0;
        if (b.pad == 0 && b.pos < b.n) {
            v = jpeg_sync_byte(r, b.pos);
            if (v != 0xFF) {
                ++b.pos;
                r.stuff <<= 1;
            } else if (b.pos + 1 < b.n && jpeg_sync_byte(r, b.pos + 1) == 0) {
                b.pos += 2;
                r.stuff = r.stuff << 1 | 1u;
            } else {
                v = 0;
                b.pad = 8;
            }
        } else {
            b.pad += 8;
        }
        b.acc |= (uint64_t)v << (56 - b.have);
        b.have += 8;
    }
}

TD_JPG_HD TD_JPG_INLINE void jpeg_sync_open(JpegSyncBits& r, const uint8_t* src, uint32_t n, JpegSyncState at) {
    r.b.p = src;
    r.b.pos = (uint32_t)at;
    r.b.n = n;
    r.b.acc = 0;
    r.b.have = 0;
    r.b.pad = 0;
    r.stuff = 0;
#ifdef __HIP_DEVICE_COMPILE__
    r.word = 0;
    r.wat = 0xFFFFFFFFu;
#endif
    jpeg_sync_fill(r);
    const int bit = (int)(at >> 32) & 7;
    r.b.acc <<= bit;
    r.b.have -= bit;
}

// The canonical byte of the next unconsumed bit (have >= pad: no padding consumed) and its bit.
TD_JPG_HD TD_JPG_INLINE uint32_t jpeg_sync_at(const JpegSyncBits& r, int& bit) {
    const int real = r.b.have - r.b.pad, nb = (real + 7) >> 3;
    bit = (8 - (real & 7)) & 7;
    return r.b.pos - (uint32_t)nb - (uint32_t)__builtin_popcount(r.stuff & ((1u << nb) - 1u));
}

// What a lane other than a window's first assumes at the start of subsequence `sub` (> 0) of S bytes.
TD_JPG_HD JpegSyncState jpeg_sync_guess(const uint8_t* src, uint32_t n, uint32_t sub, uint32_t S) {
    uint32_t at = sub * S;
    if (at < n && src[at] == 0 && src[at - 1] == 0xFF) ++at;         // the boundary fell between an FF and its stuffed 00
    return jpeg_sync_state(at, 0, 0, 0);
}

TD_JPG_HD int jpeg_sync_blocks_per_mcu(const JpegGeom& g, bool four) { return four ? 4 : (g.ncomp == 1 ? 1 : g.hmax * g.vmax + 2); }

// Block j of MCU m → its component and where its 64 coefficients start (what jpeg_decode_segment computes).
template <bool FOUR>
TD_JPG_HD TD_JPG_INLINE int64_t jpeg_sync_block_at(const JpegGeom& g, uint32_t m, int j, int& c) {
    const int mx = (int)(m % (uint32_t)g.mcus_x), my = (int)(m / (uint32_t)g.mcus_x);
    if constexpr (FOUR) {
        c = j;
        return (int64_t)j * ((int64_t)g.mcus_x * g.mcus_y * 64) + ((int64_t)my * g.mcus_x + mx) * 64;
    }
    const int ny = g.hmax * g.vmax;
    if (g.ncomp == 1 || j < ny) {
        c = 0;
        const int v = g.ncomp == 1 ? 0 : j / g.hmax, h = g.ncomp == 1 ? 0 : j - v * g.hmax;
        return ((int64_t)(my * g.vmax + v) * g.bw[0] + mx * g.hmax + h) * 64;
    }
    c = j - ny + 1;                                        // Cb or Cr (selected, not indexed: g stays in registers)
    return (c == 1 ? g.off[1] : g.off[2]) + ((int64_t)my * g.bw[1] + mx) * 64;
}

// One walk: from `entry` over the symbols that start before byte `end` of [src, src + n) (JPG_SYNC_NO_END: until the data gives out).
// → the exit state or JPG_SYNC_LOST; blocks: how many it completed. WRITE: the walk of a validated entry whose first block has ordinal
// `first` in the segment, `limit` (> 0) blocks short of the segment's last: the non-zero AC coefficients and the DC differences go to
// coef (zeroed), block by block as jpeg_sync_block_at places them; flags |= 1: corrupt data (everything jpeg_block reports but the DC
// value itself), |= 2: the walk completed the segment's last block and has checked the bits that are left as jpeg_decode_segment
// does. Without WRITE nothing is stored and g, coef, mcu0, first, limit and flags are not used.
template <bool FOUR, bool WRITE>
TD_JPG_HD TD_JPG_INLINE JpegSyncState jpeg_sync_walk(const JpegTables& T, const JpegGeom& g, const uint8_t* src, uint32_t n,
                                                     JpegSyncState entry, uint32_t end, uint32_t& blocks, int16_t* coef, uint32_t mcu0,
                                                     uint32_t first, uint32_t limit, int& flags) {
    const int bpm = jpeg_sync_blocks_per_mcu(g, FOUR), ny = bpm - 2;
    JpegSyncBits r;
    jpeg_sync_open(r, src, n, entry);
    JpegBits& b = r.b;
    int k = (int)(entry >> 35) & 63, j = (int)(entry >> 41) & 7, c = 0;
    uint32_t m = 0;
    int16_t* blk = nullptr;
    if constexpr (WRITE) {
        j = (int)(first % (uint32_t)bpm);
        m = mcu0 + first / (uint32_t)bpm;
        blk = coef + jpeg_sync_block_at<FOUR>(g, m, j, c);
    } else {
        c = FOUR || g.ncomp == 1 ? j : (j < ny ? 0 : j - ny + 1);
    }
    blocks = 0;
    for (;;) {
        if (b.have < 32) jpeg_sync_fill(r);
        if (b.have < b.pad) break;                         // consumed bits past the end of the data
        if (b.pos >= end) {                                // (the next bit lies at or before pos)
            int bit;
            const uint32_t at = jpeg_sync_at(r, bit);
            if (at >= end) return jpeg_sync_state(at, bit, k, j);
        }
        if (k == 0) {
            const int t = jpeg_huff(T.dc[c], b);
            if (t < 0 || t > 11) break;
            const int diff = t ? jpeg_extend(jpeg_bits(b, t), t) : 0;
            if constexpr (WRITE) blk[0] = (int16_t)diff;
            k = 1;
        } else {
            const int rs = jpeg_huff(T.ac[c], b);
            if (rs < 0) break;
            const int run = rs >> 4, s = rs & 15;
            if (s) {
                if (s > 10) break;
                k += run;
                if (k > 63) break;                         // a run past coefficient 63
                const int v = jpeg_extend(jpeg_bits(b, s), s);
                if constexpr (WRITE) {
                    const int z = jpeg_zigzag(k);
                    if (!jpeg_coef_ok(v, T.q[c][z])) break;
                    blk[z] = (int16_t)v;
                }
                ++k;
            } else if (run == 15) {
                k += 16;
                if (k > 64) break;
            } else {
                k = 64;                                    // end of block
            }
        }
        if (k < 64) continue;
        if (b.have < b.pad) break;
        k = 0;
        ++blocks;
        if (++j == bpm) {
            j = 0;
            ++m;
        }
        if constexpr (WRITE) {
            if (blocks == limit) {                         // the segment's last block: at most 7 bits are left, all ones
                jpeg_sync_fill(r);
                const int left = b.have - b.pad;
                if (b.pad == 0 || left >= 8 || (left > 0 && (uint32_t)(b.acc >> (64 - left)) != (1u << left) - 1u)) flags |= 1;
                flags |= 2;
                int bit;
                const uint32_t at = jpeg_sync_at(r, bit);
                return jpeg_sync_state(at, bit, 0, j);
            }
            blk = coef + jpeg_sync_block_at<FOUR>(g, m, j, c);
        } else {
            c = FOUR || g.ncomp == 1 ? j : (j < ny ? 0 : j - ny + 1);
        }
    }
    if constexpr (WRITE) flags |= 1;
    return JPG_SYNC_LOST;
}

// Block t (scan order inside the segment that starts at MCU mcu0) of component c → where its coefficients start.
template <bool FOUR>
TD_JPG_HD TD_JPG_INLINE int64_t jpeg_sync_dc_block_at(const JpegGeom& g, uint32_t mcu0, int c, uint32_t t) {
    const int ny = FOUR || g.ncomp == 1 ? 1 : g.hmax * g.vmax;
    const uint32_t per = c == 0 ? (uint32_t)ny : 1u;
    const int j = (c == 0 ? 0 : (FOUR ? c : ny + c - 1)) + (int)(t % per);
    int cc;
    return jpeg_sync_block_at<FOUR>(g, mcu0 + t / per, j, cc);
}
TD_JPG_HD uint32_t jpeg_sync_dc_blocks(const JpegGeom& g, bool four, int c, uint32_t nmcu) {
    return nmcu * (c == 0 && !four && g.ncomp != 1 ? (uint32_t)(g.hmax * g.vmax) : 1u);
}

// The window procedure with `lanes` (1 .. 64) emulated lanes on one host thread: jpeg_decode_segment's contract (coef zeroed; → 0 ok,
// 1 corrupt) by the walks above, lane after lane where a wave runs them side by side (jpegdecode.hip: jpeg_entropy_sync_kernel, which
// follows this text step by step). stats (may be null) += {rounds summed over the windows, windows, (max) the most rounds one window
// took, windows that took one round}.
template <bool FOUR>
static inline int jpeg_sync_segment(const JpegTables& T, const JpegGeom& g, const uint8_t* src, uint32_t n, uint32_t mcu0, uint32_t nmcu,
                                    int16_t* coef, uint32_t S, int lanes, int64_t* stats) {
    const uint32_t total = nmcu * (uint32_t)jpeg_sync_blocks_per_mcu(g, FOUR);
    const uint32_t nsub = n > S ? (uint32_t)(((uint64_t)n + S - 1) / S) : 1u;
    JpegSyncState entry[64], exit[64], seen[64], carry = jpeg_sync_state(0, 0, 0, 0);
    uint32_t cnt[64], base = 0;
    int none = 0;
    for (uint32_t w0 = 0; w0 < nsub; w0 += (uint32_t)lanes) {
        const int L = (int)(nsub - w0 < (uint32_t)lanes ? nsub - w0 : (uint32_t)lanes);
        auto end_of = [&](int i) { return w0 + (uint32_t)i == nsub - 1 ? JPG_SYNC_NO_END : (w0 + (uint32_t)i + 1) * S; };
        for (int i = 0; i < L; ++i) {
            entry[i] = i == 0 ? carry : jpeg_sync_guess(src, n, w0 + (uint32_t)i, S);
            exit[i] = jpeg_sync_walk<FOUR, false>(T, g, src, n, entry[i], end_of(i), cnt[i], nullptr, 0, 0, 0, none);
        }
        int rounds = 1, valid = 0;
        for (;;) {
            for (valid = 1; valid < L && entry[valid] == exit[valid - 1]; ++valid) {}
            if (valid == L || exit[valid - 1] == JPG_SYNC_LOST) break;
            for (int i = 0; i < L; ++i) seen[i] = exit[i];             // the lanes of a wave all read before any of them walks again
            for (int i = valid; i < L; ++i)
                if (seen[i - 1] != JPG_SYNC_LOST && seen[i - 1] != entry[i]) {
                    entry[i] = seen[i - 1];
                    exit[i] = jpeg_sync_walk<FOUR, false>(T, g, src, n, entry[i], end_of(i), cnt[i], nullptr, 0, 0, 0, none);
                }
            ++rounds;
        }
        if (stats) {
            stats[0] += rounds;
            stats[1] += 1;
            if (rounds > stats[2]) stats[2] = rounds;
            stats[3] += rounds == 1;
        }
        int flags = 0;
        for (int i = 0; i < valid && !(flags & 2); ++i) {
            if (base >= total) return 1;                   // (only behind a lane that has finished: cannot be reached)
            uint32_t wrote;
            jpeg_sync_walk<FOUR, true>(T, g, src, n, entry[i], end_of(i), wrote, coef, mcu0, base, total - base, flags);
            if (flags & 1) return 1;
            base += cnt[i];
        }
        if (flags & 2) return 0;
        if (valid < L) return 1;                           // (a validated lane was lost: its write walk has reported it)
        carry = exit[L - 1];
    }
    return 1;                                              // the data gave out before the last block
}

// DC differences → DC values, component by component in scan order, as jpeg_block predicts and checks them. → 0 ok, 1 corrupt.
template <bool FOUR>
static inline int jpeg_sync_dc(const JpegTables& T, const JpegGeom& g, uint32_t mcu0, uint32_t nmcu, int16_t* coef) {
    int bad = 0;
    for (int c = 0; c < g.ncomp; ++c) {
        uint32_t pred = 0;
        const uint32_t nb = jpeg_sync_dc_blocks(g, FOUR, c, nmcu);
        for (uint32_t t = 0; t < nb; ++t) {
            int16_t* blk = coef + jpeg_sync_dc_block_at<FOUR>(g, mcu0, c, t);
            pred += (uint32_t)(int32_t)blk[0];
            bad |= !jpeg_coef_ok((int32_t)pred, T.q[c][0]);
            blk[0] = (int16_t)(int32_t)pred;
        }
    }
    return bad;
}

// ---- dequantisation + accurate integer IDCT of one 8x8 block ---------------------------------------------------------------------
TD_JPG_HD uint8_t jpeg_range_limit(int64_t x) {            // the decoder's post-IDCT table, indexed by x & 1023
    const int i = (int)(x & 1023);
    return (uint8_t)(i < 128 ? i + 128 : i < 512 ? 255 : i < 896 ? 0 : i - 896);
}

TD_JPG_HD TD_JPG_INLINE void jpeg_idct_islow(const int16_t* in, const uint16_t* q, uint8_t* out, int64_t stride) {
    constexpr int CB = 13, P1 = 2;
    constexpr int64_t F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                      F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    int32_t ws[64];
    // the decoder holds quantisation values as 16-bit signed multipliers (a 16-bit DQT entry above 32767 turns negative)
    for (int c = 0; c < 8; ++c) {
        const int64_t d0 = (int64_t)in[c] * (int16_t)q[c], d1 = (int64_t)in[8 + c] * (int16_t)q[8 + c], d2 = (int64_t)in[16 + c] * (int16_t)q[16 + c],
                      d3 = (int64_t)in[24 + c] * (int16_t)q[24 + c], d4 = (int64_t)in[32 + c] * (int16_t)q[32 + c],
                      d5 = (int64_t)in[40 + c] * (int16_t)q[40 + c], d6 = (int64_t)in[48 + c] * (int16_t)q[48 + c],
                      d7 = (int64_t)in[56 + c] * (int16_t)q[56 + c];
        if ((in[8 + c] | in[16 + c] | in[24 + c] | in[32 + c] | in[40 + c] | in[48 + c] | in[56 + c]) == 0) {
            const int32_t dc = (int32_t)(d0 * (1 << P1));
            for (int r = 0; r < 8; ++r) ws[r * 8 + c] = dc;
            continue;
        }
        int64_t z1 = (d2 + d6) * F0541;
        int64_t tmp2 = z1 - d6 * F1847, tmp3 = z1 + d2 * F0765;
        int64_t tmp0 = (d0 + d4) * (1 << CB), tmp1 = (d0 - d4) * (1 << CB);
        const int64_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
        tmp0 = d7;
        tmp1 = d5;
        tmp2 = d3;
        tmp3 = d1;
        z1 = tmp0 + tmp3;
        int64_t z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F1175;
        tmp0 *= F0298;
        tmp1 *= F2053;
        tmp2 *= F3072;
        tmp3 *= F1501;
        z1 *= -F0899;
        z2 *= -F2562;
        z3 *= -F1961;
        z4 *= -F0390;
        z3 += z5;
        z4 += z5;
        tmp0 += z1 + z3;
        tmp1 += z2 + z4;
        tmp2 += z2 + z3;
        tmp3 += z1 + z4;
        constexpr int SH = CB - P1;
        constexpr int64_t RND = (int64_t)1 << (SH - 1);
        ws[0 * 8 + c] = (int32_t)((t10 + tmp3 + RND) >> SH);
        ws[7 * 8 + c] = (int32_t)((t10 - tmp3 + RND) >> SH);
        ws[1 * 8 + c] = (int32_t)((t11 + tmp2 + RND) >> SH);
        ws[6 * 8 + c] = (int32_t)((t11 - tmp2 + RND) >> SH);
        ws[2 * 8 + c] = (int32_t)((t12 + tmp1 + RND) >> SH);
        ws[5 * 8 + c] = (int32_t)((t12 - tmp1 + RND) >> SH);
        ws[3 * 8 + c] = (int32_t)((t13 + tmp0 + RND) >> SH);
        ws[4 * 8 + c] = (int32_t)((t13 - tmp0 + RND) >> SH);
    }
    for (int r = 0; r < 8; ++r) {
        const int32_t* w = ws + r * 8;
        uint8_t* o = out + r * stride;
        if ((w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) == 0) {
            const uint8_t v = jpeg_range_limit(((int64_t)w[0] + (1 << (P1 + 2))) >> (P1 + 3));
            for (int k = 0; k < 8; ++k) o[k] = v;
            continue;
        }
        int64_t z2 = w[2], z3 = w[6];
        int64_t z1 = (z2 + z3) * F0541;
        int64_t tmp2 = z1 - z3 * F1847, tmp3 = z1 + z2 * F0765;
        int64_t tmp0 = ((int64_t)w[0] + w[4]) * (1 << CB), tmp1 = ((int64_t)w[0] - w[4]) * (1 << CB);
        const int64_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
        tmp0 = w[7];
        tmp1 = w[5];
        tmp2 = w[3];
        tmp3 = w[1];
        z1 = tmp0 + tmp3;
        z2 = tmp1 + tmp2;
        z3 = tmp0 + tmp2;
        int64_t z4 = tmp1 + tmp3;
        const int64_t z5 = (z3 + z4) * F1175;
        tmp0 *= F0298;
        tmp1 *= F2053;
        tmp2 *= F3072;
        tmp3 *= F1501;
        z1 *= -F0899;
        z2 *= -F2562;
        z3 *= -F1961;
        z4 *= -F0390;
        z3 += z5;
        z4 += z5;
        tmp0 += z1 + z3;
        tmp1 += z2 + z4;
        tmp2 += z2 + z3;
        tmp3 += z1 + z4;
        constexpr int SH = CB + P1 + 3;
        constexpr int64_t RND = (int64_t)1 << (SH - 1);
        o[0] = jpeg_range_limit((t10 + tmp3 + RND) >> SH);
        o[7] = jpeg_range_limit((t10 - tmp3 + RND) >> SH);
        o[1] = jpeg_range_limit((t11 + tmp2 + RND) >> SH);
        o[6] = jpeg_range_limit((t11 - tmp2 + RND) >> SH);
        o[2] = jpeg_range_limit((t12 + tmp1 + RND) >> SH);
        o[5] = jpeg_range_limit((t12 - tmp1 + RND) >> SH);
        o[3] = jpeg_range_limit((t13 + tmp0 + RND) >> SH);
        o[4] = jpeg_range_limit((t13 - tmp0 + RND) >> SH);
    }
}

// ---- one output pixel: fancy upsampling + colour conversion ----------------------------------------------------------------------
// planes: the block's component planes (layout JpegGeom::off, row stride bw * 8); (x, y) inside the SOF size. ycc: YCbCr → RGB.
TD_JPG_HD int jpeg_plane_at(const uint8_t* planes, const JpegGeom& g, int c, int x, int y) {
    return planes[g.off[c] + (int64_t)y * (g.bw[c] * 8) + x];
}

TD_JPG_HD int jpeg_chroma(const uint8_t* planes, const JpegGeom& g, int c, int x, int y) {
    const int cw = g.cw[c], ch = g.ch[c];
    if (g.hmax == 1) return jpeg_plane_at(planes, g, c, x, y);          // 4:4:4
    const int cx = x >> 1;
    if (cw <= 2) return jpeg_plane_at(planes, g, c, cx, y >> (g.vmax - 1));      // libjpeg replicates components this narrow
    if (g.vmax == 1) {                                                   // h2v1: (3 * this + neighbour + 1 or 2) >> 2
        const int t = jpeg_plane_at(planes, g, c, cx, y);
        if (!(x & 1)) return cx == 0 ? t : (t * 3 + jpeg_plane_at(planes, g, c, cx - 1, y) + 1) >> 2;
        return cx == cw - 1 ? t : (t * 3 + jpeg_plane_at(planes, g, c, cx + 1, y) + 2) >> 2;
    }
    // h2v2: column sums 3 * near row + far row (rows outside [0, ch) replicate the edge), then 3 * this + neighbour across
    const int cy = y >> 1;
    int fy = (y & 1) ? cy + 1 : cy - 1;
    fy = fy < 0 ? 0 : (fy > ch - 1 ? ch - 1 : fy);
    const int t = jpeg_plane_at(planes, g, c, cx, cy) * 3 + jpeg_plane_at(planes, g, c, cx, fy);
    if (!(x & 1)) {
        if (cx == 0) return (t * 4 + 8) >> 4;
        const int o = jpeg_plane_at(planes, g, c, cx - 1, cy) * 3 + jpeg_plane_at(planes, g, c, cx - 1, fy);
        return (t * 3 + o + 8) >> 4;
    }
    if (cx == cw - 1) return (t * 4 + 7) >> 4;
    const int o = jpeg_plane_at(planes, g, c, cx + 1, cy) * 3 + jpeg_plane_at(planes, g, c, cx + 1, fy);
    return (t * 3 + o + 7) >> 4;
}

// Mode 4: the pixel's four samples as stored, packed in memory order (sample 0 in the low byte) — one dword of an [h][w][4] raster.
TD_JPG_HD uint32_t jpeg_pixel4(const uint8_t* planes, int mcus_x, int mcus_y, int x, int y) {
    const int64_t plane = (int64_t)mcus_x * mcus_y * 64, at = (int64_t)y * (mcus_x * 8) + x;
    return (uint32_t)planes[at] | (uint32_t)planes[plane + at] << 8 | (uint32_t)planes[2 * plane + at] << 16 |
           (uint32_t)planes[3 * plane + at] << 24;
}

TD_JPG_HD uint8_t jpeg_clamp255(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// → the pixel's samples in px[0 .. ncomp), one or three components (four: jpeg_pixel4)
TD_JPG_HD TD_JPG_INLINE void jpeg_pixel(const uint8_t* planes, const JpegGeom& g, int ycc, int x, int y, uint8_t* px) {
    const int Y = jpeg_plane_at(planes, g, 0, x, y);
    if (g.ncomp == 1) {
        px[0] = (uint8_t)Y;
        return;
    }
    const int cb = jpeg_chroma(planes, g, 1, x, y), cr = jpeg_chroma(planes, g, 2, x, y);
    if (!ycc) {
        px[0] = (uint8_t)Y;
        px[1] = (uint8_t)cb;
        px[2] = (uint8_t)cr;
        return;
    }
    // 16-bit fixed point, ONE_HALF rounding (the IJG colour converter's tables, computed in place)
    constexpr int64_t FR = 91881, FB = 116130, FGR = 46802, FGB = 22554, HALF = 1 << 15;
    const int64_t dcr = cr - 128, dcb = cb - 128;
    const int r = Y + (int)((FR * dcr + HALF) >> 16);
    const int gg = Y + (int)((-FGB * dcb + HALF - FGR * dcr) >> 16);
    const int bb = Y + (int)((FB * dcb + HALF) >> 16);
    px[0] = jpeg_clamp255(r);
    px[1] = jpeg_clamp255(gg);
    px[2] = jpeg_clamp255(bb);
}
