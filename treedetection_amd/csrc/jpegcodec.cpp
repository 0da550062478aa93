// JPEG-in-TIFF (compression 7), the host's share: the marker walk (ITU-T T.81 annex B), the Huffman lookup tables (annex C / F.2.2.3)
// and the plan that lets jpegdecode.hip decode a whole raster — and td_jpeg_decode, the decoder of jpeg_core.h run by one host thread
// on one stream (the CPU suite pins it byte for byte against Pillow's libjpeg). Pure host code.
//
// What a block decodes to is what the host reader (geotiff.py: GeoTiff._decode_jpeg_block) gets from libjpeg for the stream it builds:
// SOI, an Adobe APP14 segment (three bands and no JFIF in the block's first 32 bytes: transform 1 for PhotometricInterpretation 6,
// 0 otherwise), the JPEGTables tag without its SOI / EOI, the block without its SOI. The plan walks those pieces in that order, so a
// table the block redefines wins and the colour transform follows libjpeg's rule (JFIF → YCbCr, else the Adobe transform, else the
// component ids). Four bands get no Adobe segment: libjpeg takes four components as they are stored (CMYK) unless an Adobe segment of
// the stream itself names a transform (YCCK), and such a block is unsupported.
#include "common.h"
#include "jpeg_core.h"

#include <cstring>
#include <unordered_map>

static_assert(sizeof(JpegTables) == TD_JPEG_TABSET_BYTES, "include/treedet.h: TD_JPEG_TABSET_BYTES");

namespace {

struct HuffSpec {
    bool def = false;
    uint8_t bits[17] = {};
    uint8_t vals[256] = {};
};

struct JpegHeader {
    uint16_t q[4][64] = {};
    bool qdef[4] = {};
    HuffSpec dc[4], ac[4];
    int restart = 0;
    bool sof = false, sos = false, jfif = false, adobe = false;
    int adobe_transform = 0;
    int width = 0, height = 0, ncomp = 0;
    int id[4] = {}, hs[4] = {}, vs[4] = {}, tq[4] = {};
    int td[4] = {}, ta[4] = {};
    int64_t entropy = 0;                 // offset of the entropy-coded data in the block
    const char* why = nullptr;           // set: unsupported / malformed
};

int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers of [p, p + n) from `pos` on, until SOS (scan = true: the block) or the end (the tables). A malformed or unsupported header
// sets h.why.
void walk_markers(JpegHeader& h, const uint8_t* p, int64_t n, int64_t pos, bool scan) {
    while (!h.why) {
        if (pos >= n) {
            if (scan) h.why = "no SOS";
            return;
        }
        if (p[pos] != 0xFF) {
            h.why = "bytes between markers";
            return;
        }
        while (pos < n && p[pos] == 0xFF) ++pos;             // fill bytes
        if (pos >= n) {
            h.why = "truncated marker";
            return;
        }
        const int m = p[pos++];
        if (m == 0xD8) continue;                             // SOI
        if (m == 0xD9) {                                     // EOI
            if (scan) h.why = "EOI before SOS";
            return;
        }
        if (pos + 2 > n) {
            h.why = "truncated segment";
            return;
        }
        const int len = be16(p + pos);
        if (len < 2 || pos + len > n) {
            h.why = "truncated segment";
            return;
        }
        const uint8_t* s = p + pos + 2;
        const int sl = len - 2;
        pos += len;
        if (m == 0xDB) {                                     // DQT
            for (int o = 0; o < sl;) {
                const int pq = s[o] >> 4, tq = s[o] & 15;
                const int need = 1 + 64 * (pq ? 2 : 1);
                if (pq > 1 || tq > 3 || o + need > sl) {
                    h.why = "bad DQT";
                    return;
                }
                for (int k = 0; k < 64; ++k) h.q[tq][jpeg_zigzag(k)] = (uint16_t)(pq ? be16(s + o + 1 + 2 * k) : s[o + 1 + k]);
                h.qdef[tq] = true;
                o += need;
            }
        } else if (m == 0xC4) {                              // DHT
            for (int o = 0; o < sl;) {
                if (o + 17 > sl) {
                    h.why = "bad DHT";
                    return;
                }
                const int tc = s[o] >> 4, th = s[o] & 15;
                int count = 0;
                for (int l = 1; l <= 16; ++l) count += s[o + l];
                if (tc > 1 || th > 3 || count > 256 || o + 17 + count > sl) {
                    h.why = "bad DHT";
                    return;
                }
                HuffSpec& t = tc ? h.ac[th] : h.dc[th];
                t.def = true;
                t.bits[0] = 0;
                for (int l = 1; l <= 16; ++l) t.bits[l] = s[o + l];
                std::memset(t.vals, 0, sizeof(t.vals));
                std::memcpy(t.vals, s + o + 17, (size_t)count);
                o += 17 + count;
            }
        } else if (m == 0xDD) {                              // DRI
            if (sl < 2) {
                h.why = "bad DRI";
                return;
            }
            h.restart = be16(s);
        } else if (m == 0xE0) {                              // APP0: JFIF (libjpeg wants 14 bytes of it)
            if (sl >= 14 && !std::memcmp(s, "JFIF\0", 5)) h.jfif = true;
        } else if (m == 0xEE) {                              // APP14: Adobe, the colour transform in its 12th byte
            if (sl >= 12 && !std::memcmp(s, "Adobe", 5)) {
                h.adobe = true;
                h.adobe_transform = s[11];
            }
        } else if ((m >= 0xE1 && m <= 0xEF) || m == 0xFE) {  // other APPn, COM
        } else if (!scan) {
            h.why = "a frame marker among the tables";
            return;
        } else if (m == 0xC0 || m == 0xC1) {                 // SOF0 / SOF1: sequential Huffman
            if (h.sof || sl < 6) {
                h.why = "bad SOF";
                return;
            }
            h.sof = true;
            const int prec = s[0];
            h.height = be16(s + 1);
            h.width = be16(s + 3);
            h.ncomp = s[5];
            if (prec != 8) {
                h.why = "not 8-bit";
                return;
            }
            if ((h.ncomp != 1 && h.ncomp != 3 && h.ncomp != 4) || sl < 6 + 3 * h.ncomp) {
                h.why = "component count";
                return;
            }
            if (h.width < 1 || h.height < 1) {
                h.why = "image size (DNL)";
                return;
            }
            for (int c = 0; c < h.ncomp; ++c) {
                h.id[c] = s[6 + 3 * c];
                h.hs[c] = s[7 + 3 * c] >> 4;
                h.vs[c] = s[7 + 3 * c] & 15;
                h.tq[c] = s[8 + 3 * c];
                if (h.hs[c] < 1 || h.hs[c] > 4 || h.vs[c] < 1 || h.vs[c] > 4 || h.tq[c] > 3) {
                    h.why = "bad SOF";
                    return;
                }
            }
        } else if (m == 0xDA) {                              // SOS: one interleaved scan of every component, in frame order
            if (!h.sof || sl < 1) {
                h.why = "SOS before SOF";
                return;
            }
            const int ns = s[0];
            if (ns != h.ncomp || sl < 1 + 2 * ns + 3) {
                h.why = "a scan of part of the components";
                return;
            }
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != h.id[c]) {
                    h.why = "scan order";
                    return;
                }
                h.td[c] = s[2 + 2 * c] >> 4;
                h.ta[c] = s[2 + 2 * c] & 15;
                if (h.td[c] > 3 || h.ta[c] > 3) {
                    h.why = "bad SOS";
                    return;
                }
            }
            const uint8_t* e = s + 1 + 2 * ns;
            if (e[0] != 0 || e[1] != 63 || e[2] != 0) {
                h.why = "not a sequential scan";
                return;
            }
            h.sos = true;
            h.entropy = pos;
            return;
        } else {                                             // progressive, lossless, arithmetic, hierarchical, DNL, ...
            h.why = "unsupported marker";
            return;
        }
    }
}

// T.81 annex C + F.2.2.3, plus a JPG_LOOK-bit lookup; the checks libjpeg applies (jpeg_make_d_derived_tbl). → false: a bad table.
bool build_huff(const HuffSpec& s, bool dc, JpegHuff& H) {
    std::memset(&H, 0, sizeof(H));
    int size[257], code[257];
    int p = 0;
    for (int l = 1; l <= 16; ++l)
        for (int i = 0; i < s.bits[l]; ++i) size[p++] = l;
    size[p] = 0;
    const int n = p;
    int c = 0, si = n ? size[0] : 0;
    p = 0;
    while (p < n) {
        while (p < n && size[p] == si) code[p++] = c++;
        if (c >= (1 << si)) return false;                    // no room left (the all-ones code of a length is reserved: libjpeg's check)
        c <<= 1;
        ++si;
    }
    p = 0;
    for (int l = 1; l <= 16; ++l) {
        if (s.bits[l]) {
            H.valoff[l] = p - code[p];
            p += s.bits[l];
            H.maxcode[l] = code[p - 1];
        } else {
            H.maxcode[l] = -1;
        }
    }
    H.maxcode[17] = 0x7fffffff;
    std::memcpy(H.vals, s.vals, sizeof(H.vals));
    for (int i = 0; i < n; ++i) {
        if (dc && s.vals[i] > 15) return false;
        if (size[i] <= JPG_LOOK) {
            const int sh = JPG_LOOK - size[i];
            for (int k = 0; k < (1 << sh); ++k) H.look[(code[i] << sh) | k] = (uint16_t)((size[i] << 8) | s.vals[i]);
        }
    }
    return true;
}

// A parsed block → mode (0 grey, 1 4:4:4, 2 4:2:2, 3 4:2:0, 4 four components as stored), colour transform, resolved tables.
// → false + why: unsupported.
bool resolve(JpegHeader& h, int& mode, int& ycc, JpegTables& T) {
    if (!h.sos) {
        if (!h.why) h.why = "no scan";
        return false;
    }
    if (h.ncomp == 1) {
        mode = 0;
    } else if (h.ncomp == 4) {                               // libjpeg: CMYK as stored, unless an Adobe segment says YCCK (any transform but 0)
        for (int c = 0; c < 4; ++c)
            if (h.hs[c] != 1 || h.vs[c] != 1) {
                h.why = "sampling of a four-component frame";
                return false;
            }
        if (h.adobe && h.adobe_transform != 0) {
            h.why = "YCCK";
            return false;
        }
        mode = 4;
    } else {
        for (int c = 1; c < 3; ++c)
            if (h.hs[c] != 1 || h.vs[c] != 1) {
                h.why = "chroma sampling";
                return false;
            }
        if (h.hs[0] == 1 && h.vs[0] == 1) mode = 1;
        else if (h.hs[0] == 2 && h.vs[0] == 1) mode = 2;
        else if (h.hs[0] == 2 && h.vs[0] == 2) mode = 3;
        else {
            h.why = "luma sampling";
            return false;
        }
    }
    if (h.ncomp == 3) {                                      // libjpeg's default_decompress_parms for three components
        if (h.jfif) ycc = 1;
        else if (h.adobe) ycc = h.adobe_transform != 0;
        else ycc = !(h.id[0] == 82 && h.id[1] == 71 && h.id[2] == 66);
    } else {
        ycc = 0;
    }
    std::memset(&T, 0, sizeof(T));
    for (int c = 0; c < h.ncomp; ++c) {
        if (!h.qdef[h.tq[c]] || !h.dc[h.td[c]].def || !h.ac[h.ta[c]].def) {
            h.why = "a table the scan uses is not defined";
            return false;
        }
        std::memcpy(T.q[c], h.q[h.tq[c]], sizeof(T.q[c]));
        if (!build_huff(h.dc[h.td[c]], true, T.dc[c]) || !build_huff(h.ac[h.ta[c]], false, T.ac[c])) {
            h.why = "bad Huffman table";
            return false;
        }
    }
    return true;
}

// The entropy-coded data of a block [e0, n) → its segments: one, or one per restart interval, cut at RST0..7 in sequence. → the
// segment count, or -1 (markers out of sequence / missing: corrupt).
struct Seg { int64_t off, len; uint32_t mcu0, nmcu; };
int cut_segments(const uint8_t* p, int64_t e0, int64_t n, uint32_t nmcu, int restart, std::vector<Seg>& out) {
    if (restart <= 0 || (uint32_t)restart >= nmcu) {
        out.push_back({e0, n - e0, 0, nmcu});
        return 1;
    }
    const uint32_t nseg = (nmcu + (uint32_t)restart - 1) / (uint32_t)restart;
    int64_t start = e0, pos = e0;
    for (uint32_t i = 0; i + 1 < nseg; ++i) {
        for (;;) {
            const void* f = pos < n ? std::memchr(p + pos, 0xFF, (size_t)(n - pos)) : nullptr;
            if (!f) return -1;
            pos = static_cast<const uint8_t*>(f) - p;
            if (pos + 1 >= n) return -1;
            const int nb = p[pos + 1];
            if (nb == 0x00 || nb == 0xFF) {
                pos += 1 + (nb == 0x00);
                continue;
            }
            if (nb != 0xD0 + (int)(i & 7)) return -1;
            break;
        }
        out.push_back({start, pos - start, i * (uint32_t)restart, (uint32_t)restart});
        pos += 2;
        start = pos;
    }
    out.push_back({start, n - start, (nseg - 1) * (uint32_t)restart, nmcu - (nseg - 1) * (uint32_t)restart});
    return (int)nseg;
}

uint64_t fnv1a(const void* data, size_t n) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

}  // namespace

extern "C" td_status td_tiff_jpeg_plan(const uint8_t* tables, int64_t tables_len, const uint8_t* data, const int64_t* block_off,
                                       const int64_t* block_nbytes, int nblocks, int photometric, int bands, int block_w,
                                       const int32_t* block_rows, int64_t* block_info, int64_t* segs, int64_t seg_cap, void* tabsets,
                                       int64_t tabset_cap, int64_t* totals) {
    if ((tables_len > 0 && !tables) || tables_len < 0 || !data || !block_off || !block_nbytes || nblocks < 0 || !block_rows || !block_info ||
        !totals || seg_cap < 0 || tabset_cap < 0 || (seg_cap > 0 && !segs) || (tabset_cap > 0 && !tabsets) || (bands != 1 && bands != 3 && bands != 4) ||
        block_w < 1) {
        td_set_error("td_tiff_jpeg_plan: bad argument");
        return TD_ERR_INVALID;
    }
    // the tables once (tables_len 0: no JPEGTables tag; otherwise SOI ... EOI, as the reader requires)
    JpegHeader base;
    if (tables_len > 0) {
        if (tables_len < 4 || tables[0] != 0xFF || tables[1] != 0xD8) base.why = "JPEGTables without SOI";
        else walk_markers(base, tables, tables_len, 2, false);
    }
    JpegTables* sets = static_cast<JpegTables*>(tabsets);
    std::unordered_map<uint64_t, std::vector<int64_t>> seen;
    std::vector<JpegTables> kept;                            // every distinct set (for the comparison when the caller's array is full)
    std::vector<Seg> cut;
    int64_t nseg = 0, coef = 0, unsupported = 0;
    JpegTables T;
    for (int b = 0; b < nblocks; ++b) {
        int64_t* info = block_info + (int64_t)b * 8;
        for (int k = 0; k < 8; ++k) info[k] = 0;
        const uint8_t* p = data + block_off[b];
        const int64_t n = block_nbytes[b];
        JpegHeader h = base;
        int mode = 0, ycc = 0;
        bool ok = !h.why && n >= 4 && block_off[b] >= 0 && p[0] == 0xFF && p[1] == 0xD8;
        if (ok) {
            if (bands == 3) {                                // the reader's Adobe segment comes first: the block's own markers follow it
                bool jfif = false;
                for (int64_t i = 0; i + 5 <= (n < 32 ? n : 32); ++i) jfif |= !std::memcmp(p + i, "JFIF\0", 5);
                if (!jfif && !base.adobe) {                  // (an Adobe segment among the tables comes later and wins)
                    h.adobe = true;
                    h.adobe_transform = photometric == 6;
                }
            }
            walk_markers(h, p, n, 2, true);
            ok = resolve(h, mode, ycc, T) && h.ncomp == bands && h.width == block_w && h.height >= block_rows[b];
        }
        cut.clear();
        const JpegGeom g = jpeg_geom(mode, h.width, h.height);
        if (ok) ok = cut_segments(p, h.entropy, n, (uint32_t)g.mcus_x * (uint32_t)g.mcus_y, h.restart, cut) > 0;
        if (!ok) {
            info[0] = 1;
            ++unsupported;
            continue;
        }
        const uint64_t key = fnv1a(&T, sizeof(T));
        int64_t set = -1;
        for (int64_t s : seen[key])
            if (!std::memcmp(&kept[(size_t)s], &T, sizeof(T))) set = s;
        if (set < 0) {
            set = (int64_t)kept.size();
            kept.push_back(T);
            seen[key].push_back(set);
            if (set < tabset_cap) std::memcpy(&sets[set], &T, sizeof(T));
        }
        info[1] = set;
        info[2] = mode;
        info[3] = ycc;
        info[4] = h.width;
        info[5] = h.height;
        info[6] = coef;
        info[7] = h.restart;
        for (const Seg& s : cut) {
            if (nseg < seg_cap) {
                int64_t* o = segs + nseg * 4;
                o[0] = block_off[b] + s.off;
                o[1] = s.len;
                o[2] = b;
                o[3] = (int64_t)s.mcu0 | ((int64_t)s.nmcu << 32);
            }
            ++nseg;
        }
        coef += g.total;
    }
    totals[0] = nseg;
    totals[1] = (int64_t)kept.size();
    totals[2] = coef;
    totals[3] = unsupported;
    if (nseg > seg_cap || (int64_t)kept.size() > tabset_cap) {
        td_set_error("td_tiff_jpeg_plan: %lld segments / %lld table sets, room for %lld / %lld", (long long)nseg, (long long)kept.size(),
                     (long long)seg_cap, (long long)tabset_cap);
        return TD_ERR_CAPACITY;
    }
    return TD_OK;
}

namespace {

// One segment of a complete stream: the sequential decoder (subseq == 0), or the window procedure with `lanes` emulated lanes and the
// DC pass that follows it.
template <bool FOUR>
int decode_one_segment(const JpegTables& T, const JpegGeom& g, const uint8_t* src, const Seg& s, int16_t* coef, int subseq, int lanes,
                       int64_t* stats) {
    if (subseq == 0) return jpeg_decode_segment<FOUR>(T, g, src + s.off, (uint32_t)s.len, s.mcu0, s.nmcu, coef);
    if (jpeg_sync_segment<FOUR>(T, g, src + s.off, (uint32_t)s.len, s.mcu0, s.nmcu, coef, (uint32_t)subseq, lanes, stats)) return 1;
    return jpeg_sync_dc<FOUR>(T, g, s.mcu0, s.nmcu, coef);
}

// td_jpeg_decode (subseq == 0) and td_jpeg_decode_sync: everything but the entropy decoding of a segment is the same code.
int64_t decode_stream(const char* name, const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* shape, int subseq, int lanes,
                      int64_t* stats) {
    if (!src || n < 0 || !dst || cap < 0 || !shape || n >= ((int64_t)1 << 31)) {
        td_set_error("%s: bad argument", name);
        return TD_ERR_INVALID;
    }
    JpegHeader h;
    int mode = 0, ycc = 0;
    static thread_local JpegTables T;
    if (n < 4 || src[0] != 0xFF || src[1] != 0xD8) h.why = "no SOI";
    else walk_markers(h, src, n, 2, true);
    if (h.why || !resolve(h, mode, ycc, T)) {
        td_set_error("%s: unsupported stream (%s)", name, h.why ? h.why : "?");
        return TD_ERR_UNSUPPORTED;
    }
    shape[0] = h.height;
    shape[1] = h.width;
    shape[2] = h.ncomp;
    const int64_t need = (int64_t)h.width * h.height * h.ncomp;
    if (need > cap) {
        td_set_error("%s: %lld bytes, capacity %lld", name, (long long)need, (long long)cap);
        return TD_ERR_CAPACITY;
    }
    const JpegGeom g = jpeg_geom(mode, h.width, h.height);
    std::vector<Seg> cut;
    if (cut_segments(src, h.entropy, n, (uint32_t)g.mcus_x * (uint32_t)g.mcus_y, h.restart, cut) < 0) {
        td_set_error("%s: restart markers missing or out of sequence", name);
        return TD_ERR_INVALID;
    }
    std::vector<int16_t> coef((size_t)g.total, 0);
    for (size_t i = 0; i < cut.size(); ++i)
        if (mode == 4 ? decode_one_segment<true>(T, g, src, cut[i], coef.data(), subseq, lanes, stats)
                      : decode_one_segment<false>(T, g, src, cut[i], coef.data(), subseq, lanes, stats)) {
            td_set_error("%s: corrupt entropy-coded data (segment %d)", name, (int)i);
            return TD_ERR_INVALID;
        }
    std::vector<uint8_t> planes((size_t)g.total);
    for (int c = 0; c < g.ncomp; ++c)
        for (int by = 0; by < g.bh[c]; ++by)
            for (int bx = 0; bx < g.bw[c]; ++bx)
                jpeg_idct_islow(coef.data() + g.off[c] + ((int64_t)by * g.bw[c] + bx) * 64, T.q[c],
                                planes.data() + g.off[c] + (int64_t)by * 8 * (g.bw[c] * 8) + bx * 8, g.bw[c] * 8);
    for (int y = 0; y < h.height; ++y)
        for (int x = 0; x < h.width; ++x) {
            uint8_t* px = dst + ((int64_t)y * h.width + x) * h.ncomp;
            if (mode == 4) {
                const uint32_t v = jpeg_pixel4(planes.data(), g.mcus_x, g.mcus_y, x, y);
                for (int c = 0; c < 4; ++c) px[c] = (uint8_t)(v >> (8 * c));
            } else {
                jpeg_pixel(planes.data(), g, ycc, x, y, px);
            }
        }
    return need;
}

}  // namespace

extern "C" int64_t td_jpeg_decode(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* shape) {
    return decode_stream("td_jpeg_decode", src, n, dst, cap, shape, 0, 0, nullptr);
}

extern "C" int64_t td_jpeg_decode_sync(const uint8_t* src, int64_t n, uint8_t* dst, int64_t cap, int32_t* shape, int subseq_bytes, int lanes,
                                       int64_t* stats) {
    if (subseq_bytes < JPG_SYNC_MIN_SUBSEQ || subseq_bytes > JPG_SYNC_MAX_SUBSEQ || lanes < 1 || lanes > 64) {
        td_set_error("td_jpeg_decode_sync: subsequences of %d bytes (%d .. %d), %d lanes (1 .. 64)", subseq_bytes, JPG_SYNC_MIN_SUBSEQ,
                     JPG_SYNC_MAX_SUBSEQ, lanes);
        return TD_ERR_INVALID;
    }
    if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
    return decode_stream("td_jpeg_decode_sync", src, n, dst, cap, shape, subseq_bytes, lanes, stats);
}
