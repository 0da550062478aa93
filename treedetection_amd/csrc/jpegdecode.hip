// JPEG-in-TIFF (compression 7) rasters decoded on the GPU: the decoder of jpeg_core.h (the one td_jpeg_decode runs on the host), in
// three launches on the caller's stream after the host plan (jpegcodec.cpp: td_tiff_jpeg_plan) has parsed every block's headers once:
//   1. entropy decoding, ONE LANE per entropy-coded segment (a block, or one restart interval of it) — a Huffman stream is
//      sequential, the parallelism is the 10^3 - 10^5 segments of a raster. The waves take 64 segments at a time from a per-launch
//      counter (td_decode_ticket, as the LZW / DEFLATE decoders take blocks), one workgroup per CU at most, so a raster that decodes
//      beside the forwards leaves whole CUs to them. Coefficients land in a zeroed int16 buffer (only the non-zero ones are written);
//   2. dequantisation + the accurate integer IDCT, one thread per 8x8 block → the component planes (uint8);
//   3. fancy upsampling + YCbCr → RGB, one thread per raster pixel → image [height][width][bands], each block cropped to the raster.
// Four bands (mode 4: four components sampled 1x1, stored as they decode) take an instantiation of their own of the entropy kernel
// (four DC predictors, four blocks per MCU; the one- and three-component instantiation keeps its registers) and a pixel kernel that
// gathers the four plane samples of a pixel and writes them as ONE dword: a wave stores 256 contiguous bytes.
// Segments too long for one lane (blocks without restart markers: td_tiff_jpeg_decode_long_dev) take launch 1 in another form: ONE WAVE
// per segment, its 64 lanes walking 64 consecutive subsequences of the bytes from guessed decoder states until the states agree
// (self-synchronising Huffman decoding; jpeg_core.h describes the procedure and runs it on the host), then a launch that turns the DC
// differences the waves stored into DC values. Launches 2 and 3 are the same.
#include "common.h"
#include "jpeg_core.h"

namespace {

constexpr int JPG_WPB = 4;               // waves per workgroup of the entropy launch (no LDS: the tables are read through the caches)

template <bool FOUR>
__global__ __launch_bounds__(64 * JPG_WPB) void jpeg_entropy_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ info,
                                                                   const int64_t* __restrict__ segs, int nseg,
                                                                   const JpegTables* __restrict__ sets, int16_t* __restrict__ coef,
                                                                   int32_t* __restrict__ status, int* __restrict__ ticket) {
    const int lane = (int)threadIdx.x & 63;
    for (;;) {
        int first = 0;
        if (lane == 0) first = atomicAdd(ticket, 64);
        first = __builtin_amdgcn_readfirstlane(first);
        if (first >= nseg) break;                          // whole waves leave
        const int s = first + lane;
        if (s < nseg) {
            const int64_t* sg = segs + (int64_t)s * 4;
            const int64_t b = sg[2];
            const int64_t* bi = info + b * 8;
            const JpegGeom g = jpeg_geom((int)bi[2], (int)bi[4], (int)bi[5]);
            const uint64_t mm = (uint64_t)sg[3];
            if (jpeg_decode_segment<FOUR>(sets[bi[1]], g, comp + sg[0], (uint32_t)sg[1], (uint32_t)mm, (uint32_t)(mm >> 32), coef + bi[6]))
                status[b] = 1;
        }
    }
}

// ---- long segments: one wave per segment (jpeg_core.h: jpeg_sync_segment is this procedure on emulated lanes) -----------------------
constexpr int JPG_SYNC_WPB = 4;          // waves per workgroup, each with the table set of its segment in LDS (4 x 11 904 bytes)

__device__ __forceinline__ uint64_t jpeg_shfl_up1(uint64_t v) {          // lane i ← lane i - 1 (lane 0 keeps its own)
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint64_t jpeg_shfl(uint64_t v, int from) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, from), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), from);
    return (uint64_t)hi << 32 | lo;
}
__device__ __forceinline__ uint32_t jpeg_wave_scan(uint32_t v, int lane) {   // inclusive prefix sum over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// Every loop is bounded by data the host plan fixed: the ticket loop by nseg, the window loop by the segment's bytes (nsub windows of
// 64 subsequences), the rounds by 64 (one more validated lane per round), a walk by its subsequence — or, in the segment's last one,
// by the bytes that are left: a walk that consumes a bit past them is lost. No workgroup barrier: a wave never waits for another.
template <bool FOUR>
__global__ __launch_bounds__(64 * JPG_SYNC_WPB) void jpeg_entropy_sync_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ info,
                                                                             const int64_t* __restrict__ segs, int nseg,
                                                                             const JpegTables* __restrict__ sets, int16_t* __restrict__ coef,
                                                                             int32_t* __restrict__ status, int* __restrict__ ticket, uint32_t S,
                                                                             unsigned long long* __restrict__ stats) {
    __shared__ JpegTables lds[JPG_SYNC_WPB];
    const int lane = (int)threadIdx.x & 63;
    JpegTables& T = lds[threadIdx.x >> 6];
    int staged = -1;
    for (;;) {
        int s = 0;
        if (lane == 0) s = atomicAdd(ticket, 1);
        s = __builtin_amdgcn_readfirstlane(s);
        if (s >= nseg) break;
        const int64_t* sg = segs + (int64_t)s * 4;
        const int b = __builtin_amdgcn_readfirstlane((int)sg[2]);
        const int64_t* bi = info + (int64_t)b * 8;
        const int set = __builtin_amdgcn_readfirstlane((int)bi[1]);
        const JpegGeom g = jpeg_geom(__builtin_amdgcn_readfirstlane((int)bi[2]), __builtin_amdgcn_readfirstlane((int)bi[4]),
                                     __builtin_amdgcn_readfirstlane((int)bi[5]));
        if (set != staged) {                               // the wave's table set, a dword per lane and step
            const uint32_t* from = reinterpret_cast<const uint32_t*>(sets + set);
            uint32_t* to = reinterpret_cast<uint32_t*>(&T);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");       // (the lanes have done with the set that goes)
            for (int i = lane; i < (int)(sizeof(JpegTables) / 4); i += 64) to[i] = from[i];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            staged = set;
        }
        const uint8_t* src = comp + sg[0];
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sg[1]);
        const uint64_t mm = (uint64_t)sg[3];
        const uint32_t mcu0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)mm);
        const uint32_t nmcu = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(mm >> 32));
        int16_t* cb = coef + bi[6];
        const uint32_t total = nmcu * (uint32_t)jpeg_sync_blocks_per_mcu(g, FOUR);
        const uint32_t nsub = n > S ? (uint32_t)(((uint64_t)n + S - 1) / S) : 1u;
        JpegSyncState carry = jpeg_sync_state(0, 0, 0, 0);
        uint32_t base = 0;
        bool bad = false, finished = false;
        int none = 0;
        for (uint32_t w0 = 0; w0 < nsub; w0 += 64) {
            const int L = (int)(nsub - w0 < 64u ? nsub - w0 : 64u);
            const bool active = lane < L;
            const uint32_t sub = w0 + (uint32_t)lane;
            const uint32_t end = sub == nsub - 1 ? JPG_SYNC_NO_END : (sub + 1) * S;
            JpegSyncState entry = lane == 0 ? carry : (active ? jpeg_sync_guess(src, n, sub, S) : JPG_SYNC_LOST), exit = JPG_SYNC_LOST;
            uint32_t cnt = 0;
            bool walk = active;
            int rounds = 1, valid = 0;
            for (int it = 0; it < 64; ++it) {
                if (walk) exit = jpeg_sync_walk<FOUR, false>(T, g, src, n, entry, end, cnt, nullptr, 0, 0, 0, none);
                const JpegSyncState prev = jpeg_shfl_up1(exit);
                const unsigned long long ok = __ballot(lane == 0 || !active || entry == prev);
                valid = ~ok ? __builtin_ctzll(~ok) : 64;   // the validated lanes: the leading run of lanes that entered where their predecessor left
                if (valid > L) valid = L;
                if (valid == L || jpeg_shfl(exit, valid - 1) == JPG_SYNC_LOST) break;
                walk = active && lane > 0 && prev != JPG_SYNC_LOST && prev != entry;
                if (walk) entry = prev;
                ++rounds;
            }
            const uint32_t mine = lane < valid ? cnt : 0u, upto = jpeg_wave_scan(mine, lane), first = base + upto - mine;
            int flags = 0;
            if (lane < valid && first < total) {           // (an ordinal at or past the segment's last block: nothing is stored)
                uint32_t wrote;
                jpeg_sync_walk<FOUR, true>(T, g, src, n, entry, end, wrote, cb, mcu0, first, total - first, flags);
            }
            if (lane == 0) {
                atomicAdd(stats, (unsigned long long)rounds);
                atomicAdd(stats + 1, 1ull);
                atomicMax(stats + 2, (unsigned long long)rounds);
                if (rounds == 1) atomicAdd(stats + 3, 1ull);
            }
            base += (uint32_t)__shfl((int)upto, 63);
            bad = __ballot(flags & 1) != 0;
            finished = __ballot(flags & 2) != 0;
            if (bad || finished || valid < L) break;
            carry = jpeg_shfl(exit, L - 1);
        }
        if ((bad || !finished) && lane == 0) status[b] = 1;
    }
}

// One wave per (long segment, component): the DC differences the waves above stored, summed in scan order 64 blocks a step with a
// carried sum, checked and stored as jpeg_block does. The loop is bounded by the segment's MCU count.
template <bool FOUR>
__global__ __launch_bounds__(64) void jpeg_dc_scan_kernel(const int64_t* __restrict__ info, const int64_t* __restrict__ segs, int nseg, int ncomp,
                                                          const JpegTables* __restrict__ sets, int16_t* __restrict__ coef,
                                                          int32_t* __restrict__ status) {
    const int lane = (int)threadIdx.x, s = (int)(blockIdx.x / (unsigned)ncomp), c = (int)(blockIdx.x % (unsigned)ncomp);
    if (s >= nseg) return;
    const int64_t* sg = segs + (int64_t)s * 4;
    const int64_t b = sg[2];
    const int64_t* bi = info + b * 8;
    const JpegGeom g = jpeg_geom((int)bi[2], (int)bi[4], (int)bi[5]);
    if (c >= g.ncomp) return;
    const uint64_t mm = (uint64_t)sg[3];
    const uint32_t mcu0 = (uint32_t)mm, nb = jpeg_sync_dc_blocks(g, FOUR, c, (uint32_t)(mm >> 32));
    const uint16_t q0 = sets[bi[1]].q[c][0];
    int16_t* cb = coef + bi[6];
    uint32_t carry = 0;
    bool bad = false;
    for (uint32_t t0 = 0; t0 < nb; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)lane;
        int16_t* blk = t < nb ? cb + jpeg_sync_dc_block_at<FOUR>(g, mcu0, c, t) : nullptr;
        const uint32_t upto = jpeg_wave_scan(blk ? (uint32_t)(int32_t)blk[0] : 0u, lane), pred = carry + upto;
        if (blk) {
            bad |= !jpeg_coef_ok((int32_t)pred, q0);
            blk[0] = (int16_t)(int32_t)pred;
        }
        carry += (uint32_t)__shfl((int)upto, 63);
    }
    if (__ballot(bad) && lane == 0) status[b] = 1;
}

// the block whose coefficients hold element e: the last b with info[b][6] <= e (blocks are laid out in order)
__device__ __forceinline__ int jpeg_find_block(const int64_t* __restrict__ info, int nblocks, int64_t e) {
    int lo = 0, hi = nblocks - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (info[(int64_t)mid * 8 + 6] <= e) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, int64_t nblk8, const int64_t* __restrict__ info,
                                                        int nblocks, const JpegTables* __restrict__ sets, uint8_t* __restrict__ planes) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nblk8) return;
    const int64_t e = k * 64;
    const int b = jpeg_find_block(info, nblocks, e);
    const int64_t* bi = info + (int64_t)b * 8;
    const JpegGeom g = jpeg_geom((int)bi[2], (int)bi[4], (int)bi[5]);
    const int64_t local = e - bi[6];
    int c = 0;
    while (c + 1 < g.ncomp && local >= g.off[c + 1]) ++c;
    const int64_t idx = (local - g.off[c]) >> 6;
    const int by = (int)(idx / g.bw[c]), bx = (int)(idx - (int64_t)by * g.bw[c]);
    if (by >= g.bh[c]) return;                              // (past the last component: nothing of a block lies there)
    alignas(16) int16_t in[64];
    const int4* src = reinterpret_cast<const int4*>(coef + e);
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<int4*>(in)[i] = src[i];
    const int stride = g.bw[c] * 8;
    jpeg_idct_islow(in, sets[bi[1]].q[c], planes + bi[6] + g.off[c] + (int64_t)by * 8 * stride + bx * 8, stride);
}

template <int BANDS>
__global__ __launch_bounds__(256) void jpeg_pixels_kernel(const uint8_t* __restrict__ planes, const int64_t* __restrict__ info, int width,
                                                          int height, int block_w, int block_h, int blocks_across,
                                                          uint8_t* __restrict__ image) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)width * height) return;
    const int Y = (int)(p / width), X = (int)(p - (int64_t)Y * width);
    const int by = Y / block_h, bx = X / block_w;
    const int64_t* bi = info + ((int64_t)by * blocks_across + bx) * 8;
    const int x = X - bx * block_w, y = Y - by * block_h;
    const int w = (int)bi[4], h = (int)bi[5];
    uint8_t px[3] = {0, 0, 0};
    if (x < w && y < h) {                                   // (the plan has checked that every block covers its pixels)
        const JpegGeom g = jpeg_geom((int)bi[2], w, h);
        jpeg_pixel(planes + bi[6], g, (int)bi[3], x, y, px);
    }
#pragma unroll
    for (int c = 0; c < BANDS; ++c) image[p * BANDS + c] = px[c];
}

// Mode 4, one thread per raster pixel: the four planes of a block are read along x (a wave reads 64 consecutive bytes of each inside
// a block), the pixel leaves as one 32-bit store — consecutive lanes, consecutive dwords. Pixels a block does not cover (the plan has
// checked that there are none) are written as zero.
__global__ __launch_bounds__(256) void jpeg_pixels4_kernel(const uint8_t* __restrict__ planes, const int64_t* __restrict__ info, int width,
                                                           int height, int block_w, int block_h, int blocks_across,
                                                           uint32_t* __restrict__ image) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)width * height) return;
    const int Y = (int)(p / width), X = (int)(p - (int64_t)Y * width);
    const int by = Y / block_h, bx = X / block_w;
    const int64_t* bi = info + ((int64_t)by * blocks_across + bx) * 8;
    const int x = X - bx * block_w, y = Y - by * block_h;
    const int w = (int)bi[4], h = (int)bi[5];
    uint32_t v = 0;
    if (x < w && y < h) v = jpeg_pixel4(planes + bi[6], (w + 7) >> 3, (h + 7) >> 3, x, y);
    image[p] = v;
}

// launches 2 and 3 on s: the IDCT of every 8x8 block, then the pixels
td_status jpeg_planes_and_pixels(const int64_t* block_info, int nblocks, const void* tabsets, const int16_t* coef, uint8_t* planes,
                                 int64_t coef_count, uint8_t* image, int width, int height, int bands, int block_w, int block_h,
                                 int blocks_across, hipStream_t s) {
    const int64_t nblk8 = coef_count / 64;
    if (nblk8 > 0) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nblk8 + 255) / 256)), dim3(256), 0, s, coef, nblk8, block_info, nblocks,
                           static_cast<const JpegTables*>(tabsets), planes);
        TD_KERNEL_CHECK();
    }
    const int64_t npx = (int64_t)width * height;
    const dim3 grid((unsigned)((npx + 255) / 256));
    if (bands == 4) hipLaunchKernelGGL(jpeg_pixels4_kernel, grid, dim3(256), 0, s, planes, block_info, width, height, block_w, block_h,
                                       blocks_across, reinterpret_cast<uint32_t*>(image));
    else if (bands == 1) hipLaunchKernelGGL(jpeg_pixels_kernel<1>, grid, dim3(256), 0, s, planes, block_info, width, height, block_w, block_h,
                                       blocks_across, image);
    else hipLaunchKernelGGL(jpeg_pixels_kernel<3>, grid, dim3(256), 0, s, planes, block_info, width, height, block_w, block_h,
                            blocks_across, image);
    TD_KERNEL_CHECK();
    return TD_OK;
}

}  // namespace

extern "C" td_status td_tiff_jpeg_decode_dev(const uint8_t* comp, const int64_t* block_info, int nblocks, const int64_t* segs, int nseg,
                                             const void* tabsets, int16_t* coef, uint8_t* planes, int64_t coef_count, int32_t* status,
                                             uint8_t* image, int width, int height, int bands, int block_w, int block_h, int blocks_across,
                                             void* stream) {
    TD_REQUIRE(comp && block_info && segs && tabsets && coef && planes && status && image, "td_tiff_jpeg_decode_dev: null pointer");
    TD_REQUIRE(nblocks >= 1 && nseg >= nblocks && coef_count >= 0 && coef_count % 64 == 0, "td_tiff_jpeg_decode_dev: %d blocks, %d segments, "
               "%lld coefficients", nblocks, nseg, (long long)coef_count);
    TD_REQUIRE((bands == 1 || bands == 3 || bands == 4) && width >= 1 && height >= 1 && block_w >= 1 && block_h >= 1 && blocks_across >= 1 &&
               (int64_t)blocks_across * block_w >= width && (int64_t)(blocks_across - 1) * block_w < width &&
               nblocks % blocks_across == 0 &&
               (int64_t)(nblocks / blocks_across) * block_h >= height && (int64_t)(nblocks / blocks_across - 1) * block_h < height,
               "td_tiff_jpeg_decode_dev: %d blocks of %d x %d (%d across) do not tile a %d x %d raster", nblocks, block_w, block_h,
               blocks_across, width, height);
    TD_REQUIRE(reinterpret_cast<uintptr_t>(coef) % 16 == 0, "td_tiff_jpeg_decode_dev: coef must be 16-byte aligned");
    TD_REQUIRE(bands != 4 || reinterpret_cast<uintptr_t>(image) % 4 == 0, "td_tiff_jpeg_decode_dev: a four-band image must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    TD_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)coef_count * sizeof(int16_t), s));
    TD_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)nblocks * sizeof(int32_t), s));
    int* ticket = nullptr;
    int cus = 0;
    const td_status tst = td_decode_ticket(s, &ticket, &cus);
    if (tst < 0) return tst;
    const int waves = (nseg + 63) / 64;
    const int groups = (waves + JPG_WPB - 1) / JPG_WPB < cus ? (waves + JPG_WPB - 1) / JPG_WPB : cus;
    // (the plan gives a raster of four bands blocks of mode 4 only, and the others none of them)
    hipLaunchKernelGGL(bands == 4 ? jpeg_entropy_kernel<true> : jpeg_entropy_kernel<false>, dim3(groups), dim3(64 * JPG_WPB), 0, s, comp,
                       block_info, segs, nseg, static_cast<const JpegTables*>(tabsets), coef, status, ticket);
    TD_KERNEL_CHECK();
    return jpeg_planes_and_pixels(block_info, nblocks, tabsets, coef, planes, coef_count, image, width, height, bands, block_w, block_h,
                                  blocks_across, s);
}

extern "C" td_status td_tiff_jpeg_decode_long_dev(const uint8_t* comp, const int64_t* block_info, int nblocks, const int64_t* segs_short,
                                                  int nshort, const int64_t* segs_long, int nlong, int subseq_bytes, const void* tabsets,
                                                  int16_t* coef, uint8_t* planes, int64_t coef_count, int32_t* status, int64_t* stats,
                                                  uint8_t* image, int width, int height, int bands, int block_w, int block_h,
                                                  int blocks_across, void* stream) {
    TD_REQUIRE(comp && block_info && tabsets && coef && planes && status && stats && image && (segs_short || nshort == 0) &&
               (segs_long || nlong == 0), "td_tiff_jpeg_decode_long_dev: null pointer");
    TD_REQUIRE(nblocks >= 1 && nshort >= 0 && nlong >= 0 && (int64_t)nshort + nlong >= nblocks && (int64_t)nshort + nlong < ((int64_t)1 << 31) &&
               coef_count >= 0 && coef_count % 64 == 0, "td_tiff_jpeg_decode_long_dev: %d blocks, %d + %d segments, %lld coefficients", nblocks,
               nshort, nlong, (long long)coef_count);
    TD_REQUIRE(subseq_bytes >= JPG_SYNC_MIN_SUBSEQ && subseq_bytes <= JPG_SYNC_MAX_SUBSEQ, "td_tiff_jpeg_decode_long_dev: subsequences of %d bytes "
               "(%d .. %d)", subseq_bytes, JPG_SYNC_MIN_SUBSEQ, JPG_SYNC_MAX_SUBSEQ);
    TD_REQUIRE((bands == 1 || bands == 3 || bands == 4) && width >= 1 && height >= 1 && block_w >= 1 && block_h >= 1 && blocks_across >= 1 &&
               (int64_t)blocks_across * block_w >= width && (int64_t)(blocks_across - 1) * block_w < width &&
               nblocks % blocks_across == 0 &&
               (int64_t)(nblocks / blocks_across) * block_h >= height && (int64_t)(nblocks / blocks_across - 1) * block_h < height,
               "td_tiff_jpeg_decode_long_dev: %d blocks of %d x %d (%d across) do not tile a %d x %d raster", nblocks, block_w, block_h,
               blocks_across, width, height);
    TD_REQUIRE(reinterpret_cast<uintptr_t>(coef) % 16 == 0, "td_tiff_jpeg_decode_long_dev: coef must be 16-byte aligned");
    TD_REQUIRE(reinterpret_cast<uintptr_t>(stats) % 8 == 0, "td_tiff_jpeg_decode_long_dev: stats must be 8-byte aligned");
    TD_REQUIRE(bands != 4 || reinterpret_cast<uintptr_t>(image) % 4 == 0, "td_tiff_jpeg_decode_long_dev: a four-band image must be 4-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const JpegTables* sets = static_cast<const JpegTables*>(tabsets);
    TD_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)coef_count * sizeof(int16_t), s));
    TD_HIP_CHECK(hipMemsetAsync(status, 0, (size_t)nblocks * sizeof(int32_t), s));
    TD_HIP_CHECK(hipMemsetAsync(stats, 0, 4 * sizeof(int64_t), s));
    if (nshort > 0) {                                      // the lane-per-segment kernel, launched as td_tiff_jpeg_decode_dev launches it
        int* ticket = nullptr;
        int cus = 0;
        const td_status tst = td_decode_ticket(s, &ticket, &cus);
        if (tst < 0) return tst;
        const int waves = (nshort + 63) / 64;
        const int groups = (waves + JPG_WPB - 1) / JPG_WPB < cus ? (waves + JPG_WPB - 1) / JPG_WPB : cus;
        hipLaunchKernelGGL(bands == 4 ? jpeg_entropy_kernel<true> : jpeg_entropy_kernel<false>, dim3(groups), dim3(64 * JPG_WPB), 0, s, comp,
                           block_info, segs_short, nshort, sets, coef, status, ticket);
        TD_KERNEL_CHECK();
    }
    if (nlong > 0) {
        int* ticket = nullptr;
        int cus = 0;
        const td_status tst = td_decode_ticket(s, &ticket, &cus);
        if (tst < 0) return tst;
        const int groups = (nlong + JPG_SYNC_WPB - 1) / JPG_SYNC_WPB < cus ? (nlong + JPG_SYNC_WPB - 1) / JPG_SYNC_WPB : cus;
        hipLaunchKernelGGL(bands == 4 ? jpeg_entropy_sync_kernel<true> : jpeg_entropy_sync_kernel<false>, dim3(groups), dim3(64 * JPG_SYNC_WPB), 0,
                           s, comp, block_info, segs_long, nlong, sets, coef, status, ticket, (uint32_t)subseq_bytes,
                           reinterpret_cast<unsigned long long*>(stats));
        TD_KERNEL_CHECK();
        const int ncomp = bands == 1 ? 1 : bands;
        hipLaunchKernelGGL(bands == 4 ? jpeg_dc_scan_kernel<true> : jpeg_dc_scan_kernel<false>, dim3((unsigned)nlong * (unsigned)ncomp), dim3(64), 0, s,
                           block_info, segs_long, nlong, ncomp, sets, coef, status);
        TD_KERNEL_CHECK();
    }
    return jpeg_planes_and_pixels(block_info, nblocks, tabsets, coef, planes, coef_count, image, width, height, bands, block_w, block_h,
                                  blocks_across, s);
}
