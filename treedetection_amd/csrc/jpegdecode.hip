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
