// Zstandard blocks (TIFF compression 50000) decoded on the GPU, one wave per block: zstd_core.h, the source td_tiff_zstd_decode runs on
// a host thread. Launch shape as the DEFLATE decoder's (tiffdecode.hip): WPB decoder waves share a workgroup, one workgroup per CU at
// most, every wave takes blocks from the launch's counter until it passes the last one — the long-lived decoder waves sit together on
// few CUs and leave the others to the forwards that run meanwhile. LDS: 11 KB of tables per wave, no workgroup barrier anywhere (the
// waves of a workgroup are each inside their own loops: wave fences only). The literals of a Huffman-coded section (up to 128 KB) go to
// a buffer of the wave's own in `scratch` and are read back behind the wave's store wait; matches are copied out of the block's earlier
// output in memory behind the same wait; everything is written with ordinary vector stores.
#include "common.h"
#include "zstd_core.h"

namespace {

constexpr int ZSTD_WPB = 8;                                        // 88 KB of LDS per workgroup
constexpr int64_t ZSTD_LIT_STRIDE = (int64_t)ZSTD_BLOCK_MAX + 64;  // one wave's literal buffer (>= ZSTD_BLOCK_MAX + ZSTD_LIT_PAD)

__device__ __forceinline__ int take_zstd_block(int* ticket, int lane) {
    int v = 0;
    if (lane == 0) v = atomicAdd(ticket, 1);
    return __builtin_amdgcn_readfirstlane(v);
}

template <int WPB>
__global__ __launch_bounds__(64 * WPB) void tiff_zstd_blocks_kernel(const uint8_t* __restrict__ comp, const int64_t* __restrict__ block_off,
                                                                    const int64_t* __restrict__ block_nbytes, uint8_t* out, int64_t block_cap,
                                                                    int64_t* __restrict__ decoded, int32_t* __restrict__ status, int nblocks,
                                                                    int* __restrict__ ticket, uint8_t* scratch) {
    __shared__ ZstdScratch S[WPB];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    uint8_t* lit = scratch + ((int64_t)blockIdx.x * WPB + wave) * ZSTD_LIT_STRIDE;
    for (int b = take_zstd_block(ticket, lane); b < nblocks; b = take_zstd_block(ticket, lane)) {      // ends: the counter only grows; whole waves leave
        const int64_t n = block_nbytes[b];
        ZstdResult r{0, 1, 0, 0, 0};
        if (n >= 0 && n < ((int64_t)1 << 31))
            r = zstd_single_frame<64>(S[wave], comp + block_off[b], n, out + (int64_t)b * block_cap, (uint32_t)block_cap, lit, lane);
        if (lane == 0) {
            decoded[b] = (int64_t)r.produced;
            status[b] = r.status;
        }
        TD_INF_SYNC();                                             // the next block's set-up writes follow this block's last LDS reads
    }
}

int zstd_groups(int nblocks, int cus) {
    const int want = (nblocks + ZSTD_WPB - 1) / ZSTD_WPB;
    return want < cus ? want : cus;
}

}  // namespace

extern "C" int64_t td_tiff_zstd_scratch_bytes(int nblocks) {
    if (nblocks <= 0) return 0;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    return (int64_t)zstd_groups(nblocks, cus) * ZSTD_WPB * ZSTD_LIT_STRIDE;
}

extern "C" td_status td_tiff_zstd_decode_dev(const uint8_t* comp, const int64_t* block_off, const int64_t* block_nbytes, int nblocks,
                                             uint8_t* blocks_out, int64_t block_cap, int64_t* decoded, int32_t* status, uint8_t* scratch,
                                             int64_t scratch_bytes, void* stream) {
    TD_REQUIRE(nblocks >= 0 && block_cap >= 1 && block_cap < ((int64_t)1 << 31), "td_tiff_zstd_decode_dev: %d blocks of %lld bytes", nblocks,
               (long long)block_cap);
    if (nblocks == 0) return TD_OK;
    TD_REQUIRE(comp && block_off && block_nbytes && blocks_out && decoded && status && scratch, "td_tiff_zstd_decode_dev: null pointer");
    int* ticket = nullptr;
    int cus = 0;
    const td_status tst = td_decode_ticket(static_cast<hipStream_t>(stream), &ticket, &cus);
    if (tst < 0) return tst;
    int groups = zstd_groups(nblocks, cus);                        // one workgroup per CU at most, and no more than the scratch serves
    const int64_t slots = scratch_bytes / (ZSTD_WPB * ZSTD_LIT_STRIDE);
    TD_REQUIRE(slots >= 1, "td_tiff_zstd_decode_dev: %lld bytes of scratch, %lld needed at least", (long long)scratch_bytes,
               (long long)(ZSTD_WPB * ZSTD_LIT_STRIDE));
    if (slots < groups) groups = (int)slots;
    hipLaunchKernelGGL((tiff_zstd_blocks_kernel<ZSTD_WPB>), dim3(groups), dim3(64 * ZSTD_WPB), 0, static_cast<hipStream_t>(stream), comp, block_off,
                       block_nbytes, blocks_out, block_cap, decoded, status, nblocks, ticket, scratch);
    TD_KERNEL_CHECK();
    return TD_OK;
}
