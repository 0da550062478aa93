// conv_split_kernel: fp32 1x1 / FC contractions on the bf16 matrix cores (tile ids 34 - 37, family TILE_SPLIT), fp32 in and out.
//
// Why: the fp32 engine's 1x1 and FC layers run v_mfma_f32_32x32x2_f32 at 65 - 83 % of its 157 TFLOP/s; no fp32 tile moves that
// ceiling. v_mfma_f32_32x32x16_bf16 occupies the pipe for 32 cycles (the fp32 MFMA: 64) and contracts 16 k instead of 2. So every fp32 operand is
// written as the sum of three bf16 pieces, x = p0 + p1 + p2, each piece the round-to-nearest-even bf16 of what the earlier ones
// left over (the remainders x - p0 and x - p0 - p1 are exact in fp32; the three pieces carry 24 significand bits), and a K = 16
// slice of the product is the six piece products of second order and below, accumulated in the fp32 MFMA accumulator,
// smallest terms first:
//     p0 q2,  p2 q0,  p1 q1,  p0 q1,  p1 q0,  p0 q0            (a = sum p, w = sum q)
// The three dropped products (p1 q2, p2 q1, p2 q2) are below 2^-24 |a w| each, under the roundings of the fp32 chain itself
// (tests/test_conv_split_ref.py: RMS 0.11 - 0.15 of the fp32-accumulation scale; dropping one more product is rejected).
// Six bf16 MFMAs replace the eight fp32 MFMAs of 16 k: 192 cycles against 512, an MFMA floor of 157 x 16 / 6 = 419 TFLOP/s.
// Another rounding than the fp32 tiles: NOT bit-identical to ids 0 - 33, so a fixed rule on the layer picks it (engine.cpp),
// never the tuner; ids 34 - 37 are bit-identical to EACH OTHER (same pieces, same product order inside a slice, slices and
// k-chunks ascending, same epilogue), the tuner chooses among them. Non-finite activations: inf - inf makes the second piece NaN.
//
// Block skeleton: conv_bd_kernel's.
//   * activations (A): fp32 rows, 128 B per k-chunk (32 floats = two K = 16 slices), LDS-DMA into the XOR-swizzled image, three
//     stages, one raw s_barrier per k-chunk, the rows of chunk it + 3 requested while chunk it is contracted (they come from HBM:
//     with one chunk of cover the waves waited for them); split into pieces by each wave when it reads its fragment: per float
//     pair one v_cvt_pk_bf16_f32, two widenings (shift / mask), two subtractions, twice, and a last conversion: 11 VALU
//     instructions per pair, 5.5 per element; the next slice's rows are split under this slice's MFMAs;
//   * filters (B): split ONCE on the host (conv_split_pack: 6 B per weight) into fragment order [32-column tile][k-chunk][slice]
//     [piece][lane][8 bf16]; one wave instruction = one contiguous 1-KB read straight into the registers the MFMA takes, issued two
//     slices (one k-chunk of MFMAs) ahead into three register sets of one slice each; no split work for them in the kernel. Plain
//     loads: hipcc counts their waits itself; only the wait for the LDS-DMA rows is counted by hand (see the loop);
//   * WM x WN waves of 32 MT rows x 32 NT columns: a wave splits only the rows it multiplies, and loads only its columns' filters.
// Per k-chunk a wave of the 64 x 128 wave tile (MT 2, NT 4: tile 36) issues 2 x 6 x 8 = 96 MFMAs (3 072 pipe cycles), reads 4 A fragments
// of 2 x 16 B (ds_read_b128), splits 32 floats per lane (176 VALU instructions, ~700 cycles, in the shadow of the MFMAs) and loads
// 24 filter fragments (24 KB).
// Registers of that tile: 128 accumulators (AGPRs) + 3 x 48 filter registers + 16 A + 2 x 24 pieces: 208 VGPRs + 128 AGPRs, one
// wave per SIMD, no scratch; the 64 x 64 wave tile: 198 registers, two waves per SIMD. LDS: 3 x BM x 128 B of stages (49 152 B at
// 128 rows), re-used by the epilogue's fp32 wave-row staging (64 x 260 x 4 B = 66 560 B for the 256-column tiles, 33 792 B for 64 x 128).
// Tile 34 (128 x 256) is 1 x 4 waves of 128 x 64 (MT 4, NT 2) instead: the block's waves differ in columns only, so every filter fragment
// is requested once per CU (12 per wave and k-chunk, not 24) and every wave splits all 128 rows (8 ds_read_b128, 288 - 352 VALU
// instructions a k-chunk for the same 96 MFMAs). 188 VGPRs + 128 AGPRs, one wave per SIMD, one block per CU; LDS 133 120 B, all of it the
// epilogue's 128 x 260 floats. Its step states the order of its instructions (PACED, below): that, not the bytes, is what it gains by —
// the 2 x 2 form already shared the fragments through the vector L1 (profiles/f32_split_tall.txt: same L2 requests, 1 047 us on fc1;
// this form 1 015 us as hipcc orders it, 857 us paced, the 64 x 256 tile 904 - 949 us).
// The 3x3 of res2 (64 -> 64) runs the same arithmetic inside the fused bottleneck tail, not here: bottleneck.hip's split form uses
// split8 (conv_tiles.h), this piece and product order and conv_split_pack with taps = 9; no 3x3 form of conv_split_kernel exists.
// Batched form (ConvArgs::batch_count > 1, grid.y = the plane): the 36 plane contractions V[p] [T x C] . U[p]^T of an F(4x4,3x3) layer
// that does not fold (wino_seq.cpp; the twin bank: conv_split_pack_planes, the rule: engine.cpp f32_split_wino). Plane blockIdx.y
// advances x, w_split (by w_bs BYTES) and y in 64-bit arithmetic on the kernel's own copy of the arguments; everything below then
// sees one plane — its buffer resources, xcd_remap, the k-loop and the epilogue are those of a plain launch, so ids 34 - 37 stay
// bit-identical to each other on planes. Registers, LDS and scratch of the four instantiations are unchanged.
// Measured (profiles/f32_split.txt, batch 8): fc1 (8000 x 1024 x 12544) 1 549 -> 900 us = 228 TFLOP/s, fc2 137 -> 89 us. conv1 and the
// shortcuts of res3 - res5 and the FPN laterals (8 - 64 k-chunks per block; profiles/f32_split_backbone.txt): 2.41 -> 1.95 ms in the layer
// table, headline 697.6 -> 726.2 tiles/s: on by default with the box head (engine.cpp SPLIT_DEFAULT); conv3 ties on its fp32 tiles: off.
#include "common.h"
#include "conv_tiles.h"
#include <algorithm>
#include <utility>
#include <vector>

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // (the piece types, SPLIT_CHUNK_BYTES and split8: conv_tiles.h)

template <int... R, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, R...>, F&& f) {
    (f(std::integral_constant<int, R>{}), ...);
}

template <int MT, int NT, int WM, int WN>
__device__ __forceinline__ void conv_split_body(const ConvArgs& a, char* lds) {
    constexpr int THREADS = 64 * WM * WN;
    constexpr int BM = 32 * MT * WM, BN = 32 * NT * WN;
    constexpr int LDROWS = THREADS / 8;
    constexpr int AROWS = BM / LDROWS;
    static_assert(BM % LDROWS == 0 && AROWS >= 1 && LDROWS % 16 == 0, "tile / thread-count mismatch");
    char* As = lds;                                   // [3 stages][BM][128 B]

    int M = a.M;
    if (a.m_dyn) {
        int md = *a.m_dyn * a.m_mul - a.m_off;
        md = md < 0 ? 0 : md;
        M = md < M ? md : M;
    }
    const int tiles_n = (a.Cout + BN - 1) / BN;
    const int tiles_m = (M + BM - 1) / BM;
    const int nblk = tiles_m * tiles_n;
    if ((int)blockIdx.x >= nblk) return;
    const int pid = xcd_remap(blockIdx.x, nblk);
    const int tm = pid / tiles_n, tn = pid - tm * tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;
    const int ld_c = tid & 7, ld_r = tid >> 3;
    const int nit = a.Cin / 32;                       // k-chunks of 32 floats
    const unsigned pix_bytes = (unsigned)a.Cin * 4u;
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(a.x), 0, (int)((size_t)a.B * a.H * a.W * pix_bytes), 0x00020000);
    const int ntiles32 = (a.Cout + 31) / 32;
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<void*>(a.w_split), 0, (int)((size_t)ntiles32 * nit * SPLIT_CHUNK_BYTES), 0x00020000);
    constexpr unsigned OOB = 0xfffffff0u;
    const unsigned src_piece = (unsigned)(ld_c ^ ((ld_r >> 1) & 7)) * 16;

    unsigned a_off[AROWS];                            // 1x1, no padding: every tap of a row below M is inside the map
#pragma unroll
    for (int i = 0; i < AROWS; ++i) {
        const int m = m0 + ld_r + LDROWS * i;
        a_off[i] = OOB;
        if (m < M && a.stride == 1) {
            a_off[i] = (unsigned)m * pix_bytes + src_piece;
        } else if (m < M) {
            const int hw = a.Ho * a.Wo;
            const int b = m / hw;
            const int rem = m - b * hw;
            const int oy = rem / a.Wo;
            const int ox = rem - oy * a.Wo;
            a_off[i] = (unsigned)((b * a.H + oy * a.stride) * a.W + ox * a.stride) * pix_bytes + src_piece;
        }
    }
    // this wave's filter fragments: 32-column tiles n0/32 + wn*NT + j; a tile past Cout reads beyond num_records → zeros
    unsigned w_off[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int nt = n0 / 32 + wn * NT + j;
        w_off[j] = nt < ntiles32 ? (unsigned)nt * (unsigned)nit * (unsigned)SPLIT_CHUNK_BYTES + (unsigned)lane * 16u : OOB;
    }

    unsigned w_dead[NT], a_dead[AROWS];               // all ones where the offset is OOB (the paced step's requests)
#pragma unroll
    for (int j = 0; j < NT; ++j) w_dead[j] = w_off[j] == OOB ? ~0u : 0u;
#pragma unroll
    for (int i = 0; i < AROWS; ++i) a_dead[i] = a_off[i] == OOB ? ~0u : 0u;

    typedef __attribute__((address_space(3))) void lds_void;
    const unsigned wave_rows = (unsigned)__builtin_amdgcn_readfirstlane(wave) * 8u;
    // every issue runs whether or not its k-chunk exists (past the end: offset OOB, zeros): each step then puts the same number of
    // operations into the in-order vector-memory queue, which is what the counted wait below relies on
    auto stage_a = [&](int stage, int it) {
#pragma unroll
        for (int i = 0; i < AROWS; ++i) {
            const unsigned off = a_off[i] == OOB || it >= nit ? OOB : a_off[i] + (unsigned)it * CHUNK_BYTES;
            char* dst = As + ((unsigned)stage * BM + (unsigned)LDROWS * i + wave_rows) * CHUNK_BYTES;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_void*)dst, 16, off, 0, 0, 0);
        }
    };
    auto load_b = [&](f32x4 (&fb)[NT][3], int it, int sl) {       // the three filter pieces of slice sl of k-chunk it
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const unsigned off = w_off[j] == OOB || it >= nit ? OOB : w_off[j] + (unsigned)it * (unsigned)SPLIT_CHUNK_BYTES + (unsigned)(3 * sl + q) * 1024u;
                fb[j][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 0));
            }
    };

    f32x16 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const unsigned swz = (lane >> 1) & 7, hi = lane >> 5;
    // slice s of a k-chunk = the 16-B pieces {4 s + hi, 4 s + 2 + hi} of the row: lane (r, hi) contracts floats
    // 16 s + 4 hi .. + 3 and 16 s + 8 + 4 hi .. + 3 — the order conv_split_pack gives the filter pieces
    unsigned frag_off[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
        frag_off[kk] = (unsigned)(wm * 32 * MT + (lane & 31)) * CHUNK_BYTES + (((unsigned)(2 * kk) + hi) ^ swz) * 16;
    auto split_a = [&](int stage, int sl, bf16x8 (&pa)[MT][3]) {      // this wave's rows of slice sl of the chunk in `stage`, as pieces
        const char* Ab = &As[stage * BM * CHUNK_BYTES];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(Ab + i * 32 * CHUNK_BYTES + frag_off[2 * sl]);
            const f32x4 up = *reinterpret_cast<const f32x4*>(Ab + i * 32 * CHUNK_BYTES + frag_off[2 * sl + 1]);
            split8(lo, up, pa[i]);
        }
    };
    // the six products, smallest first; the (i, j) tiles inside: MT x NT independent MFMAs between dependent ones. MFMA q of a slice
    // (product q / (MT NT), tile q % (MT NT)); [q0, q1) for the tile that places its requests between the first ones
    auto mma_range = [&](const bf16x8 (&pa)[MT][3], const f32x4 (&fb)[NT][3], auto q0_c, auto q1_c) {
        constexpr int PA[6] = {0, 2, 1, 0, 1, 0}, QB[6] = {2, 0, 1, 1, 0, 0};
        constexpr int Q0 = decltype(q0_c)::value, Q1 = decltype(q1_c)::value;
#pragma unroll
        for (int q = Q0; q < Q1; ++q) {
            const int t = q / (MT * NT), i = (q / NT) % MT, j = q % NT;
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[i][PA[t]], __builtin_bit_cast(bf16x8, fb[j][QB[t]]), acc[i][j], 0, 0, 0);
        }
    };
    auto mma = [&](const bf16x8 (&pa)[MT][3], const f32x4 (&fb)[NT][3]) {
        mma_range(pa, fb, std::integral_constant<int, 0>{}, std::integral_constant<int, 6 * MT * NT>{});
    };

    // The pipeline runs slice by slice (g = 2 it + s), unrolled over three k-chunks so that every index below is a constant:
    //   filters   three register sets of one slice each; slice g + 2 is requested when slice g starts, into the set slice g - 1 left;
    //   A rows    three LDS stages of one k-chunk each; chunk it + 3 is requested in step (it, 1), behind the barrier that says every
    //             wave has read the last of chunk it (its second slice is split during the first one's MFMAs) and has chunk it + 1;
    //   pieces    two sets; the next slice's rows are read and split in the shadow of this slice's MFMAs.
    // hipcc counts the waits for the filter registers itself (plain loads). The LDS-DMA rows it cannot see: step (it, 1) waits until
    // all but the A_YOUNGER newest operations have completed — the filter loads of three steps and the rows of chunk it + 2 are
    // younger than the rows of chunk it + 1 (requested last in step (it - 2, 1)).
    // The tall wave tile (MT 4) splits twice the rows per MFMA (36 - 44 MT VALU instructions for 6 MT NT MFMAs of 8 passes a step) and
    // has one wave per SIMD: what the wave issues outside an MFMA's 32 cycles, the pipe waits for. Left to itself hipcc issues the MFMAs
    // in runs of 20 with the split behind them, and the step's requests (60 - 180 issue cycles each) ahead of all of them. So the order
    // of a PACED step is stated: the fragment reads; one request behind each of the first MFMAs (fenced pairs: they also cover the LDS
    // latency); then PACE_VALU instructions of the split behind every other MFMA. Nothing crosses the end of a step.
    constexpr bool PACED = MT == 4;
    constexpr int PACE_VALU = 4;
    constexpr int A_YOUNGER = 3 * NT * 3 + AROWS;
    static_assert(A_YOUNGER < 64, "vmcnt immediate");
    f32x4 fb[3][NT][3];
    bf16x8 pa[2][MT][3];
    stage_a(0, 0);
    stage_a(1, 1);
    stage_a(2, 2);
    load_b(fb[0], 0, 0);
    load_b(fb[1], 0, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    split_a(0, 0, pa[0]);
    auto step = [&](auto c_c, auto s_c, int it) {     // slice s_c of k-chunk it, it % 3 == c_c
        constexpr int C = decltype(c_c)::value, S = decltype(s_c)::value, G = 2 * C + S;
        if constexpr (S == 1) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_YOUNGER) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        if constexpr (!PACED) {
            load_b(fb[(G + 2) % 3], it + 1, S);      // slice g + 2 = the same slice of the next chunk
            if constexpr (S == 1) stage_a(C, it + 3);
            __builtin_amdgcn_sched_barrier(0);            // the requests go out first (hipcc otherwise sinks them below the MFMAs)
            if constexpr (S == 0) split_a(C, 1, pa[1]);
            else split_a((C + 1) % 3, 0, pa[0]);
            mma(pa[S], fb[G % 3]);
        } else {
            constexpr int REQS = 3 * NT + (S == 1 ? AROWS : 0), NMMA = 6 * MT * NT;
            static_assert(REQS < NMMA && PACE_VALU * (NMMA - REQS) >= 36 * MT, "the paced step has a gap for every request and for the split");
            const char* Ab = &As[(S == 0 ? C : (C + 1) % 3) * BM * CHUNK_BYTES];      // the slice split_a would read in this step
            f32x4 raw[MT][2];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) raw[i][h] = *reinterpret_cast<const f32x4*>(Ab + i * 32 * CHUNK_BYTES + frag_off[2 * (1 - S) + h]);
            __builtin_amdgcn_sched_barrier(0);
            f32x4 (&fn)[NT][3] = fb[(G + 2) % 3];          // slice g + 2 = the same slice of the next chunk
            static_for(std::make_integer_sequence<int, REQS>{}, [&](auto r_c) {
                constexpr int R = decltype(r_c)::value;
                mma_range(pa[S], fb[G % 3], std::integral_constant<int, R>{}, std::integral_constant<int, R + 1>{});
                if constexpr (R < 3 * NT) {
                    constexpr int j = R / 3, q = R % 3;
                    const unsigned dead = w_dead[j] | (it + 1 >= nit ? ~0u : 0u);      // bit arithmetic, not `?:`: inside the fences hipcc branches on it
                    const unsigned off = ((w_off[j] + (unsigned)(it + 1) * (unsigned)SPLIT_CHUNK_BYTES + (unsigned)(3 * S + q) * 1024u) & ~dead) | (OOB & dead);
                    fn[j][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, off, 0, 0));
                } else {
                    constexpr int i = R - 3 * NT;
                    const unsigned dead = a_dead[i] | (it + 3 >= nit ? ~0u : 0u);
                    const unsigned off = ((a_off[i] + (unsigned)(it + 3) * CHUNK_BYTES) & ~dead) | (OOB & dead);
                    char* dst = As + ((unsigned)C * BM + (unsigned)LDROWS * i + wave_rows) * CHUNK_BYTES;
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(xrsrc, (lds_void*)dst, 16, off, 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            });
            mma_range(pa[S], fb[G % 3], std::integral_constant<int, REQS>{}, std::integral_constant<int, NMMA>{});
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                split8(raw[i][0], raw[i][1], pa[1 - S][i]);
#pragma unroll
                for (int k = 0; k < 3; ++k) {             // the pieces are finished inside this step (hipcc otherwise sinks the split to their use)
                    u32x4 pin = __builtin_bit_cast(u32x4, pa[1 - S][i][k]);
                    asm volatile("" : "+v"(pin));
                    pa[1 - S][i][k] = __builtin_bit_cast(bf16x8, pin);
                }
            }
#pragma unroll
            for (int g = REQS; g < NMMA; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);             // MFMA
                __builtin_amdgcn_sched_group_barrier(0x002, PACE_VALU, 0);     // VALU
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    for (int it = 0; it < nit; it += 3) {
        step(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, it);
        step(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{}, it);
        if (it + 1 < nit) {                           // (nested, not `break`: one loop exit keeps the accumulators in place)
            step(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{}, it + 1);
            step(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{}, it + 1);
        }
        if (it + 2 < nit) {
            step(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, it + 2);
            step(std::integral_constant<int, 2>{}, std::integral_constant<int, 1>{}, it + 2);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the rows requested past the last chunk write zeros into the stages
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                     // LDS is the epilogue's
    conv_epilogue<float, float, MT, NT, WM, WN, 1>(a, acc, lds, M, m0, n0, tid, lane, wm, wn);
}

template <int MT, int NT, int WM, int WN, int WPE>
__global__ __launch_bounds__(64 * WM * WN, WPE)
void conv_split_kernel(const ConvArgs a_in) {
    ConvArgs a = a_in;
    if (a.batch_count > 1) {                          // batched planes (F(4x4) Winograd): plane blockIdx.y of x / w_split / y; the buffer
        const long long bz = blockIdx.y;              // resources of the body are built on the advanced bases, 32-bit offsets stay in one plane
        a.x = static_cast<const float*>(a.x) + bz * a.x_bs;
        a.w_split = static_cast<const char*>(a.w_split) + bz * a.w_bs;      // (w_bs: BYTES of one plane's split bank)
        a.y = static_cast<float*>(a.y) + bz * a.y_bs;
    }
    constexpr int STAGE_BYTES = 3 * 32 * MT * WM * CHUNK_BYTES;
    constexpr int EPI_BYTES = conv_epilogue_lds_bytes<float, MT, NT, WM, WN, 1>();
    constexpr int LDS_BYTES = STAGE_BYTES > EPI_BYTES ? STAGE_BYTES : EPI_BYTES;
    constexpr int BLOCKS_PER_CU = 4 * WPE / (WM * WN) > 0 ? 4 * WPE / (WM * WN) : 1;      // by registers: WPE waves on each of the four SIMDs
    static_assert(LDS_BYTES * BLOCKS_PER_CU <= 160 * 1024, "the blocks the registers allow on a CU must fit its LDS");
    __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
    conv_split_body<MT, NT, WM, WN>(a, lds);
}

template <int MT, int NT, int WM, int WN, int WPE>
td_status launch_split(const ConvArgs& a, hipStream_t stream) {
    const int tiles = td_cdiv(a.M, 32 * MT * WM) * td_cdiv(a.Cout, 32 * NT * WN);
    hipLaunchKernelGGL((conv_split_kernel<MT, NT, WM, WN, WPE>), dim3(tiles, a.batch_count > 1 ? a.batch_count : 1), dim3(64 * WM * WN), 0, stream, a);
    TD_KERNEL_CHECK();
    return TD_OK;
}

// round-to-nearest-even bf16 of a finite float, as its 16 bits (what v_cvt_pk_bf16_f32 gives)
inline unsigned short bf16_rne(float f) {
    unsigned u = __builtin_bit_cast(unsigned, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);      // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

}  // namespace

// fp32 filter bank [Cout][Cin] (1x1 / FC) → the split bank [ceil(Cout/32)][Cin/32 k-chunks][2 slices][3 pieces][64 lanes][8 bf16].
// Lane l = (r = l & 31, h = l >> 5) of (tile t, chunk c, slice s, piece p) holds piece p of the eight weights
// W[t*32 + r][c*32 + 16 s + 4 h .. + 3] and W[t*32 + r][c*32 + 16 s + 8 + 4 h .. + 3] — the floats the kernel's A-fragment reads hand
// that lane; columns past Cout are zero.
// taps > 1 (the 3x3 bank [Cout][taps][Cin] of the split tail, bottleneck.hip): taps * Cin/32 k-chunks, channel chunk outer and
// filter tap inner — k-chunk c = cc * taps + tap holds W[n][tap][cc*32 ..], the order in which that kernel's waves walk them.
void conv_split_pack(const float* w, int cout, int cin, std::vector<unsigned char>& out, int taps) {
    const int nit = taps * (cin / 32), nt32 = (cout + 31) / 32;
    out.assign((size_t)nt32 * nit * SPLIT_CHUNK_BYTES, (unsigned char)0);
    unsigned short* o = reinterpret_cast<unsigned short*>(out.data());
    for (int t = 0; t < nt32; ++t)
        for (int c = 0; c < nit; ++c)
            for (int s = 0; s < 2; ++s)
                for (int l = 0; l < 64; ++l) {
                    const int n = t * 32 + (l & 31), h = l >> 5;
                    if (n >= cout) continue;
                    const int cc = c / taps, tap = c - cc * taps;
                    for (int e = 0; e < 8; ++e) {
                        float v = w[((size_t)n * taps + tap) * cin + (size_t)cc * 32 + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3)];
                        for (int p = 0; p < 3; ++p) {
                            const unsigned short b = bf16_rne(v);
                            o[(((((size_t)t * nit + c) * 2 + s) * 3 + p) * 64 + l) * 8 + e] = b;
                            v = v - __builtin_bit_cast(float, (unsigned)b << 16);      // exact
                        }
                    }
                }
}

size_t conv_split_bank_bytes(int cout, int cin) { return (size_t)((cout + 31) / 32) * (size_t)(cin / 32) * SPLIT_CHUNK_BYTES; }

// the split twin of a Winograd filter bank U [planes][cout][cin]: conv_split_pack on every plane, concatenated
void conv_split_pack_planes(const float* u, int planes, int cout, int cin, std::vector<unsigned char>& out) {
    const size_t bank = conv_split_bank_bytes(cout, cin);
    out.resize((size_t)planes * bank);
    std::vector<unsigned char> one;
    for (int p = 0; p < planes; ++p) {
        conv_split_pack(u + (size_t)p * cout * cin, cout, cin, one);
        std::copy(one.begin(), one.end(), out.begin() + (size_t)p * bank);
    }
}

// A batched launch (batch_count > 1: the planes of a Winograd layer) is admitted for plain planes only: rows [M][Cin] per plane with
// static count, no residual, and w_bs = the BYTES of one plane's split bank (conv_split_pack of that plane's [Cout][Cin]).
bool conv_split_ok(const ConvArgs& a, int precision) {
    const size_t bank = (size_t)((a.Cout + 31) / 32) * (size_t)(a.Cin / 32) * SPLIT_CHUNK_BYTES;
    const bool planes_ok = a.batch_count <= 1 || (!a.res && !a.m_dyn && a.m_off == 0 && a.stride == 1 && (long long)a.B * a.H * a.W == a.M &&
                                                  a.x_bs >= (long long)a.M * a.Cin && a.y_bs >= (long long)a.M * a.Cout && a.w_bs == (long long)bank);
    return precision == TD_PRECISION_FP32 && a.w_split && a.KH == 1 && a.KW == 1 && a.pad == 0 && a.stride >= 1 && a.out_mode == 0 &&
           planes_ok && !a.out_f32 && !a.head_w && a.Cin >= 32 && a.Cin % 32 == 0 && bank < 0xfffffff0ull - (1u << 20);
}

td_status conv_split_launch(const ConvArgs& a, int variant, hipStream_t stream) {
    TD_REQUIRE(conv_split_ok(a, TD_PRECISION_FP32), "split-bf16 contraction: unsupported launch (fp32 1x1 without padding, split filter bank)");
    switch (variant) {
        case 3: return launch_split<2, 2, 1, 2, 2>(a, stream);     // 64 x 128: 1 x 2 waves of 64 x 64 (M = 5 000 with N <= 512: 158 - 316 blocks, not 80 - 160)
        case 2: return launch_split<2, 4, 1, 2, 1>(a, stream);     // 64 x 256: 1 x 2 waves of 64 x 128 (row counts that leave the 128-row grid short)
        case 1: return launch_split<2, 2, 2, 2, 2>(a, stream);     // 128 x 128: 2 x 2 waves of 64 x 64, two blocks per CU
        default: return launch_split<4, 2, 1, 4, 1>(a, stream);    // 128 x 256: 1 x 4 waves of 128 x 64, one wave per SIMD, one block per CU (every filter fragment read once per CU)
    }
}
