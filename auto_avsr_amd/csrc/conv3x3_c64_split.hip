// conv3x3_c64_split.hip -- 3x3 / stride 1 / pad 1 convolution with 64 input and 64 output channels on split hi / lo bf16 planes:
// the forward convolutions of the ResNet-18 trunk's first stage in the precise / hpf / mixed modes (frontend/resnet.py:10-35,82-98;
// 22 x 22 x 64 images, one per video frame).  f32 result + its bf16 twin + the BatchNorm partial statistics of the result.
//
// The tiled split-plane kernel (gemm_split.hip, 256 x 64 tile) is an implicit GEMM whose A tile is the im2col gather: every input
// pixel crosses L2 -> LDS once per filter tap, 2.2 GB of operand stream per launch for a 198 MB input.  This is the design of
// conv3x3_c64.hip (bf16, one MFMA per product) carried over to the split8 operands (three MFMAs per product):
//  * FILTER: wave (mg, ng) of the four-wave block (one wave per SIMD: the 512-entry register file) keeps the HI plane of the
//    32 output channels x 576 slice it multiplies with in registers (144 per lane) for the life of the block.  Both planes in
//    registers (288 + 64 accumulator + 36 offset + 64 fragment registers) spilled: 1260 bytes of scratch per lane.  The LO plane,
//    which feeds one MFMA in three, lives in LDS (72 KB, fragment-major: a wave's read is 1 KB contiguous);
//  * PATCH IN LDS, PER 32-CHANNEL HALF: a tile is a band of R full image rows (R * W <= 256 output pixels).  A split8 pixel is
//    256 bytes, so the whole (R+2) x (W+2) patch of a 22-wide band (80 KB) does not fit twice; one 32-channel half of it (hi and
//    lo planes of 32 channels = 128 bytes per pixel: the bf16 kernel's patch image, swizzle and LDS-DMA addressing unchanged)
//    does.  The k loop runs over the sequence (tile, half): 2 x 9 taps x 2 k-steps, the accumulators live across both halves,
//    and the patch half of the NEXT unit is in flight under the MFMAs of the current one;
//  * per 16-deep k-step a wave reads 9 fragments (4 pixel tiles x hi, lo + the filter's lo) for 12 MFMAs -- cross terms first,
//    into ONE f32 accumulator, as SplitKernel::run of gemm_split.hip -- so the result equals the tiled kernel's up to summation
//    order (32-channel-half-major instead of tap-major);
//  * PERSISTENT BLOCKS, one per CU, static tile map (tile = blockIdx.x + i * gridDim.x), no atomics: deterministic;
//  * the product is formed transposed (rows = channels, columns = pixels): a lane holds four consecutive channels of one pixel
//    per register quad.  With the filter's lo plane in LDS there is no room for a staging tile of the whole band, so each wave
//    turns its accumulators 16 pixels at a time through a 2 KB strip of its own (no block barrier) into whole 128-byte lines of
//    y (+ 64-byte lines of the bf16 twin), and sums what it stores for the statistics.  The stores drain under the next tile.
// Statistics: avsr_conv2d_f32s_stats promises that every row of stats_part is written and that the rows sum to the column sums /
// sums of squares of the stored values.  A block folds `group` consecutive tiles of its own (1 whenever the caller's buffer has a
// row per tile, i.e. tiles of >= 128 pixels on average) into row blockIdx.x + gridDim.x * (i / group) and zeroes the rest.
#include "prims.h"
#include "avsr_hip.h"

namespace {

template <class T> AVSR_DEV void opaque(T& v) {  // the value is unchanged, but the compiler may not reason about it
#ifndef AVSR_EMU
    asm volatile("" : "+v"(v));
#endif
}
// orders this wave's LDS writes before its own later LDS reads of OTHER lanes' data (and the reads before later writes): the
// LDS executes one wave's instructions in order, so only the compiler has to be told
AVSR_DEV void wave_lds_sync() {
#ifdef AVSR_EMU
    (void)__shfl_xor(0, 1);  // the lanes of a wave are fibers: meet
#else
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
#endif
}

constexpr int C = 64, KSTEPS = 9 * C / 16, HSTEPS = KSTEPS / 2;
constexpr int PIX_BYTES = C * 4;       // a split8 pixel in HBM
constexpr int WROW_BYTES = 9 * C * 4;  // a split8 filter row
constexpr int NTHR = 256, NWAVE = 4;   // one wave per SIMD: each may use the whole 512-register file
constexpr int WLO_BYTES = KSTEPS * C * 32;     // the filter's lo plane: [k-step][k half][64 co][16 bytes] = 72 KB
constexpr int STRIP_BYTES = 16 * 128;          // per wave: [16 pixels][32 channels] f32, 16-byte chunks XOR-swizzled like the patch
constexpr int MEET_BYTES = NWAVE * 2 * 32 * 4; // [wave][sum, sum of squares][32 channels]: where the waves' statistics meet
constexpr int LDS_LIMIT = 160 * 1024;
constexpr int PR_LIMIT = (LDS_LIMIT - WLO_BYTES - NWAVE * STRIP_BYTES - MEET_BYTES) / 2 / 1024 * 8;  // patch rows (pixels) per buffer: 312
constexpr int DMA_PER_WAVE = (PR_LIMIT / 8 + NWAVE - 1) / NWAVE;  // LDS-DMA wave-instructions per wave and patch half: 10

struct C64SParams {
    const char* src;   // split8 [N][H][W][64]
    const char* wq;    // split8 [64 co][9 taps][64 ci]
    float* y;          // [N][H][W][64]
    bf16_t* y2;        // bf16 twin of y, or null
    float* stats;      // [stats_rows][2][64] or null
    const void* zero;  // >= 16 zero bytes
    int N, H, W, R, bands, ntiles;
    int patch_bytes;   // bytes of one patch-half buffer ((R+2) * (W+2) pixels of 128 bytes, rounded up to 1 KiB)
    int stats_rows, group, ngroups;
};

__global__ __launch_bounds__(NTHR) void conv3x3_split_c64_kernel(C64SParams p) {
    AVSR_DYN_SMEM(smem);
    char* wlo = smem + 2 * p.patch_bytes;
    const int lane = threadIdx.x & 63, wave = wave_id();
    char* strip = wlo + WLO_BYTES + wave * STRIP_BYTES;
    float* meet = reinterpret_cast<float*>(wlo + WLO_BYTES + NWAVE * STRIP_BYTES);
    const int mg = wave >> 1, ng = wave & 1;  // this wave's 128 pixels (four 32-pixel accumulator tiles) and 32 channels
    const int W2 = p.W + 2, prows = (p.R + 2) * W2;
    const int khalf = lane >> 5;
    const int G = (int)gridDim.x;

    // ---- the filter.  Row n = co; k-step s = 4 tap + kk covers ci 16 kk .. + 15; a lane's 8 of them (k half khalf) are group
    // 8 tap + 2 kk + khalf of the row = byte 64 s + 32 khalf (16 bytes hi, then 16 bytes lo).  hi of this wave's rows -> registers:
    bf16x8 wh[KSTEPS];
    {
        const char* wrow = p.wq + (size_t)(ng * 32 + (lane & 31)) * WROW_BYTES + 32 * khalf;
#pragma unroll
        for (int s = 0; s < KSTEPS; s++) wh[s] = *reinterpret_cast<const bf16x8*>(wrow + 64 * s);
    }
    // lo of all rows -> LDS, fragment-major
    for (int idx = threadIdx.x; idx < KSTEPS * C * 2; idx += NTHR) {
        const int s = idx >> 7, kh = (idx >> 6) & 1, n = idx & 63;
        *reinterpret_cast<bf16x8*>(wlo + idx * 16) = *reinterpret_cast<const bf16x8*>(p.wq + (size_t)n * WROW_BYTES + 64 * s + 32 * kh + 16);
    }
    // the registers are complete BEFORE the tile loop as far as the compiler is concerned (its own wait at the first use inside the
    // loop would be a vmcnt(0), which also waits for the LDS-DMA in flight there, every iteration)
#pragma unroll
    for (int s = 0; s < KSTEPS; s++) opaque(wh[s]);
    __syncthreads();
    int wlo_ofs = khalf * 1024 + (ng * 32 + (lane & 31)) * 16;  // this lane's lo fragment of k-step s: wlo + wlo_ofs + 2048 s

    // ---- LDS-DMA of a patch half: wave-instruction j = wave + 4 i stages patch rows 8 j .. 8 j + 7, lane -> (row 8 j + (lane >> 3),
    // physical chunk lane & 7); (py, px) of the lane's row advance by the (quotient, remainder) of 32 rows by W2 with one carry
    const int step_y = (8 * NWAVE) / W2, step_x = 8 * NWAVE - step_y * W2;
    int py0, px0;
    {
        const int pr = wave * 8 + (lane >> 3);
        py0 = pr / W2;
        px0 = pr - py0 * W2;
    }
    struct Stager {
        const char* base;
        char* buf;
        int y0, py, px;
    };
    auto stage_begin = [&](int tile, int half, char* buf) {
        const int n = tile / p.bands, y0 = (tile - n * p.bands) * p.R;
        return Stager{p.src + ((size_t)n * p.H + y0) * p.W * PIX_BYTES + half * 128, buf, y0, py0, px0};
    };
    auto stage_one = [&](Stager& st, int i) {
        const int j = wave + NWAVE * i;
        if (j * 8 >= prows) return;  // wave-uniform
        const int pr = j * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((pr >> 1) & 7);  // source chunk that lands in physical chunk lane & 7
        const int yy = st.y0 - 1 + st.py;
        const bool ok = pr < prows && st.px >= 1 && st.px <= p.W && yy >= 0 && yy < p.H;
        const void* src = ok ? (const void*)(st.base + ((st.py - 1) * p.W + (st.px - 1)) * PIX_BYTES + c * 16) : p.zero;
        glds16(src, st.buf + j * 1024);
        st.px += step_x;
        st.py += step_y;
        if (st.px >= W2) {  // (W2 >= 6 and a step of 32 rows: the remainder is < W2, one carry suffices)
            st.px -= W2;
            st.py++;
        }
    };

    // ---- this lane's four accumulator columns (pixels) m_i = mg * 128 + 32 i + (lane & 31) and, per tap, the LDS offset of its
    // fragment inside a patch-half buffer with the swizzle key and the lane's k half folded in; the 16-byte chunk of a 128-byte
    // pixel is (ks << 2) | (khalf << 1) | plane, so offset(tap, i, ks, plane) = fbase[tap][i] ^ (ks << 6) ^ (plane << 4)
    int fbase[9][4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int pix = mg * 128 + 32 * i + (lane & 31);
        if (pix >= p.R * p.W) pix = 0;  // idle column: reads a valid pixel, never stored
        const int y = pix / p.W, x = pix - y * p.W;
#pragma unroll
        for (int tap = 0; tap < 9; tap++) {
            const int pr = y * W2 + x + (tap / 3) * W2 + (tap % 3);
            fbase[tap][i] = (pr * 128) ^ (((pr >> 1) & 7) << 4) ^ (khalf << 5);
        }
    }

    struct Band {
        size_t g0;  // first pixel of the band in the output
        int npix;
    };
    auto band_of = [&](int tile) {
        const int n = tile / p.bands, y0 = (tile - n * p.bands) * p.R;
        return Band{((size_t)n * p.H + y0) * p.W, min(p.R, p.H - y0) * p.W};
    };
    // ---- copy-out: through the wave's strip, lane -> pixel row (lane >> 3) + 8 rr of the strip, channels 32 ng + 4 (lane & 7) .. + 3:
    // always the same four channels, so their column sums stay in registers (across the tiles of a statistics group, too)
    float cs[4], cq[4];
#pragma unroll
    for (int e = 0; e < 4; e++) cs[e] = cq[e] = 0.f;
    // statistics of a finished group: lanes l, l + 8, ... of a wave hold the same 4 channels -> butterfly; the two waves that share
    // the channels meet in LDS (stats_meet; a barrier; stats_row)
    auto stats_meet = [&]() {
#pragma unroll
        for (int m = 32; m >= 8; m >>= 1)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                cs[e] += __shfl_xor(cs[e], m);
                cq[e] += __shfl_xor(cq[e], m);
            }
        if (lane < 8)
#pragma unroll
            for (int e = 0; e < 4; e++) {
                meet[(wave * 2 + 0) * 32 + lane * 4 + e] = cs[e];
                meet[(wave * 2 + 1) * 32 + lane * 4 + e] = cq[e];
            }
#pragma unroll
        for (int e = 0; e < 4; e++) cs[e] = cq[e] = 0.f;
        lds_wait<0>();
        sched_fence();
    };
    auto stats_row = [&](int row) {
        if (threadIdx.x < 2 * C) {
            const int j = threadIdx.x >> 6, c = threadIdx.x & 63, w0 = c >> 5, cc = c & 31;  // waves w0 (mg = 0) and w0 + 2 (mg = 1)
            p.stats[(size_t)row * 2 * C + threadIdx.x] = meet[(w0 * 2 + j) * 32 + cc] + meet[((w0 + 2) * 2 + j) * 32 + cc];
        }
    };

    // Tile loop.  A tile is two units (32-channel halves); per unit: [vmcnt(0) + barrier] its patch half has landed -> 18 k-steps of
    // twelve MFMAs each, with the LDS-DMA instructions of the NEXT unit's patch half woven in, one per step.  After the second
    // unit: [vmcnt(0): the next tile's first half has landed -- waited for HERE, so that the stores below are not waited for before
    // the next tile's MFMAs] accumulators -> strip -> y, y2, column sums.
    int tile = blockIdx.x;
    if (tile < p.ntiles) {
        Stager st = stage_begin(tile, 0, smem);
#pragma unroll
        for (int i = 0; i < DMA_PER_WAVE; i++) stage_one(st, i);
        wait_vmcnt<0>();
    }
    int it = 0, pending_row = -1;
    static_assert(DMA_PER_WAVE <= HSTEPS, "the woven pieces must fit the k-steps");
    for (; tile < p.ntiles; tile += G, it++) {
        const bool more = tile + G < p.ntiles;
        f32x16 acc[4];  // [pixel tile i]
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[i][r] = 0.f;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const char* patch = smem + h * p.patch_bytes;
            // the offset table and the filter's address change every unit as far as the compiler is concerned: otherwise it forms
            // all 2 x 18 x 9 fragment addresses of a tile ahead of the tile loop and keeps them in scratch (a scratch reload waits
            // on vmcnt(0), i.e. on the LDS-DMA in flight)
#pragma unroll
            for (int tap = 0; tap < 9; tap++)
#pragma unroll
                for (int i = 0; i < 4; i++) opaque(fbase[tap][i]);
            opaque(wlo_ofs);
            if (h == 1) wait_vmcnt<0>();
            block_barrier_raw();
            if (h == 0 && pending_row >= 0) {  // (block-uniform)
                stats_row(pending_row);
                pending_row = -1;
            }
            const bool do_stage = h == 0 || more;
            Stager st = stage_begin(h == 0 || !more ? tile : tile + G, 1 - h, smem + (1 - h) * p.patch_bytes);

            // fragments of local step t (tap t >> 1, 16 channels 32 h + 16 (t & 1) ..) are requested two steps ahead, each into the
            // registers of an MFMA that has just been issued (issued = has read its operands), ONE request per MFMA gap: a
            // request costs the wave address arithmetic + issue, and behind a block of twelve MFMAs instead of between them
            // that time is the MFMA pipe's idle time (first version: 205 us per launch against 191 us with the requests spread)
            i32x4 xh[2][4], xl[2][4], wl[2];
            auto req_x = [&](int t, int i, int plane) {
                return lds_read16_async(patch + (fbase[t >> 1][i] ^ ((t & 1) << 6) ^ (plane << 4)));
            };
            auto req_w = [&](int t) { return lds_read16_async(wlo + wlo_ofs + 2048 * (4 * (t >> 1) + 2 * h + (t & 1))); };
#pragma unroll
            for (int t = 0; t < 2; t++) {  // (the request order of a set: lo fragments, filter, hi fragments)
#pragma unroll
                for (int i = 0; i < 4; i++) xl[t][i] = req_x(t, i, 1);
                wl[t] = req_w(t);
#pragma unroll
                for (int i = 0; i < 4; i++) xh[t][i] = req_x(t, i, 0);
            }
#pragma unroll
            for (int t = 0; t < HSTEPS; t++) {
                // a step waits for its own nine fragments only: the nine requests of the following step may still be out
                // (the caller-ordered reads of prims.h return in order)
                if (t + 1 < HSTEPS) lds_wait<9>();
                else lds_wait<0>();
                const int s = 4 * (t >> 1) + 2 * h + (t & 1), cur = t & 1;
                const bool ahead = t + 2 < HSTEPS;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    lds_tie(xh[cur][i]);
                    lds_tie(xl[cur][i]);
                }
                lds_tie(wl[cur]);
                // the small cross terms first, into the same accumulator, as SplitKernel::run (rows = channels, columns = pixels)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    acc[i] = mfma32(wh[s], __builtin_bit_cast(bf16x8, xl[cur][i]), acc[i]);
                    sched_fence();
                    if (ahead) xl[cur][i] = req_x(t + 2, i, 1);
                    sched_fence();
                }
                const bf16x8 wlc = __builtin_bit_cast(bf16x8, wl[cur]);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    acc[i] = mfma32(wlc, __builtin_bit_cast(bf16x8, xh[cur][i]), acc[i]);
                    sched_fence();
                    if (i == 3 && ahead) wl[cur] = req_w(t + 2);
                    if (i == 1 && t < DMA_PER_WAVE && do_stage) stage_one(st, t);
                    sched_fence();
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    acc[i] = mfma32(wh[s], __builtin_bit_cast(bf16x8, xh[cur][i]), acc[i]);
                    sched_fence();
                    if (ahead) xh[cur][i] = req_x(t + 2, i, 0);
                    sched_fence();
                }
            }
        }
        wait_vmcnt<0>();
        // ---- accumulators -> y: register quad q of accumulator i = channels 32 ng + 8 q + 4 khalf .. + 3 of pixel
        // mg * 128 + 32 i + (lane & 31) = 16-byte chunk 2 q + khalf of its 128-byte strip row; 16 pixels at a time
        const Band b = band_of(tile);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                if (((lane >> 4) & 1) == hf) {
                    const int r = lane & 15;
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        *reinterpret_cast<f32x4*>(strip + r * 128 + (((2 * q + khalf) ^ ((r >> 1) & 7)) << 4)) =
                            f32x4{acc[i][4 * q], acc[i][4 * q + 1], acc[i][4 * q + 2], acc[i][4 * q + 3]};
                }
                wave_lds_sync();
                f32x4 vv[2];  // (both reads of the strip before the first store: one LDS round trip per strip, not two)
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    const int r = (lane >> 3) + 8 * rr, ch = lane & 7;
                    vv[rr] = *reinterpret_cast<const f32x4*>(strip + r * 128 + ((ch ^ ((r >> 1) & 7)) << 4));
                }
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    const int r = (lane >> 3) + 8 * rr, ch = lane & 7;
                    const f32x4 v = vv[rr];
                    const int pix = mg * 128 + 32 * i + 16 * hf + r;
                    if (pix < b.npix) {
                        const size_t o = (b.g0 + pix) * C + ng * 32 + ch * 4;
                        *reinterpret_cast<f32x4*>(p.y + o) = v;
                        if (p.y2)
                            *reinterpret_cast<bf16x4*>(p.y2 + o) = bf16x4{(short)f2bf(v[0]), (short)f2bf(v[1]), (short)f2bf(v[2]), (short)f2bf(v[3])};
                        if (p.stats) {
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                cs[e] += v[e];
                                cq[e] += v[e] * v[e];
                            }
                        }
                    }
                }
                wave_lds_sync();
            }
        if (p.stats && (!more || it % p.group == p.group - 1)) {  // this tile closes a statistics group (block-uniform)
            stats_meet();
            pending_row = (int)blockIdx.x + G * (it / p.group);
        }
    }
    if (p.stats) {
        block_barrier_raw();
        if (pending_row >= 0) stats_row(pending_row);
        if (threadIdx.x < 2 * C) {
            // rows of this block's groups that held no tile, and the rows behind all groups: they must read as zero for the fold
            for (int g = it > 0 ? (it - 1) / p.group + 1 : 0; g < p.ngroups; g++)
                p.stats[((size_t)blockIdx.x + (size_t)G * g) * 2 * C + threadIdx.x] = 0.f;
            for (int r = G * p.ngroups + (int)blockIdx.x; r < p.stats_rows; r += G) p.stats[(size_t)r * 2 * C + threadIdx.x] = 0.f;
        }
    }
}

int patch_bytes_of(int H, int W, int* R_out) {
    int R = 256 / W;  // rows per band: at most 256 output pixels, and a patch that fits its buffer
    if (R > H) R = H;
    while (R > 0 && (R + 2) * (W + 2) > PR_LIMIT) R--;
    if (R_out) *R_out = R;
    return ((R + 2) * (W + 2) * 128 + 1023) / 1024 * 1024;
}

}  // namespace

// 1 when the image geometry is one this kernel takes (the caller keeps the tiled kernel otherwise)
int avsr_conv3x3_c64_split_supported(int H, int W) {
    if (W < 4 || W > 254 || H < 1) return 0;
    int R;
    patch_bytes_of(H, W, &R);
    return R >= 1;
}

// y[N,H,W,64] (f32; y2: bf16 twin or null) = conv3x3(x[N,H,W,64] split8, wq[64][3][3][64] split8); stats_part: null, or
// [stats_rows][2][64], every row written, the rows summing to the column sums / sums of squares of y
int avsr_conv3x3_c64_split_launch(const void* x, const void* wq, float* y, void* y2, float* stats_part, int stats_rows,
                                  const void* zero_page, int N, int H, int W, hipStream_t stream) {
    C64SParams p{};
    p.src = (const char*)x; p.wq = (const char*)wq; p.y = y; p.y2 = (bf16_t*)y2;
    p.stats = stats_rows > 0 ? stats_part : nullptr;
    p.zero = zero_page;
    p.N = N; p.H = H; p.W = W;
    p.patch_bytes = patch_bytes_of(H, W, &p.R);
    p.bands = (H + p.R - 1) / p.R;
    p.ntiles = N * p.bands;
    int grid = p.ntiles < 256 ? p.ntiles : 256;  // one persistent block per CU
    p.stats_rows = stats_rows; p.group = 1; p.ngroups = 0;
    if (p.stats) {
        // a row per (block, group of `group` consecutive tiles of the block): the smallest group that fits the caller's rows
        if (grid > stats_rows) grid = stats_rows;
        const int iters = (p.ntiles + grid - 1) / grid, max_groups = stats_rows / grid;
        p.group = (iters + max_groups - 1) / max_groups;
        p.ngroups = (iters + p.group - 1) / p.group;
    }
    const size_t lds = 2 * (size_t)p.patch_bytes + WLO_BYTES + NWAVE * STRIP_BYTES + MEET_BYTES;
    AVSR_LAUNCH(conv3x3_split_c64_kernel, dim3(grid), dim3(NTHR), lds, stream, p);
    return 0;
}
