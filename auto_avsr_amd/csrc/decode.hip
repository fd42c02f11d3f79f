// decode.hip -- the hybrid CTC / attention beam search of the evaluation path, one decoding step per HOST CALL.
//
// What it replaces: one iteration of BatchBeamSearch.search (espnet/nets/batch_beam_search.py:208-349 over
// beam_search.py:330-406) with the scorers the reference wires (lightning.py:126-158): TransformerDecoder.batch_score
// (decoder/transformer_decoder.py:260-334 -> forward_one_step :226-258), CTCPrefixScorer.batch_score_partial
// (scorers/ctc.py:101-126 over ctc_prefix_score.py:71-187), LengthBonus (scorers/length_bonus.py), the pre-beam on the
// decoder scores and the top-k over beam x vocabulary.
//
// Why a host-side step function.  The python form of this loop (auto_avsr_amd/decoding.py: BatchBeamSearch._step) issues
// ~120 launches per emitted token through ctypes / ATen and is bound by that (2.2 ms per token at beam 40, the GPU idle
// most of the time), and -- like the reference -- it re-projects keys and values of ALL previous positions and of the
// whole encoder memory for every hypothesis at every step.  Here
//  * the step is one C call: ~75 launches issued back to back from C++, one 1 KB device-to-host copy, one stream sync;
//  * the source-attention K / V of every layer are projected ONCE per utterance (they do not depend on the hypothesis);
//  * self-attention K / V live in a per-layer cache indexed [position][slot]; a hypothesis carries the list of slots of
//    its ancestors (`anc`), so that re-ordering the beam copies a row of 4-byte indices per hypothesis instead of
//    gathering the cache -- the attention kernel below follows the indirection;
//  * only the NEW position of every hypothesis goes through LayerNorm / projections / FFN (n <= beam rows);
//  * arithmetic: the split-plane GEMM of the precise mode (three bf16 MFMAs per product, ~f32) and f32 everywhere else,
//    whatever numerical mode the encoder ran in -- at n <= 40 rows the step is launch-bound, cheaper operands buy nothing.
// Values are those of the reference's recomputation (same weights, same inputs per row); the python path stays as the
// implementation of the generic scorer API and as the cross-check (tests/test_decoding.py).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "prims.h"
#include "avsr_hip.h"
#include "search_tables.h"

#ifdef AVSR_EMU
static inline int avsr_copy_to_host_sync(void* dst, const void* src, size_t n, hipStream_t) {
    memcpy(dst, src, n);
    return 0;
}
// a second result of a step, copied ahead of avsr_copy_to_host_sync on the same stream (that call's synchronisation covers it)
static inline int avsr_copy_to_host_async(void* dst, const void* src, size_t n, hipStream_t) {
    memcpy(dst, src, n);
    return 0;
}
static inline float* avsr_host_floats(size_t n) { return static_cast<float*>(malloc(n * sizeof(float))); }
static inline void avsr_host_floats_free(float* p) { free(p); }
#else
static inline int avsr_copy_to_host_async(void* dst, const void* src, size_t n, hipStream_t s) {
    return (int)hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s);
}
static inline float* avsr_host_floats(size_t n) {  // page-locked, so that the copy above does not wait on the host
    void* p = nullptr;
    return hipHostMalloc(&p, n * sizeof(float), hipHostMallocDefault) == hipSuccess ? static_cast<float*>(p) : nullptr;
}
static inline void avsr_host_floats_free(float* p) {
    if (p) (void)hipHostFree(p);
}
static inline int avsr_copy_to_host_sync(void* dst, const void* src, size_t n, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
}
#endif

namespace {

constexpr float LOGZERO = -10000000000.0f;
constexpr int MAX_BEAM = 128;

// A GROUP of utterances decoded together (avsr_beam_*_batch; a search of one utterance is a group of one): the running hypotheses
// of all of them are one packed row list, every utterance at the same position L.  Utterance u owns rows [off, off + n) of the current beam and rows [noff, noff + nn) of the
// beam a kernel writes; f0 = frames of the utterances before it (its memory K / V, CTC state and r_new regions start there);
// g0 = its first block of the source attention.  Passed to the kernels by value (1 KB of kernel arguments).
constexpr int MAX_UTT = 32, MAX_ROWS = 1024;
struct Utt {
    int off, n, noff, nn, T, g0;
    long f0;
};
struct Group {
    int U, rows, blocks, spare;  // rows of the current beam, blocks of the source attention
    Utt u[MAX_UTT];
};
struct RowList {
    unsigned short from[MAX_ROWS];
};
struct PtrList {
    const float* p[MAX_UTT];
};

AVSR_DEV float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
AVSR_DEV float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Single-query attention (attention.py:59-104 with one query row): block = (hypothesis b, head h), d_k = 64, `len` keys.
// Key / value row j of hypothesis b lives at kv + j * step_j + slot * step_slot (+ koff / voff) + h * 64 with
//     slot = anc == NULL ? 0 : (j == len - 1 ? b : anc[b * ld_anc + j])
// -- self-attention: the [position][slot] cache, the hypothesis' own ancestry; source attention: the utterance's memory
// projection, shared by every hypothesis.  16 lanes share a key (one float4 of the 64 dimensions each), a block of four
// waves takes 16 keys per iteration; scores are parked in LDS, softmax in f32 with expf.
__global__ __launch_bounds__(1024) void dec_attn_kernel(const float* __restrict__ q, long ldq, const float* __restrict__ kv, long step_j,
                                                       long step_slot, int koff, int voff, const int* __restrict__ anc, int ld_anc,
                                                       int len, float scale, float* __restrict__ out, long ldo) {
    AVSR_DYN_SMEM(smem);
    const int nwv = blockDim.x >> 6;             // 4, 8 or 16 waves: 16 keys per wave and chunk
    float* sc = reinterpret_cast<float*>(smem);  // [len] scores, then probabilities
    float* part = sc + len;                      // [nwv][64]
    __shared__ float red[16];
    const int b = blockIdx.x, h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, c = lane & 15;
    const f32x4 q4 = *reinterpret_cast<const f32x4*>(q + (size_t)b * ldq + h * 64 + 4 * c);
    auto row_of = [&](int j) -> const float* {
        const long slot = anc ? (j == len - 1 ? b : anc[(size_t)b * ld_anc + j]) : 0;
        return kv + (size_t)j * step_j + slot * step_slot + h * 64 + 4 * c;
    };
    // four keys per lane and pass: the loads of a chunk of 64 keys are requested together (a loop of one key per iteration is a
    // chain of exposed L2 round trips: 8 us for 100 keys)
    for (int j0 = 0; j0 < len; j0 += 16 * nwv) {
        f32x4 k4[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
            k4[u] = j < len ? *reinterpret_cast<const f32x4*>(row_of(j) + koff) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
            float s = q4[0] * k4[u][0] + q4[1] * k4[u][1] + q4[2] * k4[u][2] + q4[3] * k4[u][3];
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            if (c == 0 && j < len) sc[j] = s * scale;
        }
    }
    __syncthreads();
    float m = -INFINITY;
    for (int j = threadIdx.x; j < len; j += blockDim.x) m = fmaxf(m, sc[j]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < nwv; w++) m = fmaxf(m, red[w]);
    __syncthreads();
    float l = 0.f;
    for (int j = threadIdx.x; j < len; j += blockDim.x) {
        const float p = expf(sc[j] - m);
        sc[j] = p;
        l += p;
    }
    l = wave_sum(l);
    if (lane == 0) red[wave] = l;
    __syncthreads();
    l = 0.f;
    for (int w = 0; w < nwv; w++) l += red[w];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < len; j0 += 16 * nwv) {
        f32x4 v4[4];
        float p[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
            v4[u] = j < len ? *reinterpret_cast<const f32x4*>(row_of(j) + voff) : f32x4{0.f, 0.f, 0.f, 0.f};
            p[u] = j < len ? sc[j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] += p[u] * v4[u][e];
    }
#pragma unroll
    for (int e = 0; e < 4; e++) {
        acc[e] += __shfl_xor(acc[e], 16);
        acc[e] += __shfl_xor(acc[e], 32);
    }
    if (g == 0) {
#pragma unroll
        for (int e = 0; e < 4; e++) part[wave * 64 + 4 * c + e] = acc[e];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        float v = 0.f;
        for (int w = 0; w < nwv; w++) v += part[w * 64 + threadIdx.x];
        out[(size_t)b * ldo + h * 64 + threadIdx.x] = v / l;
    }
}

// Source attention of a decoding step (transformer_decoder.py:109-117): every hypothesis attends to the SAME projected memory,
// so a block takes HB hypotheses of one head and reads each key / value row once for all of them (with one hypothesis per
// block the 480 blocks of a beam-40 step pull 98 MB through the L2s at T = 400: 35 us per launch).  Layout as dec_attn_kernel:
// 16 lanes per key, 16 keys per block iteration, four iterations' loads in flight; wave w owns the softmax of hypothesis w.
constexpr int SRC_HB = 4;
// rows [b0, min(b0 + SRC_HB, n)) against `len` keys with nwv waves.  The block may have more waves than nwv (a launch over
// utterances of different lengths has the block size of the longest); the spare waves only meet the barriers, so that keys are
// dealt to waves and partial sums are added exactly as in a launch of nwv waves.
AVSR_DEV void src_attn_block(char* smem, float* s_l, const float* __restrict__ q, long ldq, const float* __restrict__ kv, long step_j, int voff,
                             int b0, int n, int len, int nwv, float scale, float* __restrict__ out, long ldo) {
    float* sc = reinterpret_cast<float*>(smem);  // [SRC_HB][len]
    float* part = sc + SRC_HB * len;             // [nwv][SRC_HB][64]
    const int h = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool busy = wave < nwv;
    const int g = lane >> 4, c = lane & 15;
    f32x4 q4[SRC_HB];
#pragma unroll
    for (int i = 0; i < SRC_HB; i++)
        q4[i] = b0 + i < n ? *reinterpret_cast<const f32x4*>(q + (size_t)(b0 + i) * ldq + h * 64 + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* base = kv + h * 64 + 4 * c;
    for (int j0 = 0; busy && j0 < len; j0 += 16 * nwv) {
        f32x4 k4[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
            k4[u] = j < len ? *reinterpret_cast<const f32x4*>(base + (size_t)j * step_j) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
#pragma unroll
            for (int i = 0; i < SRC_HB; i++) {
                float s = q4[i][0] * k4[u][0] + q4[i][1] * k4[u][1] + q4[i][2] * k4[u][2] + q4[i][3] * k4[u][3];
#pragma unroll
                for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m);
                if (c == 0 && j < len) sc[i * len + j] = s * scale;
            }
        }
    }
    __syncthreads();
    if (wave < SRC_HB) {  // softmax of hypothesis `wave`
        float* row = sc + wave * len;
        float m = -INFINITY;
        for (int j = lane; j < len; j += 64) m = fmaxf(m, row[j]);
        m = wave_max(m);
        float l = 0.f;
        for (int j = lane; j < len; j += 64) {
            const float p = expf(row[j] - m);
            row[j] = p;
            l += p;
        }
        l = wave_sum(l);
        if (lane == 0) s_l[wave] = l;
    }
    __syncthreads();
    f32x4 acc[SRC_HB];
#pragma unroll
    for (int i = 0; i < SRC_HB; i++) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; busy && j0 < len; j0 += 16 * nwv) {
        f32x4 v4[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
            v4[u] = j < len ? *reinterpret_cast<const f32x4*>(base + (size_t)j * step_j + voff) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + 4 * nwv * u + 4 * wave + g;
            if (j < len) {
#pragma unroll
                for (int i = 0; i < SRC_HB; i++) {
                    const float p = sc[i * len + j];
#pragma unroll
                    for (int e = 0; e < 4; e++) acc[i][e] += p * v4[u][e];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < SRC_HB; i++)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            acc[i][e] += __shfl_xor(acc[i][e], 16);
            acc[i][e] += __shfl_xor(acc[i][e], 32);
        }
    if (g == 0 && busy) {
#pragma unroll
        for (int i = 0; i < SRC_HB; i++)
#pragma unroll
            for (int e = 0; e < 4; e++) part[(wave * SRC_HB + i) * 64 + 4 * c + e] = acc[i][e];
    }
    __syncthreads();
    if (threadIdx.x < 64 * SRC_HB) {
        const int i = threadIdx.x >> 6, d = threadIdx.x & 63;
        if (b0 + i < n) {
            float v = 0.f;
            for (int w = 0; w < nwv; w++) v += part[(w * SRC_HB + i) * 64 + d];
            out[(size_t)(b0 + i) * ldo + h * 64 + d] = v / s_l[i];
        }
    }
}

// Over the utterances of a group: block x belongs to the utterance whose block range [g0, ...) holds it, takes SRC_HB of ITS
// rows (a block never holds rows of two utterances) against ITS memory projection kv + f0 * step_j and length, with the wave count
// a launch for that length alone would have.  Dynamic LDS is sized for the longest utterance.
__global__ __launch_bounds__(1024) void dec_src_attn_group_kernel(Group grp, const float* __restrict__ q, long ldq, const float* __restrict__ kv,
                                                                 long step_j, int voff, float scale, float* __restrict__ out, long ldo) {
    AVSR_DYN_SMEM(smem);
    __shared__ float s_l[SRC_HB];
    int u = 0;
    while (u + 1 < grp.U && (int)blockIdx.x >= grp.u[u + 1].g0) u++;
    const Utt d = grp.u[u];
    const int nwv = d.T <= 64 ? 4 : (d.T <= 256 ? 8 : 16);
    src_attn_block(smem, s_l, q, ldq, kv + (size_t)d.f0 * step_j, step_j, voff, d.off + ((int)blockIdx.x - d.g0) * SRC_HB, d.off + d.n, d.T,
                   nwv, scale, out, ldo);
}

// ---------------------------------------------------------------------------------------------------------------------
// The linear layers of a decoding step (transformer_decoder.py:84-126 on ONE position per hypothesis): C[M][N] =
// act(LN?(A)[M][K] . W[N][K]^T + bias) + resid with M <= beam rows.  On the tiled GEMM (64 x 64 tile, 12 - 48 sequential
// k-tiles behind a two-stage ring) such a launch takes 25 us whatever M is: with 12 - 48 blocks on 256 CUs it is a chain of
// dependent HBM round trips.  Here a block owns 16 weight rows and 64 NW columns of K (all of K = 768: NW = 12 waves), wave w
// its own 64 columns; split hi / lo bf16 planes are formed in registers, three MFMAs per product (the precise mode's
// arithmetic); the NW partial tiles meet in LDS.
// LayerNorm in front of a sub-layer's first projection (pre-norm blocks) is applied to the A fragments; the row statistics it
// needs were left behind by whatever produced the rows (st_out below: per-row sum and sum of squares of every block's 16
// columns, summed by the consumer) -- the 19 stand-alone LayerNorm launches of a step disappear and no kernel reads its input
// twice.
// History of the kernel (MI355X, per launch at M = 40, K = 768): 32-row MFMA fragments streamed by every lane from its own row:
// 43 us -- 32 distinct cache lines per wave-instruction, the CU's address path (one line per cycle) was the bound -- and 19 us
// more when the LayerNorm statistics re-read A; the same tile staged by LDS-DMA (8 lanes per 128-byte row piece, XOR-swizzled
// wave-private regions, two phases): 9.4 us; the 16-row form below (whole cache lines per four lanes, no staging, one round
// trip): 9.5 us.  The last two differ in everything but the result: what remains is the price of ANY dependent launch that
// touches fresh HBM lines here (a 40-block row-sum of 120 KB takes 6 us), not of the data path.
struct SkinnyArgs {
    const float* A;
    long lda;
    const float* W;
    long ldw;
    const float *bias, *ln_g, *ln_b;
    float eps;
    const float* st_in;  // LN: [M][st_in_nt][2] partial (sum, sum of squares) of every row of A
    int st_in_nt;
    const float* resid;
    long ldr;
    float* C;
    long ldc;
    float* st_out;  // [M][gridDim.x][2] or NULL: the same statistics of the rows written here
    int M, N, K, act;
    int Z;           // K slices (blockIdx.z); Z > 1: raw partial sums to partial[z][M][N], finished by rowsum_kernel
    float* partial;
};

AVSR_DEV void split8(const float* x, bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; e++) {
        const bf16_t h = f2bf(x[e]);
        hi[e] = (short)h;
        lo[e] = (short)f2bf(x[e] - bf2f(h));
    }
}

// v_mfma_f32_16x16x32, no staging.  In the 16-row fragment layout a lane holds 8 consecutive k of row (lane & 15) and the four lanes lane, lane + 16, +32, +48 hold the
// next 8 each: a wave-instruction reads 16 rows x 128 contiguous bytes -- whole cache lines, four lanes per line -- so the
// fragments can come straight from global memory without the one-line-per-lane address traffic that sank the first 32-row
// version.  A block owns 16 weight rows (twice the blocks of the staged kernel: 48 - 316 of them), wave w its 64 columns of K
// = two MFMA steps; every operand of a wave is requested up front (4 + 12 16-byte loads per lane) and arrives in ONE round trip
// instead of the staged kernel's two DMA phases.
constexpr int SK16_ROWS = 48;  // three 16-row tiles per block

template <int NW>
__global__ __launch_bounds__(64 * NW) void skinny16_kernel(SkinnyArgs a) {
    AVSR_DYN_SMEM(smem);
    float* red = reinterpret_cast<float*>(smem);  // [NW][48][17]
    __shared__ float s_mean[SK16_ROWS], s_rstd[SK16_ROWS];
    constexpr int NT = 64 * NW, RP = 17;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * 16, m0 = blockIdx.y * SK16_ROWS;
    const int rows = min(SK16_ROWS, a.M - m0);
    const int li = lane & 15, kq = lane >> 4;
    const int kb = (blockIdx.z * NW + wave) * 64 + 8 * kq;  // this lane's first column
    // every operand of this wave, requested before anything else (LayerNorm statistics below overlap the round trip)
    const bool nv = n0 + li < a.N;
    const float* wrow = a.W + (size_t)(nv ? n0 + li : 0) * a.ldw + kb;
    float w8[2][8], x8[3][2][8];
#pragma unroll
    for (int s = 0; s < 2; s++) load8(wrow + 32 * s, w8[s]);
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int r = li + 16 * t;
        const float* arow = a.A + (size_t)(m0 + min(r, rows - 1)) * a.lda + kb;
#pragma unroll
        for (int s = 0; s < 2; s++) load8(arow + 32 * s, x8[t][s]);
    }
    if (a.ln_g) {  // row statistics from the producer's partial sums: 16 lanes per row
        const int sub = tid & 15;
        for (int r0 = 0; r0 < rows; r0 += NT >> 4) {
            const int r = r0 + (tid >> 4);
            float s1 = 0.f, s2 = 0.f;
            if (r < rows)
                for (int j = sub; j < a.st_in_nt; j += 16) {
                    const float* q = a.st_in + ((size_t)(m0 + r) * a.st_in_nt + j) * 2;
                    s1 += q[0];
                    s2 += q[1];
                }
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) {
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            if (r < rows && sub == 0) {
                const float mean = s1 / (float)a.K;
                s_mean[r] = mean;
                s_rstd[r] = 1.0f / sqrtf(fmaxf(s2 / (float)a.K - mean * mean, 0.f) + a.eps);
            }
        }
        __syncthreads();
    }
    f32x4 acc[3];
#pragma unroll
    for (int t = 0; t < 3; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; s++) {
        if (!nv) {
#pragma unroll
            for (int e = 0; e < 8; e++) w8[s][e] = 0.f;
        }
        bf16x8 whi, wlo;
        split8(w8[s], whi, wlo);
        float g8v[8], b8v[8];
        if (a.ln_g) {
            load8(a.ln_g + kb + 32 * s, g8v);
            load8(a.ln_b + kb + 32 * s, b8v);
        }
#pragma unroll
        for (int t = 0; t < 3; t++) {
            const int r = li + 16 * t;
            if (a.ln_g) {
                const float mean = r < rows ? s_mean[r] : 0.f, rstd = r < rows ? s_rstd[r] : 0.f;
#pragma unroll
                for (int e = 0; e < 8; e++) x8[t][s][e] = (x8[t][s][e] - mean) * rstd * g8v[e] + b8v[e];
            }
            bf16x8 ahi, alo;
            split8(x8[t][s], ahi, alo);
            acc[t] = mfma16(alo, whi, acc[t]);
            acc[t] = mfma16(ahi, wlo, acc[t]);
            acc[t] = mfma16(ahi, whi, acc[t]);
        }
    }
    float* mine = red + (size_t)wave * SK16_ROWS * RP;
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) mine[(16 * t + 4 * kq + r) * RP + li] = acc[t][r];
    __syncthreads();
    for (int idx = tid; idx < SK16_ROWS * 16; idx += NT) {  // (wave-uniform trip count: 768 and NT are multiples of 64)
        const int row = idx >> 4, col = idx & 15;
        const bool ok = row < rows && n0 + col < a.N;
        float v = 0.f;
        if (ok) {
#pragma unroll
            for (int w = 0; w < NW; w++) v += red[((size_t)w * SK16_ROWS + row) * RP + col];
            if (a.Z > 1) {
                a.partial[((size_t)blockIdx.z * a.M + m0 + row) * a.N + n0 + col] = v;
            } else {
                if (a.bias) v += a.bias[n0 + col];
                if (a.act == 1) v = fmaxf(v, 0.f);
                if (a.resid) v += a.resid[(size_t)(m0 + row) * a.ldr + n0 + col];
                a.C[(size_t)(m0 + row) * a.ldc + n0 + col] = v;
            }
        }
        if (a.st_out) {  // (never with Z > 1)
            float s1 = v, s2 = v * v;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) {
                s1 += __shfl_xor(s1, m);
                s2 += __shfl_xor(s2, m);
            }
            if (col == 0 && row < rows) {
                float* q = a.st_out + ((size_t)(m0 + row) * gridDim.x + blockIdx.x) * 2;
                q[0] = s1;
                q[1] = s2;
            }
        }
    }
}

// C[m][n] = sum_z partial[z][m][n] + bias[n] + resid[m][n]: the K slices of a split contraction, summed in slice order; block =
// row; st_out [M][1][2]: the row's (sum, sum of squares) for the LayerNorm that follows
__global__ __launch_bounds__(256) void rowsum_kernel(const float* __restrict__ partial, int Z, int M, int N, const float* __restrict__ bias,
                                                     const float* __restrict__ resid, long ldr, float* __restrict__ C, long ldc,
                                                     float* __restrict__ st_out) {
    __shared__ float red[2][4];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float s1 = 0.f, s2 = 0.f;
    for (int n = threadIdx.x; n < N; n += 256) {
        float v = 0.f;
        for (int z = 0; z < Z; z++) v += partial[((size_t)z * M + m) * N + n];
        if (bias) v += bias[n];
        if (resid) v += resid[(size_t)m * ldr + n];
        C[(size_t)m * ldc + n] = v;
        s1 += v;
        s2 += v * v;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        red[0][wave] = s1;
        red[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0 && st_out) {
        st_out[2 * m] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        st_out[2 * m + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// x[r] = embed[last[r]] * scale + pe  (transformer_decoder.py:186-189, embedding.py:78-87; one position for every hypothesis) and
// the row's LayerNorm statistics; block = row
__global__ __launch_bounds__(256) void dec_embed_kernel(const int64_t* __restrict__ last, const float* __restrict__ table,
                                                        const float* __restrict__ pe, float scale, int D, float* __restrict__ x,
                                                        float* __restrict__ st_out) {
    __shared__ float red[2][4];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* row = table + (size_t)last[m] * D;
    float s1 = 0.f, s2 = 0.f;
    for (int n = threadIdx.x; n < D; n += 256) {
        const float v = row[n] * scale + pe[n];
        x[(size_t)m * D + n] = v;
        s1 += v;
        s2 += v * v;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        red[0][wave] = s1;
        red[1][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        st_out[2 * m] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        st_out[2 * m + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    }
}

// Input layer of the language model (ESPnet TransformerLM: embed -> Linear E->D -> LayerNorm -> ReLU -> x * sqrt(D) + pe) for the
// last token of every hypothesis.  `table` [V][D] is embed followed by the Linear, contracted once at bind time, so the step
// gathers a row instead of multiplying; block = row.  LayerNorm as torch computes it (mean, then the mean of the squared
// deviations); st_out [M][1][2]: (sum, sum of squares) of the row written, for the LayerNorm-fused projection that follows.
__global__ __launch_bounds__(256) void lm_input_kernel(const int64_t* __restrict__ last, const float* __restrict__ table,
                                                       const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                       const float* __restrict__ pe, float scale, int D, float* __restrict__ x,
                                                       float* __restrict__ st_out) {
    __shared__ float red[4];
    const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* row = table + (size_t)last[m] * D;
    auto block_sum = [&](float v) -> float {
        v = wave_sum(v);
        __syncthreads();  // (the previous round's readers are done with red[])
        if (lane == 0) red[wave] = v;
        __syncthreads();
        return (red[0] + red[1]) + (red[2] + red[3]);
    };
    float s = 0.f;
    for (int n = threadIdx.x; n < D; n += 256) s += row[n];
    const float mean = block_sum(s) / (float)D;
    s = 0.f;
    for (int n = threadIdx.x; n < D; n += 256) {
        const float d = row[n] - mean;
        s += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum(s) / (float)D + eps);
    float s1 = 0.f, s2 = 0.f;
    for (int n = threadIdx.x; n < D; n += 256) {
        const float v = fmaxf((row[n] - mean) * rstd * g[n] + b[n], 0.f) * scale + pe[n];
        x[(size_t)m * D + n] = v;
        s1 += v;
        s2 += v * v;
    }
    s1 = block_sum(s1);
    s2 = block_sum(s2);
    if (threadIdx.x == 0) {
        st_out[2 * m] = s1;
        st_out[2 * m + 1] = s2;
    }
}

// logp[row] = logits[row] - logsumexp(logits[row]) over the whole vocabulary (the language model's scores: no pre-beam of their
// own, the selection reads them at the decoder's candidates); block = row
__global__ __launch_bounds__(1024) void lm_logsoftmax_kernel(const float* __restrict__ logits, float* __restrict__ logp, long ld, int V) {
    __shared__ float redf[16];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (size_t)row * ld;
    float m = -INFINITY;
    for (int i = tid; i < V; i += 1024) m = fmaxf(m, x[i]);
    m = wave_max(m);
    if (lane == 0) redf[wave] = m;
    __syncthreads();
    m = redf[0];
    for (int w = 1; w < 16; w++) m = fmaxf(m, redf[w]);
    __syncthreads();
    float l = 0.f;
    for (int i = tid; i < V; i += 1024) l += expf(x[i] - m);
    l = wave_sum(l);
    if (lane == 0) redf[wave] = l;
    __syncthreads();
    float lsum = 0.f;
    for (int w = 0; w < 16; w++) lsum += redf[w];
    const float lse = m + logf(lsum);
    float* y = logp + (size_t)row * ld;
    for (int i = tid; i < V; i += 1024) y[i] = x[i] - lse;
}

// ---------------------------------------------------------------------------------------------------------------------
// Top-S selection by radix select on the order-preserving integer image of the floats (keys in LDS).  The
// digits are taken from key - min(key), most significant byte of the SPAN first: log-probabilities share sign and exponent,
// so the top byte of the raw key is the same for nearly every element -- a histogram pass on it is thousands of LDS atomics
// on one address (measured: 57 us for 5 049 values); relative to the span the first digit already spreads.
AVSR_DEV unsigned f2key(float f) {
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
AVSR_DEV unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
AVSR_DEV unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }
AVSR_DEV int wave_incl_scan(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

constexpr int SEL_NT = 1024;  // threads of the selection kernels (the per-element passes are latency chains: more lanes, fewer trips)

struct RadixScratch {
    int hist[256];
    unsigned wmin[SEL_NT / 64], wmax[SEL_NT / 64];
    unsigned prefix, mask;
    int remaining;
    int wtot[2][SEL_NT / 64];
};

// keys[0 .. n): finds the S-th largest key `thr`; returns the number of keys above it, `eq_take` = how many keys equal to it
// belong to the selection (taken in index order).  S <= n.  All SEL_NT threads call it.
AVSR_DEV void radix_select(const unsigned* keys, int n, int S, RadixScratch& sc, unsigned& thr, int& n_gt, int& eq_take) {
    constexpr int NWV = SEL_NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned lo = 0xffffffffu, hi = 0u;
    for (int i = tid; i < n; i += SEL_NT) {
        lo = umin(lo, keys[i]);
        hi = umax(hi, keys[i]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo = umin(lo, (unsigned)__shfl_xor((int)lo, m));
        hi = umax(hi, (unsigned)__shfl_xor((int)hi, m));
    }
    if (lane == 0) {
        sc.wmin[wave] = lo;
        sc.wmax[wave] = hi;
    }
    if (tid == 0) {
        sc.prefix = 0u;
        sc.mask = 0u;
        sc.remaining = S;
    }
    __syncthreads();
    unsigned kmin = sc.wmin[0], kmax = sc.wmax[0];
#pragma unroll
    for (int w = 1; w < NWV; w++) {
        kmin = umin(kmin, sc.wmin[w]);
        kmax = umax(kmax, sc.wmax[w]);
    }
    const unsigned span = kmax - kmin;
    int bits = 0;
    while (bits < 32 && (span >> bits) != 0u) bits++;
    const int npass = (bits + 7) / 8;
    for (int pass = npass - 1; pass >= 0; pass--) {
        if (tid < 256) sc.hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = sc.prefix, mask = sc.mask;
        for (int i = tid; i < n; i += SEL_NT) {
            const unsigned k = keys[i] - kmin;
            if ((k & mask) == prefix) atomicAdd(&sc.hist[(k >> (8 * pass)) & 255u], 1);
        }
        __syncthreads();
        // digit d with  #(digits > d) < remaining <= #(digits >= d):  thread t < 256 looks at digit 255 - t; inclusive scan from the top
        const int rem = sc.remaining, own = tid < 256 ? sc.hist[255 - tid] : 0;
        int incl = tid < 256 ? wave_incl_scan(own, lane) : 0;  // (waves 0 - 3 whole: wave-uniform)
        if (tid < 256 && lane == 63) sc.wtot[0][wave] = incl;
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < wave; w++) incl += sc.wtot[0][w];
            if (incl >= rem && incl - own < rem) {  // exactly one thread
                sc.remaining = rem - (incl - own);  // entries still to take among the keys that share the prefix extended by this digit
                sc.prefix = prefix | ((unsigned)(255 - tid) << (8 * pass));
                sc.mask = mask | (255u << (8 * pass));
            }
        }
        __syncthreads();
    }
    thr = sc.prefix + kmin;
    eq_take = sc.remaining;
    n_gt = S - eq_take;
}

// the selected keys' indices in index order (greater-than-threshold ones first, then the ties): out[0 .. S)
AVSR_DEV void radix_compact(const unsigned* keys, int n, unsigned thr, int n_gt, int eq_take, RadixScratch& sc, int* out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (n + SEL_NT - 1) / SEL_NT;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    int ngt = 0, neq = 0;
    for (int i = lo; i < hi; i++) {
        ngt += keys[i] > thr;
        neq += keys[i] == thr;
    }
    const int sg = wave_incl_scan(ngt, lane), se = wave_incl_scan(neq, lane);
    if (lane == 63) {
        sc.wtot[0][wave] = sg;
        sc.wtot[1][wave] = se;
    }
    __syncthreads();
    int og = sg - ngt, oe = se - neq;
    for (int w = 0; w < wave; w++) {
        og += sc.wtot[0][w];
        oe += sc.wtot[1][w];
    }
    for (int i = lo; i < hi; i++) {
        const unsigned k = keys[i];
        if (k > thr) out[og++] = i;
        else if (k == thr) {
            if (oe < eq_take) out[n_gt + oe] = i;
            oe++;
        }
    }
}

// Pre-beam (beam_search.py:240-262 with pre_beam_score_key = "decoder" / "full"): the S best tokens of every row of the
// decoder's scores, as a SET -- fused with the log-softmax that produces those scores (transformer_decoder.py:256:
// logp = logits - logsumexp(logits), written for the selection kernel; the order of a row is that of its logits).
__global__ __launch_bounds__(SEL_NT) void logsoftmax_prebeam_kernel(const float* __restrict__ logits, float* __restrict__ logp, long ld, int V,
                                                                 int S, int64_t* __restrict__ cand) {
    AVSR_DYN_SMEM(smem);
    unsigned* keys = reinterpret_cast<unsigned*>(smem);  // [V]
    int* picked = reinterpret_cast<int*>(keys + V);      // [S]
    __shared__ RadixScratch sc;
    __shared__ float redf[SEL_NT / 64];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* x = logits + (size_t)row * ld;
    float m = -INFINITY;
    for (int i = tid; i < V; i += SEL_NT) {
        const float v = x[i];
        keys[i] = f2key(v);
        m = fmaxf(m, v);
    }
    m = wave_max(m);
    if (lane == 0) redf[wave] = m;
    __syncthreads();
    m = redf[0];
    for (int w = 1; w < SEL_NT / 64; w++) m = fmaxf(m, redf[w]);
    __syncthreads();
    float l = 0.f;
    for (int i = tid; i < V; i += SEL_NT) l += expf(x[i] - m);
    l = wave_sum(l);
    if (lane == 0) redf[wave] = l;
    __syncthreads();
    float lsum = 0.f;
    for (int w = 0; w < SEL_NT / 64; w++) lsum += redf[w];
    const float lse = m + logf(lsum);
    float* y = logp + (size_t)row * ld;
    for (int i = tid; i < V; i += SEL_NT) y[i] = x[i] - lse;
    unsigned thr;
    int n_gt, eq_take;
    radix_select(keys, V, S, sc, thr, n_gt, eq_take);
    radix_compact(keys, V, thr, n_gt, eq_take, sc, picked);
    __syncthreads();
    for (int i = tid; i < S; i += SEL_NT) cand[(size_t)row * S + i] = picked[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// Scores of the viable extensions and the beam's K best (beam_search.py:264-297, batch_beam_search.py:107-129): hypothesis b
// extended by one of its S candidates or by <eos> (scorers/ctc.py gives <eos> its complete-sequence probability whether
// or not the pre-beam kept it; every other token outside the candidates carries the CTC scorer's LOGZERO and cannot
// reach a beam of K <= n * (S - 1) -- the host refuses configurations where it could).  Arithmetic order as the python
// form: ((w_dec * logp [+ w_lm * lm_logp] + w_len) + w_ctc * (log_psi - s_prev)) + score, f32; the language model's term
// (shallow fusion, scorers["lm"]) only with a session that carries one, then, with a bias list, + w_bias * gain (the order of the
// python step over the full scorers: decoder, lm, bias, length_bonus); with an n-gram model + w_ngram * log p_ngram after the CTC
// term (the partial scorers in their listed order: ctc, ngram), before the hypothesis' score.  ONE block: radix select of the
// K best values, then a rank sort of those K (value descending, entry ascending).
// ---------------------------------------------------------------------------------------------------------------------
// the lookup on its own (avsr_bias_score): entry (row, c) of gain / next [n][S + 1], column S = <eos>
__global__ __launch_bounds__(256) void bias_score_kernel(BiasTab t, const int* __restrict__ node, const int64_t* __restrict__ cand, int n, int S,
                                                         int eos, float* __restrict__ gain, int* __restrict__ next) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * (S + 1)) return;
    const int row = (int)(i / (S + 1)), c = (int)(i - (long)row * (S + 1));
    int g = 0, nx = 0;
    if (t.n_nodes > 0) g = bias_gain(t, node[row], c < S ? (int)cand[(size_t)row * S + c] : eos, nx);
    gain[i] = (float)g;
    next[i] = nx;
}

// the lookup on its own (avsr_ngram_score): entry (row, c) of score / next [n][S + 1], column S = <eos>
__global__ __launch_bounds__(256) void ngram_score_kernel(NgramTab t, const int* __restrict__ node, const int64_t* __restrict__ cand, int n, int S,
                                                          int eos, int blank, float* __restrict__ score, int* __restrict__ next) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * (S + 1)) return;
    const int row = (int)(i / (S + 1)), c = (int)(i - (long)row * (S + 1));
    float r = 0.f;
    int nx = 0;
    if (t.n_nodes > 0) r = ngram_logp(t, node[row], c < S ? (int)cand[(size_t)row * S + c] : eos, blank, nx);
    score[i] = r;
    next[i] = nx;
}

struct SelectArgs {
    const float* logp;  // [n][ld] decoder log-probabilities
    long ld;
    const int64_t* cand;  // [n][S]
    const float *psi, *psi_eos, *s_prev, *score;
    int n, S, K;
    int eos, blank, has_len;
    float w_dec, w_ctc, w_len;
    const float* lm_logp;  // [n][ld] language-model log-probabilities, NULL: no language model
    float w_lm;
    int* sel;     // [K][4]: prev, tok, candidate column (-1: <eos> outside the candidates), trie node reached (0 without a bias list)
    float* selv;  // [K][4]: total, decoder term logp, ctc term (log_psi - s_prev), ctc log_psi
    BiasTab bias;      // contextual biasing: the trie, n_nodes == 0 without a list
    const int* node;   // [n] trie node of every hypothesis
    float w_bias;
    float* selg;       // [K] gain of the selected extensions
    NgramTab ng;         // n-gram model: the tables, n_nodes == 0 without one
    const int* ng_node;  // [n] the model's node of every hypothesis
    float w_ng;
    float* selng;  // [K] the model's log-probability of the selected extensions
    int* selnn;    // [K] the node they reach
};

// row0: the packed row of the utterance's hypothesis 0 (what `prev` counts from)
AVSR_DEV void beam_select_block(char* smem, RadixScratch& sc, const SelectArgs& a, int row0) {
    const int NE = a.n * (a.S + 1);
    float* val = reinterpret_cast<float*>(smem);            // [NE]
    unsigned* keys = reinterpret_cast<unsigned*>(val + NE);  // [NE]
    int* picked = reinterpret_cast<int*>(keys + NE);         // [K]
    int* cnd = picked + a.K;                                 // [n][S] candidate tokens
    int* has_eos = cnd + a.n * a.S;                          // [n] <eos> is among the candidates of hypothesis b
    const int tid = threadIdx.x;
    for (int i = tid; i < a.n; i += SEL_NT) has_eos[i] = 0;
    __syncthreads();
    for (int i = tid; i < a.n * a.S; i += SEL_NT) {
        const int t = (int)a.cand[i];
        cnd[i] = t;
        if (t == a.eos) has_eos[i / a.S] = 1;
    }
    __syncthreads();
    auto decode = [&](int e, int& b, int& c, int& tok, float& dec, float& ctc_rel, float& log_psi) -> bool {
        b = e / (a.S + 1);
        c = e - b * (a.S + 1);
        bool valid = true;
        if (c < a.S) tok = cnd[b * a.S + c];
        else {
            tok = a.eos;
            valid = !has_eos[b];
            c = -1;
        }
        log_psi = tok == a.blank ? LOGZERO : (tok == a.eos ? a.psi_eos[b] : a.psi[(size_t)b * a.S + c]);
        ctc_rel = log_psi - a.s_prev[b];
        dec = a.logp[(size_t)b * a.ld + tok];
        return valid;
    };
    for (int e = tid; e < NE; e += SEL_NT) {
        int b, c, tok;
        float dec, ctc_rel, log_psi, v = -INFINITY;
        if (decode(e, b, c, tok, dec, ctc_rel, log_psi)) {
            float w = a.w_dec * dec;
            if (a.lm_logp) w = w + a.w_lm * a.lm_logp[(size_t)b * a.ld + tok];
            if (a.bias.n_nodes) {
                int nx;
                w = w + a.w_bias * (float)bias_gain(a.bias, a.node[b], tok, nx);
            }
            if (a.has_len) w = w + a.w_len;
            w = w + a.w_ctc * ctc_rel;
            if (a.ng.n_nodes) {  // a partial scorer after the CTC term, the order of the python step
                int nx;
                w = w + a.w_ng * ngram_logp(a.ng, a.ng_node[b], tok, a.blank, nx);
            }
            v = w + a.score[b];
            if (!(v == v)) v = -INFINITY;
        }
        val[e] = v;
        keys[e] = f2key(v);
    }
    __syncthreads();
    unsigned thr;
    int n_gt, eq_take;
    radix_select(keys, NE, a.K, sc, thr, n_gt, eq_take);
    radix_compact(keys, NE, thr, n_gt, eq_take, sc, picked);
    __syncthreads();
    for (int r = tid; r < a.K; r += SEL_NT) {
        const int e = picked[r];
        const float v = val[e];
        int rank = 0;
        for (int j = 0; j < a.K; j++) {
            const int ej = picked[j];
            const float vj = val[ej];
            rank += vj > v || (vj == v && ej < e);
        }
        int b, c, tok;
        float dec, ctc_rel, log_psi;
        decode(e, b, c, tok, dec, ctc_rel, log_psi);
        a.sel[4 * rank + 0] = row0 + b;
        a.sel[4 * rank + 1] = tok;
        a.sel[4 * rank + 2] = c;
        int nx = 0;
        if (a.bias.n_nodes) a.selg[rank] = (float)bias_gain(a.bias, a.node[b], tok, nx);
        a.sel[4 * rank + 3] = nx;
        if (a.ng.n_nodes) {
            int nn;
            a.selng[rank] = ngram_logp(a.ng, a.ng_node[b], tok, a.blank, nn);
            a.selnn[rank] = nn;
        }
        a.selv[4 * rank + 0] = v;
        a.selv[4 * rank + 1] = dec;
        a.selv[4 * rank + 2] = ctc_rel;
        a.selv[4 * rank + 3] = log_psi;
    }
}

// One block per utterance of a group on that utterance's entries: `a` describes the packed tables (row 0 of the group), the block
// moves to its own rows.  K best of the utterance's n * (S + 1) entries, same order of additions, same tie rule.
__global__ __launch_bounds__(SEL_NT) void beam_select_group_kernel(SelectArgs a, Group grp) {
    AVSR_DYN_SMEM(smem);
    __shared__ RadixScratch sc;
    const Utt d = grp.u[blockIdx.x];
    if (d.n == 0) return;
    a.logp += (size_t)d.off * a.ld;
    if (a.lm_logp) a.lm_logp += (size_t)d.off * a.ld;
    a.cand += (size_t)d.off * a.S;
    a.psi += (size_t)d.off * a.S;
    a.psi_eos += d.off;
    a.s_prev += d.off;
    a.score += d.off;
    a.n = d.n;
    a.sel += 4 * d.noff;
    a.selv += 4 * d.noff;
    if (a.bias.n_nodes) {
        a.node += d.off;
        a.selg += d.noff;
    }
    if (a.ng.n_nodes) {
        a.ng_node += d.off;
        a.selng += d.noff;
        a.selnn += d.noff;
    }
    beam_select_block(smem, sc, a, d.off);
}

// ---------------------------------------------------------------------------------------------------------------------
// Beam state (device): hypothesis-major token and ancestry tables + per-hypothesis scalars + the CTC forward variables.
struct BeamBuf {
    int64_t* yseq;  // [beam][ldy]
    int* anc;       // [beam][ldy]: slot of the hypothesis' ancestor at position j (the row its K / V were written to)
    int64_t* last;  // [beam] last token
    float* sc;      // [6][beam]: total, decoder sum, ctc sum, length sum, ctc log prefix probability s, language-model sum
    float* r;       // [T][2][n] (pitch = current n)
    int* node;      // [beam] trie node of the bias list, NULL without one
    float* bias;    // [beam] running sum of the bias gains, NULL without a list
    int* ng_node;   // [beam] node of the n-gram model, NULL without one
    float* ng_sum;  // [beam] running sum of the model's log-probabilities, NULL without one
};

// what the n-gram model adds to the update of a step: log-probabilities and nodes of the selected entries, the running sums of the
// new beam for the host (avsr_beam_ngram_sums); all NULL without a model
struct NgramSel {
    const float* selng;
    const int* selnn;
    float* host_sum;
};

// new hypothesis k = hypothesis prev[k] extended by tok[k]  (batch_beam_search.py:131-176 merge + select states)
// k, prev: rows of the tables (pitch `beam` of the scalars); kl, pl: the same hypotheses counted within their utterance, whose CTC
// state is r_new [T][2][n_src][S] -> dst_r [T][2][K]
AVSR_DEV void beam_update_row(const BeamBuf& src, const BeamBuf& dst, int ldy, int beam, int L, int n_src, int K, int T, int S, int k, int kl,
                              int row0, const int* __restrict__ sel, const float* __restrict__ selv, const float* __restrict__ r_new,
                              float* __restrict__ dst_r, const float* __restrict__ lm_logp, long ld_lm, const float* __restrict__ selg,
                              float* __restrict__ host_row, const NgramSel& ng) {
    const int tid = threadIdx.x;
    const int prev = sel[4 * k], tok = sel[4 * k + 1], pl = prev - row0;
    int pos = sel[4 * k + 2];
    if (pos < 0) pos = S - 1;  // <eos> outside the candidates: the hypothesis ends here, its CTC state is never read
    for (int j = tid; j < L; j += 256) {
        dst.yseq[(size_t)k * ldy + j] = src.yseq[(size_t)prev * ldy + j];
        if (j < L - 1) dst.anc[(size_t)k * ldy + j] = src.anc[(size_t)prev * ldy + j];
    }
    if (tid == 0) {
        dst.yseq[(size_t)k * ldy + L] = tok;
        dst.anc[(size_t)k * ldy + L - 1] = prev;
        dst.last[k] = tok;
        const float total = selv[4 * k], dec = selv[4 * k + 1], ctc_rel = selv[4 * k + 2], log_psi = selv[4 * k + 3];
        const float s_dec = src.sc[1 * beam + prev] + dec, s_ctc = src.sc[2 * beam + prev] + ctc_rel, s_len = src.sc[3 * beam + prev] + 1.f;
        dst.sc[0 * beam + k] = total;
        dst.sc[1 * beam + k] = s_dec;
        dst.sc[2 * beam + k] = s_ctc;
        dst.sc[3 * beam + k] = s_len;
        dst.sc[4 * beam + k] = log_psi;
        const float s_lm = src.sc[5 * beam + prev] + (lm_logp ? lm_logp[(size_t)prev * ld_lm + tok] : 0.f);
        dst.sc[5 * beam + k] = s_lm;
        float* h = host_row + 8 * k;
        h[0] = (float)tok;
        h[1] = (float)prev;
        h[2] = total;
        h[3] = s_dec;
        h[4] = s_ctc;
        h[5] = s_len;
        h[6] = s_lm;
        float s_bias = 0.f;
        if (dst.node) {  // the node the select kernel found for (prev, tok) and the running sum of gains
            dst.node[k] = sel[4 * k + 3];
            dst.bias[k] = s_bias = src.bias[prev] + selg[k];
        }
        h[7] = s_bias;
        if (dst.ng_node) {  // as the bias: the node the select kernel found for (prev, tok), the running f32 sum
            dst.ng_node[k] = ng.selnn[k];
            ng.host_sum[k] = dst.ng_sum[k] = src.ng_sum[prev] + ng.selng[k];
        }
    }
    // CTC forward variables of (prev, candidate column pos): r_new [T][2][n_src][S] -> dst.r [T][2][K]
    for (int i = tid; i < 2 * T; i += 256) dst_r[(size_t)i * K + kl] = r_new[((size_t)i * n_src + pl) * S + pos];
}

// the utterance that owns row k of the beam being written
AVSR_DEV int utt_of_new_row(const Group& g, int k) {
    int u = 0;
    while (u + 1 < g.U && k >= g.u[u + 1].noff) u++;
    return u;
}

// block = new packed row; the scalars have pitch `pitch` (the group's rows), an utterance's CTC regions the pitch
// `beam` rows per frame: r at 2 * f0 * beam, r_new at 2 * f0 * beam * S
__global__ __launch_bounds__(256) void beam_update_group_kernel(BeamBuf src, BeamBuf dst, Group grp, int ldy, int pitch, int beam, int L, int S,
                                                                const int* __restrict__ sel, const float* __restrict__ selv,
                                                                const float* __restrict__ r_new, const float* __restrict__ lm_logp, long ld_lm,
                                                                const float* __restrict__ selg, float* __restrict__ host_row, NgramSel ng) {
    const int k = blockIdx.x;
    const Utt d = grp.u[utt_of_new_row(grp, k)];
    beam_update_row(src, dst, ldy, pitch, L, d.n, d.nn, d.T, S, k, k - d.noff, d.off, sel, selv, r_new + (size_t)2 * d.f0 * beam * S,
                    dst.r + (size_t)2 * d.f0 * beam, lm_logp, ld_lm, selg, host_row, ng);
}

// the listed hypotheses survive (ended ones are taken off the beam, batch_beam_search.py:178-206): new packed row k = current packed
// row keep.from[k] (of the same utterance); utterance u goes from n to nn rows
__global__ __launch_bounds__(256) void beam_keep_group_kernel(BeamBuf src, BeamBuf dst, Group grp, int ldy, int pitch, int beam, int L, RowList keep) {
    const int k = blockIdx.x, tid = threadIdx.x, from = keep.from[k];
    const Utt d = grp.u[utt_of_new_row(grp, k)];
    for (int j = tid; j < L; j += 256) {
        dst.yseq[(size_t)k * ldy + j] = src.yseq[(size_t)from * ldy + j];
        if (j < L - 1) dst.anc[(size_t)k * ldy + j] = src.anc[(size_t)from * ldy + j];
    }
    if (tid < 6) dst.sc[tid * pitch + k] = src.sc[tid * pitch + from];
    if (tid == 6) dst.last[k] = src.last[from];
    if (tid == 7 && src.node) {
        dst.node[k] = src.node[from];
        dst.bias[k] = src.bias[from];
    }
    if (tid == 8 && src.ng_node) {
        dst.ng_node[k] = src.ng_node[from];
        dst.ng_sum[k] = src.ng_sum[from];
    }
    const float* sr = src.r + (size_t)2 * d.f0 * beam;
    float* dr = dst.r + (size_t)2 * d.f0 * beam;
    const int kl = k - d.noff, fl = from - d.off;
    for (int i = tid; i < 2 * d.T; i += 256) dr[(size_t)i * d.nn + kl] = sr[(size_t)i * d.n + fl];
}

// block (x, u); utterance u starts as the one row u
__global__ void beam_init_group_kernel(BeamBuf st, Group grp, PtrList r_init, int ldy, int pitch, int beam, int sos, int ng_start) {
    const int u = blockIdx.y, tid = blockIdx.x * blockDim.x + threadIdx.x;
    const Utt d = grp.u[u];
    if (tid == 0) {
        st.yseq[(size_t)d.off * ldy] = sos;
        st.last[d.off] = sos;
        for (int i = 0; i < 6; i++) st.sc[i * pitch + d.off] = 0.f;
        if (st.node) {  // the root of the bias trie
            st.node[d.off] = 0;
            st.bias[d.off] = 0.f;
        }
        if (st.ng_node) {  // the n-gram model's node of <s>
            st.ng_node[d.off] = ng_start;
            st.ng_sum[d.off] = 0.f;
        }
    }
    if (tid < 2 * d.T) st.r[(size_t)2 * d.f0 * beam + tid] = r_init.p[u][tid];
}

// ---------------------------------------------------------------------------------------------------------------------
struct Layer {
    const float *n1g, *n1b, *wqkv, *bqkv, *wo, *bo, *n2g, *n2b, *wq2, *bq2, *wkv2, *bkv2, *wo2, *bo2, *n3g, *n3b, *w1, *b1, *w2, *b2;
};

struct LmLayer {
    const float *n1g, *n1b, *wqkv, *bqkv, *wo, *bo, *n2g, *n2b, *w1, *b1, *w2, *b2;
};

// The language model a session may carry next to the decoder (avsr_beam_attach_lm): ESPnet's TransformerLM, pre-norm encoder layers
// under the causal mask = the decoder's layers without source attention, on the same ancestry table.
struct Lm {
    int on = 0, D = 0, H = 0, FF = 0, nl = 0, pe_rows = 0;
    float w = 0.f, scale = 0.f, eps = 0.f;
    const float *table = nullptr, *eg = nullptr, *eb = nullptr, *pe = nullptr;  // [V][D] embed . Linear, its LayerNorm, positions
    std::vector<LmLayer> layers;
    const float *ang = nullptr, *anb = nullptr, *wout = nullptr, *bout = nullptr;
    std::vector<float*> cache;  // per layer [Lmax][beam][3 D]
    float *x = nullptr, *x1 = nullptr, *att = nullptr, *ff = nullptr, *part = nullptr, *stx = nullptr, *st1 = nullptr, *logits = nullptr,
          *logp = nullptr;
};

// The bias list a session may carry (avsr_beam_set_bias): device tables owned by the caller.
struct Bias {
    BiasTab tab{nullptr, nullptr, nullptr, nullptr, 0};
    float w = 0.f;
};

// The n-gram model a session may carry (avsr_beam_set_ngram): device tables owned by the caller.
struct Ngram {
    NgramTab tab{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    int start = 0;  // node of <s>
    float w = 0.f;
};

struct Session {
    Lm lm;
    Bias bias, bias_next;  // the list of the running utterance / group; the list the next avsr_beam_begin* takes over
    float* selg = nullptr;
    Ngram ng, ng_next;  // likewise the n-gram model
    float *selng = nullptr, *ng_host_dev = nullptr;  // [rows] log-probabilities of the selected entries, running sums of the new beam
    int* selnn = nullptr;                            // [rows] nodes the selected entries reach
    float* ng_host = nullptr;  // [MAX_ROWS] host copy of the sums of the last step (allocated with the first model, page-locked)
    int ng_host_n = 0;         // entries of it that are valid
    int D, H, FF, V, nl, beam, S, sos, eos, blank, has_len;
    float w_dec, w_ctc, w_len, emb_scale, eps;
    const float *embed, *pe;
    int pe_rows;
    std::vector<Layer> layers;
    const float *ang, *anb, *wout, *bout;
    // per group of utterances (avsr_beam_begin_batch; avsr_beam_begin: a group of one): the tables carved for U * beam rows and the
    // frames of all of them.  T: frames of the longest utterance (0: nothing begun), n: running hypotheses of all utterances
    int T = 0, Lmax = 0, ldy = 0, ldv = 0, n = 0, L = 0, cur = 0;
    BeamBuf st[2];
    std::vector<float*> cache;   // per layer [Lmax][beam][3 D]: q | k | v of the position's row
    std::vector<float*> memkv;   // per layer [T][2 D]
    float *x, *x1, *x2, *h, *att, *q2, *ff, *part, *stx, *st1, *st2, *mean, *rstd, *logits, *logp, *lse, *psi, *psi_eos, *r_new, *selv, *host_dev;
    int64_t* cand;
    int* sel;
    int U = 0;
    Utt utt[MAX_UTT];  // off / n / T / f0 of every utterance (n == 0: retired); the per-launch fields are filled by group_of
    const float* u_logp[MAX_UTT];
    int32_t u_ld[MAX_UTT];
};

// the group's descriptor for the kernels of one step: rows of the current beam, `nn[u]` rows per utterance in the beam being written
Group group_of(Session& s, const int* nn) {
    Group g;
    g.U = s.U;
    int off = 0, noff = 0, g0 = 0;
    for (int u = 0; u < MAX_UTT; u++) {
        Utt d = u < s.U ? s.utt[u] : Utt{0, 0, 0, 0, 0, 0, 0};
        d.off = off;
        d.noff = noff;
        d.nn = u < s.U ? nn[u] : 0;
        d.g0 = g0;
        off += d.n;
        noff += d.nn;
        g0 += (d.n + SRC_HB - 1) / SRC_HB;
        g.u[u] = d;
        if (u < s.U) s.utt[u].off = d.off;
    }
    g.rows = off;
    g.blocks = g0;
    g.spare = 0;
    return g;
}

struct Carver {
    char* base;
    size_t off = 0;
    template <class T> T* take(size_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

// rows: hypotheses the tables hold (U * beam), T: frames (of all utterances of the group: the per-utterance regions
// of the CTC state, of r_new and of the memory projection lie behind one another, `beam` rows per frame)
void carve(Session& s, Carver& c, size_t rows, size_t T, int Lmax) {
    const size_t per = s.beam, beam = rows, D = s.D;
    const int ldy = Lmax + 2, ldv = (s.V + 7) / 8 * 8;
    s.ldy = ldy;
    s.ldv = ldv;
    for (int i = 0; i < 2; i++) {
        s.st[i].yseq = c.take<int64_t>(beam * ldy);
        s.st[i].anc = c.take<int>(beam * ldy);
        s.st[i].last = c.take<int64_t>(beam);
        s.st[i].sc = c.take<float>(6 * beam);
        s.st[i].r = c.take<float>((size_t)2 * T * per);
    }
    s.cache.resize(s.nl);
    s.memkv.resize(s.nl);
    for (int l = 0; l < s.nl; l++) {
        s.cache[l] = c.take<float>((size_t)Lmax * beam * 3 * D);
        s.memkv[l] = c.take<float>((size_t)T * 2 * D);
    }
    s.x = c.take<float>(beam * D);
    s.x1 = c.take<float>(beam * D);
    s.x2 = c.take<float>(beam * D);
    s.h = c.take<float>(beam * D);
    s.att = c.take<float>(beam * D);
    s.q2 = c.take<float>(beam * D);
    s.ff = c.take<float>(beam * (size_t)s.FF);
    s.part = c.take<float>((size_t)8 * beam * D);
    s.stx = c.take<float>(beam * (D / 16) * 2);
    s.st1 = c.take<float>(beam * (D / 16) * 2);
    s.st2 = c.take<float>(beam * (D / 16) * 2);  // K slices of the FFN's second contraction (at most 8)
    s.mean = c.take<float>(beam);
    s.rstd = c.take<float>(beam);
    s.logits = c.take<float>(beam * (size_t)ldv);
    s.logp = c.take<float>(beam * (size_t)ldv);
    s.lse = c.take<float>(beam);
    s.cand = c.take<int64_t>(beam * (size_t)s.S);
    s.psi = c.take<float>(beam * (size_t)s.S);
    s.psi_eos = c.take<float>(beam);
    s.r_new = c.take<float>((size_t)2 * T * per * s.S);
    s.sel = c.take<int>(4 * beam);
    s.selv = c.take<float>(4 * beam);
    s.host_dev = c.take<float>(8 * beam);
    // a bias list (the one the utterance being begun takes over): per-row node and running sum, gains of the selected entries;
    // nothing is carved without one, so such a session's workspace is what it was
    for (int i = 0; i < 2; i++) {
        s.st[i].node = s.bias_next.tab.n_nodes ? c.take<int>(beam) : nullptr;
        s.st[i].bias = s.bias_next.tab.n_nodes ? c.take<float>(beam) : nullptr;
    }
    s.selg = s.bias_next.tab.n_nodes ? c.take<float>(beam) : nullptr;
    // an n-gram model, on the same terms: per-row node and running sum, log-probability and node of the selected entries, the sums
    // of the new beam for the host
    const bool ng = s.ng_next.tab.n_nodes != 0;
    for (int i = 0; i < 2; i++) {
        s.st[i].ng_node = ng ? c.take<int>(beam) : nullptr;
        s.st[i].ng_sum = ng ? c.take<float>(beam) : nullptr;
    }
    s.selng = ng ? c.take<float>(beam) : nullptr;
    s.selnn = ng ? c.take<int>(beam) : nullptr;
    s.ng_host_dev = ng ? c.take<float>(beam) : nullptr;
    if (s.lm.on) {
        Lm& m = s.lm;
        const size_t Dl = m.D;
        m.cache.resize(m.nl);
        for (int l = 0; l < m.nl; l++) m.cache[l] = c.take<float>((size_t)Lmax * beam * 3 * Dl);
        m.x = c.take<float>(beam * Dl);
        m.x1 = c.take<float>(beam * Dl);
        m.att = c.take<float>(beam * Dl);
        m.ff = c.take<float>(beam * (size_t)m.FF);
        m.part = c.take<float>((size_t)8 * beam * Dl);
        m.stx = c.take<float>(beam * (Dl / 16) * 2);
        m.st1 = c.take<float>(beam * (Dl / 16) * 2);
        m.logits = c.take<float>(beam * (size_t)ldv);
        m.logp = c.take<float>(beam * (size_t)ldv);
    }
}

int gemm(const float* A, int lda, const float* B, int M, int N, int K, const float* bias, int act, const float* resid, int ldr, float* C,
         int ldc, hipStream_t stream) {
    return avsr_gemm_f32s_nt(A, lda, B, K, M, N, K, bias, act, nullptr, 0, 0, 1.f, 0.f, 0, nullptr, 1.f, nullptr, resid, 0, ldr, C, 0, ldc,
                             0, 1, 0, nullptr, 0, nullptr, 0, stream);
}

// Contraction lengths skinny16_kernel takes: K = 64 * nw * Z with nw waves of an instantiated block size, Z K slices (<= max_slices).
// Returns Z, 0 when there is none.  The ONE statement of the rule on the device side (decode_native.skinny_len_ok on the host side).
int skinny_slices(int K, int max_slices) {
    auto ok_nw = [](int nw) { return nw >= 1 && nw <= 12 && (nw <= 4 || nw % 2 == 0); };  // the instantiated block sizes
    if (K < 64 || K % 64) return 0;
    for (int Z = 1; Z <= max_slices; Z++)
        if (K % (64 * Z) == 0 && ok_nw(K / (64 * Z))) return Z;
    return 0;
}
bool skinny_len_ok(int K, bool sliced_ok) { return skinny_slices(K, sliced_ok ? 8 : 1) != 0; }

// per-row (sum, sum of squares) partials left by the producer of a [M][D] activation for the LayerNorm that consumes it
struct RowStats {
    float* buf;  // [M][nt][2]
    int nt;
};

// C = act(LN?(A) W^T + bias) + resid for the <= beam rows of a decoding step (skinny16_kernel).  ln_g == NULL: no LayerNorm;
// otherwise `in` holds the statistics of A's rows.  out (may be NULL): receives the statistics of C's rows.
int skinny(const float* A, int lda, const float* W, int M, int N, int K, const float* bias, const float* ln_g, const float* ln_b, float eps,
           const RowStats* in, int act, const float* resid, int ldr, float* C, int ldc, RowStats* out, float* partial, hipStream_t stream) {
    // K slices across blocks when K exceeds the 16 waves x 64 columns of a block (the FFN's second contraction: K = 2048 /
    // 3072): partial sums, finished by rowsum_kernel
    const int Z = skinny_slices(K, 8);
    if (Z == 0 || (Z > 1 && (ln_g || act != 0 || !partial))) {
        avsr_set_error("beam_step: unsupported contraction length");
        return 1;
    }
    const int nw = K / (64 * Z);
    const dim3 grid((N + 15) / 16, (M + SK16_ROWS - 1) / SK16_ROWS, Z);
    SkinnyArgs a{A, lda, W, K, bias, ln_g, ln_b, eps, in ? in->buf : nullptr, in ? in->nt : 0, resid, ldr, C, ldc,
                 (out && Z == 1) ? out->buf : nullptr, M, N, K, act, Z, partial};
    if (out) out->nt = Z == 1 ? (int)grid.x : 1;
#define SKINNY_CASE(NW) AVSR_LAUNCH((skinny16_kernel<NW>), grid, dim3(64 * NW), (size_t)NW * SK16_ROWS * 17 * sizeof(float), stream, a)
    switch (nw) {
        case 1: SKINNY_CASE(1); break;
        case 2: SKINNY_CASE(2); break;
        case 3: SKINNY_CASE(3); break;
        case 4: SKINNY_CASE(4); break;
        case 6: SKINNY_CASE(6); break;
        case 8: SKINNY_CASE(8); break;
        case 10: SKINNY_CASE(10); break;
        case 12: SKINNY_CASE(12); break;
        default: avsr_set_error("beam_step: unsupported contraction length"); return 1;
    }
#undef SKINNY_CASE
    if (Z > 1)
        AVSR_LAUNCH(rowsum_kernel, dim3(M), dim3(256), 0, stream, (const float*)partial, Z, M, N, bias, resid, (long)ldr, C, (long)ldc,
                    out ? out->buf : (float*)nullptr);
    return 0;
}

__global__ void iota_rows_kernel(int* __restrict__ t, int len) {
    for (int j = threadIdx.x; j < len; j += blockDim.x) t[(size_t)blockIdx.x * len + j] = blockIdx.x;
}


void lm_release(Lm& m) { m.on = 0; }

// The language model's pass over the new position of the n running hypotheses: log-probabilities of the next token into lm.logp
// [n][ldv].  Same shape as the decoder's pass without source attention: 2 + 5 launches per layer (6 with a sliced second FFN
// contraction) + 1.
int lm_step(Session& s, const BeamBuf& st, int n, int L, int pitch, hipStream_t stream) {
    Lm& m = s.lm;
    const int D = m.D, beam = pitch;  // slots per position of the cache
    const float scale = 1.0f / sqrtf(64.f);
    RowStats sx{m.stx, 1}, s1{m.st1, 0};
    AVSR_LAUNCH(lm_input_kernel, dim3(n), dim3(256), 0, stream, (const int64_t*)st.last, m.table, m.eg, m.eb, m.eps, m.pe + (size_t)(L - 1) * D,
                m.scale, D, m.x, sx.buf);
    const int wv = L <= 64 ? 4 : (L <= 256 ? 8 : 16);
    for (int l = 0; l < m.nl; l++) {
        const LmLayer& w = m.layers[l];
        float* row = m.cache[l] + (size_t)(L - 1) * beam * 3 * D;
        int rc = skinny(m.x, D, w.wqkv, n, 3 * D, D, w.bqkv, w.n1g, w.n1b, m.eps, &sx, 0, nullptr, 0, row, 3 * D, nullptr, nullptr, stream);
        if (rc) return rc;
        AVSR_LAUNCH(dec_attn_kernel, dim3(n, m.H), dim3(64 * wv), (size_t)(L + 64 * wv) * sizeof(float), stream, (const float*)row, (long)3 * D,
                    (const float*)m.cache[l], (long)beam * 3 * D, (long)3 * D, D, 2 * D, (const int*)st.anc, s.ldy, L, scale, m.att, (long)D);
        if ((rc = skinny(m.att, D, w.wo, n, D, D, w.bo, nullptr, nullptr, 0.f, nullptr, 0, m.x, D, m.x1, D, &s1, nullptr, stream))) return rc;
        if ((rc = skinny(m.x1, D, w.w1, n, m.FF, D, w.b1, w.n2g, w.n2b, m.eps, &s1, 1, nullptr, 0, m.ff, m.FF, nullptr, nullptr, stream))) return rc;
        if ((rc = skinny(m.ff, m.FF, w.w2, n, D, m.FF, w.b2, nullptr, nullptr, 0.f, nullptr, 0, m.x1, D, m.x, D, &sx, m.part, stream))) return rc;
    }
    const int rc = skinny(m.x, D, m.wout, n, s.V, D, m.bout, m.ang, m.anb, m.eps, &sx, 0, nullptr, 0, m.logits, s.ldv, nullptr, nullptr, stream);
    if (rc) return rc;
    AVSR_LAUNCH(lm_logsoftmax_kernel, dim3(n), dim3(1024), 0, stream, (const float*)m.logits, m.logp, (long)s.ldv, s.V);
    return 0;
}

}  // namespace

#define DEC_TRY(call)             \
    do {                          \
        const int rc__ = (call);  \
        if (rc__ != 0) return rc__; \
    } while (0)

// The linear layer of a decoding step on its own (tests, microbenchmarks): C = act(LN?(A) W^T + bias) + resid, M <= 128 rows.
// st_in [M][st_in_nt][2]: per-row (sum, sum of squares) partials of A (LN only); st_out [M][ceil(N / 16)][2] or NULL (one partial per 16-column block: size it from out->nt): the same
// for the rows of C; partial: >= 8 * M * N floats, needed when K > 768 (K slices).  Returns the number of partials per row of
// st_out through st_out_nt (may be NULL).
extern "C" int avsr_decode_linear(const float* A, int lda, const float* W, int M, int N, int K, const float* bias, const float* ln_g,
                                  const float* ln_b, float eps, const float* st_in, int st_in_nt, int act, const float* resid, int ldr,
                                  float* C, int ldc, float* st_out, int* st_out_nt, float* partial, hipStream_t stream) {
    RowStats in{const_cast<float*>(st_in), st_in_nt}, out{st_out, 0};
    const int rc = skinny(A, lda, W, M, N, K, bias, ln_g, ln_b, eps, ln_g ? &in : nullptr, act, resid, ldr, C, ldc, st_out ? &out : nullptr,
                          partial, stream);
    if (rc != 0) return rc;
    AVSR_CHECK_LAUNCH("decode_linear");
    if (st_out_nt) *st_out_nt = out.nt;
    return 0;
}

// The single-query attention of a decoding step on its own (the python-issued step of the language model, tests): query row b of
// q [n][ldq] (H heads of 64) against keys / values kv[b][j] = kv + b * step_b + j * step_j (+ koff / voff), j < len; out [n][ldo].
extern "C" int avsr_decode_attention(const float* q, int ldq, const float* kv, int64_t step_b, int64_t step_j, int koff, int voff, int n, int H,
                                     int len, float* out, int ldo, int32_t* anc_scratch, hipStream_t stream) {
    AVSR_REQUIRE(n >= 1 && H >= 1 && len >= 1 && len <= 8192, "decode_attention: bad sizes (1 <= len <= 8192)");
    // dec_attn_kernel follows an ancestry table [n][len]: here every position of row b lives in slot b
    AVSR_LAUNCH(iota_rows_kernel, dim3(n), dim3(256), 0, stream, anc_scratch, len);
    const int wv = len <= 64 ? 4 : (len <= 256 ? 8 : 16);
    AVSR_LAUNCH(dec_attn_kernel, dim3(n, H), dim3(64 * wv), (size_t)(len + 64 * wv) * sizeof(float), stream, q, (long)ldq, kv, (long)step_j, (long)step_b,
                koff, voff, (const int*)anc_scratch, len, len, 1.0f / sqrtf(64.f), out, (long)ldo);
    AVSR_CHECK_LAUNCH("decode_attention");
    return 0;
}

// cfg: D, H, FF, V, n_layers, beam, S (pre-beam size), sos, eos, blank, has_length_bonus, pe_rows
// fcfg: w_decoder, w_ctc, w_length_bonus, embedding scale (sqrt(D), embedding.py:84), LayerNorm eps
// w: embed [V][D], pe [pe_rows][D], then per layer 20 pointers in the order of `struct Layer` (wqkv = rows of linear_q, linear_k,
// linear_v stacked; wkv2 = source attention's linear_k, linear_v stacked), then after_norm gamma, beta, output_layer W [V][D], b
extern "C" int64_t avsr_beam_create(const int32_t* cfg, const float* fcfg, const void* const* w, int n_w) {
    const int nl = cfg[4];
    if (n_w != 2 + 20 * nl + 4 || cfg[0] % 64 != 0 || cfg[0] != 64 * cfg[1] || cfg[2] % 64 != 0 || cfg[5] < 2 || cfg[5] > MAX_BEAM ||
        cfg[6] < 1 || cfg[6] > cfg[3] || (int64_t)cfg[5] * (cfg[6] + 1) > 8192 || cfg[5] > cfg[6] - 1) {
        avsr_set_error("beam_create: unsupported configuration (d_k = 64, beam in [2, 128], beam <= pre-beam - 1, beam * (pre-beam + 1) <= 8192)");
        return 0;
    }
    Session* s = new (std::nothrow) Session();
    if (!s) return 0;
    s->D = cfg[0]; s->H = cfg[1]; s->FF = cfg[2]; s->V = cfg[3]; s->nl = nl; s->beam = cfg[5]; s->S = cfg[6];
    s->sos = cfg[7]; s->eos = cfg[8]; s->blank = cfg[9]; s->has_len = cfg[10]; s->pe_rows = cfg[11];
    s->w_dec = fcfg[0]; s->w_ctc = fcfg[1]; s->w_len = fcfg[2]; s->emb_scale = fcfg[3]; s->eps = fcfg[4];
    const float* const* p = reinterpret_cast<const float* const*>(w);
    s->embed = p[0];
    s->pe = p[1];
    s->layers.resize(nl);
    for (int l = 0; l < nl; l++) memcpy(&s->layers[l], p + 2 + 20 * l, sizeof(Layer));
    static_assert(sizeof(Layer) == 20 * sizeof(void*), "Layer is 20 pointers");
    s->ang = p[2 + 20 * nl];
    s->anb = p[3 + 20 * nl];
    s->wout = p[4 + 20 * nl];
    s->bout = p[5 + 20 * nl];
    return (int64_t)(intptr_t)s;
}

extern "C" int avsr_beam_destroy(int64_t h) {
    Session* s = reinterpret_cast<Session*>((intptr_t)h);
    if (s) lm_release(s->lm);
    if (s) avsr_host_floats_free(s->ng_host);
    delete s;
    return 0;
}

// Attach a language model (shallow fusion, the reference's scorers["lm"] / weights["lm"]) to a session: ESPnet TransformerLM,
// pre-norm, vocabulary = the decoder's.  Call between avsr_beam_create and avsr_beam_begin; the workspace grows by the model's share.
// cfg: D, H, FF, n_layers, vocabulary, pe_rows
// fcfg: weight of the model's log-probabilities, input scale (sqrt(D)), LayerNorm eps
// w: table [V][D] (embed . encoder.embed.0, contracted by the caller), encoder.embed.1 gamma, beta, pe [pe_rows][D], then per layer
// 12 pointers in the order of `struct LmLayer` (wqkv = rows of linear_q, linear_k, linear_v stacked), then after_norm gamma, beta,
// decoder W [V][D], b
extern "C" int avsr_beam_attach_lm(int64_t h, const int32_t* cfg, const float* fcfg, const void* const* w, int n_w) {
    Session* sp = reinterpret_cast<Session*>((intptr_t)h);
    AVSR_REQUIRE(sp != nullptr, "beam_attach_lm: no session");
    Session& s = *sp;
    // (the workspace of a session that has begun was carved without the model's share: its steps would run on buffers that do not exist)
    AVSR_REQUIRE(s.T == 0, "beam_attach_lm: the session has begun an utterance (attach between avsr_beam_create and the first avsr_beam_begin)");
    const int D = cfg[0], H = cfg[1], FF = cfg[2], nl = cfg[3];
    AVSR_REQUIRE(nl >= 1 && n_w == 4 + 12 * nl + 4, "beam_attach_lm: pointer count does not match the layer count");
    AVSR_REQUIRE(D >= 64 && D == 64 * H && skinny_len_ok(D, false), "beam_attach_lm: unsupported width (d_k = 64, D / 64 an instantiated block size)");
    AVSR_REQUIRE(FF >= 64 && skinny_len_ok(FF, true), "beam_attach_lm: unsupported feed-forward width");
    AVSR_REQUIRE(cfg[4] == s.V, "beam_attach_lm: the language model's vocabulary differs from the decoder's");
    AVSR_REQUIRE(cfg[5] >= 2, "beam_attach_lm: bad position table");
    lm_release(s.lm);
    Lm& m = s.lm;
    m.D = D; m.H = H; m.FF = FF; m.nl = nl; m.pe_rows = cfg[5];
    m.w = fcfg[0]; m.scale = fcfg[1]; m.eps = fcfg[2];
    const float* const* p = reinterpret_cast<const float* const*>(w);
    m.table = p[0]; m.eg = p[1]; m.eb = p[2]; m.pe = p[3];
    m.layers.resize(nl);
    static_assert(sizeof(LmLayer) == 12 * sizeof(void*), "LmLayer is 12 pointers");
    for (int l = 0; l < nl; l++) memcpy(&m.layers[l], p + 4 + 12 * l, sizeof(LmLayer));
    m.ang = p[4 + 12 * nl]; m.anb = p[5 + 12 * nl]; m.wout = p[6 + 12 * nl]; m.bout = p[7 + 12 * nl];
    m.on = 1;
    return 0;
}

// The trie lookup of contextual biasing on its own (tests, the python-issued step's cross-check): row r stands at node[r]; entry
// (r, c) of gain / next [n][S + 1] is the gain of extending it by cand[r][c] (c < S) or by <eos> (c = S) and the node reached.
// n_nodes == 0 (no list): zeros.  The tables are device memory in the layout of `struct BiasTab` (search_tables.h); they are not validated.
extern "C" int avsr_bias_score(const int32_t* first, const int32_t* tok, const int32_t* child, const int32_t* unc, int n_nodes, int n_edges,
                               const int32_t* node, const int64_t* cand, int n, int S, int eos, float* gain, int32_t* next, hipStream_t stream) {
    AVSR_REQUIRE_NONE("bias_score", bias_sizes_refusal(n_nodes, n_edges));
    AVSR_REQUIRE(n >= 1 && S >= 0 && (int64_t)n * (S + 1) <= ((int64_t)1 << 30), "bias_score: bad sizes");
    const BiasTab t{first, tok, child, unc, tables_given(n_nodes, n_edges) ? n_nodes : 0};
    const long total = (long)n * (S + 1);
    AVSR_LAUNCH(bias_score_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, t, node, cand, n, S, eos, gain, next);
    AVSR_CHECK_LAUNCH("bias_score");
    return 0;
}

// Bind a bias list to a session (contextual biasing, scorers["bias"] / weights["bias"]), or replace / remove the one it has:
// cfg: n_nodes, n_edges (either 0: no list); fcfg: weight.  May be called at any time after avsr_beam_create, as often as wanted; the
// list takes effect at the next avsr_beam_begin / avsr_beam_begin_batch (a running utterance keeps the list it began with, whose
// tables must stay alive until then), and the workspace sizes reported from now on are those of a session with the new list.
extern "C" int avsr_beam_set_bias(int64_t h, const int32_t* cfg, const float* fcfg, const int32_t* first, const int32_t* tok,
                                  const int32_t* child, const int32_t* unc) {
    Session* sp = reinterpret_cast<Session*>((intptr_t)h);
    AVSR_REQUIRE(sp != nullptr, "beam_set_bias: no session");
    const int n_nodes = cfg[0], n_edges = cfg[1];
    AVSR_REQUIRE_NONE("beam_set_bias", bias_sizes_refusal(n_nodes, n_edges));
    Bias b;
    if (tables_given(n_nodes, n_edges)) {
        b.tab = BiasTab{first, tok, child, unc, n_nodes};
        AVSR_REQUIRE_NONE("beam_set_bias", missing_table(b.tab));
        AVSR_REQUIRE_NONE("beam_set_bias", weight_refusal(fcfg[0], WEIGHT_NOT_NAN));
        b.w = fcfg[0];
    }
    sp->bias_next = b;
    return 0;
}

// The n-gram lookup on its own (tests, the python-issued step's cross-check): row r stands at node[r]; entry (r, c) of score / next
// [n][S + 1] is log p of extending it by cand[r][c] (c < S) or by <eos> (c = S) and the node reached; the blank scores 0 and keeps
// the node.  n_nodes == 0 (no model): zeros.  The tables are device memory in the layout of `struct NgramTab` (search_tables.h); they are not validated.
extern "C" int avsr_ngram_score(const int32_t* first, const int32_t* tok, const float* logp, const int32_t* next_tab, const float* bow,
                                const int32_t* back, int n_nodes, int n_edges, const int32_t* node, const int64_t* cand, int n, int S, int eos,
                                int blank, float* score, int32_t* next, hipStream_t stream) {
    AVSR_REQUIRE_NONE("ngram_score", ngram_sizes_refusal(n_nodes, n_edges));
    AVSR_REQUIRE(n >= 1 && S >= 0 && (int64_t)n * (S + 1) <= ((int64_t)1 << 30), "ngram_score: bad sizes");
    const NgramTab t{first, tok, logp, next_tab, bow, back, tables_given(n_nodes, n_edges) ? n_nodes : 0};
    if (t.n_nodes != 0) AVSR_REQUIRE_NONE("ngram_score", missing_table(t));
    const long total = (long)n * (S + 1);
    AVSR_LAUNCH(ngram_score_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, t, node, cand, n, S, eos, blank, score, next);
    AVSR_CHECK_LAUNCH("ngram_score");
    return 0;
}

// Bind an n-gram model to a session (shallow fusion, scorers["ngram"] / weights["ngram"]), or replace / remove the one it has:
// cfg: n_nodes, n_edges (either 0: no model), start_node (the node of <s>); fcfg: weight.  The lifetime rules of avsr_beam_set_bias:
// any time after avsr_beam_create, as often as wanted; the model takes effect at the next avsr_beam_begin / avsr_beam_begin_batch (a
// running utterance keeps the one it began with, whose tables must stay alive until then), and the workspace sizes reported from now
// on are those of a session with the new model.
extern "C" int avsr_beam_set_ngram(int64_t h, const int32_t* cfg, const float* fcfg, const int32_t* first, const int32_t* tok, const float* logp,
                                   const int32_t* next_tab, const float* bow, const int32_t* back) {
    Session* sp = reinterpret_cast<Session*>((intptr_t)h);
    AVSR_REQUIRE(sp != nullptr, "beam_set_ngram: no session");
    const int n_nodes = cfg[0], n_edges = cfg[1], start = cfg[2];
    AVSR_REQUIRE_NONE("beam_set_ngram", ngram_sizes_refusal(n_nodes, n_edges));
    Ngram m;
    if (tables_given(n_nodes, n_edges)) {
        m.tab = NgramTab{first, tok, logp, next_tab, bow, back, n_nodes};
        AVSR_REQUIRE_NONE("beam_set_ngram", missing_table(m.tab));
        AVSR_REQUIRE(start >= 0 && start < n_nodes, "beam_set_ngram: the start node is not a node");
        AVSR_REQUIRE_NONE("beam_set_ngram", weight_refusal(fcfg[0], WEIGHT_FINITE));
        if (!sp->ng_host) sp->ng_host = avsr_host_floats(MAX_ROWS);
        AVSR_REQUIRE(sp->ng_host != nullptr, "beam_set_ngram: no host memory for the running sums");
        m.start = start;
        m.w = fcfg[0];
    }
    sp->ng_next = m;
    return 0;
}

// The n-gram running sums of the records of the last avsr_beam_step / avsr_beam_step_batch, in the packed order of the records: out
// [*n_out] (at most U * beam).  Read from a host copy made inside the step's own synchronisation; *n_out = 0 without a model.
extern "C" int avsr_beam_ngram_sums(int64_t h, float* out, int* n_out) {
    Session* sp = reinterpret_cast<Session*>((intptr_t)h);
    AVSR_REQUIRE(sp != nullptr && out != nullptr && n_out != nullptr, "beam_ngram_sums: no session / no output");
    const int n = sp->ng.tab.n_nodes ? sp->ng_host_n : 0;
    if (n > 0) memcpy(out, sp->ng_host, (size_t)n * sizeof(float));
    *n_out = n;
    return 0;
}

// The decoder's pass over the new position of the n running hypotheses (rows of st), L tokens each: log-probabilities into s.logp,
// pre-beam candidates into s.cand.  pitch: slots per position of the K / V caches (the rows the group's tables hold); grp: the
// utterances of the group (s.T = the longest one's frames).
static int dec_pass(Session& s, BeamBuf& st, int n, int L, int pitch, const Group& grp, hipStream_t stream) {
    const int D = s.D, beam = pitch;  // slots per position of the cache
    const float scale = 1.0f / sqrtf(64.f);
    if (s.lm.on) DEC_TRY(lm_step(s, st, n, L, pitch, stream));
    // embedding of the last token at position L - 1 (transformer_decoder.py:186-189, embedding.py:78-87) + its row statistics
    RowStats sx{s.stx, 1}, s1{s.st1, 0}, s2{s.st2, 0};
    AVSR_LAUNCH(dec_embed_kernel, dim3(n), dim3(256), 0, stream, (const int64_t*)st.last, s.embed, s.pe + (size_t)(L - 1) * D, s.emb_scale, D,
                s.x, sx.buf);
    float* x = s.x;
    for (int l = 0; l < s.nl; l++) {
        const Layer& w = s.layers[l];
        float* row = s.cache[l] + (size_t)(L - 1) * beam * 3 * D;  // this position's q | k | v rows, slot b = hypothesis b
        DEC_TRY(skinny(x, D, w.wqkv, n, 3 * D, D, w.bqkv, w.n1g, w.n1b, s.eps, &sx, 0, nullptr, 0, row, 3 * D, nullptr, nullptr, stream));
        const int wv_self = L <= 64 ? 4 : (L <= 256 ? 8 : 16), wv_src = s.T <= 64 ? 4 : (s.T <= 256 ? 8 : 16);  // waves per attention block
        AVSR_LAUNCH(dec_attn_kernel, dim3(n, s.H), dim3(64 * wv_self), (size_t)(L + 64 * wv_self) * sizeof(float), stream, (const float*)row, (long)3 * D,
                    (const float*)s.cache[l], (long)beam * 3 * D, (long)3 * D, D, 2 * D, (const int*)st.anc, s.ldy, L, scale, s.att, (long)D);
        DEC_TRY(skinny(s.att, D, w.wo, n, D, D, w.bo, nullptr, nullptr, 0.f, nullptr, 0, x, D, s.x1, D, &s1, nullptr, stream));
        DEC_TRY(skinny(s.x1, D, w.wq2, n, D, D, w.bq2, w.n2g, w.n2b, s.eps, &s1, 0, nullptr, 0, s.q2, D, nullptr, nullptr, stream));
        // (block size and LDS of the longest utterance; every block works with the waves of its own)
        AVSR_LAUNCH(dec_src_attn_group_kernel, dim3(grp.blocks, s.H), dim3(64 * wv_src), (size_t)SRC_HB * (s.T + 64 * wv_src) * sizeof(float), stream,
                    grp, (const float*)s.q2, (long)D, (const float*)s.memkv[l], (long)2 * D, D, scale, s.att, (long)D);
        DEC_TRY(skinny(s.att, D, w.wo2, n, D, D, w.bo2, nullptr, nullptr, 0.f, nullptr, 0, s.x1, D, s.x2, D, &s2, nullptr, stream));
        DEC_TRY(skinny(s.x2, D, w.w1, n, s.FF, D, w.b1, w.n3g, w.n3b, s.eps, &s2, 1, nullptr, 0, s.ff, s.FF, nullptr, nullptr, stream));
        DEC_TRY(skinny(s.ff, s.FF, w.w2, n, D, s.FF, w.b2, nullptr, nullptr, 0.f, nullptr, 0, s.x2, D, s.x, D, &sx, s.part, stream));
    }
    DEC_TRY(skinny(x, D, s.wout, n, s.V, D, s.bout, s.ang, s.anb, s.eps, &sx, 0, nullptr, 0, s.logits, s.ldv, nullptr, nullptr, stream));
    AVSR_LAUNCH(logsoftmax_prebeam_kernel, dim3(n), dim3(SEL_NT), (size_t)(s.V + s.S) * sizeof(unsigned), stream, (const float*)s.logits, s.logp,
                (long)s.ldv, s.V, s.S, s.cand);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// A GROUP of utterances through the same steps (batch_beam_search.py:208-349 once per utterance in the reference: the searches are
// independent, a label-synchronous step serves them together).  The running hypotheses of all utterances are one packed row list --
// utterance u owns rows [off[u], off[u] + n[u]) -- at the same position L (they start together), so embedding, linear layers,
// self-attention (cache pitch U * beam, ancestry = packed row of the ancestor at that step), pre-beam and the language model's pass
// run on the packed rows as they are, n = all rows; source attention, CTC prefix scores, the selection (one block per utterance,
// K = beam each) and the state update take the per-utterance row range / length / regions from a descriptor.  A row's arithmetic
// does not depend on what else is in the group.
static bool group_sizes(const Session& s, int U, const int32_t* T, size_t& frames, int& Tmax) {
    if (U < 1 || U > MAX_UTT || U * s.beam > MAX_ROWS) return false;
    frames = 0;
    Tmax = 0;
    for (int u = 0; u < U; u++) {
        if (T[u] < 1) return false;
        frames += (size_t)T[u];
        Tmax = T[u] > Tmax ? T[u] : Tmax;
    }
    return true;
}

// 0 (and the error text) for a group the session does not take: more than 32 utterances or more than 1024 rows (U * beam)
extern "C" int64_t avsr_beam_batch_workspace_bytes(int64_t h, int U, const int32_t* T, int Lmax) {
    Session tmp = *reinterpret_cast<Session*>((intptr_t)h);
    size_t frames;
    int Tmax;
    if (!group_sizes(tmp, U, T, frames, Tmax) || Lmax < 1) {
        avsr_set_error("beam_batch_workspace_bytes: bad group (1 <= U <= 32, U * beam <= 1024, T >= 1)");
        return 0;
    }
    Carver c{nullptr};
    carve(tmp, c, (size_t)U * tmp.beam, frames, Lmax);
    return (int64_t)c.off + 256;
}

// New group (arrays of length U in host memory): per utterance memory [T][D] f32 (encoder output), ctc_logp [T][ld_ctc] f32
// log-softmax of the CTC head, r_init [T][2] the CTC state of the empty prefix (ctc_prefix_score.py:60-66); ONE workspace of
// avsr_beam_batch_workspace_bytes(handle, U, T, Lmax), Lmax = the most steps any of them takes.  Projects every memory's K / V for
// every layer, resets every beam to <sos>; the session takes over the bias list bound last.
extern "C" int avsr_beam_begin_batch(int64_t h, int U, const float* const* memory, const int32_t* T, const float* const* ctc_logp,
                                     const int32_t* ld_ctc, const float* const* r_init, void* ws, int64_t ws_bytes, int Lmax, hipStream_t stream) {
    Session& s = *reinterpret_cast<Session*>((intptr_t)h);
    size_t frames;
    int Tmax;
    AVSR_REQUIRE(group_sizes(s, U, T, frames, Tmax), "beam_begin_batch: group too large or empty (1 <= U <= 32, U * beam <= 1024 rows, T >= 1)");
    AVSR_REQUIRE(Lmax >= 1 && Lmax + 1 <= s.pe_rows, "beam_begin_batch: bad lengths (position table too short?)");
    AVSR_REQUIRE(!s.lm.on || Lmax + 1 <= s.lm.pe_rows, "beam_begin_batch: the language model's position table is too short");
    Carver c{reinterpret_cast<char*>(ws)};
    carve(s, c, (size_t)U * s.beam, frames, Lmax);
    AVSR_REQUIRE((int64_t)c.off <= ws_bytes, "beam_begin_batch: workspace too small");
    s.bias = s.bias_next;
    s.ng = s.ng_next;
    s.ng_host_n = 0;
    s.U = U;
    s.T = Tmax;
    s.Lmax = Lmax;
    s.n = U;
    s.L = 1;
    s.cur = 0;
    long f0 = 0;
    PtrList ri;
    int ones[MAX_UTT];
    for (int u = 0; u < MAX_UTT; u++) {
        ri.p[u] = u < U ? r_init[u] : nullptr;
        ones[u] = 1;
        if (u >= U) continue;
        s.utt[u] = Utt{u, 1, u, 1, T[u], 0, f0};
        s.u_logp[u] = ctc_logp[u];
        s.u_ld[u] = ld_ctc[u];
        for (int l = 0; l < s.nl; l++)
            DEC_TRY(gemm(memory[u], s.D, s.layers[l].wkv2, T[u], 2 * s.D, s.D, s.layers[l].bkv2, 0, nullptr, 0, s.memkv[l] + (size_t)f0 * 2 * s.D,
                         2 * s.D, stream));
        f0 += T[u];
    }
    const Group g = group_of(s, ones);
    AVSR_LAUNCH(beam_init_group_kernel, dim3((2 * Tmax + 255) / 256, U), dim3(256), 0, stream, s.st[0], g, ri, s.ldy, U * s.beam, s.beam, s.sos, s.ng.start);
    AVSR_CHECK_LAUNCH("beam_begin_batch");
    return 0;
}

// ONE step for all running hypotheses (all of length L) of all running utterances: decoder pass over the new position, pre-beam,
// CTC prefix scores, top-K per utterance, new beam state; one device-to-host copy of [rows][8] f32 records, utterance after
// utterance -- token, parent (counted within the utterance), total score, decoder / ctc / length-bonus sums, language-model sum (0
// without one), bias sum (0 without a list) -- valid on return (the call synchronises the stream).  n_out [U]: records per utterance
// (beam; 0 for a retired one: n * V >= beam always, the viable entries n * (S - 1) >= beam by the create-time check).
// With a language model attached its pass is issued first, in line on the same stream.  A bias list adds no
// launch: the selection looks the gains up where it forms the scores, the update stores the node reached.  Nor does an n-gram
// model: its back-off lookups run in the selection too; the running sums of the K records go to the session's own host buffer
// (avsr_beam_ngram_sums) by a copy issued ahead of the records' copy, under the same synchronisation -- the records stay [K][8].
extern "C" int avsr_beam_step_batch(int64_t h, float* host_out, int* n_out, hipStream_t stream) {
    Session& s = *reinterpret_cast<Session*>((intptr_t)h);
    const int U = s.U, L = s.L, beam = s.beam, pitch = U * beam;
    int nn[MAX_UTT], off[MAX_UTT], cnt[MAX_UTT], Ts[MAX_UTT];
    int64_t f0[MAX_UTT];
    for (int u = 0; u < U; u++) nn[u] = s.utt[u].n > 0 ? beam : 0;
    const Group g = group_of(s, nn);
    const int n = g.rows;
    AVSR_REQUIRE(n >= 1 && L <= s.Lmax, "beam_step_batch: no running hypotheses / maximum length reached");
    int K = 0, n_max = 0;
    for (int u = 0; u < U; u++) {
        off[u] = g.u[u].off;
        cnt[u] = g.u[u].n;
        Ts[u] = g.u[u].T;
        f0[u] = g.u[u].f0;
        K += nn[u];
        n_max = cnt[u] > n_max ? cnt[u] : n_max;
    }
    BeamBuf& st = s.st[s.cur];
    BeamBuf& nx = s.st[s.cur ^ 1];
    DEC_TRY(dec_pass(s, st, n, L, pitch, g, stream));
    DEC_TRY(avsr_ctc_prefix_score_batch(U, s.u_logp, Ts, s.u_ld, s.V, st.r, st.last, s.cand, off, cnt, f0, beam, s.S, L - 1, s.blank, s.r_new,
                                        s.psi, s.psi_eos, stream));
    SelectArgs a{s.logp, (long)s.ldv, s.cand, s.psi, s.psi_eos, st.sc + 4 * pitch, st.sc, 0, s.S, beam, s.eos, s.blank, s.has_len,
                 s.w_dec, s.w_ctc, s.w_len, s.lm.on ? s.lm.logp : nullptr, s.lm.w, s.sel, s.selv, s.bias.tab, st.node, s.bias.w, s.selg,
                 s.ng.tab, st.ng_node, s.ng.w, s.selng, s.selnn};
    AVSR_LAUNCH(beam_select_group_kernel, dim3(U), dim3(SEL_NT), (size_t)(2 * n_max * (s.S + 1) + beam + n_max * s.S + n_max) * 4, stream, a, g);
    AVSR_LAUNCH(beam_update_group_kernel, dim3(K), dim3(256), 0, stream, st, nx, g, s.ldy, pitch, beam, L, s.S, (const int*)s.sel,
                (const float*)s.selv, (const float*)s.r_new, (const float*)(s.lm.on ? s.lm.logp : nullptr), (long)s.ldv, (const float*)s.selg, s.host_dev,
                NgramSel{s.selng, s.selnn, s.ng_host_dev});
    AVSR_CHECK_LAUNCH("beam_step_batch");
    if (s.ng.tab.n_nodes) {  // the sums of the K records, into the session's own host buffer ahead of the records' copy and its sync
        const int ec = avsr_copy_to_host_async(s.ng_host, s.ng_host_dev, (size_t)K * sizeof(float), stream);
        if (ec != 0) {
            avsr_set_error2("beam_step_batch", hipGetErrorString((hipError_t)ec));
            return 2;
        }
        s.ng_host_n = K;
    }
    const int e = avsr_copy_to_host_sync(host_out, s.host_dev, (size_t)K * 8 * sizeof(float), stream);
    if (e != 0) {
        avsr_set_error2("beam_step_batch", hipGetErrorString((hipError_t)e));
        return 2;
    }
    s.cur ^= 1;
    s.L = L + 1;
    int o = 0;
    for (int u = 0; u < U; u++) {
        // (`parent` of a record is a packed row of the previous beam: the host sees it within the utterance)
        for (int k = 0; k < nn[u]; k++) host_out[(size_t)(o + k) * 8 + 1] -= (float)off[u];
        s.utt[u].n = nn[u];
        s.utt[u].off = o;
        o += nn[u];
        n_out[u] = nn[u];
    }
    s.n = K;
    return 0;
}

// Take hypotheses off the beams: keep = for utterance after utterance the ascending indices WITHIN that utterance's current beam
// that survive, n_keep [U] how many per utterance; n_keep[u] == 0 retires utterance u (it takes no further part in the steps).
extern "C" int avsr_beam_keep_batch(int64_t h, const int32_t* keep, const int32_t* n_keep, hipStream_t stream) {
    Session& s = *reinterpret_cast<Session*>((intptr_t)h);
    int nn[MAX_UTT];
    bool same = true;
    int total = 0;
    for (int u = 0; u < s.U; u++) {
        AVSR_REQUIRE(n_keep[u] >= 0 && n_keep[u] <= s.utt[u].n, "beam_keep_batch: bad count");
        nn[u] = n_keep[u];
        same = same && n_keep[u] == s.utt[u].n;
        total += n_keep[u];
    }
    if (same) return 0;
    if (total > 0) {
        const Group g = group_of(s, nn);
        RowList rl;
        int k = 0;
        for (int u = 0; u < s.U; u++)
            for (int i = 0; i < nn[u]; i++, k++) {
                AVSR_REQUIRE(keep[k] >= 0 && keep[k] < g.u[u].n, "beam_keep_batch: index out of range");
                rl.from[k] = (unsigned short)(g.u[u].off + keep[k]);
            }
        for (; k < MAX_ROWS; k++) rl.from[k] = 0;
        AVSR_LAUNCH(beam_keep_group_kernel, dim3(total), dim3(256), 0, stream, s.st[s.cur], s.st[s.cur ^ 1], g, s.ldy, s.U * s.beam, s.beam, s.L, rl);
        AVSR_CHECK_LAUNCH("beam_keep_batch");
        s.cur ^= 1;
    }
    int o = 0;
    for (int u = 0; u < s.U; u++) {
        s.utt[u].n = nn[u];
        s.utt[u].off = o;
        o += nn[u];
    }
    s.n = total;
    return 0;
}

// token sequences of all current beams: host_yseq [rows][ldy] int64, utterance after utterance (n of the last step / keep each), the
// first L entries of every row valid (synchronises)
extern "C" int avsr_beam_fetch_yseq_batch(int64_t h, int64_t* host_yseq, int* ldy_out, int* L_out, hipStream_t stream) {
    Session& s = *reinterpret_cast<Session*>((intptr_t)h);
    const int e = avsr_copy_to_host_sync(host_yseq, s.st[s.cur].yseq, (size_t)s.n * s.ldy * sizeof(int64_t), stream);
    if (e != 0) {
        avsr_set_error2("beam_fetch_yseq_batch", hipGetErrorString((hipError_t)e));
        return 2;
    }
    *ldy_out = s.ldy;
    *L_out = s.L;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// One utterance: a group of one.  The scalars of these calls are the arrays of length one of the calls above; the records, the
// workspace size (the tables of 1 * beam rows and T frames) and the results are those calls' own.
extern "C" int64_t avsr_beam_workspace_bytes(int64_t h, int T, int Lmax) { return avsr_beam_batch_workspace_bytes(h, 1, &T, Lmax); }

extern "C" int avsr_beam_begin(int64_t h, const float* memory, int T, const float* ctc_logp, int ld_ctc, const float* r_init, void* ws,
                               int64_t ws_bytes, int Lmax, hipStream_t stream) {
    return avsr_beam_begin_batch(h, 1, &memory, &T, &ctc_logp, &ld_ctc, &r_init, ws, ws_bytes, Lmax, stream);
}

extern "C" int avsr_beam_step(int64_t h, float* host_out, int* n_out, hipStream_t stream) { return avsr_beam_step_batch(h, host_out, n_out, stream); }

// take the hypotheses NOT listed off the beam (keep: ascending indices into the current beam)
extern "C" int avsr_beam_keep(int64_t h, const int32_t* keep, int n_keep, hipStream_t stream) { return avsr_beam_keep_batch(h, keep, &n_keep, stream); }

extern "C" int avsr_beam_fetch_yseq(int64_t h, int64_t* host_yseq, int* ldy_out, int* L_out, hipStream_t stream) {
    return avsr_beam_fetch_yseq_batch(h, host_yseq, ldy_out, L_out, stream);
}
