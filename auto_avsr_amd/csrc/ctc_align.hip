// ctc_align.hip -- CTC forced alignment (ctc.py:95-242: CTC.forced_align / CTC.forced_align_batch) on the device.
//
// The reference walks the Viterbi trellis of the blank-interleaved label sequence on the host (a python double loop in float64,
// or a numpy loop over frames on a copy of the whole (T, B, V) log-softmax).  Here: the emissions come from the CTC loss's own
// helpers (row log-sum-exp, label builder, gather of the 2L+1 extended-label log-probs: ctc_common.h), then ONE wave per utterance
// runs the max-product sibling of the alpha recursion (loss.hip: SPL contiguous states per lane, neighbours by DPP wave shift,
// the next CTC_PF frames of emissions already in registers) and leaves a 2-bit back-pointer per state and frame -- the 2 SPL <= 16
// bits of a lane packed into one 16-bit word, 128 bytes per frame, stored to the workspace off the dependent chain.  The same
// wave then walks the back-pointers from the last frame to the first with the words of 64 frames at a time in registers and
// the current state in a scalar register (a walk over global memory or LDS would be T dependent round trips), and writes the
// token ids of those 64 frames with one coalesced store.
#include "prims.h"
#include "avsr_hip.h"
#include "ctc_common.h"

namespace {

constexpr int ALIGN_MAX_T = 32768;

// a wave-uniform value as a scalar / the value another lane holds (v_readfirstlane, v_readlane)
AVSR_DEV int wave_first(int v) {
#ifdef AVSR_EMU
    return __shfl(v, 0);
#else
    return __builtin_amdgcn_readfirstlane(v);
#endif
}
AVSR_DEV unsigned wave_read_lane(unsigned v, int src_lane) {
#ifdef AVSR_EMU
    return __shfl(v, src_lane);
#else
    return (unsigned)__builtin_amdgcn_readlane((int)v, src_lane);
#endif
}

template <int SPL>
__global__ __launch_bounds__(64) void ctc_viterbi_kernel(const float* __restrict__ lpg, const int* __restrict__ ext,
                                                         const int* __restrict__ lens, const int64_t* __restrict__ in_lens,
                                                         uint16_t* __restrict__ bp, int32_t* __restrict__ ali,
                                                         float* __restrict__ score, int ignore_id, int Tlen, int Smax) {
    constexpr int PF = CTC_PF;  // frames of emissions in flight (8 - 16 where a wave's 63 outstanding memory operations allow it: no faster)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int L = lens[b], S = 2 * L + 1;
    int Tb = (int)in_lens[b];
    if (Tb > Tlen) Tb = Tlen;
    if (Tb < 0) Tb = 0;
    const int* e = ext + (long)b * Smax;
    const float* lp = lpg + (long)b * Tlen * Smax;
    uint16_t* bpb = bp + (long)b * Tlen * 64;
    int32_t* out = ali + (long)b * Tlen;
    const int blank = e[0];
    const int s0 = lane * SPL;
    // can state s be entered from s-2?  (the skip[] rule of the alpha recursion)
    bool skip[SPL], valid[SPL];
    float cur[SPL];
#pragma unroll
    for (int i = 0; i < SPL; i++) {
        const int s = s0 + i;
        valid[i] = s < S;
        skip[i] = valid[i] && (s >= 2) && (e[s] != blank) && (e[s] != e[s - 2]);
        cur[i] = (valid[i] && s < 2 && Tb > 0) ? lp[s] : LOG_ZERO;
    }
    float pre[PF][SPL];
    auto fetch = [&](int t, float (&dst)[SPL]) {
#pragma unroll
        for (int i = 0; i < SPL; i++) dst[i] = (t < Tb && valid[i]) ? lp[(long)t * Smax + s0 + i] : 0.f;
    };
#pragma unroll
    for (int j = 0; j < PF; j++) fetch(1 + j, pre[j]);
    for (int t0 = 1; t0 < Tb; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            const int t = t0 + j;
            if (t >= Tb) break;
            // values owned by the lane below: n1 = its last state, n2 = the one before
            const float n1 = wave_up1(cur[SPL - 1], LOG_ZERO);
            const float n2 = SPL >= 2 ? wave_up1(cur[SPL >= 2 ? SPL - 2 : 0], LOG_ZERO) : wave_up1(n1, LOG_ZERO);
            float nxt[SPL];
            unsigned bits = 0;
#pragma unroll
            for (int i = 0; i < SPL; i++) {
                const float a1 = i >= 1 ? cur[i >= 1 ? i - 1 : 0] : n1;
                const float a2 = i >= 2 ? cur[i >= 2 ? i - 2 : 0] : (i == 1 ? n1 : n2);
                // ties go to the smallest step: stay, then s-1, then s-2 (np.argmax over the candidate order of ctc.py:130-142)
                float best = cur[i];
                unsigned k = 0;
                if (a1 > best) {
                    best = a1;
                    k = 1;
                }
                if (skip[i] && a2 > best) {
                    best = a2;
                    k = 2;
                }
                const float v = best + pre[j][i];
                nxt[i] = (valid[i] && best > LOG_ZERO) ? v : LOG_ZERO;
                bits |= k << (2 * i);
            }
#pragma unroll
            for (int i = 0; i < SPL; i++) cur[i] = nxt[i];
            bpb[(long)t * 64 + lane] = (uint16_t)bits;
            fetch(t + PF, pre[j]);
        }
    }
    // the path ends in state S-1 or S-2, whichever scores higher (S-1 on a tie, ctc.py:146-150)
    float m1 = LOG_ZERO, m2 = LOG_ZERO;
#pragma unroll
    for (int i = 0; i < SPL; i++) {
        const int s = s0 + i;
        if (valid[i] && s == S - 1) m1 = cur[i];
        if (valid[i] && s == S - 2) m2 = cur[i];
    }
    m1 = wave_max(m1);
    m2 = wave_max(m2);
    const float best = fmaxf(m1, m2);
    const bool feasible = Tb > 0 && best > LOG_ZERO * 0.5f;
    if (lane == 0) score[b] = feasible ? best : -INFINITY;
    for (int t = (feasible ? Tb : 0) + lane; t < Tlen; t += 64) out[t] = ignore_id;
    if (!feasible) return;
    // Back-trace.  Lane l reads back the very words it stored (frame f: bpb[f * 64 + l]), 64 frames at a time into registers, so
    // no load sits on the chain and nothing crosses lanes through memory; the word of the lane that owns the current state comes
    // through v_readlane, and the state itself lives in a scalar register.  Lane j keeps the state of frame fb + j, so the token
    // ids of the 64 frames leave in one coalesced store.  (Frame 0 and the frames beyond Tb carry a zero word: the state stays.)
    int s = wave_first(m1 >= m2 ? S - 1 : S - 2);
    for (int fb = (Tb - 1) & ~63; fb >= 0; fb -= 64) {
        unsigned w[64];
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const int f = fb + j;
            w[j] = (f >= 1 && f < Tb) ? (unsigned)bpb[(long)f * 64 + lane] : 0u;
        }
        int mine = 0;
#pragma unroll
        for (int j = 63; j >= 0; j--) {
            if (lane == j) mine = s;
            const unsigned word = wave_read_lane(w[j], s / SPL);
            s -= (int)((word >> (2 * (s % SPL))) & 3u);
        }
        if (fb + lane < Tb) out[fb + lane] = e[mine];
    }
}

}  // namespace

// Workspace layout: lse[B*T] f32 | lpg[B*T*Smax] f32 | ext[B*Smax] i32 | lens[B] i32 | (to 16 bytes) bp[B*T*64] u16
static int64_t align_bp_offset(int B, int T, int Lmax) {
    const int64_t Smax = 2 * (int64_t)Lmax + 1;
    const int64_t words = (int64_t)B * T * (1 + Smax) + (int64_t)B * Smax + B;
    return (words * 4 + 15) / 16 * 16;
}

extern "C" int64_t avsr_ctc_align_workspace_bytes(int B, int T, int Lmax) {
    if (B <= 0 || T <= 0 || Lmax < 0) return 64;
    return align_bp_offset(B, T, Lmax) + (int64_t)B * T * 64 * 2 + 64;
}

extern "C" int avsr_ctc_align(const void* logits, int dtype, int64_t ld, const int64_t* labels, int Lmax, int ignore_id,
                              const int64_t* in_lens, int blank, int32_t* ali, float* score, void* workspace, int B, int T,
                              int V, hipStream_t stream) {
    AVSR_REQUIRE(Lmax >= 0 && Lmax <= 255, "ctc_align: at most 255 labels per utterance");
    AVSR_REQUIRE(T <= ALIGN_MAX_T, "ctc_align: at most 32768 frames per utterance");
    AVSR_REQUIRE(ld % 8 == 0, "ctc_align: ld must be a multiple of 8");
    AVSR_REQUIRE(dtype == 0 || dtype == 1, "ctc_align: logits must be f32 or bf16");
    AVSR_REQUIRE(blank >= 0 && blank < V && V <= ld, "ctc_align: blank id outside the vocabulary");
    AVSR_REQUIRE(ignore_id < 0 || ignore_id >= V, "ctc_align: ignore_id must not be a token id");
    AVSR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "ctc_align: workspace must be 4-byte aligned");
    if (B <= 0 || T <= 0) return 0;
    const int Smax = 2 * Lmax + 1;
    float* lse = reinterpret_cast<float*>(workspace);
    float* lpg = lse + (long)B * T;
    int* ext = reinterpret_cast<int*>(lpg + (long)B * T * Smax);
    int* lens = ext + (long)B * Smax;
    uint16_t* bp = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(workspace) + align_bp_offset(B, T, Lmax));
    int rc = avsr_row_lse(logits, dtype, ld, lse, (int64_t)B * T, V, stream);
    if (rc) return rc;
    AVSR_LAUNCH(ctc_prepare_kernel, dim3(B), dim3(64), 0, stream, labels, Lmax, ignore_id, blank, ext, Smax, lens);
    if (dtype == 0)
        AVSR_LAUNCH((ctc_gather_kernel<float>), dim3(B * T), dim3(256), 0, stream, (const float*)logits, (long)ld, lse, ext, lens, lpg, T, Smax);
    else
        AVSR_LAUNCH((ctc_gather_kernel<bf16_t>), dim3(B * T), dim3(256), 0, stream, (const bf16_t*)logits, (long)ld, lse, ext, lens, lpg, T, Smax);
    const int spl = (Smax + 63) / 64;  // states per lane for the widest row of the batch (Lmax <= 255 -> at most 8)
#define AVSR_CTC_VIT(N) AVSR_LAUNCH(ctc_viterbi_kernel<N>, dim3(B), dim3(64), 0, stream, lpg, ext, lens, in_lens, bp, ali, score, ignore_id, T, Smax)
    if (spl <= 1) AVSR_CTC_VIT(1);
    else if (spl == 2) AVSR_CTC_VIT(2);
    else if (spl == 3) AVSR_CTC_VIT(3);
    else if (spl == 4) AVSR_CTC_VIT(4);
    else if (spl <= 6) AVSR_CTC_VIT(6);
    else AVSR_CTC_VIT(8);
#undef AVSR_CTC_VIT
    AVSR_CHECK_LAUNCH("ctc_align");
    return 0;
}
