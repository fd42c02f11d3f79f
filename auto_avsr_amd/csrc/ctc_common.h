// ctc_common.h -- what the CTC loss (loss.hip) and the CTC forced alignment (ctc_align.hip) share: the log-zero constant, the
// states-per-lane limits of the one-wave trellis recursions, the blank-interleaved label builder and the emission gather.
#pragma once
#include "prims.h"

namespace {

constexpr float LOG_ZERO = -1e30f;
constexpr int CTC_MAXSPL = 8;  // states per lane -> S <= 512, L <= 255
constexpr int CTC_PF = 6;      // frames of emissions kept in flight ahead of the trellis recursion

// ---- per utterance: strip ignore_id from the padded label row, build the blank-interleaved sequence
__global__ void ctc_prepare_kernel(const int64_t* __restrict__ labels, int Lmax, int ignore_id, int blank,
                                   int* __restrict__ ext, int Smax, int* __restrict__ lens /* [B]: L_b */) {
    const int b = blockIdx.x;
    if (threadIdx.x != 0) return;
    int L = 0;
    int* e = ext + (long)b * Smax;
    e[0] = blank;
    for (int i = 0; i < Lmax; i++) {
        const int64_t y = labels[(long)b * Lmax + i];
        if (y == ignore_id) continue;
        e[2 * L + 1] = (int)y;
        e[2 * L + 2] = blank;
        L++;
    }
    lens[b] = L;
}

// ---- lpg[b,t,s] = logit[b,t,ext[b,s]] - lse[b,t]
template <class T>
__global__ __launch_bounds__(256) void ctc_gather_kernel(const T* __restrict__ logits, long ld,
                                                         const float* __restrict__ lse, const int* __restrict__ ext,
                                                         const int* __restrict__ lens, float* __restrict__ lpg, int Tlen,
                                                         int Smax) {
    const long bt = blockIdx.x;
    const int b = (int)(bt / Tlen);
    const int S = 2 * lens[b] + 1;
    const float l = lse[bt];
    for (int s = threadIdx.x; s < S; s += 256)
        lpg[bt * Smax + s] = Elem<T>::ld(logits + bt * ld + ext[(long)b * Smax + s]) - l;
}

}  // namespace
