// ctc_beam.hip -- the first pass of two-pass decoding: a time-synchronous CTC prefix beam search over a batch of utterances, and
// the exact CTC log-likelihood of its n-best (the CTC term of the rescoring objective).  Neither is in the reference.
//
//   avsr_ctc_beam_search   two launches.  (1) ctc_topk_kernel, one block per (utterance, frame): the K non-blank tokens of
//       largest log-posterior, sorted, with their values and the blank's -- embarrassingly parallel, off the chain.  (2)
//       ctc_beam_kernel, ONE workgroup per utterance (grid = B) that walks all of its frames: the beam (<= 64 entries, double
//       buffered) and the <= W (K + 1) <= 2112 candidates of a frame live in LDS; the (token, lp) rows of the next CB_FCH
//       frames are already in registers while a chunk is processed.  A frame is four barriers (which order LDS only):
//         P1  pairs (i, j) / (i, k) of beam entries and tokens: which entry j is the parent prefix of entry i, which token slot
//             holds i's last token, and which extension (j, k) therefore IS entry i (its mass goes to i, the extension dies);
//         P2  one thread per candidate: entry i staying (blank, repeated last token, merged extension of its parent) or entry i
//             extended by token k;
//         P3  rank of every live candidate among all of them (value descending, index ascending; the N^2 compares are spread over
//             every thread of the block, partial counts meet in LDS): rank r < W is slot r of the next beam, which is
//             therefore always sorted -- no selection network;
//         P4  the W winners write the next beam and its record.
//       Prefix identity is a pair of 32-bit integers, the two halves of a 64-bit hash chained over the tokens (h' = mix(h, c)),
//       so "the same prefix" is one integer compare wherever the two copies come from; an entry also carries its parent's
//       hash and its length.  (Two different prefixes of one utterance would have to collide in 64 bits to be confused:
//       < 1e-11 per utterance at T = 400, W = 64.)  Every prefix that enters the beam as an extension gets a node id and a
//       (parent node, token) record in the workspace; with the per-frame beam records (node, length, pb, pnb) and the token
//       sets these are the history from which the host can replay every frame -- all of it plain stores that nothing waits for.
//       The n-best token sequences are read back from the node records at the end (len(prefix) steps per hypothesis).
//   avsr_ctc_beam_search_bias   the same search with a list of boosted phrases (the trie of auto_avsr_amd/bias.py, its rules 1 to 3):
//       ctc_beam_kernel<true>.  Every beam entry also carries its trie node and its running sum of gains -- functions of the prefix'
//       tokens alone, so a staying candidate keeps them and the merge of P1 needs no new case -- and P3 ranks by total + weight *
//       sum; the masses of the recursion and every stored record stay pure CTC.  Lookups from the ROOT (rule 1 at the root, the retry
//       of rule 2) depend on the frame's tokens only: ctc_root_child_kernel resolves them off the chain, one binary search per (b, t,
//       k) among the root's children, and the search stages the result with the token rows.  Only an entry that stands at a
//       non-root node reads the tables inside the frame loop (P1: its unc; P2: its own edges, for the live extensions).
//   avsr_ctc_beam_search_ngram   the same search (plain or biased) with a back-off n-gram model (the tables and the lookup rule of
//       auto_avsr_amd/ngram.py): ctc_beam_kernel<BIAS, true>.  Every beam entry also carries the model's node of its prefix and the
//       running f32 sum G of its log-probabilities -- again functions of the tokens alone -- and P3 ranks by total (+ bias) + weight *
//       G + len_bonus * length.  Every back-off walk ends at the root, whose edge on a token depends on the frame's tokens only:
//       ctc_ngram_root_kernel resolves (logp, next) of the root per (b, t, k) off the chain and the search stages them with the token
//       rows.  P2 walks the levels below the root for the live extensions of an entry that stands below it (binary search among the
//       node's own edges, then back[]) and, without a bias list, keeps (G', next) of all W K extensions in LDS for the winners of P4
//       (65 120 bytes of static LDS); with a list those two arrays would take the kernel to 76 640 bytes, so there the W winners redo
//       their walk (60 256 bytes).  Keeping measured 15 - 17 % faster on the first pass than walking twice.
//   avsr_ctc_score   N label sequences per utterance against one [T][V] matrix of log-posteriors: label builder of ctc_common.h
//       per sequence, a gather of the 2L+1 extended-label columns, and the alpha recursion of the loss (one wave per sequence).
#include "prims.h"
#include "avsr_hip.h"
#include "ctc_common.h"
#include "search_tables.h"

namespace {

constexpr int CB_MAXW = 64, CB_MAXK = 32;
constexpr int CB_MAXC = CB_MAXW * (CB_MAXK + 1);  // candidates of a frame
constexpr int CB_FCH = 8;                         // frames per staged chunk of (token, lp) rows
constexpr int CB_STG = 3;                         // registers per thread that hold the next chunk: 8 * 65 words <= 3 * 256
constexpr int CB_STG_BIAS = 4;                    // ... with the root children of the tokens: 8 * 97 words <= 4 * 256
constexpr int CB_STG_NGRAM = 5;                   // ... with the root's (logp, next) on the tokens: 8 * 129 words <= 5 * 256
constexpr int CB_STG_BIAS_NGRAM = 6;              // ... with both: 8 * 161 words <= 6 * 256
constexpr int CB_NT_MIN = 256, CB_NT_MAX = 1024;  // threads of the search's block
constexpr int TK_NT = 256;

AVSR_DEV float neg_inf() { return -INFINITY; }
// log(e^a + e^b) with -inf as the empty sum; expf / logf of normal accuracy (the frame-by-frame tests assume it)
AVSR_DEV float lse2(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == neg_inf()) return m;
    return m + logf(1.0f + expf(-fabsf(a - b)));
}
// Barrier between the phases of a frame: orders LDS only.  __syncthreads() would also wait for every global store in flight -- the
// search's history, which nothing in the frame loop reads back -- and put a memory round trip on every frame of the chain.
AVSR_DEV void lds_barrier() {
#ifdef AVSR_EMU
    emu::sync_threads();
#else
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
#endif
}
AVSR_DEV unsigned cb_f2key(float f) {  // order-preserving integer image of a float; > 0 for every non-NaN value
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
AVSR_DEV uint64_t cb_hash(uint64_t h, int c) {  // splitmix64 finalizer over (hash of the prefix, next token)
    uint64_t z = h + ((uint64_t)(unsigned)(c + 1)) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t CB_ROOT_HASH = 0x243F6A8885A308D3ull, CB_NO_PARENT = 0ull;

// ---- per (utterance, frame): the K largest non-blank log-posteriors, by decreasing value (ties: the smaller token id first)
__global__ __launch_bounds__(TK_NT) void ctc_topk_kernel(const float* __restrict__ lp, long ld, const int64_t* __restrict__ in_lens,
                                                         int blank, int K, int Tlen, int V, int32_t* __restrict__ tok,
                                                         float* __restrict__ val, float* __restrict__ blk) {
    AVSR_DYN_SMEM(smem);
    unsigned* keys = reinterpret_cast<unsigned*>(smem);  // [V]; a thread only ever touches the elements tid, tid + TK_NT, ...
    __shared__ unsigned red[2][TK_NT / 64][2];
    const long row = blockIdx.x;
    const int b = (int)(row / Tlen), t = (int)(row % Tlen), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int64_t)t >= in_lens[b]) return;  // (block-uniform) frames beyond the utterance are not read
    const float* x = lp + row * ld;
    unsigned bk = 0u, bi = 0u;  // this thread's best remaining (key, ~index); key 0 = nothing left
    auto rescan = [&]() {
        bk = 0u;
        bi = 0u;
        for (int i = tid; i < V; i += TK_NT) {
            const unsigned k = keys[i];
            if (k > bk) {  // (ascending i: the first of equal keys stays)
                bk = k;
                bi = ~(unsigned)i;
            }
        }
    };
    for (int i = tid; i < V; i += TK_NT) keys[i] = i == blank ? 0u : cb_f2key(x[i]);
    if (tid == 0) blk[row] = x[blank];
    rescan();
    for (int k = 0; k < K; k++) {
        unsigned mk = bk, mi = bi;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned ok = (unsigned)__shfl_xor((int)mk, m), oi = (unsigned)__shfl_xor((int)mi, m);
            if (ok > mk || (ok == mk && oi > mi)) {
                mk = ok;
                mi = oi;
            }
        }
        if (lane == 0) {
            red[k & 1][wave][0] = mk;
            red[k & 1][wave][1] = mi;
        }
        __syncthreads();
        mk = red[k & 1][0][0];
        mi = red[k & 1][0][1];
#pragma unroll
        for (int w = 1; w < TK_NT / 64; w++) {
            const unsigned ok = red[k & 1][w][0], oi = red[k & 1][w][1];
            if (ok > mk || (ok == mk && oi > mi)) {
                mk = ok;
                mi = oi;
            }
        }
        const int idx = (int)~mi;  // (K <= V - 1: a key is always left)
        if (tid == 0) {
            tok[row * K + k] = idx;
            val[row * K + k] = x[idx];
        }
        if (idx % TK_NT == tid) {
            keys[idx] = 0u;
            rescan();
        }
    }
}

// ---- contextual biasing: per (utterance, frame, token slot) the root's child on that token, -1 if the root has no such edge
__global__ __launch_bounds__(256) void ctc_root_child_kernel(const int32_t* __restrict__ tok, const int64_t* __restrict__ in_lens,
                                                             BiasTab t, int K, int Tlen, long total, int32_t* __restrict__ rootc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / K;
    if ((int64_t)(row % Tlen) >= in_lens[row / Tlen]) return;  // (no token set was written for this frame)
    const int e = tab_edge(t.first, t.tok, 0, tok[i]);
    rootc[i] = e >= 0 ? t.child[e] : -1;
}

// ---- n-gram model: per (utterance, frame, token slot) the root's log-probability of the token and the node reached
__global__ __launch_bounds__(256) void ctc_ngram_root_kernel(const int32_t* __restrict__ tok, const int64_t* __restrict__ in_lens,
                                                             NgramTab g, int K, int Tlen, long total, float* __restrict__ ulogp,
                                                             int32_t* __restrict__ unext) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long row = i / K;
    if ((int64_t)(row % Tlen) >= in_lens[row / Tlen]) return;  // (no token set was written for this frame)
    const int e = tab_root_edge(g.first, g.tok, tok[i]);
    ulogp[i] = e >= 0 ? g.logp[e] : 0.f;  // (a root without the edge: the caller's tables are broken, the token scores 0)
    unext[i] = e >= 0 ? g.next[e] : 0;
}

struct BeamArgs {
    const int32_t* tok;  // [B][T][K]
    const float* val;    // [B][T][K]
    const float* blk;    // [B][T]
    int32_t* cnt;        // [B][T]
    int32_t* node;       // [B][T*W+1][2]
    int32_t* beam;       // [B][T][W][4]
    const int64_t* in_lens;
    int32_t *tokens, *lens, *n_valid;
    float *score, *pb, *pnb;
    int W, K, nbest, T;
};
struct BeamArgsBias : BeamArgs {  // contextual biasing: what ctc_beam_kernel<true> takes on top
    const int32_t* rootc;  // [B][T][K]
    BiasTab bias;  // n_nodes == 0: no list
    float b_weight;
    float* bias_sum;     // [B][nbest]
    int32_t* bias_node;  // [B][nbest]
};
struct BeamArgsNgram : BeamArgsBias {  // n-gram model: what ctc_beam_kernel<*, true> takes on top (the bias fields unused without a list)
    const float* ulogp;    // [B][T][K]
    const int32_t* unext;  // [B][T][K]
    NgramTab ng;  // n_nodes == 0: no model
    int ng_start, ng_eos;
    float ng_weight, len_bonus;
    float* ngram_sum;     // [B][nbest]
    int32_t* ngram_node;  // [B][nbest]
};
template <bool BIAS, bool NGRAM>
struct BeamArgsOf {
    typedef BeamArgs type;
};
template <>
struct BeamArgsOf<true, false> {
    typedef BeamArgsBias type;
};
template <bool BIAS>
struct BeamArgsOf<BIAS, true> {
    typedef BeamArgsNgram type;
};

// a candidate's bias step in one word: the node reached (< 2^24 = AVSR_BIAS_MAX_NODES), +1 taken, unc of the parent's node taken back
constexpr int CB_BIAS_PLUS = 1 << 24, CB_BIAS_BACK = 1 << 25, CB_BIAS_NODE = (1 << 24) - 1;

// ---- one workgroup per utterance walks its frames
template <bool BIAS, bool NGRAM>
__global__ __launch_bounds__(CB_NT_MAX) void ctc_beam_kernel(typename BeamArgsOf<BIAS, NGRAM>::type a) {
    // the beam, double buffered: hash of the prefix and of its parent prefix, last token, length, node id, pb, pnb, total
    __shared__ uint64_t s_h[2][CB_MAXW], s_hp[2][CB_MAXW];
    __shared__ int s_last[2][CB_MAXW], s_len[2][CB_MAXW], s_node[2][CB_MAXW];
    __shared__ float s_pb[2][CB_MAXW], s_pnb[2][CB_MAXW], s_tot[2][CB_MAXW];
    __shared__ int s_n[2];
    __shared__ int s_par[CB_MAXW], s_kpos[CB_MAXW];  // of the current beam: slot of the parent prefix / token slot of the last token, -1: none
    __shared__ int s_kill[CB_MAXW * CB_MAXK];        // extension (j, k) was merged into a staying entry at frame (value - 1)
    __shared__ __attribute__((aligned(16))) float s_cv[CB_MAXC + 4];  // candidate totals
    __shared__ float s_cpnb[CB_MAXC], s_cpb[CB_MAXW];
    __shared__ int s_rank[CB_MAXC];  // candidates that beat candidate s, summed over the parts of the block
    __shared__ int s_live;           // candidates of the frame that carry mass
    // per frame of a chunk: K tokens, K values, the blank's value (BIAS: and the K root children of the tokens; NGRAM: and the root's
    // K log-probabilities and K next nodes on the tokens)
    constexpr int ROWS = 2 + (BIAS ? 1 : 0) + (NGRAM ? 2 : 0);
    __shared__ int s_stage[2][CB_FCH * (ROWS * CB_MAXK + 1)];
    // BIAS: trie node and sum of gains of the beam's entries, unc of the current entries' nodes, the candidates' packed steps
    __shared__ int s_bn[2][BIAS ? CB_MAXW : 1], s_bg[2][BIAS ? CB_MAXW : 1], s_bu[BIAS ? CB_MAXW : 1];
    __shared__ int s_cb[BIAS ? CB_MAXW * CB_MAXK : 1];
    // NGRAM: the model's node and running sum G (f32 bits) of the beam's entries
    __shared__ int s_nn[2][NGRAM ? CB_MAXW : 1], s_ng[2][NGRAM ? CB_MAXW : 1];
    // ... and, where 64 KB of LDS hold them (without a bias list), G and node of every extension, so that the winners of P4 need not
    // walk again (with a list they do: the same loads a moment later)
    constexpr bool KEEP = NGRAM && !BIAS;
    __shared__ int s_cr[KEEP ? CB_MAXW * CB_MAXK : 1], s_cx[KEEP ? CB_MAXW * CB_MAXK : 1];
    constexpr int STG = NGRAM ? (BIAS ? CB_STG_BIAS_NGRAM : CB_STG_NGRAM) : (BIAS ? CB_STG_BIAS : CB_STG);
    static_assert(CB_FCH * (ROWS * CB_MAXK + 1) <= STG * CB_NT_MIN, "the staged chunk must fit the registers that hold it");
    const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
    const int W = a.W, K = a.K, T = a.T, K1 = K + 1, RW = ROWS * K + 1;
    // P3: the block is `parts` groups of Cw threads (whole waves); group g compares every candidate with its share of the others
    const int Cw = (W * K1 + 63) / 64 * 64, parts = Cw <= NT ? NT / Cw : 1;
    const int part = parts > 1 ? tid / Cw : 0, s_first = parts > 1 ? tid - part * Cw : tid, s_step = parts > 1 ? Cw : NT;
    int Tb = (int)(a.in_lens[b] < (int64_t)T ? a.in_lens[b] : (int64_t)T);
    if (Tb < 0) Tb = 0;
    const int32_t* g_tok = a.tok + (long)b * T * K;
    const float* g_val = a.val + (long)b * T * K;
    const float* g_blk = a.blk + (long)b * T;
    int32_t* g_cnt = a.cnt + (long)b * T;
    int32_t* g_node = a.node + (long)b * ((long)T * W + 1) * 2;
    int32_t* g_beam = a.beam + (long)b * T * W * 4;
    const int32_t* g_root = nullptr;
    if constexpr (BIAS) g_root = a.rootc + (long)b * T * K;
    const float* g_ulogp = nullptr;
    const int32_t* g_unext = nullptr;
    if constexpr (NGRAM) {
        g_ulogp = a.ulogp + (long)b * T * K;
        g_unext = a.unext + (long)b * T * K;
    }

    if (tid == 0) {
        if constexpr (NGRAM) {
            s_nn[0][0] = a.ng_start;
            s_ng[0][0] = __builtin_bit_cast(int, 0.f);
        }
        if constexpr (BIAS) {
            s_bn[0][0] = 0;
            s_bg[0][0] = 0;
        }
        s_h[0][0] = CB_ROOT_HASH;
        s_hp[0][0] = CB_NO_PARENT;
        s_last[0][0] = -1;
        s_len[0][0] = 0;
        s_node[0][0] = 0;
        s_pb[0][0] = 0.f;
        s_pnb[0][0] = neg_inf();
        s_tot[0][0] = 0.f;
        s_n[0] = 1;
        s_par[0] = -1;
        s_kpos[0] = -1;
        g_node[0] = -1;
        g_node[1] = -1;
    }
    for (int i = tid; i < CB_MAXW * CB_MAXK; i += NT) s_kill[i] = 0;

    // staging of the token rows: chunk c = frames [c * FCH, (c + 1) * FCH), word w = f * RW + x of a chunk
    int pre[STG];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int q = 0; q < STG; q++) {
            const int w = tid + q * NT, f = w / RW, x = w - f * RW, t = chunk * CB_FCH + f;
            int v = 0;
            if (f < CB_FCH && t < Tb) {
                if (x < K) v = g_tok[(long)t * K + x];
                else if (x < 2 * K) v = __builtin_bit_cast(int, g_val[(long)t * K + x - K]);
                else if ((!BIAS && !NGRAM) || x == 2 * K) v = __builtin_bit_cast(int, g_blk[t]);
                else if (BIAS && (!NGRAM || x < 3 * K + 1)) v = g_root[(long)t * K + x - 2 * K - 1];
                else if constexpr (NGRAM) {
                    const int y = x - (BIAS ? 3 : 2) * K - 1;
                    v = y < K ? __builtin_bit_cast(int, g_ulogp[(long)t * K + y]) : g_unext[(long)t * K + y - K];
                }
            }
            pre[q] = v;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int q = 0; q < STG; q++) {
            const int w = tid + q * NT;
            if (w < CB_FCH * RW) s_stage[buf][w] = pre[q];
        }
    };
    fetch(0);
    stash(0);
    fetch(1);
    __syncthreads();

    int cur = 0;
    for (int t = 0; t < Tb; t++) {
        const int chunk = t / CB_FCH, f = t - chunk * CB_FCH;
        const int* st_tok = &s_stage[chunk & 1][f * RW];
        const float* st_val = reinterpret_cast<const float*>(st_tok + K);
        const float lpb = st_val[K];
        const int* st_root = st_tok + 2 * K + 1;  // (BIAS only)
        const int* st_unext = st_tok + (BIAS ? 3 : 2) * K + 1 + K;  // (NGRAM only: the root's next nodes, after its log-probabilities)
        const float* st_ulogp = reinterpret_cast<const float*>(st_unext - K);
        const int n = s_n[cur], nxt = cur ^ 1, N = n * K1, stamp = t + 1;
        // ---- P1: parent slots, token slots of the last tokens, merged extensions
        for (int p = tid; p < n * n; p += NT) {
            const int i = p / n, j = p - i * n;
            if (s_hp[cur][i] == s_h[cur][j] && s_len[cur][i] == s_len[cur][j] + 1) {
                s_par[i] = j;
                const int c = s_last[cur][i];
                for (int k = 0; k < K; k++)
                    if (st_tok[k] == c) s_kill[j * K + k] = stamp;
            }
        }
        for (int p = tid; p < n * K; p += NT) {
            const int i = p / K, k = p - i * K;
            if (st_tok[k] == s_last[cur][i]) s_kpos[i] = k;
        }
        if (tid == 0) {
            s_n[nxt] = 0;
            s_live = 0;
        }
        if constexpr (BIAS)  // what a mismatch at entry i takes back: the one table read of an entry that does not stand at the root
            for (int i = tid; i < n; i += NT) s_bu[i] = s_bn[cur][i] ? a.bias.unc[s_bn[cur][i]] : 0;
        lds_barrier();
        // ---- P2: the candidates.  Slot i * (K + 1) + k: entry i extended by token k (k < K) or staying (k == K)
        int alive = 0;
        for (int s = tid; s < N; s += NT) {
            const int i = s / K1, k = s - i * K1;
            float v;
            if (k == K) {
                const float pbn = s_tot[cur][i] + lpb;
                const int kp = s_kpos[i], j = s_par[i];
                float pnbn = neg_inf();
                if (kp >= 0) {
                    const float lpc = st_val[kp];
                    pnbn = s_pnb[cur][i] + lpc;
                    if (j >= 0) pnbn = lse2(pnbn, (s_last[cur][j] != s_last[cur][i] ? s_tot[cur][j] : s_pb[cur][j]) + lpc);
                }
                s_cpb[i] = pbn;
                s_cpnb[s] = pnbn;
                v = lse2(pbn, pnbn);
            } else {
                v = (st_tok[k] != s_last[cur][i] ? s_tot[cur][i] : s_pb[cur][i]) + st_val[k];
                if (s_kill[i * K + k] == stamp) v = neg_inf();
                s_cpnb[s] = v;
            }
            if constexpr (BIAS) {  // the ranking key: total + weight * (sum of gains of the candidate's prefix); a dead candidate stays dead
                int g = s_bg[cur][i];
                if (k < K && v > neg_inf()) {
                    const int sn = s_bn[cur][i], rc = st_root[k];
                    int step = -1;
                    if (sn != 0) {  // rule 1 below the root: binary search among the node's own edges
                        const int e = tab_edge(a.bias.first, a.bias.tok, sn, st_tok[k]);
                        if (e >= 0) step = a.bias.child[e] | CB_BIAS_PLUS;
                    }
                    if (step < 0) step = (sn != 0 ? CB_BIAS_BACK : 0) | (rc >= 0 ? rc | CB_BIAS_PLUS : 0);  // rule 2 (at the root: rule 1)
                    s_cb[i * K + k] = step;
                    g += ((step & CB_BIAS_PLUS) != 0) - ((step & CB_BIAS_BACK) ? s_bu[i] : 0);
                }
                v += a.b_weight * (float)g;
            }
            if constexpr (NGRAM) {  // ... + weight * G(prefix) + len_bonus * len(prefix); only an extension below the root reads the tables
                float G = __builtin_bit_cast(float, s_ng[cur][i]);
                int len = s_len[cur][i];
                if (k < K && v > neg_inf()) {
                    int nx;
                    G += ng_lookup(a.ng, s_nn[cur][i], st_tok[k], st_ulogp[k], st_unext[k], nx);
                    len += 1;
                    if constexpr (KEEP) {
                        s_cr[i * K + k] = __builtin_bit_cast(int, G);
                        s_cx[i * K + k] = nx;
                    }
                }
                v += a.ng_weight * G + a.len_bonus * (float)len;
            }
            s_cv[s] = v;
            s_rank[s] = 0;
            alive += v > neg_inf();
        }
        alive = (int)wave_sum((float)alive);
        if ((tid & 63) == 0 && alive) atomicAdd(&s_live, alive);
        if (tid < 4) s_cv[N + tid] = neg_inf();  // (the rank loop reads whole groups of 4)
        lds_barrier();
        // ---- P3: rank r < W = slot r of the next beam.  Part g of the block counts, for every candidate, those of ITS quarter (or
        // so) of the candidates that beat it; the counts meet in LDS
        if (part < parts) {
            const int groups = (N + 3) / 4, per = (groups + parts - 1) / parts;
            const int u0 = 4 * part * per, u1 = min(4 * groups, u0 + 4 * per);
            for (int s = s_first; s < N; s += s_step) {
                const float v = s_cv[s];
                if (!(v > neg_inf())) continue;
                // the 64 candidates of a wave are consecutive: groups of 4 wholly below all of them beat one on a tie, groups wholly
                // above never do, and only the <= 17 groups in between need the index compare
                const int s_lo = s - (tid & 63);
                const int ua = max(u0, min(u1, s_lo / 4 * 4)), uc = min(u1, max(ua, (s_lo + 63) / 4 * 4 + 4));
                int rank = 0;
#pragma unroll 4
                for (int u = u0; u < ua; u += 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&s_cv[u]);
#pragma unroll
                    for (int e = 0; e < 4; e++) rank += q[e] >= v;
                }
                for (int u = ua; u < uc; u += 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&s_cv[u]);
#pragma unroll
                    for (int e = 0; e < 4; e++) rank += (q[e] > v) | ((q[e] == v) & (u + e < s));
                }
#pragma unroll 4
                for (int u = uc; u < u1; u += 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(&s_cv[u]);
#pragma unroll
                    for (int e = 0; e < 4; e++) rank += q[e] > v;
                }
                if (rank) atomicAdd(&s_rank[s], rank);
            }
        }
        lds_barrier();
        for (int s = tid; s < N; s += NT) {
            float v = s_cv[s];
            if (!(v > neg_inf())) continue;
            const int rank = s_rank[s], live = s_live;
            if (rank >= W) continue;
            const int i = s / K1, k = s - i * K1, r = rank;
            if constexpr (BIAS || NGRAM) v = k == K ? lse2(s_cpb[i], s_cpnb[s]) : s_cpnb[s];  // the pure CTC total, as P2 computed it
            if constexpr (NGRAM) {  // the model's state of the prefix: a winner that is an extension reads what P2 kept, or walks once more
                int nn = s_nn[cur][i];
                float G = __builtin_bit_cast(float, s_ng[cur][i]);
                if (k < K && KEEP) {
                    G = __builtin_bit_cast(float, s_cr[i * K + k]);
                    nn = s_cx[i * K + k];
                } else if (k < K) G += ng_lookup(a.ng, nn, st_tok[k], st_ulogp[k], st_unext[k], nn);
                s_nn[nxt][r] = nn;
                s_ng[nxt][r] = __builtin_bit_cast(int, G);
            }
            if constexpr (BIAS) {  // the bias state of the prefix
                const int step = k == K ? 0 : s_cb[i * K + k];
                s_bn[nxt][r] = k == K ? s_bn[cur][i] : step & CB_BIAS_NODE;
                s_bg[nxt][r] = s_bg[cur][i] + ((step & CB_BIAS_PLUS) != 0) - ((step & CB_BIAS_BACK) ? s_bu[i] : 0);
            }
            int node = s_node[cur][i], len = s_len[cur][i];
            float pbn = neg_inf();
            if (k == K) {
                s_h[nxt][r] = s_h[cur][i];
                s_hp[nxt][r] = s_hp[cur][i];
                s_last[nxt][r] = s_last[cur][i];
                pbn = s_cpb[i];
            } else {
                const int c = st_tok[k];
                s_h[nxt][r] = cb_hash(s_h[cur][i], c);
                s_hp[nxt][r] = s_h[cur][i];
                s_last[nxt][r] = c;
                const int parent = node;
                node = 1 + t * W + r;
                len += 1;
                g_node[2 * (long)node] = parent;
                g_node[2 * (long)node + 1] = c;
            }
            const float pnbn = s_cpnb[s];
            s_len[nxt][r] = len;
            s_node[nxt][r] = node;
            s_pb[nxt][r] = pbn;
            s_pnb[nxt][r] = pnbn;
            s_tot[nxt][r] = v;
            i32x4 rec;
            rec[0] = node;
            rec[1] = len;
            rec[2] = __builtin_bit_cast(int, pbn);
            rec[3] = __builtin_bit_cast(int, pnbn);
            *reinterpret_cast<i32x4*>(&g_beam[((long)t * W + r) * 4]) = rec;
            const int n_new = live < W ? live : W;
            if (r == n_new - 1) {
                s_n[nxt] = n_new;
                g_cnt[t] = n_new;
            }
        }
        for (int i = tid; i < W; i += NT) {  // (slots of the next beam; P1 of the next frame fills them in)
            s_par[i] = -1;
            s_kpos[i] = -1;
        }
        if (f == CB_FCH - 1) {  // the next chunk's rows go from the registers to the other stage buffer; the one after is requested
            stash((chunk + 1) & 1);
            fetch(chunk + 2);
        }
        lds_barrier();
        if (tid == 0 && s_n[nxt] == 0) g_cnt[t] = 0;  // (every candidate -inf: the search of this utterance is over)
        cur = nxt;
    }

    // ---- the n-best: the beam is sorted; token sequences come back from the node records
#ifndef AVSR_EMU
    __threadfence();
#endif
    __syncthreads();
    const int n = s_n[cur], nbest = a.nbest;
    const int nv = n < nbest ? n : nbest;
    if (tid == 0) a.n_valid[b] = nv;
    int32_t* out = a.tokens + (long)b * nbest * T;
    for (int r = 0; r < nbest; r++) {
        const int len = r < nv ? s_len[cur][r] : 0;
        for (int i = len + tid; i < T; i += NT) out[(long)r * T + i] = -1;
    }
    if (tid < nbest) {
        const int r = tid;
        const bool ok = r < nv;
        a.lens[(long)b * nbest + r] = ok ? s_len[cur][r] : 0;
        a.score[(long)b * nbest + r] = ok ? s_tot[cur][r] : neg_inf();
        a.pb[(long)b * nbest + r] = ok ? s_pb[cur][r] : neg_inf();
        a.pnb[(long)b * nbest + r] = ok ? s_pnb[cur][r] : neg_inf();
        if constexpr (BIAS) {  // <eos> is never in the trie: it takes the uncommitted part back
            a.bias_sum[(long)b * nbest + r] = ok ? (float)(s_bg[cur][r] - a.bias.unc[s_bn[cur][r]]) : 0.f;
            a.bias_node[(long)b * nbest + r] = ok ? s_bn[cur][r] : 0;
        }
        if constexpr (NGRAM) {  // a finished hypothesis also pays for its </s>
            float G = 0.f;
            if (ok) {
                const int e = tab_root_edge(a.ng.first, a.ng.tok, a.ng_eos);
                int nx;
                G = __builtin_bit_cast(float, s_ng[cur][r]);
                G += ng_lookup(a.ng, s_nn[cur][r], a.ng_eos, e >= 0 ? a.ng.logp[e] : 0.f, e >= 0 ? a.ng.next[e] : 0, nx);
            }
            a.ngram_sum[(long)b * nbest + r] = G;
            a.ngram_node[(long)b * nbest + r] = ok ? s_nn[cur][r] : 0;
        }
        if (ok) {
            int node = s_node[cur][r];
            for (int i = s_len[cur][r] - 1; i >= 0 && node > 0; i--) {
                out[(long)r * T + i] = g_node[2 * (long)node + 1];
                node = g_node[2 * (long)node];
            }
        }
    }
}

// ---- avsr_ctc_score: lpg[q, t, s] = lp[q / N, t, ext[q, s]] for the sequences q = b * N + i
__global__ __launch_bounds__(256) void ctc_score_gather_kernel(const float* __restrict__ lp, long ld, const int* __restrict__ ext,
                                                               const int* __restrict__ lens, const int64_t* __restrict__ in_lens,
                                                               float* __restrict__ lpg, int N, int Tlen, int Smax) {
    const long qt = blockIdx.x;
    const int q = (int)(qt / Tlen), t = (int)(qt % Tlen), b = q / N;
    if ((int64_t)t >= in_lens[b]) return;
    const int S = 2 * lens[q] + 1;
    const float* x = lp + ((long)b * Tlen + t) * ld;
    for (int s = threadIdx.x; s < S; s += 256) lpg[qt * Smax + s] = x[ext[(long)q * Smax + s]];
}

AVSR_DEV float score_add3(float a, float b, float c) {
    const float m = fmaxf(a, fmaxf(b, c));
    if (m <= LOG_ZERO) return LOG_ZERO;
    return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// the alpha recursion of loss.hip (one wave per sequence, SPL contiguous states per lane, CTC_PF frames of emissions in flight),
// forward only and without the stored trellis
template <int SPL>
__global__ __launch_bounds__(64) void ctc_score_alpha_kernel(const float* __restrict__ lpg, const int* __restrict__ ext,
                                                             const int* __restrict__ lens, const int64_t* __restrict__ in_lens,
                                                             float* __restrict__ loglik, int N, int Tlen, int Smax) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const int L = lens[q], S = 2 * L + 1;
    int Tb = (int)(in_lens[q / N] < (int64_t)Tlen ? in_lens[q / N] : (int64_t)Tlen);
    const int* e = ext + (long)q * Smax;
    const float* lp = lpg + (long)q * Tlen * Smax;
    const int blank = e[0], s0 = lane * SPL;
    if (Tb <= 0) {
        if (lane == 0) loglik[q] = L == 0 ? 0.f : -INFINITY;
        return;
    }
    bool skip[SPL], valid[SPL];
    float cur[SPL];
#pragma unroll
    for (int i = 0; i < SPL; i++) {
        const int s = s0 + i;
        valid[i] = s < S;
        skip[i] = valid[i] && (s >= 2) && (e[s] != blank) && (e[s] != e[s - 2]);
        cur[i] = (valid[i] && s < 2) ? lp[s] : LOG_ZERO;
    }
    float pre[CTC_PF][SPL];
    auto fetch = [&](int t, float (&dst)[SPL]) {
#pragma unroll
        for (int i = 0; i < SPL; i++) dst[i] = (t < Tb && valid[i]) ? lp[(long)t * Smax + s0 + i] : 0.f;
    };
#pragma unroll
    for (int j = 0; j < CTC_PF; j++) fetch(1 + j, pre[j]);
    for (int t0 = 1; t0 < Tb; t0 += CTC_PF) {
#pragma unroll
        for (int j = 0; j < CTC_PF; j++) {
            const int t = t0 + j;
            if (t >= Tb) break;
            const float n1 = wave_up1(cur[SPL - 1], LOG_ZERO);
            const float n2 = SPL >= 2 ? wave_up1(cur[SPL >= 2 ? SPL - 2 : 0], LOG_ZERO) : wave_up1(n1, LOG_ZERO);
            float nxt[SPL];
#pragma unroll
            for (int i = 0; i < SPL; i++) {
                const float a1 = i >= 1 ? cur[i >= 1 ? i - 1 : 0] : n1;
                const float a2 = i >= 2 ? cur[i >= 2 ? i - 2 : 0] : (i == 1 ? n1 : n2);
                const float v = score_add3(cur[i], a1, skip[i] ? a2 : LOG_ZERO) + pre[j][i];
                nxt[i] = (valid[i] && v > LOG_ZERO) ? v : LOG_ZERO;
            }
#pragma unroll
            for (int i = 0; i < SPL; i++) cur[i] = nxt[i];
            fetch(t + CTC_PF, pre[j]);
        }
    }
    float m1 = LOG_ZERO, m2 = LOG_ZERO;  // alpha(S - 1), alpha(S - 2)
#pragma unroll
    for (int i = 0; i < SPL; i++) {
        const int s = s0 + i;
        if (valid[i] && s == S - 1) m1 = cur[i];
        if (valid[i] && s == S - 2) m2 = cur[i];
    }
    m1 = wave_max(m1);
    m2 = wave_max(m2);
    const float tot = score_add3(m1, m2, LOG_ZERO);
    if (lane == 0) loglik[q] = tot <= LOG_ZERO * 0.5f ? -INFINITY : tot;
}

int64_t align16(int64_t x) { return (x + 15) / 16 * 16; }

// the outputs of a scorer that took no part (no bias list / no n-gram model): sums and nodes of the n-best are zeros
__global__ __launch_bounds__(256) void ctc_zero_outputs_kernel(float* __restrict__ sum, int32_t* __restrict__ node, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        sum[i] = 0.f;
        node[i] = 0;
    }
}

}  // namespace

// Workspace layout (header): tok | val | blk | cnt | node | (to 16 bytes) beam
static int64_t beam_rec_offset(int B, int T, int W, int K) {
    const int64_t words = (int64_t)B * T * K * 2 + (int64_t)B * T * 2 + (int64_t)B * ((int64_t)T * W + 1) * 2;
    return align16(words * 4);
}

extern "C" int64_t avsr_ctc_beam_workspace_bytes(int B, int T, int W, int K) {
    if (B <= 0 || T <= 0 || W <= 0 || K <= 0) return 16;
    return beam_rec_offset(B, T, W, K) + (int64_t)B * T * W * 16;
}

// The search.  `a` arrives with the scorers' part filled in by the entry point (tables, weights, outputs) and everything else zero:
// a.bias.n_nodes != 0 is the search with a bias list, whose root-child table follows the plain workspace layout; a.ng.n_nodes != 0
// the search with an n-gram model, whose root (logp, next) tables follow either.
static int beam_search(const float* lp, int64_t ld, const int64_t* in_lens, int blank, int W, int K, int nbest, int32_t* tokens,
                       int32_t* lens, float* score, float* pb, float* pnb, int32_t* n_valid, void* workspace, int B, int T, int V,
                       hipStream_t stream, BeamArgsNgram a) {
    AVSR_REQUIRE(W >= 2 && W <= CB_MAXW, "ctc_beam_search: beam must be 2 .. 64");
    AVSR_REQUIRE(K >= 1 && K <= CB_MAXK && K <= V - 1, "ctc_beam_search: token budget must be 1 .. min(32, V - 1)");
    AVSR_REQUIRE(nbest >= 1 && nbest <= W, "ctc_beam_search: nbest must be 1 .. beam");
    AVSR_REQUIRE(blank >= 0 && blank < V && V <= ld, "ctc_beam_search: blank id outside the vocabulary");
    AVSR_REQUIRE(V <= 16000, "ctc_beam_search: at most 16000 tokens (the row's keys live in LDS)");
    AVSR_REQUIRE(T >= 1 && (int64_t)T * W < (1 << 30), "ctc_beam_search: 1 .. 2^30 / beam frames");
    AVSR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ctc_beam_search: workspace must be 16-byte aligned");
    if (B <= 0) return 0;
    const bool biased = a.bias.n_nodes != 0, ngram = a.ng.n_nodes != 0;
    int32_t* tok = reinterpret_cast<int32_t*>(workspace);
    float* val = reinterpret_cast<float*>(tok + (int64_t)B * T * K);
    float* blk = val + (int64_t)B * T * K;
    a.tok = tok;
    a.val = val;
    a.blk = blk;
    a.cnt = reinterpret_cast<int32_t*>(blk + (int64_t)B * T);
    a.node = a.cnt + (int64_t)B * T;
    a.beam = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + beam_rec_offset(B, T, W, K));
    a.in_lens = in_lens;
    a.tokens = tokens;
    a.lens = lens;
    a.n_valid = n_valid;
    a.score = score;
    a.pb = pb;
    a.pnb = pnb;
    a.W = W;
    a.K = K;
    a.nbest = nbest;
    a.T = T;
    AVSR_LAUNCH(ctc_topk_kernel, dim3((unsigned)((int64_t)B * T)), dim3(TK_NT), (size_t)V * sizeof(unsigned), stream, lp, (long)ld,
                in_lens, blank, K, T, V, tok, val, blk);
    // four threads per candidate where a block can hold them (the rank loop of P3 is the longest stretch of a frame), whole waves
    int nt = (W * (K + 1) + 63) / 64 * 64 * 4;
    nt = nt < CB_NT_MIN ? CB_NT_MIN : (nt > CB_NT_MAX ? CB_NT_MAX : nt);
    const long total = (long)B * T * K;
    if (ngram) {
        char* after = reinterpret_cast<char*>(workspace) +
                      (biased ? avsr_ctc_beam_bias_workspace_bytes(B, T, W, K) : avsr_ctc_beam_workspace_bytes(B, T, W, K));
        float* ulogp = reinterpret_cast<float*>(after);
        int32_t* unext = reinterpret_cast<int32_t*>(after + align16(total * 4));
        a.ulogp = ulogp;
        a.unext = unext;
        AVSR_LAUNCH(ctc_ngram_root_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tok, in_lens, a.ng, K, T, total, ulogp,
                    unext);
    }
    if (!biased) {
        if (!ngram) AVSR_LAUNCH((ctc_beam_kernel<false, false>), dim3(B), dim3(nt), 0, stream, static_cast<const BeamArgs&>(a));
        else AVSR_LAUNCH((ctc_beam_kernel<false, true>), dim3(B), dim3(nt), 0, stream, a);
    } else {
        int32_t* rootc = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + avsr_ctc_beam_workspace_bytes(B, T, W, K));
        a.rootc = rootc;
        AVSR_LAUNCH(ctc_root_child_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, tok, in_lens, a.bias, K, T, total, rootc);
        if (!ngram) AVSR_LAUNCH((ctc_beam_kernel<true, false>), dim3(B), dim3(nt), 0, stream, static_cast<const BeamArgsBias&>(a));
        else AVSR_LAUNCH((ctc_beam_kernel<true, true>), dim3(B), dim3(nt), 0, stream, a);
    }
    AVSR_CHECK_LAUNCH("ctc_beam_search");
    return 0;
}

static int zero_outputs(const char* where, float* sum, int32_t* node, int n, hipStream_t stream) {
    AVSR_LAUNCH(ctc_zero_outputs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sum, node, n);
    AVSR_CHECK_LAUNCH(where);
    return 0;
}

extern "C" int avsr_ctc_beam_search(const float* lp, int64_t ld, const int64_t* in_lens, int blank, int W, int K, int nbest,
                                    int32_t* tokens, int32_t* lens, float* score, float* pb, float* pnb, int32_t* n_valid,
                                    void* workspace, int B, int T, int V, hipStream_t stream) {
    return beam_search(lp, ld, in_lens, blank, W, K, nbest, tokens, lens, score, pb, pnb, n_valid, workspace, B, T, V, stream, BeamArgsNgram{});
}

extern "C" int64_t avsr_ctc_beam_bias_workspace_bytes(int B, int T, int W, int K) {
    if (B <= 0 || T <= 0 || W <= 0 || K <= 0) return 16;
    return avsr_ctc_beam_workspace_bytes(B, T, W, K) + align16((int64_t)B * T * K * 4);
}

extern "C" int avsr_ctc_beam_search_bias(const float* lp, int64_t ld, const int64_t* in_lens, int blank, int W, int K, int nbest,
                                         const int32_t* first, const int32_t* tok, const int32_t* child, const int32_t* unc, int n_nodes,
                                         int n_edges, float weight, int32_t* tokens, int32_t* lens, float* score, float* pb, float* pnb,
                                         int32_t* n_valid, float* bias_sum, int32_t* bias_node, void* workspace, int B, int T, int V,
                                         hipStream_t stream) {
    AVSR_REQUIRE_NONE("ctc_beam_search_bias", bias_sizes_refusal(n_nodes, n_edges));
    AVSR_REQUIRE_NONE("ctc_beam_search_bias", weight_refusal(weight, WEIGHT_UP_TO_1E30));
    const bool biased = tables_given(n_nodes, n_edges);
    BeamArgsNgram a{};
    if (biased) {
        a.bias = BiasTab{first, tok, child, unc, n_nodes};
        a.b_weight = weight;
        a.bias_sum = bias_sum;
        a.bias_node = bias_node;
    }
    const int rc = beam_search(lp, ld, in_lens, blank, W, K, nbest, tokens, lens, score, pb, pnb, n_valid, workspace, B, T, V, stream, a);
    if (rc != 0 || B <= 0 || biased) return rc;
    return zero_outputs("ctc_beam_search_bias", bias_sum, bias_node, B * nbest, stream);  // no list: the plain search, nothing was boosted
}

extern "C" int64_t avsr_ctc_beam_ngram_workspace_bytes(int B, int T, int W, int K, int with_bias) {
    if (B <= 0 || T <= 0 || W <= 0 || K <= 0) return 16;
    return (with_bias ? avsr_ctc_beam_bias_workspace_bytes(B, T, W, K) : avsr_ctc_beam_workspace_bytes(B, T, W, K)) +
           2 * align16((int64_t)B * T * K * 4);
}

extern "C" int avsr_ctc_beam_search_ngram(const float* lp, int64_t ld, const int64_t* in_lens, int blank, int W, int K, int nbest,
                                          const int32_t* first, const int32_t* tok, const int32_t* child, const int32_t* unc, int b_nodes,
                                          int b_edges, float bias_weight, const int32_t* n_first, const int32_t* n_tok, const float* n_logp,
                                          const int32_t* n_next, const float* n_bow, const int32_t* n_back, int n_nodes, int n_edges,
                                          int start_node, int eos, float ngram_weight, float len_bonus, int32_t* tokens, int32_t* lens,
                                          float* score, float* pb, float* pnb, int32_t* n_valid, float* bias_sum, int32_t* bias_node,
                                          float* ngram_sum, int32_t* ngram_node, void* workspace, int B, int T, int V, hipStream_t stream) {
    AVSR_REQUIRE_NONE("ctc_beam_search_ngram", bias_sizes_refusal(b_nodes, b_edges));
    AVSR_REQUIRE(!weight_refusal(bias_weight, WEIGHT_UP_TO_1E30), "ctc_beam_search_ngram: the bias weight must be finite");
    AVSR_REQUIRE_NONE("ctc_beam_search_ngram", ngram_sizes_refusal(n_nodes, n_edges));
    AVSR_REQUIRE(!weight_refusal(ngram_weight, WEIGHT_UP_TO_1E30) && !weight_refusal(len_bonus, WEIGHT_UP_TO_1E30),
                 "ctc_beam_search_ngram: the n-gram weight and the length bonus must be finite");
    if (!tables_given(n_nodes, n_edges)) {  // no model: the biased or the plain search, and nothing was scored
        const int rc = avsr_ctc_beam_search_bias(lp, ld, in_lens, blank, W, K, nbest, first, tok, child, unc, b_nodes, b_edges, bias_weight,
                                                 tokens, lens, score, pb, pnb, n_valid, bias_sum, bias_node, workspace, B, T, V, stream);
        if (rc != 0 || B <= 0) return rc;
        return zero_outputs("ctc_beam_search_ngram", ngram_sum, ngram_node, B * nbest, stream);
    }
    AVSR_REQUIRE(start_node >= 0 && start_node < n_nodes, "ctc_beam_search_ngram: start node outside the model");
    AVSR_REQUIRE(blank == 0, "ctc_beam_search_ngram: the model's tables take the blank to be id 0");
    AVSR_REQUIRE(eos == V - 1, "ctc_beam_search_ngram: </s> must be the last id of the vocabulary");
    const bool biased = tables_given(b_nodes, b_edges);
    BeamArgsNgram a{};
    a.ng = NgramTab{n_first, n_tok, n_logp, n_next, n_bow, n_back, n_nodes};
    AVSR_REQUIRE_NONE("ctc_beam_search_ngram", missing_table(a.ng));
    a.ng_start = start_node;
    a.ng_eos = eos;
    a.ng_weight = ngram_weight;
    a.len_bonus = len_bonus;
    a.ngram_sum = ngram_sum;
    a.ngram_node = ngram_node;
    if (biased) {
        a.bias = BiasTab{first, tok, child, unc, b_nodes};
        a.b_weight = bias_weight;
        a.bias_sum = bias_sum;
        a.bias_node = bias_node;
    }
    const int rc = beam_search(lp, ld, in_lens, blank, W, K, nbest, tokens, lens, score, pb, pnb, n_valid, workspace, B, T, V, stream, a);
    if (rc != 0 || B <= 0 || biased) return rc;
    return zero_outputs("ctc_beam_search_ngram", bias_sum, bias_node, B * nbest, stream);
}

// Workspace layout: lpg[B*N*T*Smax] f32 | ext[B*N*Smax] i32 | lens[B*N] i32
extern "C" int64_t avsr_ctc_score_workspace_bytes(int B, int N, int T, int Lmax) {
    if (B <= 0 || N <= 0 || T <= 0 || Lmax < 0) return 16;
    const int64_t Smax = 2 * (int64_t)Lmax + 1, Q = (int64_t)B * N;
    return align16((Q * T * Smax + Q * Smax + Q) * 4);
}

extern "C" int avsr_ctc_score(const float* lp, int64_t ld, const int64_t* labels, int N, int Lmax, int ignore_id,
                              const int64_t* in_lens, int blank, float* loglik, void* workspace, int B, int T, int V,
                              hipStream_t stream) {
    AVSR_REQUIRE(Lmax >= 0 && Lmax <= 255, "ctc_score: at most 255 labels per sequence");
    AVSR_REQUIRE(blank >= 0 && blank < V && V <= ld, "ctc_score: blank id outside the vocabulary");
    AVSR_REQUIRE(ignore_id < 0 || ignore_id >= V, "ctc_score: ignore_id must not be a token id");
    AVSR_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3) == 0, "ctc_score: workspace must be 4-byte aligned");
    AVSR_REQUIRE(T >= 0 && (int64_t)B * N * (T > 0 ? T : 1) < (1ll << 31), "ctc_score: too many (sequence, frame) pairs");
    if (B <= 0 || N <= 0) return 0;
    const int Smax = 2 * Lmax + 1, Q = B * N;
    float* lpg = reinterpret_cast<float*>(workspace);
    int* ext = reinterpret_cast<int*>(lpg + (int64_t)Q * T * Smax);
    int* lens = ext + (int64_t)Q * Smax;
    AVSR_LAUNCH(ctc_prepare_kernel, dim3(Q), dim3(64), 0, stream, labels, Lmax, ignore_id, blank, ext, Smax, lens);
    if (T > 0)
        AVSR_LAUNCH(ctc_score_gather_kernel, dim3((unsigned)((int64_t)Q * T)), dim3(256), 0, stream, lp, (long)ld, ext, lens, in_lens, lpg, N,
                    T, Smax);
    const int spl = (Smax + 63) / 64;
#define AVSR_CTC_SC(NS) AVSR_LAUNCH(ctc_score_alpha_kernel<NS>, dim3(Q), dim3(64), 0, stream, lpg, ext, lens, in_lens, loglik, N, T, Smax)
    if (spl <= 1) AVSR_CTC_SC(1);
    else if (spl == 2) AVSR_CTC_SC(2);
    else if (spl == 3) AVSR_CTC_SC(3);
    else if (spl == 4) AVSR_CTC_SC(4);
    else if (spl <= 6) AVSR_CTC_SC(6);
    else AVSR_CTC_SC(8);
#undef AVSR_CTC_SC
    AVSR_CHECK_LAUNCH("ctc_score");
    return 0;
}
