// search_tables.h -- the two table formats that the scorers of both searches read, the one-call hybrid beam search (decode.hip) and
// the CTC prefix beam search of two-pass decoding (ctc_beam.hip): the CSR trie of contextual biasing and the back-off n-gram tables,
// their device lookups, and the host-side checks of the entry points that take them.  The tables are device memory owned by the
// caller (bias.py / ngram.py: device_tables); they are not validated.
#pragma once
#include <math.h>

#include "prims.h"
#include "avsr_hip.h"

namespace {

// Contextual biasing (auto_avsr_amd/bias.py: ContextBiasScorer): a trie of phrases in CSR form -- node s owns the edges
// [first[s], first[s + 1]) with tokens tok[] ascending and targets child[] (an end node without children already replaced by the
// root 0), unc[s] = edges from s up to its nearest end ancestor-or-self (or the root).  A hypothesis carries one node.
struct BiasTab {
    const int32_t *first, *tok, *child, *unc;
    int n_nodes;  // 0: no list
};

// Back-off n-gram language model (auto_avsr_amd/ngram.py: NgramScorer), a PARTIAL scorer: a node is a context (an n-gram of order
// < N, node 0 the empty one) that owns the edges [first[s], first[s + 1]) with tokens tok[] ascending, log-probabilities logp[] and
// next[] = the node of the extended context; bow[s] is the node's back-off weight, back[s] the node of its longest proper suffix
// that is a node.  A hypothesis carries one node.
struct NgramTab {
    const int32_t *first, *tok;
    const float* logp;
    const int32_t* next;
    const float* bow;
    const int32_t* back;
    int n_nodes;  // 0: no model
};

// edge of node s on token v, -1 if there is none (tok[] ascending within a node).  A plain binary search: one workgroup's scattered
// loads are bounded by the number of load instructions rather than by their latency -- a search that narrows by 8 with 7 probes in
// flight, and level headers requested a level ahead, measured 12 % slower on the first pass of two-pass decoding than this one.
AVSR_DEV int tab_edge(const int32_t* first, const int32_t* tok, int s, int v) {
    int lo = first[s], hi = first[s + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1, x = tok[mid];
        if (x == v) return mid;
        if (x < v) lo = mid + 1;
        else hi = mid;
    }
    return -1;
}
// the ordered-root shortcut: the root of NgramScorer's tables holds the tokens 1 .. V - 1 in order, so its edge on v is looked for at
// its place -- one load instead of a 13-step search at the node every back-off chain ends at.  -1: not there, the search decides.
AVSR_DEV int tab_root_hit(const int32_t* first, const int32_t* tok, int v) {
    const int lo = first[0], hi = first[1], e = lo + v - 1;
    return e >= lo && e < hi && tok[e] == v ? e : -1;
}
// the root's edge on v of such a table
AVSR_DEV int tab_root_edge(const int32_t* first, const int32_t* tok, int v) {
    const int e = tab_root_hit(first, tok, v);
    return e >= 0 ? e : tab_edge(first, tok, 0, v);
}

// gain of extending a hypothesis at node s by token v and the node it reaches: +1 along an edge; otherwise the uncommitted reward of
// s is taken back and v alone is retried from the root (no failure links)
AVSR_DEV int bias_gain(const BiasTab& t, int s, int v, int& next) {
    int e = tab_edge(t.first, t.tok, s, v);
    if (e >= 0) {
        next = t.child[e];
        return 1;
    }
    int g = -t.unc[s];
    next = 0;
    if (s != 0 && (e = tab_edge(t.first, t.tok, 0, v)) >= 0) {
        next = t.child[e];
        g += 1;
    }
    return g;
}

// edge of any node of the n-gram tables: tab_root_edge at the root, tab_edge elsewhere, written so that a kernel holds the search once
AVSR_DEV int ngram_edge(const NgramTab& t, int s, int v) {
    const int e = s == 0 ? tab_root_hit(t.first, t.tok, v) : -1;
    return e >= 0 ? e : tab_edge(t.first, t.tok, s, v);
}

// log p(v | node s) by ARPA back-off and the node reached: walk s, back[s], ... to the first node with an edge e on v; logp[e] if
// that is s itself, else r = bow[s0]; r += bow[s1]; ...; r += logp[e] (f32, this order: ngram.py's host lookup adds alike; additions
// only, there is nothing to contract).  The walk is cut after AVSR_NGRAM_MAX_ORDER hops (tables are not validated: a cycle in back[]
// must not hang a search).  Two walks and not one: the prefix search resolves the root's edge on a frame's tokens off its chain, so
// its walk takes that edge from the caller and never reads the root -- a root branch inside ctc_beam_kernel's walk costs it time --
// and the two differ on broken tables (a root without the edge) and in what the hop limit leaves.
//
// ngram_logp, the hybrid search's: resolves the root itself.  The blank scores 0 and keeps the node; a token without an edge at the
// root gets the back-offs alone.
AVSR_DEV float ngram_logp(const NgramTab& t, int s, int v, int blank, int& next) {
    next = s;
    if (v == blank) return 0.f;
    int e = ngram_edge(t, s, v);
    if (e >= 0) {
        next = t.next[e];
        return t.logp[e];
    }
    float r = t.bow[s];
    for (int hop = 0; s != 0 && hop < AVSR_NGRAM_MAX_ORDER; hop++) {
        s = t.back[s];
        e = ngram_edge(t, s, v);
        if (e >= 0) {
            next = t.next[e];
            return r + t.logp[e];
        }
        r += t.bow[s];
    }
    next = 0;
    return r;
}
// ng_lookup, the prefix search's: (ur, un) is the root's (logp, next) on v, resolved by the caller, so the levels below the root are
// all this reads.
AVSR_DEV float ng_lookup(const NgramTab& t, int s, int v, float ur, int un, int& next) {
    float r = 0.f;
    bool fresh = true;
    for (int hop = 0; s != 0 && hop < AVSR_NGRAM_MAX_ORDER; hop++) {
        const int e = tab_edge(t.first, t.tok, s, v);
        if (e >= 0) {
            next = t.next[e];
            return fresh ? t.logp[e] : r + t.logp[e];
        }
        r = fresh ? t.bow[s] : r + t.bow[s];
        fresh = false;
        s = t.back[s];
    }
    if (s != 0) {
        next = 0;
        return r;
    }
    next = un;
    return fresh ? ur : r + ur;
}

// ---- host side: what every entry point that takes the tables checks.  A check returns the refusal or NULL; AVSR_REQUIRE_NONE puts
// the entry point's own name in front of it.
#define AVSR_REQUIRE_NONE(where, refusal)      \
    do {                                       \
        const char* r__ = (refusal);           \
        if (r__ != nullptr) {                  \
            avsr_set_error2(where, r__);       \
            return 1;                          \
        }                                      \
    } while (0)

inline const char* bias_sizes_refusal(int n_nodes, int n_edges) {
    return n_nodes >= 0 && n_nodes <= AVSR_BIAS_MAX_NODES && n_edges >= 0 && n_edges <= AVSR_BIAS_MAX_EDGES
               ? nullptr
               : "too many nodes or edges (AVSR_BIAS_MAX_NODES / AVSR_BIAS_MAX_EDGES)";
}
inline const char* ngram_sizes_refusal(int n_nodes, int n_edges) {
    return n_nodes >= 0 && n_nodes <= AVSR_NGRAM_MAX_NODES && n_edges >= 0 && n_edges <= AVSR_NGRAM_MAX_EDGES
               ? nullptr
               : "too many nodes or edges (AVSR_NGRAM_MAX_NODES / AVSR_NGRAM_MAX_EDGES)";
}
// a list / a model is there when it has nodes and edges (sizes that passed the check above)
inline bool tables_given(int n_nodes, int n_edges) { return n_nodes > 0 && n_edges > 0; }
inline const char* missing_table(const BiasTab& t) { return t.first && t.tok && t.child && t.unc ? nullptr : "missing table"; }
inline const char* missing_table(const NgramTab& t) {
    return t.first && t.tok && t.logp && t.next && t.bow && t.back ? nullptr : "missing table";
}
// What an entry point asks of a weight.  The rules differ and stay as each entry point had them: the session's bias weight only has
// to be a number (inf passes), its n-gram weight has to be finite, and the weights of the prefix search at most 1e30 in magnitude.
enum WeightRule { WEIGHT_NOT_NAN, WEIGHT_FINITE, WEIGHT_UP_TO_1E30 };
inline const char* weight_refusal(float w, WeightRule rule) {
    switch (rule) {
        case WEIGHT_NOT_NAN: return w == w ? nullptr : "the weight is not a number";
        case WEIGHT_FINITE: return w - w == 0.f ? nullptr : "the weight is not a finite number";
        default: return w == w && fabsf(w) <= 1e30f ? nullptr : "the weight must be finite";
    }
}

}  // namespace
