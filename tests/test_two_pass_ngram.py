"""Back-off n-gram model in two-pass decoding: the CTC prefix beam search with the model inside (csrc/ctc_beam.hip:
avsr_ctc_beam_search_ngram), the n-gram term of the rescoring objective (auto_avsr_amd/two_pass.py) and the plumbing through
TwoPassDecoder.set_ngram / ModelModule.  Kernels through the emulator (CPU suite) or on the MI355X (-m gpu).

The search is checked FRAME BY FRAME from the kernel's own previous beam, as tests/test_two_pass_bias.py checks the biased search (its
helpers are restated here): a float64 step gives every candidate's pure CTC masses, `NgramScorer.walk(prefix)` on the host gives the
model's running f32 sum G, and the kernel's next beam must be a valid top-W by

    key = total + bias_weight * gains + ngram_weight * G + len_bonus * len(prefix)

in key order, carrying the unchanged pure CTC masses.

Tolerance of a mass or a key s: 1e-5 * max(1, |s|) + 1e-5.  A frame update is at most W + 2 f32 operations per value (W <= 64); each of
the three key terms adds a multiplication and an addition, and G itself is the same f32 sum on both sides (no error): (66 + 6) * 6e-8 =
4.3e-6 relative to the largest term, which the shapes here (T <= 40 frames, |log p| <= 9 per token, weights <= 2) keep within 2 |s|."""
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
from synth import synth_state_dict  # noqa: E402

from auto_avsr_amd import functional as AF  # noqa: E402
from auto_avsr_amd import nets, ops  # noqa: E402
from auto_avsr_amd.bias import ContextBiasScorer  # noqa: E402
from auto_avsr_amd.decoding import CTCPrefixScorer, LengthBonus  # noqa: E402
from auto_avsr_amd.ngram import NgramScorer  # noqa: E402
from auto_avsr_amd.two_pass import TwoPassDecoder  # noqa: E402

NEG = float("-inf")
WEIGHT, BONUS, BIAS_WEIGHT = 0.5, 0.7, 2.0
GOLD = torch.load(os.path.join(HERE, "golden", "golden_ngram_v1.pt"), weights_only=False)["cases"]


def _tol(s):
    return 1e-5 * max(1.0, abs(s)) + 1e-5


def _lae(a, b):
    return float(np.logaddexp(a, b))


def _step64(beam, toks, row, blank):
    """One frame of the prefix beam search in float64 (tests/test_ctc_beam.py): beam [(prefix, pb, pnb)], the frame's non-blank
    tokens, its log-posterior row -> {prefix: [pb', pnb']} of every candidate (contributions to the same prefix merged)."""
    cand = {}

    def add(p, which, v):
        e = cand.setdefault(p, [NEG, NEG])
        e[which] = _lae(e[which], v)

    for p, pb, pnb in beam:
        s, e = _lae(pb, pnb), (p[-1] if p else None)
        add(p, 0, s + row[blank])
        for c in toks:
            if c != e:
                add(p + (c,), 1, s + row[c])
            else:
                add(p, 1, pnb + row[c])
                if pb > NEG:
                    add(p + (c,), 1, pb + row[c])
    return cand


def _logits(B, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * 3
    x[..., 0] += 6
    return x


def _search(dev, lp, in_lens, W, K, nbest=None, **kw):
    return AF.ctc_beam_search(lp, torch.as_tensor(in_lens), blank=0, beam=W, topk=K, nbest=nbest, **kw)


def _final(res, b=0):
    return [tuple(res["tokens"][b, r, : int(res["lens"][b, r])].cpu().tolist()) for r in range(int(res["n_valid"][b]))]


def _phrases(res, in_lens, V, seed):
    """tests/test_two_pass_bias.py's list that bites, built from the UNBIASED run of utterance 0: runs of 2 to 4 tokens through
    consecutive frames' token sets, pieces of the winner, a proper prefix of another phrase, a single-token phrase, and one that shares
    only its first token with the winner."""
    rng = np.random.RandomState(seed)
    ok = lambda c: 1 <= c <= V - 2  # noqa: E731
    Tb = min(int(in_lens[0]), res["topk_tok"].shape[1])
    sets = [[c for c in row if ok(c)] for row in res["topk_tok"][0, :Tb].cpu().tolist()]
    win = [c for c in res["tokens"][0, 0, : int(res["lens"][0, 0])].cpu().tolist()]
    out = []
    for _ in range(12):
        n = int(rng.randint(2, 5))
        t0 = int(rng.randint(0, max(1, Tb - n)))
        ph = [sets[t][int(rng.randint(len(sets[t])))] for t in range(t0, min(Tb, t0 + n)) if sets[t]]
        ph = [c for i, c in enumerate(ph) if i == 0 or c != ph[i - 1]]
        if len(ph) >= 2:
            out.append(ph)
    pieces = [win[i:i + n] for i, n in ((0, 2), (1, 3), (max(0, len(win) - 2), 2))]
    out += [p for p in pieces if len(p) >= 2 and all(ok(c) for c in p)]
    long = next(p for p in out if len(p) >= 3)
    out.append(long[:2])
    out.append([sets[Tb // 2][-1]])
    first = next(c for c in win if ok(c))
    other = next(c for s in sets for c in s if c not in win[:3] and c != first)
    out.append([first, other, other % (V - 2) + 1])
    return out


# ---------------------------------------------------------------------------------------------------- the models
def _random_model(V, n_bi, n_tri, seed, pool=None):
    """The construction of tests/test_ngram_lm.py::_random_model: a unigram for every token, random bigrams (also after <s> = V) and
    trigrams that extend them, back-offs where a context has entries.  pool: the tokens the bigrams and trigrams are drawn from (default
    all) -- with 5049 tokens, n-grams over tokens that no frame offers would never be looked up."""
    rng = random.Random(seed)
    P = {(t,): -rng.uniform(2.0, 9.0) for t in range(1, V)}
    P[(V,)] = -99.0
    B = {(V,): -rng.uniform(0.1, 1.0)}
    pool = sorted(pool) if pool is not None else list(range(1, V))
    heads = [t for t in pool if t != V - 1] + [V]
    bis = set()
    while len(bis) < n_bi:
        bis.add((rng.choice(heads), rng.choice(pool)))
    bis = sorted(bis)
    for g in bis:
        P[g] = -rng.uniform(0.1, 6.0)
    inner = [g for g in bis if g[1] != V - 1]
    tris = set()
    while len(tris) < n_tri:
        tris.add(rng.choice(inner) + (rng.choice(pool),))
    for g in tris:
        P[g] = -rng.uniform(0.1, 5.0)
        B[g[:2]] = -rng.uniform(0.05, 2.0)
    for g in bis:
        B.setdefault((g[0],), -rng.uniform(0.05, 2.0))
    return P, B


def _model(kind, V, plain, in_lens, seed):
    """tri: the random 3-gram over the tokens the frames offer; uni: unigrams only (one node, no <s> context); skip: a 4-gram whose
    chains run through consecutive frames' token sets, with <unk> fill-ins, so that `back` of a 3-token context skips the bigram level
    (and, where the last token has no unigram of its own, goes straight to the root)."""
    sets = []
    for b, Tb in enumerate(in_lens):
        sets += [[c for c in row] for row in plain["topk_tok"][b, : min(Tb, plain["topk_tok"].shape[1])].cpu().tolist()]
    pool = sorted({c for row in sets for c in row} | {V - 1})
    rng = random.Random(seed)
    if kind == "uni":
        sc = NgramScorer(V, {(t,): -rng.uniform(0.5, 9.0) for t in range(1, V)}, {}, order=1)
        assert sc.n_nodes == 1 and sc.start_node == 0
        return sc
    if kind == "tri":
        n = len(pool)
        P, B = _random_model(V, min(n * n // 3, 12 * n), min(n * n * n // 9, 24 * n), seed, pool)
        sc = NgramScorer(V, P, B, order=3)
        assert sc.start_node != 0
        return sc
    P = {(V - 1,): -3.0, (V,): -99.0}
    B = {(V,): -0.3}
    for t in pool[::2]:  # every other offered token has a unigram of its own (and is a context); the rest take <unk>'s
        P[(t,)] = -rng.uniform(2.0, 8.0)
    for _ in range(30 * len(sets)):
        n = rng.randint(2, 4)
        t0 = rng.randrange(0, max(1, len(sets) - n))
        g = tuple(rng.choice(sets[t]) for t in range(t0, min(len(sets), t0 + n)))
        if any(x == y for x, y in zip(g, g[1:])) or V - 1 in g[:-1]:
            continue
        for i in range(1, len(g) + 1):
            P.setdefault(g[:i], -rng.uniform(0.1, 4.0))
            if i < len(g):
                B.setdefault(g[:i], -rng.uniform(0.05, 1.5))
    sc = NgramScorer(V, P, B, order=4, unk_logp=-6.5)
    order = [len(c) for c in sc.contexts]
    assert any(order[s] >= 2 and order[int(sc.back[s])] < order[s] - 1 for s in range(sc.n_nodes))  # `back` skips a level
    return sc


class _Walker:
    """sc.walk(prefix) of every prefix, each token looked up once: (G f32, node), the same f32 additions in the same order."""

    def __init__(self, sc):
        self.sc = sc
        self.memo = {(): (np.float32(0.0), sc.start_node)}
        self.edge = {}
        for s in range(sc.n_nodes):
            for e in range(int(sc.first[s]), int(sc.first[s + 1])):
                self.edge[(s, int(sc.tok[e]))] = e

    def __call__(self, p):
        got = self.memo.get(p)
        if got is None:
            g, s = self(p[:-1])
            r, nx = self.sc.step(s, p[-1])
            got = self.memo[p] = (np.float32(g + r), nx)
        return got

    def backoffs(self, p):
        """How the lookup of p's last token went: (back-off steps, hit at the entry's own node, that node is not the root)."""
        s = self(p[:-1])[1]
        own, n = s, 0
        while (s, p[-1]) not in self.edge:
            s, n = int(self.sc.back[s]), n + 1
        return n, n == 0, own != 0


def _check_frames(lp, res, in_lens, W, K, sc, weight, bonus, bias=None, bias_weight=0.0):
    """-> (worst error as a fraction of the tolerance, counts): every frame of every utterance is a valid step by the key from the
    kernel's own previous beam.  counts, all from the host reference: lookups of live extensions that backed off at least once / at
    least twice / hit at the entry's own non-root node; frames whose top-W by the key differs from the plain top-W of the same
    candidates."""
    trace, topk = ops.ctc_beam_trace(res, in_lens)
    walk = _Walker(sc)
    worst, n_back1, n_back2, n_own, n_frames = 0.0, 0, 0, 0, 0
    for b, Tb in enumerate(in_lens):
        rows = lp[b].cpu().double().numpy()
        Tb = min(Tb, rows.shape[0])
        assert len(trace[b]) == Tb
        beam = [((), 0.0, NEG)]
        for t in range(Tb):
            row, toks = rows[t], topk[b][t]
            assert len(set(toks)) == K and 0 not in toks and all(0 < c < len(row) for c in toks)
            rest = np.delete(row, [0] + toks)
            assert rest.size == 0 or rest.max() <= min(row[c] for c in toks), (b, t)
            cand = _step64(beam, toks, row, 0)
            tot = {p: _lae(v[0], v[1]) for p, v in cand.items()}
            live = [p for p in cand if tot[p] > NEG]

            def key_of(p, s):
                k = s
                if bias is not None:
                    k += bias_weight * bias.walk(p)[0]
                return k + weight * float(walk(p)[0]) + bonus * len(p)

            key = {p: key_of(p, tot[p]) for p in live}
            before = {p for p, _, _ in beam}
            for p in live:
                if p not in before:  # an extension: its last token was looked up at its parent's node
                    nb, hit, below = walk.backoffs(p)
                    n_back1 += nb >= 1
                    n_back2 += nb >= 2
                    n_own += hit and below
            new = trace[b][t]
            assert len(new) == min(W, len(live)), (b, t, len(new), len(live))
            kept = [p for p, _, _ in new]
            assert len(set(kept)) == len(kept), (b, t)
            by_key = set(sorted(live, key=lambda p: -key[p])[:W])
            by_tot = set(sorted(live, key=lambda p: -tot[p])[:W])
            n_frames += by_key != by_tot
            for p, pb, pnb in new:
                assert p in cand and tot[p] > NEG, (b, t, p)
                s = tot[p]  # the stored masses are pure CTC
                err = abs(_lae(pb, pnb) - s)
                worst = max(worst, err / _tol(s))
                assert err <= _tol(s), (b, t, p, pb, pnb, cand[p])
                for got, ref in ((pb, cand[p][0]), (pnb, cand[p][1])):
                    if ref >= s - 20:
                        assert abs(got - ref) <= _tol(s), (b, t, p, got, ref)
            # the beam is in the order of the key, and no candidate outside exceeds its smallest key by more than the tolerance
            ks = [key_of(p, _lae(pb, pnb)) for p, pb, pnb in new]
            for x, y in zip(ks, ks[1:]):
                assert y <= x + _tol(x), (b, t, ks)
            floor = min(key[p] for p in kept)
            out = [key[p] for p in live if p not in set(kept)]
            if out:
                worst = max(worst, (max(out) - floor) / _tol(floor))
                assert max(out) <= floor + _tol(floor), (b, t, max(out), floor)
            beam = new
    return worst, (n_back1, n_back2, n_own, n_frames)


def _needed(kind, counts):
    """The conditions the host reference has to meet for a model of this kind, so that the test cannot pass vacuously."""
    n_back1, n_back2, n_own, n_frames = counts
    if kind == "uni":  # one node: nothing to back off from
        return n_frames > 0
    return n_back1 > 0 and n_back2 > 0 and n_own > 0 and n_frames > 0


# ---------------------------------------------------------------------------------------------------- test 1: frame by frame
@pytest.mark.parametrize("kind", ["tri", "uni", "skip"])
@pytest.mark.parametrize("T,V,W,K", [(12, 20, 4, 4), (40, 64, 8, 8), (37, 5049, 16, 16), (8, 40, 64, 32)])
def test_every_frame_is_a_valid_step_by_the_ngram_key_from_the_kernels_own_beam(dev, T, V, W, K, kind):
    lp = AF.log_softmax(_logits(1, T, V, T + V).to(dev))
    if V == 5049:
        assert lp.stride(-2) == 5056
    plain = _search(dev, lp, [T], W, K)
    sc = _model(kind, V, plain, [T], T + V)
    for bonus in (0.0, BONUS):
        res = _search(dev, lp, [T], W, K, ngram=sc, ngram_weight=WEIGHT, len_bonus=bonus)
        worst, counts = _check_frames(lp, res, [T], W, K, sc, WEIGHT, bonus)
        print(f"T={T} V={V} W={W} K={K} {kind} len_bonus={bonus}: worst error {worst:.3f} of the tolerance; lookups that backed off once / "
              f"twice / hit at their own non-root node, frames whose kept set differs from the plain one: {counts}; {sc.n_nodes} nodes, "
              f"{sc.n_edges} edges")
        assert _needed(kind, counts), counts
        assert _final(res) != _final(plain)  # the model changed what the search keeps


# ---------------------------------------------------------------------------------------------------- test 2: a batch
BATCH = dict(in_lens=[23, 1, 0, 9], T=23, V=31, W=8, K=6)
_SHARED = {}


def _batch(dev, nbest=None):
    """The batch of tests 2 to 4 with its plain run and its model (computed once per device and n-best, never changed)."""
    k = (str(dev), nbest)
    if k not in _SHARED:
        c = BATCH
        lp = AF.log_softmax(_logits(4, c["T"], c["V"], 11).to(dev))
        plain = _search(dev, lp, c["in_lens"], c["W"], c["K"], nbest=nbest)
        _SHARED[k] = (lp, plain, _model("tri", c["V"], plain, c["in_lens"], 5))
    return _SHARED[k]


def test_every_frame_of_a_batch_that_shares_a_model(dev):
    in_lens, T, V, W, K = (BATCH[k] for k in ("in_lens", "T", "V", "W", "K"))
    lp, plain, sc = _batch(dev)
    res = _search(dev, lp, in_lens, W, K, ngram=sc, ngram_weight=WEIGHT, len_bonus=BONUS)
    worst, counts = _check_frames(lp, res, in_lens, W, K, sc, WEIGHT, BONUS)
    print(f"B=4 in_lens={in_lens}: worst error {worst:.3f} of the tolerance; counts {counts}")
    assert _needed("tri", counts), counts
    assert _final(res, 0) != _final(plain, 0)
    # the empty utterance: one empty hypothesis, which still pays for its </s>
    assert int(res["n_valid"][2]) == 1 and int(res["lens"][2, 0]) == 0 and float(res["score"][2, 0]) == 0.0
    assert float(res["ngram_sum"][2, 0]) == float(sc.walk([V - 1])[0]) != 0.0


# ---------------------------------------------------------------------------------------------------- test 3: the n-best
def test_nbest_carries_the_models_sum_and_the_pure_ctc_masses(dev):
    in_lens, T, V, W, K, N = tuple(BATCH[k] for k in ("in_lens", "T", "V", "W", "K")) + (5,)
    lp, plain, sc = _batch(dev, N)
    res = _search(dev, lp, in_lens, W, K, nbest=N, ngram=sc, ngram_weight=WEIGHT, len_bonus=BONUS)
    trace, _ = ops.ctc_beam_trace(res, in_lens)
    toks, lens, nv = res["tokens"].cpu(), res["lens"].cpu(), res["n_valid"].cpu()
    score, pb, pnb = res["score"].cpu(), res["pb"].cpu(), res["pnb"].cpu()
    nsum, nnode = res["ngram_sum"].cpu(), res["ngram_node"].cpu()
    assert nsum.shape == nnode.shape == (4, N) and nsum.dtype == torch.float32 and nnode.dtype == torch.int32
    assert float(res["bias_sum"].abs().max()) == 0.0 and int(res["bias_node"].abs().max()) == 0
    below = 0
    for b, Tb in enumerate(in_lens):
        last = trace[b][-1] if Tb > 0 else [((), 0.0, NEG)]  # (already in the key's order)
        assert int(nv[b]) == min(N, len(last))
        for r in range(N):
            if r >= int(nv[b]):
                assert int(lens[b, r]) == 0 and float(score[b, r]) == NEG and (toks[b, r] == -1).all()
                assert float(pb[b, r]) == NEG and float(pnb[b, r]) == NEG
                assert float(nsum[b, r]) == 0.0 and int(nnode[b, r]) == 0
                continue
            p, rpb, rpnb = last[r]
            assert tuple(toks[b, r, : int(lens[b, r])].tolist()) == p and int(lens[b, r]) == len(p)
            assert (toks[b, r, len(p):] == -1).all()
            assert float(pb[b, r]) == rpb and float(pnb[b, r]) == rpnb
            assert abs(float(score[b, r]) - _lae(rpb, rpnb)) <= _tol(float(score[b, r]))  # the pure total
            assert float(nsum[b, r]) == float(sc.walk(list(p) + [V - 1])[0]), (b, r, p)  # bit for bit
            assert int(nnode[b, r]) == sc.walk(p)[1], (b, r, p)
            below += int(nnode[b, r]) != 0
    assert below > 0


# ---------------------------------------------------------------------------------------------------- test 4: with a bias list
def test_every_frame_with_a_bias_list_and_a_model(dev):
    in_lens, T, V, W, K = (BATCH[k] for k in ("in_lens", "T", "V", "W", "K"))
    lp, plain, sc = _batch(dev)
    bias = ContextBiasScorer(_phrases(plain, in_lens, V, 5), V)
    biased = _search(dev, lp, in_lens, W, K, bias=bias, bias_weight=BIAS_WEIGHT)
    res = _search(dev, lp, in_lens, W, K, bias=bias, bias_weight=BIAS_WEIGHT, ngram=sc, ngram_weight=WEIGHT, len_bonus=BONUS)
    worst, counts = _check_frames(lp, res, in_lens, W, K, sc, WEIGHT, BONUS, bias=bias, bias_weight=BIAS_WEIGHT)
    print(f"bias + n-gram: worst error {worst:.3f} of the tolerance; counts {counts}")
    assert _needed("tri", counts), counts
    assert _final(res, 0) != _final(biased, 0) and _final(res, 0) != _final(plain, 0)
    gains = 0
    for b in range(4):
        for r, p in enumerate(_final(res, b)):
            g, node = bias.walk(p)
            assert float(res["bias_sum"][b, r]) == g + bias.step(node, V - 1)[0] and int(res["bias_node"][b, r]) == node
            assert float(res["ngram_sum"][b, r]) == float(sc.walk(list(p) + [V - 1])[0])
            gains += g != 0
    assert gains > 0


# ---------------------------------------------------------------------------------------------------- test 5: a constructed flip
def _host_search(rows, W, K, key):
    """The whole search in float64: top-W by key(prefix, total) per frame -> the last beam, best first."""
    beam = [((), 0.0, NEG)]
    for row in rows:
        toks = sorted(range(1, len(row)), key=lambda c: (-row[c], c))[:K]
        cand = _step64(beam, toks, row, 0)
        live = [(p, v) for p, v in cand.items() if _lae(v[0], v[1]) > NEG]
        live.sort(key=lambda pv: -key(pv[0], _lae(pv[1][0], pv[1][1])))
        beam = [(p, v[0], v[1]) for p, v in live[:W]]
    return [p for p, _, _ in beam]


def test_the_model_flips_a_close_call(dev):
    """V = 6: blank, a = 1, b = 2, c = 3, d = 4, </s>.  Two frames say `a`, then two say `c` a little louder than `b`: the plain search ends
    on (a, c) with (a, b) close behind; a bigram that makes `b` after `a` far likelier than `c` turns them round."""
    a, b, c = 1, 2, 3
    p = torch.full((6, 6), 0.02)
    for t, row in enumerate(([0.1, 0.8], [0.5, 0.4], [0.9, 0.02], [0.1, 0.0, 0.38, 0.44], [0.5, 0.0, 0.2, 0.22], [0.9, 0.02])):
        for i, v in enumerate(row):
            if v:
                p[t, i] = v
    lp = AF.log_softmax(torch.log(p / p.sum(1, keepdim=True)).unsqueeze(0).to(dev))
    P = {(t,): -3.0 for t in range(1, 6)}
    P.update({(6,): -99.0, (a, b): -0.05, (a, c): -5.0})
    sc = NgramScorer(6, P, {(6,): -0.1, (a,): -0.2}, order=2)
    rows = lp[0].cpu().double().numpy()
    W, K, w = 4, 3, 1.0
    walk = _Walker(sc)
    ref_plain = _host_search(rows, W, K, lambda y, s: s)
    ref_fused = _host_search(rows, W, K, lambda y, s: s + w * float(walk(y)[0]))
    assert ref_plain[0] == (a, c) and ref_plain[1] == (a, b) and ref_fused[0] == (a, b)
    plain = _search(dev, lp, [6], W, K)
    fused = _search(dev, lp, [6], W, K, ngram=sc, ngram_weight=w)
    assert _final(plain)[:2] == [(a, c), (a, b)] and _final(fused)[0] == (a, b)
    assert float(fused["ngram_sum"][0, 0]) == float(sc.walk([a, b, 5])[0])


# ---------------------------------------------------------------------------------------------------- test 6: without a model
HISTORY = ("topk_tok", "topk_val", "blank_val", "count")
OUTS = ("tokens", "lens", "score", "pb", "pnb", "n_valid", "bias_sum", "bias_node", "ngram_sum", "ngram_node")


def _same_run(a, b, in_lens, keys):
    """The outputs bit for bit, and the history where the search writes it: the per-frame rows t < in_lens[b], and the beam of every
    frame as ctc_beam_trace rebuilds it from the node and slot records (masses compared as the floats they are)."""
    for k in keys:
        x, y = a[k].cpu(), b[k].cpu()
        if k in HISTORY:
            for i, Tb in enumerate(in_lens):
                assert torch.equal(x[i, :Tb], y[i, :Tb]), k
        else:
            assert torch.equal(x, y), k
    assert ops.ctc_beam_trace(a, in_lens) == ops.ctc_beam_trace(b, in_lens)


def test_no_model_is_the_search_it_was(dev):
    in_lens, T, V, W, K = [17, 5], 17, 29, 6, 5
    lp = AF.log_softmax(_logits(2, T, V, 2).to(dev))
    plain = _search(dev, lp, in_lens, W, K)
    assert float(plain["ngram_sum"].abs().max()) == 0.0 and int(plain["ngram_node"].abs().max()) == 0
    sc = _model("tri", V, plain, in_lens, 3)
    sizes = [ops.call("avsr_ctc_beam_workspace_bytes", 2, T, W, K), ops.call("avsr_ctc_beam_bias_workspace_bytes", 2, T, W, K)]
    assert sizes[1] == sizes[0] + (2 * T * K * 4 + 15) // 16 * 16
    off = (dict(ngram=None, ngram_weight=WEIGHT), dict(ngram=None, ngram_weight=0.0), dict(ngram=sc, ngram_weight=0.0))
    for kw in off:
        res = _search(dev, lp, in_lens, W, K, **kw)
        assert res["topk_tok"].untyped_storage().nbytes() == sizes[0]  # the plain workspace
        _same_run(res, plain, in_lens, OUTS + HISTORY)
    bias = ContextBiasScorer(_phrases(plain, in_lens, V, 1), V)
    biased = _search(dev, lp, in_lens, W, K, bias=bias, bias_weight=BIAS_WEIGHT)
    assert _final(biased) != _final(plain)
    for kw in off:
        res = _search(dev, lp, in_lens, W, K, bias=bias, bias_weight=BIAS_WEIGHT, **kw)
        assert res["topk_tok"].untyped_storage().nbytes() == sizes[1]
        _same_run(res, biased, in_lens, OUTS + HISTORY)
    assert [ops.call("avsr_ctc_beam_workspace_bytes", 2, T, W, K), ops.call("avsr_ctc_beam_bias_workspace_bytes", 2, T, W, K)] == sizes
    table = (2 * T * K * 4 + 15) // 16 * 16
    assert ops.call("avsr_ctc_beam_ngram_workspace_bytes", 2, T, W, K, 0) == sizes[0] + 2 * table
    assert ops.call("avsr_ctc_beam_ngram_workspace_bytes", 2, T, W, K, 1) == sizes[1] + 2 * table
    # the entry point itself without a model (n_nodes == 0): the biased or the plain search, the new outputs zero-filled
    for with_bias, want in ((False, plain), (True, biased)):
        got = _raw(lp, in_lens, W, K, V, sc, bias if with_bias else None, n_nodes=0)
        for k, v in got.items():
            assert torch.equal(v.cpu(), want[k].cpu()), (with_bias, k)


def _raw(lp, in_lens, W, K, V, sc, bias=None, **over):
    """avsr_ctc_beam_search_ngram called directly; `over` replaces scalar arguments by name."""
    dev = lp.device
    B, T = lp.shape[0], lp.shape[1]
    a = dict(blank=0, b_nodes=bias.n_nodes if bias else 0, b_edges=bias.n_edges if bias else 0, bias_weight=BIAS_WEIGHT if bias else 0.0,
             n_nodes=sc.n_nodes, n_edges=sc.n_edges, start_node=int(sc.start_node), eos=V - 1, ngram_weight=WEIGHT, len_bonus=0.0)
    assert set(over) <= set(a)
    a.update(over)
    ws = torch.zeros(ops.call("avsr_ctc_beam_ngram_workspace_bytes", B, T, W, K, int(bias is not None)) // 4, dtype=torch.int32, device=dev)
    tokens = torch.zeros(B, W, T, dtype=torch.int32, device=dev)
    lens, n_valid = torch.zeros(B, W, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    score, pb, pnb, bsum, nsum = (torch.zeros(B, W, dtype=torch.float32, device=dev) for _ in range(5))
    bnode, nnode = (torch.zeros(B, W, dtype=torch.int32, device=dev) for _ in range(2))
    btabs = bias.device_tables(dev) if bias else (None,) * 4
    il = torch.as_tensor(in_lens, dtype=torch.int64, device=dev)
    ops.call("avsr_ctc_beam_search_ngram", ops._ptr(lp), lp.stride(-2), ops._ptr(il), a["blank"], W, K, W, *[ops._ptr(t) for t in btabs],
             a["b_nodes"], a["b_edges"], a["bias_weight"], *[ops._ptr(t) for t in sc.device_tables(dev)], a["n_nodes"], a["n_edges"],
             a["start_node"], a["eos"], a["ngram_weight"], a["len_bonus"], ops._ptr(tokens), ops._ptr(lens), ops._ptr(score), ops._ptr(pb),
             ops._ptr(pnb), ops._ptr(n_valid), ops._ptr(bsum), ops._ptr(bnode), ops._ptr(nsum), ops._ptr(nnode), ops._ptr(ws), B, T, V,
             ops._stream(lp))
    return {"tokens": tokens, "lens": lens, "score": score, "pb": pb, "pnb": pnb, "n_valid": n_valid, "bias_sum": bsum, "bias_node": bnode,
            "ngram_sum": nsum, "ngram_node": nnode}


# ---------------------------------------------------------------------------------------------------- test 7: refusals
def test_refusals(dev):
    V = 9
    lp = AF.log_softmax(_logits(1, 4, V, 0).to(dev))
    P, B = _random_model(V, 6, 4, 0)
    sc = NgramScorer(V, P, B, order=3)
    with pytest.raises(ValueError, match="vocabulary"):
        P10, B10 = _random_model(V + 1, 6, 4, 0)
        _search(dev, lp, [4], 4, 3, ngram=NgramScorer(V + 1, P10, B10, order=3), ngram_weight=1.0)
    with pytest.raises(ValueError, match="blank"):
        AF.ctc_beam_search(lp, torch.as_tensor([4]), blank=2, beam=4, topk=3, ngram=sc, ngram_weight=1.0)
    for kw in (dict(len_bonus=0.5), dict(ngram=sc, ngram_weight=0.0, len_bonus=0.5)):
        with pytest.raises(ValueError, match="len_bonus"):
            _search(dev, lp, [4], 4, 3, **kw)
    for kw in (dict(ngram_weight=float("inf")), dict(ngram_weight=1.0, len_bonus=float("nan"))):
        with pytest.raises(ValueError, match="finite"):
            _search(dev, lp, [4], 4, 3, ngram=sc, **kw)
    ok = _raw(lp, [4], 4, 3, V, sc)
    assert int(ok["n_valid"][0]) >= 1
    for over in (dict(n_nodes=(1 << 26) + 1), dict(n_edges=(1 << 27) + 1), dict(n_nodes=-1), dict(n_edges=-1), dict(start_node=-1),
                 dict(start_node=sc.n_nodes), dict(ngram_weight=float("inf")), dict(ngram_weight=float("nan")), dict(len_bonus=float("inf")),
                 dict(len_bonus=float("nan")), dict(blank=1), dict(eos=V - 2)):
        with pytest.raises(Exception):
            _raw(lp, [4], 4, 3, V, sc, **over)


# ---------------------------------------------------------------------------------------------------- test 8: the second pass
def _models(case, dev):
    """Decoder and CTC head exactly as tests/test_ngram_lm.py builds them for the reference-made fixture."""
    odim, D = case["odim"], case["D"]
    torch.manual_seed(0)
    dec = nets.TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = nets.CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), case["seed"]))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), case["seed"] + 1))
    return dec.to(dev), ctc.to(dev)


def _enc(case, dev, T=None, seed=None):
    g = torch.Generator().manual_seed(500 + case["seed"] if seed is None else seed)
    return (torch.randn(T or case["T"], case["D"], generator=g) * 1.5).to(dev)


def _case_model(case):
    return NgramScorer(case["odim"], case["probs"], case["backoffs"], order=case["order"])


def _two_pass(case, dev, ngram="case", weight=None, beam=10, topk=10, models=None, **kw):
    dec, ctc = models or _models(case, dev)
    odim = case["odim"]
    if isinstance(ngram, str):
        ngram = _case_model(case)
    scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": None, "ngram": ngram, "length_bonus": LengthBonus(odim)}
    weights = {"decoder": 1.0 - case["ctc_weight"], "ctc": case["ctc_weight"], "lm": 0.0,
               "ngram": (case["ngram_weight"] if weight is None else weight) if ngram is not None else 0.0, "length_bonus": case["penalty"]}
    return TwoPassDecoder(scorers, weights, sos=odim - 1, eos=odim - 1, token_list=[str(i) for i in range(odim)], beam_size=beam,
                          topk=topk, **kw)


def test_rescoring_equals_the_references_stored_ngram_scores(dev):
    """The reference-made fixture of the hybrid search with an n-gram model: `rescore` of its finished hypotheses reproduces the stored
    score and per-scorer scores within the tolerances of tests/test_two_pass.py (1e-3 of the score, 2e-3 per scorer) and of
    tests/test_ngram_lm.py::_check_vs_reference for scores["ngram"] (2e-3).  Force-ended hypotheses (len(yseq) - 2 == T, <eos> not
    scored) are excluded by that rule alone, as there -- which, with the fixture's short utterances (T <= 12), leaves few."""
    checked, forced, worst, worst_ng = 0, 0, 0.0, 0.0
    AF.set_precise(True)
    try:
        for case in GOLD:
            natural = [h for h in case["hyps"] if len(h["yseq"]) - 2 < case["T"]]
            forced += len(case["hyps"]) - len(natural)
            assert all(len(h["yseq"]) - 2 == case["T"] for h in case["hyps"] if h not in natural)
            if not natural:
                continue
            tp = _two_pass(case, dev)
            got = tp.rescore(_enc(case, dev), [h["yseq"] for h in natural])
            for g, ref in zip(got, natural):
                d = g.asdict()
                assert d["yseq"] == ref["yseq"]
                err = abs(d["score"] - ref["score"]) / max(1.0, abs(ref["score"]))
                worst = max(worst, err)
                assert err < 1e-3, (case["seed"], d["score"], ref["score"])
                assert set(d["scores"]) == set(ref["scores"]) and "ngram" in ref["scores"]
                for k, v in ref["scores"].items():
                    assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), (case["seed"], k, d["scores"][k], v)
                worst_ng = max(worst_ng, abs(d["scores"]["ngram"] - ref["scores"]["ngram"]) / max(1.0, abs(ref["scores"]["ngram"])))
                assert d["scores"]["ngram"] != 0.0
                checked += 1
    finally:
        AF.set_precise(False)
    print(f"n-gram rescoring: {checked} hypotheses ({forced} force-ended ones excluded), worst relative error of the score {worst:.2e}, of the n-gram term {worst_ng:.2e}")
    assert checked > 0


# ---------------------------------------------------------------------------------------------------- test 9: the decoder
def _host_ngram(sc, yseq, eos):
    return float(sc.walk([int(t) for t in yseq][1:-1] + [eos])[0])


def _model_along(seqs, V, seed):
    """A 3-gram that likes the given sequences: flat unigrams, near-certain bigrams and trigrams along them (also from <s>)."""
    rng = random.Random(seed)
    P = {(t,): -rng.uniform(4.0, 5.0) for t in range(1, V)}
    P[(V,)] = -99.0
    B = {(V,): -0.4}
    for y in seqs:
        y = [V] + list(y) + [V - 1]
        for n in (2, 3):
            for i in range(len(y) - n + 1):
                g = tuple(y[i:i + n])
                if V in g[1:] or V - 1 in g[:-1]:
                    continue
                P.setdefault(g[:-1], -0.3)
                P.setdefault(g, -0.05 * n)
                B.setdefault(g[:-1], -0.6)
    return NgramScorer(V, P, B, order=3)


def _check_hyps(nbest, tp, plain, enc, sc):
    again = plain.rescore(enc, [h.yseq for h in nbest])
    given = tp.rescore(enc, [h.yseq for h in nbest])  # (walks the sequences on the host)
    for h, ref, g in zip(nbest, again, given):
        d, r = h.asdict(), ref.asdict()
        assert d["yseq"] == r["yseq"] and set(d["scores"]) == set(r["scores"]) | {"ngram"}
        assert d["scores"]["ngram"] == _host_ngram(sc, d["yseq"], tp.eos)  # exactly
        assert g.scores["ngram"] == d["scores"]["ngram"] and set(g.scores) == set(d["scores"])
        total = sum(tp.weights[k] * v for k, v in d["scores"].items())
        assert abs(d["score"] - total) < 1e-4 * max(1.0, abs(total)), (d["score"], total)
        assert abs(float(g.score) - d["score"]) < 1e-4 * max(1.0, abs(d["score"]))
        for k, v in r["scores"].items():
            assert abs(d["scores"][k] - v) < 1e-4 * max(1.0, abs(v)), k
            assert abs(g.scores[k] - v) < 1e-4 * max(1.0, abs(v)), k
    sc_ = [float(h.score) for h in nbest]
    assert sc_ == sorted(sc_, reverse=True)


def _dicts(many):
    return [[h.asdict() for h in nbest] for nbest in many]


def test_two_pass_decoder_with_a_model(dev):
    case = dict(next(c for c in GOLD if c["odim"] < 1000), penalty=0.5)
    odim = case["odim"]
    AF.set_precise(True)
    try:
        models = _models(case, dev)
        plain = _two_pass(case, dev, ngram=None, models=models)
        assert plain.ngram is None and "ngram" not in plain.scorers
        xs = [_enc(case, dev, T=T, seed=900 + T) for T in (23, 14)]
        base = plain.forward_many(xs)
        assert all("ngram" not in h.scores for nbest in base for h in nbest)
        # a model that likes what the model-less first pass ranks LOW, so that it reorders the n-best
        low = [[int(t) for t in hyps[-1].yseq[1:-1]] for hyps in base]
        sc = _model_along(low, odim, 1)
        tp = _two_pass(case, dev, ngram=sc, weight=0.8, models=models, len_bonus=0.5)
        assert tp.ngram is sc and tp.weights["ngram"] == 0.8 and tp.len_bonus == 0.5
        many = tp.forward_many(xs)
        assert float(tp.last_first_pass["ngram_sum"].abs().max()) > 0
        for enc, nbest in zip(xs, many):
            assert 1 <= len(nbest) <= 10
            _check_hyps(nbest, tp, plain, enc, sc)
        assert [sorted(d["yseq"] for d in nbest) for nbest in _dicts(many)] != [sorted(d["yseq"] for d in nbest) for nbest in _dicts(base)]
        # set_ngram(None, 0): the model-less results, bit for bit
        tp.set_ngram(None, 0)
        assert tp.ngram is None and "ngram" not in tp.scorers and tp.len_bonus == 0.5
        assert _dicts(tp.forward_many(xs)) == _dicts(base)
        # another model between two calls takes effect; the first one again gives the first results again
        other = _model_along([list(reversed(y)) for y in low], odim, 2)
        tp.set_ngram(other, 0.8)
        swapped = tp.forward_many(xs)
        assert tp.ngram is other and tp.len_bonus == 0.5
        assert all(h.scores["ngram"] == _host_ngram(other, h.yseq.tolist(), tp.eos) for nbest in swapped for h in nbest)
        assert [[d["scores"]["ngram"] for d in nbest] for nbest in _dicts(swapped)] != [[d["scores"]["ngram"] for d in nbest]
                                                                                         for nbest in _dicts(many)]
        tp.set_ngram(sc, 0.8, len_bonus=0.5)
        assert _dicts(tp.forward_many(xs)) == _dicts(many)
    finally:
        AF.set_precise(False)
    # the slot takes this build's scorer over the head's vocabulary, nothing else
    for bad in (object(), _model_along([[1, 2]], odim + 1, 0)):
        with pytest.raises(TypeError):
            _two_pass(case, dev, ngram=bad, weight=0.5, models=models)


# ---------------------------------------------------------------------------------------------------- test 10: the module
def _small_e2e(odim, dev):
    from auto_avsr_amd.e2e import E2E

    return E2E(odim, "video", adim=128, aheads=2, eunits=256, elayers=1, dunits=256, dlayers=1, cnn_module_kernel=7).to(dev).eval()


def _ids_arpa(tmp_path, odim, name="lm.arpa"):
    """An ARPA file over token ids (tests/test_ngram_lm.py's): unigrams for the odd ids and <unk>, a few bigrams and trigrams."""
    uni = [(-1.0, ("<s>",), -0.5), (-1.2, ("</s>",), None), (-2.0, ("<unk>",), None)]
    uni += [(-0.02 * t - 0.8, (str(t),), -0.01 * t) for t in range(1, odim - 1, 2)]
    bi = [(-0.3, ("<s>", "3"), -0.1), (-0.2, ("3", "5"), -0.2), (-0.4, ("5", "</s>"), None), (-0.5, ("7", "9"), None)]
    tri = [(-0.1, ("<s>", "3", "5"), None), (-0.2, ("3", "5", "7"), None)]
    sections = {1: uni, 2: bi, 3: tri}
    lines = ["", "\\data\\"] + [f"ngram {k}={len(v)}" for k, v in sorted(sections.items())] + [""]
    for k, rows in sorted(sections.items()):
        lines.append(f"\\{k}-grams:")
        lines += ["\t".join([repr(p), " ".join(w)] + ([repr(b)] if b is not None else [])) for p, w, b in rows]
        lines.append("")
    lines.append("\\end\\")
    path = tmp_path / name
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_the_module_in_the_two_pass_mode_takes_the_model(dev, tmp_path):
    import lightning

    odim = 40
    m = _small_e2e(odim, dev)
    toks = [str(i) for i in range(odim)]
    path = _ids_arpa(tmp_path, odim)
    mod = lightning.ModelModule.__new__(lightning.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.model, mod.token_list, mod.text_transform = m, toks, None
    mod.args = types.SimpleNamespace(decode_mode="rescore", rescore_beam=6, rescore_topk=5, ngram_path=path, ngram_weight=0.4,
                                     rescore_len_bonus=0.3)
    tp = mod._make_beam_search()
    assert isinstance(tp, TwoPassDecoder) and (tp.beam_size, tp.topk) == (6, 5)
    assert isinstance(tp.ngram, NgramScorer) and tp.ngram.order == 3 and tp.weights["ngram"] == 0.4 and tp.len_bonus == 0.3
    assert mod._make_beam_search().ngram is tp.ngram  # the ARPA file is read once
    g = torch.Generator().manual_seed(3)
    enc = (torch.randn(9, 128, generator=g) * 1.5).to(dev)
    with torch.no_grad():
        nbest = tp(enc)
    assert len(nbest) >= 1 and all(h.scores["ngram"] == _host_ngram(tp.ngram, h.yseq.tolist(), odim - 1) for h in nbest)
    mod.args = types.SimpleNamespace(decode_mode="rescore", ngram_path=path, ngram_weight=0.4)  # no bonus given: 0
    assert mod._make_beam_search().len_bonus == 0.0
    mod.args = types.SimpleNamespace(decode_mode="rescore")
    assert mod._make_beam_search().ngram is None
    # the getter's keyword is still refused
    with pytest.raises(NotImplementedError, match="n-gram"):
        lightning.get_two_pass_decoder(m, toks, ngram=path, ngram_weight=0.4)
    AF.invalidate_weight_cache()
