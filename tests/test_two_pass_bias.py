"""Contextual biasing in two-pass decoding: the CTC prefix beam search with a phrase list (csrc/ctc_beam.hip:
avsr_ctc_beam_search_bias), the bias term of the rescoring objective (auto_avsr_amd/two_pass.py) and the plumbing through
lightning.get_two_pass_decoder / ModelModule.  Kernels through the emulator (CPU suite) or on the MI355X (-m gpu).

The search is checked FRAME BY FRAME from the kernel's own previous beam, as tests/test_ctc_beam.py checks the plain search (its
helpers are restated here): a float64 step gives every candidate's pure CTC masses, `ContextBiasScorer.walk(prefix)` on the host
gives its sum of gains, and the kernel's next beam must be a valid top-W by  total + weight * sum  that carries the unchanged pure
CTC masses.

Tolerance of a mass or a key s: 1e-5 * max(1, |s|) + 1e-5.  A frame update is at most W + 2 f32 operations per value (W <= 64) and
the key adds a multiplication and an addition: 68 * 6e-8 = 4.1e-6."""
import os
import sys
import types
import warnings

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
from auto_avsr_amd.two_pass import TwoPassDecoder  # noqa: E402

NEG = float("-inf")
WEIGHT = 2.0
GOLD = torch.load(os.path.join(HERE, "golden", "golden_bias_v1.pt"), weights_only=False)["cases"]


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


def _phrases(res, in_lens, V, seed):
    """A list that bites, built from the UNBIASED run of utterance 0: runs of 2 to 4 tokens through consecutive frames' token sets,
    pieces of the winner, a phrase that is a proper prefix of another (an end node with children), a single-token phrase (rule 3), and
    one that shares only its first token with the winner (its second token is taken back)."""
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
    out.append(long[:2])  # a proper prefix of `long`
    out.append([sets[Tb // 2][-1]])  # a single token
    first = next(c for c in win if ok(c))
    other = next(c for s in sets for c in s if c not in win[:3] and c != first)
    out.append([first, other, other % (V - 2) + 1])
    return out


def _check_frames(lp, res, in_lens, W, K, sc, weight):
    """-> (worst error as a fraction of the tolerance, counts): every frame of every utterance is a valid biased step from the kernel's own
    previous beam.  counts: kept entries with a non-zero sum of gains; live candidates whose extension took an uncommitted reward back
    (and, for the print-out, those of them that were kept); kept entries that have passed an end node (they hold a committed reward)."""
    trace, topk = ops.ctc_beam_trace(res, in_lens)
    unc = sc.unc
    worst, n_gain, n_back, n_back_kept, n_end = 0.0, 0, 0, 0, 0
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
            walk = {p: sc.walk(p) for p in live}
            key = {p: tot[p] + weight * walk[p][0] for p in live}
            new = trace[b][t]
            assert len(new) == min(W, len(live)), (b, t, len(new), len(live))
            kept = [p for p, _, _ in new]
            assert len(set(kept)) == len(kept), (b, t)
            before = {p for p, _, _ in beam}
            back = set()
            for p, _, _ in beam:
                node = sc.walk(p)[1]
                if int(unc[node]) > 0:
                    back |= {p + (c,) for c in toks if p + (c,) in walk and sc.step(node, c)[0] <= 0}
            n_back += len(back - before)
            n_back_kept += len((back - before) & set(kept))
            for p, pb, pnb in new:
                assert p in cand and tot[p] > NEG, (b, t, p)
                s = tot[p]  # the stored masses are pure CTC
                err = abs(_lae(pb, pnb) - s)
                worst = max(worst, err / _tol(s))
                assert err <= _tol(s), (b, t, p, pb, pnb, cand[p])
                for got, ref in ((pb, cand[p][0]), (pnb, cand[p][1])):
                    if ref >= s - 20:
                        assert abs(got - ref) <= _tol(s), (b, t, p, got, ref)
                g, node = walk[p]
                n_gain += g != 0
                n_end += g - int(unc[node]) > 0
            # the beam is in the order of the biased key, and no candidate outside exceeds its smallest key by more than the tolerance
            ks = [_lae(pb, pnb) + weight * walk[p][0] for p, pb, pnb in new]
            for x, y in zip(ks, ks[1:]):
                assert y <= x + _tol(x), (b, t, ks)
            floor = min(key[p] for p in kept)
            out = [key[p] for p in live if p not in set(kept)]
            if out:
                worst = max(worst, (max(out) - floor) / _tol(floor))
                assert max(out) <= floor + _tol(floor), (b, t, max(out), floor)
            beam = new
    return worst, (n_gain, n_back, n_end), n_back_kept


def _final(res, b=0):
    return [tuple(res["tokens"][b, r, : int(res["lens"][b, r])].cpu().tolist()) for r in range(int(res["n_valid"][b]))]


# ---------------------------------------------------------------------------------------------------- test 1: frame by frame
@pytest.mark.parametrize("T,V,W,K", [(12, 20, 4, 4), (40, 64, 8, 8), (37, 5049, 16, 16), (8, 40, 64, 32)])
def test_every_frame_is_a_valid_biased_step_from_the_kernels_own_beam(dev, T, V, W, K):
    lp = AF.log_softmax(_logits(1, T, V, T + V).to(dev))
    if V == 5049:
        assert lp.stride(-2) == 5056
    plain = _search(dev, lp, [T], W, K)
    sc = ContextBiasScorer(_phrases(plain, [T], V, T), V)
    res = _search(dev, lp, [T], W, K, bias=sc, bias_weight=WEIGHT)
    worst, counts, back_kept = _check_frames(lp, res, [T], W, K, sc, WEIGHT)
    print(f"T={T} V={V} W={W} K={K}: worst error {worst:.3f} of the tolerance; kept entries with gains / candidates after a take-back / "
          f"kept entries past an end node: {counts} ({back_kept} of the take-backs kept); {sc.n_nodes} nodes")
    assert all(c > 0 for c in counts), counts
    assert _final(res) != _final(plain)  # the list changed what the search keeps


def test_every_frame_of_a_batch_that_shares_a_list(dev):
    in_lens, T, V, W, K = [23, 1, 0, 9], 23, 31, 8, 6
    lp = AF.log_softmax(_logits(4, T, V, 11).to(dev))
    plain = _search(dev, lp, in_lens, W, K)
    sc = ContextBiasScorer(_phrases(plain, in_lens, V, 5), V)
    res = _search(dev, lp, in_lens, W, K, bias=sc, bias_weight=WEIGHT)
    worst, counts, back_kept = _check_frames(lp, res, in_lens, W, K, sc, WEIGHT)
    print(f"B=4 in_lens={in_lens}: worst error {worst:.3f} of the tolerance; counts {counts} ({back_kept} of the take-backs kept)")
    assert all(c > 0 for c in counts), counts
    assert _final(res, 0) != _final(plain, 0)


# ---------------------------------------------------------------------------------------------------- test 2: the n-best
def test_nbest_carries_the_committed_gains_and_the_pure_ctc_masses(dev):
    in_lens, T, V, W, K, N = [23, 1, 0, 9], 23, 31, 8, 6, 5
    lp = AF.log_softmax(_logits(4, T, V, 11).to(dev))
    plain = _search(dev, lp, in_lens, W, K, nbest=N)
    sc = ContextBiasScorer(_phrases(plain, in_lens, V, 5), V)
    res = _search(dev, lp, in_lens, W, K, nbest=N, bias=sc, bias_weight=WEIGHT)
    trace, _ = ops.ctc_beam_trace(res, in_lens)
    toks, lens, nv = res["tokens"].cpu(), res["lens"].cpu(), res["n_valid"].cpu()
    score, pb, pnb = res["score"].cpu(), res["pb"].cpu(), res["pnb"].cpu()
    bsum, bnode = res["bias_sum"].cpu(), res["bias_node"].cpu()
    assert bsum.shape == bnode.shape == (4, N) and bsum.dtype == torch.float32 and bnode.dtype == torch.int32
    kept_reward = 0
    for b, Tb in enumerate(in_lens):
        last = trace[b][-1] if Tb > 0 else [((), 0.0, NEG)]  # (already in the biased order)
        assert int(nv[b]) == min(N, len(last))
        for r in range(N):
            if r >= int(nv[b]):
                assert int(lens[b, r]) == 0 and float(score[b, r]) == NEG and (toks[b, r] == -1).all()
                assert float(bsum[b, r]) == 0.0 and int(bnode[b, r]) == 0
                continue
            p, rpb, rpnb = last[r]
            assert tuple(toks[b, r, : int(lens[b, r])].tolist()) == p and int(lens[b, r]) == len(p)
            assert (toks[b, r, len(p):] == -1).all()
            assert float(pb[b, r]) == rpb and float(pnb[b, r]) == rpnb
            assert abs(float(score[b, r]) - _lae(rpb, rpnb)) <= _tol(float(score[b, r]))
            g, node = sc.walk(p)
            assert float(bsum[b, r]) == g + sc.step(node, V - 1)[0], (b, r, p)
            assert int(bnode[b, r]) == node, (b, r, p)
            kept_reward += float(bsum[b, r]) > 0
    assert kept_reward > 0
    assert int(nv[2]) == 1 and int(lens[2, 0]) == 0 and float(score[2, 0]) == 0.0 and float(bsum[2, 0]) == 0.0


# ---------------------------------------------------------------------------------------------------- test 3: without a list
HISTORY = ("topk_tok", "topk_val", "blank_val", "count")


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


def test_no_list_is_the_plain_search(dev):
    in_lens, T, V, W, K = [17, 5], 17, 29, 6, 5
    x = _logits(2, T, V, 2)
    x[..., 20:23] -= 60  # three tokens that no frame offers
    lp = AF.log_softmax(x.to(dev))
    plain = _search(dev, lp, in_lens, W, K)
    outs = ("tokens", "lens", "score", "pb", "pnb", "n_valid", "bias_sum", "bias_node")
    assert float(plain["bias_sum"].abs().max()) == 0.0 and int(plain["bias_node"].abs().max()) == 0
    before = ops.call("avsr_ctc_beam_workspace_bytes", 2, T, W, K)
    for kw in (dict(bias=None, bias_weight=WEIGHT), dict(bias=ContextBiasScorer([], V), bias_weight=WEIGHT),
               dict(bias=ContextBiasScorer([[3, 4], [5]], V), bias_weight=0.0)):
        res = _search(dev, lp, in_lens, W, K, **kw)
        _same_run(res, plain, in_lens, outs + HISTORY)
    assert ops.call("avsr_ctc_beam_workspace_bytes", 2, T, W, K) == before
    assert ops.call("avsr_ctc_beam_bias_workspace_bytes", 2, T, W, K) == before + (2 * T * K * 4 + 15) // 16 * 16
    # phrases over tokens that no frame offers: the biased kernel runs and changes nothing
    seen = set(plain["topk_tok"][0, :17].cpu().flatten().tolist()) | set(plain["topk_tok"][1, :5].cpu().flatten().tolist())
    unseen = [c for c in range(1, V - 1) if c not in seen]
    assert unseen == [20, 21, 22]
    sc = ContextBiasScorer([unseen[:2], [unseen[1]], [unseen[0], unseen[0]]], V)
    res = _search(dev, lp, in_lens, W, K, bias=sc, bias_weight=WEIGHT)
    _same_run(res, plain, in_lens, ("tokens", "lens", "score", "n_valid", "bias_sum") + HISTORY)


def test_rejects_a_list_of_another_vocabulary_or_size(dev):
    lp = AF.log_softmax(_logits(1, 4, 9, 0).to(dev))
    with pytest.raises(ValueError):
        _search(dev, lp, [4], 4, 3, bias=ContextBiasScorer([[3, 4]], 10), bias_weight=1.0)
    sc = ContextBiasScorer([[3, 4]], 9)
    tabs = sc.device_tables(lp.device)
    ws = torch.zeros(ops.call("avsr_ctc_beam_bias_workspace_bytes", 1, 4, 4, 3) // 4, dtype=torch.int32, device=lp.device)
    o = [torch.zeros(64, dtype=torch.int32, device=lp.device) for _ in range(8)]
    lens = torch.tensor([4], dtype=torch.int64, device=lp.device)
    for nn, ne, w in (((1 << 24) + 1, 2, 1.0), (3, (1 << 24) + 1, 1.0), (-1, 2, 1.0), (3, 2, float("inf")), (3, 2, float("nan"))):
        with pytest.raises(Exception):
            ops.call("avsr_ctc_beam_search_bias", ops._ptr(lp), lp.stride(-2), ops._ptr(lens), 0, 4, 3, 4, *[ops._ptr(t) for t in tabs], nn, ne,
                   w, *[ops._ptr(t) for t in o], ops._ptr(ws), 1, 4, 9, ops._stream(lp))


# ---------------------------------------------------------------------------------------------------- test 4: the second pass
def _models(case, dev):
    """Decoder and CTC head exactly as tests/test_context_bias.py builds them for the reference-made fixture."""
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


def _two_pass(case, dev, bias="case", beam=10, topk=10, models=None):
    dec, ctc = models or _models(case, dev)
    odim = case["odim"]
    if isinstance(bias, str):
        bias = ContextBiasScorer(case["phrases"], odim)
    scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": None, "bias": bias, "length_bonus": LengthBonus(odim)}
    weights = {"decoder": 1.0 - case["ctc_weight"], "ctc": case["ctc_weight"], "lm": 0.0,
               "bias": case["bias_weight"] if bias is not None else 0.0, "length_bonus": case["penalty"]}
    return TwoPassDecoder(scorers, weights, sos=odim - 1, eos=odim - 1, token_list=[str(i) for i in range(odim)], beam_size=beam,
                          topk=topk)


def test_rescoring_equals_the_references_stored_biased_scores(dev):
    """The reference-made fixture of the biased hybrid search: `rescore` of its finished hypotheses reproduces the stored score and
    per-scorer scores within the tolerances tests/test_two_pass.py uses for the unbiased fixtures (1e-3 / 2e-3 relative, set against
    the reference's own stored values), the bias sums exactly.  Force-ended hypotheses (len(yseq) - 2 == T, <eos> not scored) are
    excluded by that rule alone, as there."""
    checked, boosted, worst = 0, 0, 0.0
    AF.set_precise(True)
    try:
        for case in GOLD:
            natural = [h for h in case["hyps"] if len(h["yseq"]) - 2 < case["T"]]
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
                assert set(d["scores"]) == set(ref["scores"]) and "bias" in ref["scores"]
                for k, v in ref["scores"].items():
                    assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), (case["seed"], k, d["scores"][k], v)
                assert d["scores"]["bias"] == ref["scores"]["bias"]
                checked += 1
                boosted += ref["scores"]["bias"] != 0
    finally:
        AF.set_precise(False)
    print(f"biased rescoring: {checked} hypotheses ({boosted} with a non-zero bias sum), worst relative score error {worst:.2e}")
    assert checked >= len(GOLD) and boosted > 0


# ---------------------------------------------------------------------------------------------------- test 5: the decoder
def _host_bias(sc, yseq, eos):
    y = [int(t) for t in yseq][1:-1]
    g, s = sc.walk(y)
    return float(g + sc.step(s, eos)[0])


def _check_hyps(nbest, tp, plain, enc, sc):
    again = plain.rescore(enc, [h.yseq for h in nbest])
    for h, ref in zip(nbest, again):
        d, r = h.asdict(), ref.asdict()
        assert d["yseq"] == r["yseq"] and set(d["scores"]) == set(r["scores"]) | {"bias"}
        assert d["scores"]["bias"] == _host_bias(sc, d["yseq"], tp.eos)
        total = sum(tp.weights[k] * v for k, v in d["scores"].items())
        assert abs(d["score"] - total) < 1e-4 * max(1.0, abs(total)), (d["score"], total)
        for k, v in r["scores"].items():
            assert abs(d["scores"][k] - v) < 1e-4 * max(1.0, abs(v)), k
    sc_ = [float(h.score) for h in nbest]
    assert sc_ == sorted(sc_, reverse=True)


def test_two_pass_decoder_with_a_list(dev):
    case = dict(next(c for c in GOLD if c["odim"] < 1000), penalty=0.5)
    odim = case["odim"]
    AF.set_precise(True)
    try:
        models = _models(case, dev)
        plain = _two_pass(case, dev, bias=None, models=models)
        xs = [_enc(case, dev, T=T, seed=900 + T) for T in (23, 14)]
        base = plain.forward_many(xs)
        # phrases cut out of what the unbiased first pass ranks LOW, so that the list reorders the n-best
        low = [[int(t) for t in hyps[-1].yseq[1:-1]] for hyps in base]
        phrases = [y[i:i + 3] for y in low for i in range(0, max(1, len(y) - 2), 3) if len(y[i:i + 3]) >= 2] + [[1, 2], [1, 2, 3]]
        phrases = [p for p in phrases if all(1 <= c <= odim - 2 for c in p)]
        sc = ContextBiasScorer(phrases, odim)
        tp = _two_pass(case, dev, bias=sc, models=models)
        assert tp.bias is sc and tp.weights["bias"] == case["bias_weight"]
        many = tp.forward_many(xs)
        assert float(tp.last_first_pass["bias_sum"].abs().max()) > 0
        for enc, nbest in zip(xs, many):
            assert 1 <= len(nbest) <= 10
            _check_hyps(nbest, tp, plain, enc, sc)
        assert any(float(h.scores["bias"]) > 0 for nbest in many for h in nbest)
        # two utterances at once equal one at a time
        for enc, a in zip(xs, many):
            b = tp(enc)
            a = {tuple(h.yseq.tolist()): h.asdict() for h in a}
            b = {tuple(h.yseq.tolist()): h.asdict() for h in b}
            assert set(a) == set(b)
            for y in a:
                assert abs(a[y]["score"] - b[y]["score"]) < 1e-4 * max(1.0, abs(b[y]["score"]))
                assert a[y]["scores"]["bias"] == b[y]["scores"]["bias"]
        # rescore of sequences given from outside walks them on the host
        given = tp.rescore(xs[0], [h.yseq for h in many[0]])
        for g, h in zip(given, many[0]):
            assert g.scores["bias"] == h.scores["bias"] and abs(float(g.score) - float(h.score)) < 1e-4 * max(1.0, abs(float(h.score)))
        # set_phrases between two calls: the next call runs with the new list, no rebuild
        first = [[h.asdict() for h in nbest] for nbest in many]
        sc.set_phrases([])
        empty = tp.forward_many(xs)
        for nbest, ref in zip(empty, base):
            assert [h.yseq.tolist() for h in nbest] == [h.yseq.tolist() for h in ref]
            assert all(h.scores["bias"] == 0.0 for h in nbest)
            for h, r in zip(nbest, ref):
                assert abs(float(h.score) - float(r.score)) < 1e-4 * max(1.0, abs(float(r.score)))
        sc.set_phrases(phrases)
        back = tp.forward_many(xs)
        assert [[h.asdict()["yseq"] for h in nbest] for nbest in back] == [[d["yseq"] for d in nbest] for nbest in first]
        assert [[h.scores["bias"] for h in nbest] for nbest in back] == [[d["scores"]["bias"] for d in nbest] for nbest in first]
    finally:
        AF.set_precise(False)
    # the slot takes this build's scorer over the head's vocabulary, nothing else
    for bad in (object(), ContextBiasScorer([[3, 4]], odim + 1)):
        with pytest.raises(TypeError):
            _two_pass(case, dev, bias=bad, models=models)


def _small_e2e(odim, dev):
    from auto_avsr_amd.e2e import E2E

    return E2E(odim, "video", adim=128, aheads=2, eunits=256, elayers=1, dunits=256, dlayers=1, cnn_module_kernel=7).to(dev).eval()


def test_get_two_pass_decoder_and_the_module_with_bias(dev, tmp_path):
    import eval as EV
    import lightning

    odim = 40
    m = _small_e2e(odim, dev)
    toks = [str(i) for i in range(odim)]
    for kw in (dict(), dict(bias_phrases=[[3, 4]], bias_weight=0.0)):
        tp = lightning.get_two_pass_decoder(m, toks, beam_size=4, topk=4, **kw)
        assert tp.bias is None and "bias" not in tp.scorers
    with pytest.warns(UserWarning, match="without a bias list"):
        tp = lightning.get_two_pass_decoder(m, toks, beam_size=4, topk=4, bias_weight=0.8)
    assert tp.bias is None
    tp = lightning.get_two_pass_decoder(m, toks, beam_size=4, topk=4, bias_phrases=[[3, 4], [5]], bias_weight=0.8, penalty=0.5)
    assert isinstance(tp.bias, ContextBiasScorer) and tp.weights["bias"] == 0.8 and tp.bias.phrases == [(3, 4), (5,)]
    sc = ContextBiasScorer([], odim)
    tp = lightning.get_two_pass_decoder(m, toks, beam_size=4, topk=4, bias_phrases=sc, bias_weight=0.8)
    assert tp.bias is sc
    with pytest.raises(ValueError):
        lightning.get_two_pass_decoder(m, toks, beam_size=4, topk=4, bias_phrases=[[odim - 1]], bias_weight=0.8)
    with pytest.raises(ValueError):
        lightning.get_two_pass_decoder(m, toks + ["x"], beam_size=4, topk=4, bias_phrases=sc, bias_weight=0.8)
    # the module in the two-pass mode gets the scorer, and set_bias swaps its list in place
    path = tmp_path / "bias.txt"
    path.write_text("3 4 5\n17\n")
    mod = lightning.ModelModule.__new__(lightning.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.model, mod.token_list, mod.text_transform = m, toks, None
    mod.args = types.SimpleNamespace(decode_mode="rescore", rescore_beam=6, rescore_topk=5, bias_list=str(path), bias_weight=1.5)
    tp = mod._make_beam_search()
    assert isinstance(tp, TwoPassDecoder) and (tp.beam_size, tp.topk) == (6, 5)
    assert isinstance(tp.bias, ContextBiasScorer) and tp.bias.phrases == [(3, 4, 5), (17,)] and tp.weights["bias"] == 1.5
    mod.beam_search = tp
    mod.set_bias([[5, 6]])
    assert tp.bias.phrases == [(5, 6)] and mod._make_beam_search().bias is tp.bias
    g = torch.Generator().manual_seed(3)
    enc = (torch.randn(9, 128, generator=g) * 1.5).to(dev)
    with torch.no_grad():
        nbest = tp(enc)
    assert all(h.scores["bias"] == _host_bias(tp.bias, h.yseq.tolist(), odim - 1) for h in nbest)
    mod.args = types.SimpleNamespace(decode_mode="rescore", bias_list=str(path), bias_weight=0.0)
    with pytest.warns(UserWarning, match="without a bias weight"):
        assert mod._make_beam_search().bias is None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError):
            mod.set_bias([[5]])
    # eval.py's command line is as it was: the flags are still refused together with --decode-mode rescore
    with pytest.raises(SystemExit):
        EV.parse_args(["--bias-list", str(path), "--bias-weight", "1.5", "--decode-mode", "rescore"])
    AF.invalidate_weight_cache()
