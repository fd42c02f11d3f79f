"""Golden vectors for n-gram shallow fusion: the REFERENCE BatchBeamSearch (PyTorch CPU) with the scorers
lightning.get_beam_search_decoder wires -- the reference's decoder, CTC prefix scorer and length bonus -- and a back-off n-gram
PARTIAL scorer in an `ngram` slot after `ctc`.  The scorer below is the ARPA definition as a float64 recursion over two dicts that
re-walks the whole prefix of every hypothesis at every step: no state, no tables, no code shared with auto_avsr_amd/ngram.py (whose
docstring states the semantics).  It scores the pre-beam candidates and the <eos> column, 0 elsewhere.  A case's model is estimated
(absolute discounting) from counts over the n-gram-free search's 2nd-4th hypotheses plus random sequences, at a weight that changes
the winner.  The model's two dicts (values rounded to f32, which is what both sides then read) and the results are stored.
Run in the build container only:   python tests/golden/make_golden_ngram.py <path of the reference checkout>
                                   ->  tests/golden/golden_ngram_v1.pt"""
import math
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, HERE)
from synth import synth_state_dict  # noqa: E402

from espnet.nets.batch_beam_search import BatchBeamSearch  # noqa: E402
from espnet.nets.pytorch_backend.ctc import CTC  # noqa: E402
from espnet.nets.pytorch_backend.decoder.transformer_decoder import TransformerDecoder  # noqa: E402
from espnet.nets.scorer_interface import BatchPartialScorerInterface  # noqa: E402
from espnet.nets.scorers.ctc import CTCPrefixScorer  # noqa: E402
from espnet.nets.scorers.length_bonus import LengthBonus  # noqa: E402

MIN_GAP = 5e-3  # adjacent recorded scores differ by at least this much: an ordering flip inside the tests' tolerance cannot decide a test
ORDER = 3


class RefNgram(BatchPartialScorerInterface):
    """P {n-gram: ln p}, B {n-gram: ln back-off}; <s> = n_vocab, </s> = n_vocab - 1."""

    def __init__(self, P, B, n_vocab, order):
        self.P, self.B, self.n, self.N = P, B, n_vocab, order

    def p(self, v, h):
        g = h + (v,)
        if g in self.P:
            return self.P[g]
        assert h, v
        return self.B.get(h, 0.0) + self.p(v, h[1:])

    def batch_score_partial(self, ys, ids, states, x):
        out = torch.zeros(len(ys), self.n, dtype=torch.float64)
        for b, y in enumerate(ys.tolist()):
            h = tuple(([self.n] + y[1:])[-(self.N - 1):]) if self.N > 1 else ()
            for v in set(ids[b].tolist()) | {self.n - 1}:
                if v != 0:
                    out[b, v] = self.p(v, h)
        return out, None


def estimate(seqs, odim, order=ORDER, d=0.4):
    """Absolute discounting with back-off to the lower order; every token 1 .. odim - 1 has a unigram.  Values rounded to f32."""
    S, E = odim, odim - 1
    cnt = [{} for _ in range(order + 1)]
    for s in seqs:
        w = [S] + list(s) + [E]
        for k in range(1, order + 1):
            for i in range(len(w) - k + 1):
                g = tuple(w[i: i + k])
                cnt[k][g] = cnt[k].get(g, 0) + 1
    P, B = {}, {}
    total = sum(c for g, c in cnt[1].items() if g != (S,))
    for v in range(1, odim):
        P[(v,)] = math.log((cnt[1].get((v,), 0) + 0.1) / (total + 0.1 * (odim - 1)))
    P[(S,)] = -99.0 * math.log(10.0)
    for k in range(2, order + 1):
        ctx_total, ctx_types = {}, {}
        for g, c in cnt[k].items():
            ctx_total[g[:-1]] = ctx_total.get(g[:-1], 0) + c
            ctx_types[g[:-1]] = ctx_types.get(g[:-1], 0) + 1
        for g, c in cnt[k].items():
            P[g] = math.log((c - d) / ctx_total[g[:-1]])
        for h, t in ctx_total.items():
            B[h] = math.log(d * ctx_types[h] / t)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    return {g: f32(v) for g, v in P.items()}, {g: f32(v) for g, v in B.items()}


def ngram_case(seed, odim, T, beam, ctc_weight, penalty, ngram_weight, D=128):
    torch.manual_seed(0)
    dec = TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    g = torch.Generator().manual_seed(500 + seed)
    enc = torch.randn(T, D, generator=g) * 1.5
    token_list = [str(i) for i in range(odim)]

    def search(model, w):
        scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc=ctc, eos=odim - 1), "lm": None, "ngram": model,
                   "length_bonus": LengthBonus(len(token_list))}
        weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": 0.0, "ngram": w, "length_bonus": penalty}
        bs = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                             token_list=token_list, pre_beam_score_key="decoder")
        assert w == 0.0 or list(bs.part_scorers) == ["ctc", "ngram"]
        with torch.no_grad():
            return bs(enc)

    plain = [h.asdict() for h in search(None, 0.0)]
    rng = random.Random(seed)
    seqs = [h["yseq"][1:-1] for h in plain[1:4]] * 2
    seqs += [[rng.randint(1, odim - 2) for _ in range(rng.randint(2, 8))] for _ in range(12)]
    P, B = estimate(seqs, odim)
    nbest = search(RefNgram(P, B, odim, ORDER), ngram_weight)
    hyps = [h.asdict() for h in nbest[:4]]
    assert len(hyps) == 4
    for a, b in zip(hyps, hyps[1:]):
        assert a["score"] - b["score"] >= MIN_GAP, (seed, ngram_weight, a["score"], b["score"])
    assert hyps[0]["yseq"] != plain[0]["yseq"], (seed, ngram_weight, "the model does not change the winner")
    return dict(seed=seed, odim=odim, T=T, beam=beam, ctc_weight=ctc_weight, penalty=penalty, D=D, ngram_weight=ngram_weight, order=ORDER,
                probs=P, backoffs=B, n_ended=len(nbest), hyps=[dict(yseq=h["yseq"], score=h["score"], scores=h["scores"]) for h in hyps])


if __name__ == "__main__":
    cases = []
    # (weights at which the model changes the winner AND the four recorded scores keep MIN_GAP: the asserts above decide)
    for args, ws in (((1, 40, 9, 4, 0.1, 0.0), (0.3, 0.6)), ((2, 50, 12, 5, 0.3, 0.5), (0.3, 0.7)), ((4, 64, 11, 6, 0.1, 0.0), (0.3, 0.6))):
        for w in ws:
            cases.append(ngram_case(*args, w))
    cases.append(ngram_case(6, 5049, 10, 5, 0.1, 0.0, 0.5))
    torch.save({"cases": cases}, os.path.join(HERE, "golden_ngram_v1.pt"))
    for c in cases:
        print(c["seed"], c["ngram_weight"], c["n_ended"], len(c["probs"]), [(len(h["yseq"]), round(h["score"], 4), round(h["scores"]["ngram"], 4)) for h in c["hyps"]])
