"""Golden vectors for contextual biasing: the REFERENCE BatchBeamSearch (PyTorch CPU) with the scorers
lightning.get_beam_search_decoder wires -- the reference's decoder, CTC prefix scorer and length bonus -- and a bias scorer in a
`bias` slot between them.  The reference ships no such scorer; the one below is a plain dict trie that re-walks the whole prefix of
every hypothesis at every step: no state, no cache, no code shared with auto_avsr_amd/bias.py (whose docstring states the
semantics).  The phrases of a case are cut out of the UNBIASED search's 2nd-4th hypotheses, so that the list decides the result.
Only results are stored.
Run in the build container only:   python tests/golden/make_golden_bias.py <path of the reference checkout>
                                   ->  tests/golden/golden_bias_v1.pt"""
import os
import sys

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
from espnet.nets.scorer_interface import BatchScorerInterface  # noqa: E402
from espnet.nets.scorers.ctc import CTCPrefixScorer  # noqa: E402
from espnet.nets.scorers.length_bonus import LengthBonus  # noqa: E402

MIN_GAP = 5e-3  # adjacent recorded scores differ by at least this much: an ordering flip inside the tests' tolerance cannot decide a test


class RefBias(BatchScorerInterface):
    """Trie of nested dicts; key None marks a node where a phrase ends."""

    def __init__(self, phrases, n_vocab):
        self.root, self.n = {}, n_vocab
        for ph in phrases:
            d = self.root
            for t in ph:
                d = d.setdefault(t, {})
            d[None] = True

    @staticmethod
    def _children(d):
        return [k for k in d if k is not None]

    def _walk(self, tokens):
        """node after the tokens and its uncommitted edge count"""
        d, unc = self.root, 0
        for t in tokens:
            d, unc, _ = self._extend(d, unc, t)
        return d, unc

    def _extend(self, d, unc, t):
        if t in d:
            nd, nu, g = d[t], unc + 1, 1
        else:
            g = -unc
            if t in self.root:
                nd, nu, g = self.root[t], 1, g + 1
            else:
                nd, nu = self.root, 0
        if None in nd:
            nu = 0
            if not self._children(nd):
                nd = self.root
        return nd, nu, g

    def score(self, y, state, x):
        d, unc = self._walk(y.tolist()[1:])
        return torch.tensor([float(self._extend(d, unc, v)[2]) for v in range(self.n)]), None

    def batch_score(self, ys, states, xs):
        return torch.stack([self.score(y, None, None)[0] for y in ys]), [None] * len(ys)


def make_phrases(nbest, odim):
    win = nbest[0]["yseq"]
    ok = lambda ph: len(ph) > 0 and all(1 <= t <= odim - 2 for t in ph)  # noqa: E731
    other = lambda t: t % (odim - 2) + 1  # noqa: E731  -- another legal token
    phrases, around = [], []
    for h in nbest[1:4]:
        ys = h["yseq"]
        d = next((i for i in range(1, min(len(ys), len(win))) if ys[i] != win[i]), None)
        if d is None:
            continue
        lo = max(1, min(d - 1, len(ys) - 4))
        ph = ys[lo: lo + 3]
        if len(ph) == 3 and ok(ph):
            around.append(ph)
    assert around
    phrases += around
    phrases.append(around[0][:2] + [other(other(around[0][2]))])  # shares two tokens, then diverges: never completes
    phrases.append(win[1:3] + [other(win[3])])  # the winner's start with its third token changed: its reward is taken back
    phrases.append([around[-1][1]])  # one token
    phrases.append(around[-1][:2])  # a proper prefix of another phrase
    assert all(ok(p) for p in phrases)
    return phrases


def bias_case(seed, odim, T, beam, ctc_weight, penalty, bias_weight, D=128):
    torch.manual_seed(0)
    dec = TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    g = torch.Generator().manual_seed(500 + seed)
    enc = torch.randn(T, D, generator=g) * 1.5
    token_list = [str(i) for i in range(odim)]

    def search(phrases, w):
        scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc=ctc, eos=odim - 1), "lm": None, "bias": RefBias(phrases, odim),
                   "length_bonus": LengthBonus(len(token_list))}
        weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": 0.0, "bias": w, "length_bonus": penalty}
        bs = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                             token_list=token_list, pre_beam_score_key="decoder")
        with torch.no_grad():
            return bs(enc)

    plain = [h.asdict() for h in search([], 0.0)]
    phrases = make_phrases(plain, odim)
    nbest = search(phrases, bias_weight)
    hyps = [h.asdict() for h in nbest[:4]]
    assert len(hyps) == 4
    for a, b in zip(hyps, hyps[1:]):
        assert a["score"] - b["score"] >= MIN_GAP, (seed, bias_weight, a["score"], b["score"])
    assert hyps[0]["yseq"] != plain[0]["yseq"], (seed, bias_weight, "the bias does not change the winner")
    return dict(seed=seed, odim=odim, T=T, beam=beam, ctc_weight=ctc_weight, penalty=penalty, D=D, bias_weight=bias_weight,
                phrases=phrases, n_ended=len(nbest), hyps=[dict(yseq=h["yseq"], score=h["score"], scores=h["scores"]) for h in hyps])


if __name__ == "__main__":
    cases = []
    for args in ((1, 40, 15, 5, 0.1, 0.0), (2, 50, 23, 8, 0.3, 0.5), (4, 64, 31, 10, 0.1, 0.0)):
        for w in (0.5, 1.5):
            cases.append(bias_case(*args, w))
    cases.append(bias_case(6, 5049, 20, 10, 0.1, 0.0, 1.0))
    torch.save({"cases": cases}, os.path.join(HERE, "golden_bias_v1.pt"))
    for c in cases:
        print(c["seed"], c["bias_weight"], c["n_ended"], c["phrases"], [(len(h["yseq"]), round(h["score"], 4), h["scores"]["bias"]) for h in c["hyps"]])
