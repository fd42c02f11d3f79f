"""Golden vectors for language-model shallow fusion: the REFERENCE BatchBeamSearch (/root/reference, PyTorch CPU) with the
scorers lightning.get_beam_search_decoder wires and a Transformer LM in its `lm` slot.  The reference ships no LM class; the
one below is composed of the reference's own blocks (MultiHeadedAttention, PositionwiseFeedForward, LayerNorm,
PositionalEncoding, subsequent_mask, BatchScorerInterface) in ESPnet's TransformerLM layout (pre-norm), with ESPnet's
state-dict keys, so that tests/golden/synth.py gives it and auto_avsr_amd.lm.TransformerLM the same weights.  It keeps no
cache: every step recomputes the prefix.  Only results are stored; the forward log-probabilities keep at most 65 evenly spaced
vocabulary columns per row, which makes the file 140 KB (69 rows x <= 65 columns x 8 cases, f32).
Run in the build container only:   python tests/golden/make_golden_lm.py   ->  tests/golden/golden_lm_v1.pt"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
from synth import synth_state_dict  # noqa: E402

from espnet.nets.batch_beam_search import BatchBeamSearch  # noqa: E402
from espnet.nets.pytorch_backend.ctc import CTC  # noqa: E402
from espnet.nets.pytorch_backend.decoder.transformer_decoder import TransformerDecoder  # noqa: E402
from espnet.nets.pytorch_backend.transformer.attention import MultiHeadedAttention  # noqa: E402
from espnet.nets.pytorch_backend.transformer.embedding import PositionalEncoding  # noqa: E402
from espnet.nets.pytorch_backend.transformer.layer_norm import LayerNorm  # noqa: E402
from espnet.nets.pytorch_backend.transformer.mask import subsequent_mask  # noqa: E402
from espnet.nets.pytorch_backend.transformer.positionwise_feed_forward import PositionwiseFeedForward  # noqa: E402
from espnet.nets.scorer_interface import BatchScorerInterface  # noqa: E402
from espnet.nets.scorers.ctc import CTCPrefixScorer  # noqa: E402
from espnet.nets.scorers.length_bonus import LengthBonus  # noqa: E402

MIN_GAP = 5e-3  # adjacent recorded scores differ by at least this much: an ordering flip inside the tests' tolerance cannot decide a test


class _Layer(torch.nn.Module):
    def __init__(self, size, heads, units):
        super().__init__()
        self.self_attn = MultiHeadedAttention(heads, size, 0.0)
        self.feed_forward = PositionwiseFeedForward(size, units, 0.0)
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)

    def forward(self, x, mask):
        h = self.norm1(x)
        x = x + self.self_attn(h, h, h, mask)
        return x + self.feed_forward(self.norm2(x))


class _Encoder(torch.nn.Module):
    def __init__(self, idim, size, heads, units, layers):
        super().__init__()
        self.embed = torch.nn.Sequential(torch.nn.Linear(idim, size), LayerNorm(size), torch.nn.Dropout(0.0), torch.nn.ReLU(),
                                         PositionalEncoding(size, 0.0))
        self.encoders = torch.nn.ModuleList(_Layer(size, heads, units) for _ in range(layers))
        self.after_norm = LayerNorm(size)

    def forward(self, x, mask):
        x = self.embed(x)
        for e in self.encoders:
            x = e(x, mask)
        return self.after_norm(x)


class RefTransformerLM(torch.nn.Module, BatchScorerInterface):
    def __init__(self, n_vocab, embed_unit, att_unit, head, unit, layer):
        super().__init__()
        self.embed = torch.nn.Embedding(n_vocab, embed_unit)
        self.encoder = _Encoder(embed_unit, att_unit, head, unit, layer)
        self.decoder = torch.nn.Linear(att_unit, n_vocab)

    def forward(self, ys):
        mask = subsequent_mask(ys.size(-1), device=ys.device).unsqueeze(0)
        return torch.log_softmax(self.decoder(self.encoder(self.embed(ys), mask)), dim=-1)

    def score(self, y, state, x):
        return self.forward(y.unsqueeze(0))[0, -1], None

    def batch_score(self, ys, states, xs):
        return self.forward(ys)[:, -1], [None] * len(ys)


def lm_case(seed, odim, T, beam, ctc_weight, penalty, lm_weight, lm_dims, D=128):
    E, Dl, H, FF, NL = lm_dims
    torch.manual_seed(0)
    dec = TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = CTC(odim, D, 0.1, reduce=True).eval()
    lm = RefTransformerLM(odim, E, Dl, H, FF, NL).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    lm.load_state_dict(synth_state_dict(lm.state_dict(), seed + 2))
    g = torch.Generator().manual_seed(500 + seed)
    enc = torch.randn(T, D, generator=g) * 1.5
    token_list = [str(i) for i in range(odim)]

    def search(w_lm):
        scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc=ctc, eos=odim - 1), "lm": lm, "length_bonus": LengthBonus(len(token_list))}
        weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": w_lm, "length_bonus": penalty}
        bs = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                             token_list=token_list, pre_beam_score_key="decoder")
        with torch.no_grad():
            return bs(enc)

    nbest = search(lm_weight)
    hyps = [h.asdict() for h in nbest[:4]]
    for a, b in zip(hyps, hyps[1:]):
        assert a["score"] - b["score"] >= MIN_GAP, (seed, lm_weight, a["score"], b["score"])
    changes_winner = search(0.0)[0].asdict()["yseq"] != hyps[0]["yseq"]
    # the LM alone: teacher-forced log-probabilities on two fixed token matrices (at most 64 evenly spaced vocabulary columns kept)
    gt = torch.Generator().manual_seed(900 + seed)
    cols = torch.arange(0, odim, max(1, odim // 64))
    fwd = []
    for B, L in ((2, 9), (3, 17)):
        ys = torch.randint(0, odim, (B, L), generator=gt)
        with torch.no_grad():
            fwd.append(dict(ys=ys, cols=cols, logp=lm(ys)[..., cols].clone()))
    return dict(seed=seed, odim=odim, T=T, beam=beam, ctc_weight=ctc_weight, penalty=penalty, D=D, lm_weight=lm_weight, lm_dims=lm_dims,
                n_ended=len(nbest), changes_winner=changes_winner, forward=fwd,
                hyps=[dict(yseq=h["yseq"], score=h["score"], scores=h["scores"]) for h in hyps])


if __name__ == "__main__":
    small = (32, 64, 1, 128, 3)
    cases = []
    for args in ((1, 40, 15, 5, 0.1, 0.0), (2, 50, 23, 8, 0.3, 0.5), (4, 64, 31, 10, 0.1, 0.0)):
        for w in (0.3, 0.6):
            cases.append(lm_case(*args, w, small))
    cases.append(lm_case(7, 48, 19, 6, 0.2, 0.3, 0.4, (64, 128, 2, 256, 2)))
    cases.append(lm_case(6, 5049, 20, 10, 0.1, 0.0, 0.3, (128, 512, 8, 2048, 4)))
    torch.save({"cases": cases}, os.path.join(HERE, "golden_lm_v1.pt"))
    for c in cases:
        print(c["seed"], c["lm_weight"], c["n_ended"], c["changes_winner"], [(len(h["yseq"]), round(h["score"], 4)) for h in c["hyps"]])
