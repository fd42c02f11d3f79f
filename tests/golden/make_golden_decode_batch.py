"""Golden vectors for the batched beam search (BatchBeamSearch.forward_batch): runs the REFERENCE BatchBeamSearch (/root/reference,
PyTorch CPU) ONE UTTERANCE AT A TIME with the scorers lightning.get_beam_search_decoder wires (decoder + CTCPrefixScorer +
LengthBonus, pre-beam on the decoder scores) on two lists of utterances of different lengths that share a model -- the lists the test
then decodes as groups.
Run in the build container only:   python tests/golden/make_golden_decode_batch.py   ->  tests/golden/golden_decode_batch_v1.pt"""
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
from espnet.nets.scorers.ctc import CTCPrefixScorer  # noqa: E402
from espnet.nets.scorers.length_bonus import LengthBonus  # noqa: E402

GAP = 5e-3  # an order inside a gap of GAP * max(1, |score|) is not robust to the 1e-3 score tolerance of the comparison


def encoder_output(seed, T, D=128):
    return torch.randn(T, D, generator=torch.Generator().manual_seed(7000 + 100 * seed + T)) * 1.5


def group_case(seed, odim, beam, ctc_weight, penalty, lengths, D=128):
    torch.manual_seed(0)
    dec = TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    token_list = [str(i) for i in range(odim)]
    scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc=ctc, eos=odim - 1), "lm": None, "length_bonus": LengthBonus(len(token_list))}
    weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": 0.0, "length_bonus": penalty}
    bs = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                         token_list=token_list, pre_beam_score_key="decoder")
    utts = []
    for T in lengths:
        with torch.no_grad():
            nbest = bs(encoder_output(seed, T, D))
        hyps = [h.asdict() for h in nbest[:5] if float(h.score) > -1e8]
        keep = len(hyps)
        for i in range(len(hyps) - 1):
            if abs(hyps[i]["score"] - hyps[i + 1]["score"]) < GAP * max(1.0, abs(hyps[i]["score"])):
                keep = i + 1
                break
        assert keep >= 2, (seed, T, [h["score"] for h in hyps])
        utts.append(dict(T=T, n_ended=len(nbest), hyps=[dict(yseq=h["yseq"], score=h["score"], scores=h["scores"]) for h in hyps[:keep]]))
    return dict(seed=seed, odim=odim, beam=beam, ctc_weight=ctc_weight, penalty=penalty, D=D, lengths=list(lengths), utts=utts)


if __name__ == "__main__":
    out = {"groups": [group_case(11, 40, 5, 0.1, 0.0, (9, 1, 36, 15, 2, 26, 12, 31, 3, 19, 5)),
                      group_case(14, 50, 8, 0.3, 0.0, (27, 1, 11, 3, 8))]}
    torch.save(out, os.path.join(HERE, "golden_decode_batch_v1.pt"))
    for g in out["groups"]:
        for u in g["utts"]:
            print(g["seed"], u["T"], u["n_ended"], len(u["hyps"]), [len(h["yseq"]) for h in u["hyps"]], round(u["hyps"][0]["score"], 4))
