"""Two-pass decoding (auto_avsr_amd/two_pass.py): the rescoring objective against the scores the REFERENCE's BatchBeamSearch stored
(golden_decode_v1.pt, golden_lm_v1.pt), the whole decoder end to end on the emulator, the trained fixture on the MI355X, and the
plumbing through lightning.ModelModule / eval.py.

The reference's stored score of a hypothesis that ended with a SCORED <eos> is a closed form -- teacher-forced decoder sum (<eos>
included), exact log P_ctc, language-model sum, len(y) + 1 -- which is the rescoring objective.  It does not hold for the hypotheses
the reference force-ended at maxlen (beam_search.py:430-436 appends <eos> without scoring it): those have len(yseq) - 2 == T and are
excluded by exactly that rule.

Worst observed (emulator, precise arithmetic): see the print-out of test_rescoring_equals_the_references_stored_scores."""
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
from synth import synth_state_dict  # noqa: E402

from auto_avsr_amd import functional as AF  # noqa: E402
from auto_avsr_amd import nets  # noqa: E402
from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus  # noqa: E402
from auto_avsr_amd.two_pass import TwoPassDecoder  # noqa: E402

GOLD_DEC = torch.load(os.path.join(HERE, "golden", "golden_decode_v1.pt"), weights_only=False)["beam"]
GOLD_LM = torch.load(os.path.join(HERE, "golden", "golden_lm_v1.pt"), weights_only=False)["cases"]


def _models(case, dev):
    """Decoder, CTC head, encoder output and (with `lm_dims`) the LM, exactly as test_decoding.py / test_lm_fusion.py build them."""
    odim, D = case["odim"], case["D"]
    torch.manual_seed(0)
    dec = nets.TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = nets.CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), case["seed"]))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), case["seed"] + 1))
    lm = None
    if "lm_dims" in case:
        from auto_avsr_amd.lm import TransformerLM

        E, DL, H, FF, NL = case["lm_dims"]
        lm = TransformerLM(odim, embed_unit=E, att_unit=DL, head=H, unit=FF, layer=NL)
        lm.load_state_dict(synth_state_dict(lm.state_dict(), case["seed"] + 2))
        lm = lm.to(dev)
    return dec.to(dev), ctc.to(dev), lm


def _enc(case, dev, T=None, seed=None):
    g = torch.Generator().manual_seed(500 + case["seed"] if seed is None else seed)
    return (torch.randn(T or case["T"], case["D"], generator=g) * 1.5).to(dev)


def _two_pass(case, dev, beam=10, topk=10):
    dec, ctc, lm = _models(case, dev)
    odim = case["odim"]
    scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": lm, "length_bonus": LengthBonus(odim)}
    weights = {"decoder": 1.0 - case["ctc_weight"], "ctc": case["ctc_weight"], "lm": case.get("lm_weight", 0.0),
               "length_bonus": case["penalty"]}
    return TwoPassDecoder(scorers, weights, sos=odim - 1, eos=odim - 1, token_list=[str(i) for i in range(odim)], beam_size=beam,
                          topk=topk)


# ---------------------------------------------------------------------------------------------------- test 5
def test_rescoring_equals_the_references_stored_scores(dev):
    checked, with_lm, forced, worst = 0, 0, 0, 0.0
    AF.set_precise(True)
    try:
        for case in list(GOLD_DEC) + list(GOLD_LM):
            natural = [h for h in case["hyps"] if len(h["yseq"]) - 2 < case["T"]]
            forced += len(case["hyps"]) - len(natural)
            assert all(len(h["yseq"]) - 2 == case["T"] for h in case["hyps"] if h not in natural)  # excluded by the length rule alone
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
                assert set(d["scores"]) == set(ref["scores"])
                for k, v in ref["scores"].items():
                    assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), (case["seed"], k, d["scores"][k], v)
                checked += 1
                with_lm += "lm" in ref["scores"]
    finally:
        AF.set_precise(False)
    print(f"rescoring: {checked} hypotheses ({with_lm} with an lm term), {forced} force-ended excluded, worst relative score error {worst:.2e}")
    assert (checked, with_lm) == (11, 5) and forced > 0


# ---------------------------------------------------------------------------------------------------- test 6
def _seed4():
    return [c for c in GOLD_DEC if c["seed"] == 4][0]


def test_two_pass_end_to_end(dev):
    case = _seed4()
    AF.set_precise(True)
    try:
        tp = _two_pass(case, dev, beam=10, topk=10)
        enc = _enc(case, dev)
        nbest = tp(enc)
        assert 1 <= len(nbest) <= 10
        sc = [float(h.score) for h in nbest]
        assert sc == sorted(sc, reverse=True)
        again = tp.rescore(enc, [h.yseq for h in nbest])
        for a, b in zip(nbest, again):
            a, b = a.asdict(), b.asdict()
            assert a["yseq"] == b["yseq"] and a["yseq"][0] == a["yseq"][-1] == case["odim"] - 1
            assert abs(a["score"] - b["score"]) < 1e-4 * max(1.0, abs(b["score"]))
            assert set(a["scores"]) == set(b["scores"]) == {"decoder", "ctc"}  # (penalty 0, no LM: the non-zero weights)
            for k in a["scores"]:
                assert abs(a["scores"][k] - b["scores"][k]) < 1e-4 * max(1.0, abs(b["scores"][k])), k
        assert len({tuple(h.yseq.tolist()) for h in nbest}) == len(nbest)
        # keys follow the non-zero weights: with a penalty and an LM all four
        lm_case = dict([c for c in GOLD_LM if c["seed"] == 4 and c["lm_weight"] == 0.3][0], penalty=0.5)
        full = _two_pass(lm_case, dev, beam=6, topk=6)(_enc(lm_case, dev))
        assert set(full[0].scores) == {"decoder", "ctc", "lm", "length_bonus"}
        assert float(full[0].scores["length_bonus"]) == len(full[0].yseq) - 1
    finally:
        AF.set_precise(False)


def test_forward_many_equals_one_at_a_time(dev):
    case = _seed4()
    AF.set_precise(True)
    try:
        tp = _two_pass(case, dev, beam=10, topk=10)
        xs = [_enc(case, dev, T=T, seed=900 + T) for T in (9, 23, 14)]
        many = tp.forward_many(xs)
        single = [tp(x) for x in xs]
    finally:
        AF.set_precise(False)
    assert len(many) == len(single) == 3
    for a, b in zip(many, single):
        assert len(a) == len(b) >= 1
        a = {tuple(h.yseq.tolist()): h.asdict() for h in a}
        b = {tuple(h.yseq.tolist()): h.asdict() for h in b}
        assert set(a) == set(b)
        for y in a:
            assert abs(a[y]["score"] - b[y]["score"]) < 1e-4 * max(1.0, abs(b[y]["score"]))


# ---------------------------------------------------------------------------------------------------- test 7
@pytest.mark.gpu
def test_trained_fixture_two_pass_scores_at_least_the_reference_best():
    """32 trained utterances (T = 12 ... 400) through ModelModule with decode_mode = "rescore".  Wherever the reference's best
    hypothesis ended naturally AND is among the first pass' n-best, the two-pass winner is the maximum of the same objective over
    a set that contains it: its score is at least the stored one (minus the score tolerance of test_decoding.py).  WER figures
    are printed, none is asserted."""
    import lightning
    import trained_common as TC
    from auto_avsr_amd.e2e import E2E

    fx = torch.load(TC.FIXTURE, weights_only=False)
    AF.invalidate_weight_cache()
    m = E2E(TC.ODIM, "video", adim=TC.D, aheads=TC.H, eunits=TC.U, elayers=TC.NENC, dunits=TC.U, dlayers=TC.NDEC)
    sd = synth_state_dict(m.state_dict(), TC.SEED)
    sd.update(fx["weights"])
    m.load_state_dict(sd, strict=True)
    mod = lightning.ModelModule.__new__(lightning.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.args = types.SimpleNamespace(decode_mode="rescore")
    mod.model = m.cuda().eval()
    mod.token_list = [str(i) for i in range(TC.ODIM)]
    mod.beam_search = mod._make_beam_search()
    assert isinstance(mod.beam_search, TwoPassDecoder)
    AF.set_mode("precise")
    tot, contained, natural, ge = 0, 0, 0, 0
    try:
        for i, u in enumerate(fx["utts"]):
            with torch.no_grad():
                x = TC.video(i, u["T"]).unsqueeze(0).cuda()
                enc, _ = m.encoder(m.proj_encoder(m.frontend(x)), None)
                nbest = mod.beam_search(enc.squeeze(0).float())
            assert len(nbest) >= 1
            got, ref = nbest[0].asdict(), u["hyps"][0]
            tot += TC.edit_distance(u["label"], [int(t) for t in got["yseq"][1:-1]])
            if len(ref["yseq"]) - 2 < u["T"]:
                natural += 1
                if any([int(t) for t in h.yseq.tolist()] == ref["yseq"] for h in nbest):
                    contained += 1
                    ge += got["score"] >= ref["score"]
                    assert got["score"] >= ref["score"] - 1e-3 * max(1.0, abs(ref["score"])), (i, u["T"], got["score"], ref["score"])
    finally:
        AF.set_mode("bf16")
        AF.invalidate_weight_cache()
    print(f"\ntwo-pass (beam 16, topk 16): reference best contained in the n-best for {contained} of {natural} natural-ended utterances "
          f"(of {len(fx['utts'])}); WER {tot}/{fx['total_length']} = {tot / fx['total_length']:.4f} (reference search {fx['wer']:.4f})")


# ---------------------------------------------------------------------------------------------------- test 8
def test_plumbing(dev):
    import eval as EV
    import lightning
    from auto_avsr_amd.e2e import E2E

    args = EV.parse_args(["--decode-mode", "rescore"])
    assert (args.decode_mode, args.rescore_beam, args.rescore_topk) == ("rescore", 16, 16)
    plain = EV.parse_args([])
    assert plain.decode_mode == "search"
    args = EV.parse_args(["--decode-mode", "rescore", "--rescore-beam", "6", "--rescore-topk", "5"])
    odim = 40
    m = E2E(odim, "video", adim=128, aheads=2, eunits=256, elayers=1, dunits=256, dlayers=1, cnn_module_kernel=7).to(dev).eval()
    mod = lightning.ModelModule.__new__(lightning.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.model, mod.token_list = m, [str(i) for i in range(odim)]
    mod.args = args
    tp = mod._make_beam_search()
    assert isinstance(tp, TwoPassDecoder) and (tp.beam_size, tp.topk, tp.nbest) == (6, 5, 6)
    assert tp.weights["ctc"] == 0.1 and tp.lm is None and tp.ctc is m.ctc and tp.decoder is m.decoder
    mod.args = plain
    assert isinstance(mod._make_beam_search(), BatchBeamSearch)
    with pytest.raises(TypeError):
        lightning.get_two_pass_decoder(m, mod.token_list, rnnlm=object(), lm_weight=0.3)
    with pytest.raises(TypeError):
        lightning.get_beam_search_decoder(m, mod.token_list, rnnlm=object(), lm_weight=0.3)
    # the module decodes with it: one utterance at a time and several at once
    mod.args = args
    mod.beam_search = mod._make_beam_search()

    class Text:
        def post_process(self, ids):
            return " ".join(str(int(i)) for i in ids if int(i) not in (-1, odim - 1))

    mod.text_transform = Text()
    g = torch.Generator().manual_seed(3)
    xs = [torch.randn(T, 1, 88, 88, generator=g).to(dev) for T in (2, 3)]
    with torch.no_grad():
        one = [mod._decode(x) for x in xs]
        many = mod.decode_many(xs, workers=2)
    assert one == many and all(isinstance(s, str) for s in one)
    AF.invalidate_weight_cache()
