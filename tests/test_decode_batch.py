"""The batched native beam search (BatchBeamSearch.forward_batch -> decode_native.search_batch -> avsr_beam_*_batch of csrc/decode.hip):
one decoding step serves a GROUP of utterances whose running hypotheses are one packed row list.  Checked against golden vectors of
the reference's BatchBeamSearch run one utterance at a time (tests/golden/make_golden_decode_batch.py), against the per-utterance
native search `bs(x)`, at the kernel corners (more than 128 packed rows, source attention with 4 / 8 / 16 waves in one launch, K
slices), with a language model attached, and on the trained fixture.  Kernels through the emulator (CPU suite) or on the MI355X."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
from synth import synth_state_dict  # noqa: E402

from auto_avsr_amd import functional as AF  # noqa: E402
from auto_avsr_amd import nets  # noqa: E402
from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "golden_decode_batch_v1.pt"), weights_only=False)["groups"]
GOLD_LM = torch.load(os.path.join(HERE, "golden", "golden_lm_v1.pt"), weights_only=False)["cases"]
GROUP_A = GOLD[0]


def _bs(dev, seed, odim, beam, ctc_weight, penalty, linear_units=256, lm=None, lm_weight=0.0, D=128):
    torch.manual_seed(0)
    dec = nets.TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=linear_units, num_blocks=2).eval()
    ctc = nets.CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    dec, ctc = dec.to(dev), ctc.to(dev)
    scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": lm, "length_bonus": LengthBonus(odim)}
    weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": lm_weight, "length_bonus": penalty}
    return BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                           token_list=[str(i) for i in range(odim)], pre_beam_score_key="decoder")


def _enc(dev, seed, T, D=128):
    return (torch.randn(T, D, generator=torch.Generator().manual_seed(7000 + 100 * seed + T)) * 1.5).to(dev)


def _group_bs(dev, g, **kw):
    return _bs(dev, g["seed"], g["odim"], g["beam"], g["ctc_weight"], g["penalty"], **kw)


class _precise:
    def __enter__(self):
        AF.set_precise(True)

    def __exit__(self, *a):
        AF.set_precise(False)


def _same_as_single(batched, single, min_live=3, tol=1e-4):
    """Every ended hypothesis of every utterance equals the per-utterance search's (those the CTC scorer rules out, score < -1e8, tie
    and are ordered arbitrarily: excluded); at least min_live live ones compared per utterance where the search has that many."""
    assert len(batched) == len(single)
    for a, b in zip(batched, single):
        assert len(a) == len(b) and len(a) >= 1
        live = 0
        for x, y in zip(a, b):
            x, y = x.asdict(), y.asdict()
            if y["score"] < -1e8:
                assert x["score"] < -1e8
                continue
            live += 1
            assert x["yseq"] == y["yseq"]
            assert abs(x["score"] - y["score"]) < tol * max(1.0, abs(y["score"]))
            assert set(x["scores"]) == set(y["scores"])
            for k, v in y["scores"].items():
                assert abs(x["scores"][k] - v) < tol * max(1.0, abs(v)), k
        assert live >= min(min_live, sum(1 for y in b if float(y.score) >= -1e8))


# ------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("batch", ["all", 4])
@pytest.mark.parametrize("g", GOLD, ids=lambda g: f"seed{g['seed']}")
def test_forward_batch_vs_reference(dev, g, batch):
    """The reference's n-best of every utterance (searched one at a time) from ONE group of all utterances and from groups of four:
    count of ended hypotheses, token sequences, total score within 1e-3, per-scorer scores within 2e-3 (the tolerances of
    test_beam_search_vs_reference).  Six of the sixteen utterances end on <eos> before their last step, the others at their own T."""
    bs = _group_bs(dev, g)
    xs = [_enc(dev, g["seed"], T) for T in g["lengths"]]
    with _precise():
        out = bs.forward_batch(xs, batch=len(xs) if batch == "all" else batch)
    assert bs._native and len(out) == len(xs)
    for nbest, ref in zip(out, g["utts"]):
        assert len(nbest) == ref["n_ended"] and len(ref["hyps"]) >= 2
        for got, want in zip(nbest, ref["hyps"]):
            d = got.asdict()
            assert d["yseq"] == want["yseq"]
            assert abs(d["score"] - want["score"]) < 1e-3 * max(1.0, abs(want["score"]))
            for k, v in want["scores"].items():
                assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), k


# ------------------------------------------------------------------------------------------------------- 2. against bs(x)
@pytest.fixture
def group_a_single(dev):
    """Group A's search object, encoder outputs and the per-utterance results for the three length rules (computed once per backend)."""
    key = str(dev)
    if key not in _SINGLE:
        bs = _group_bs(dev, GROUP_A)
        xs = [_enc(dev, GROUP_A["seed"], T) for T in GROUP_A["lengths"]]
        with _precise():
            _SINGLE[key] = (bs, xs, {r: [bs(x, maxlenratio=r) for x in xs] for r in (0.0, -4, 0.5)})
    return _SINGLE[key]


_SINGLE = {}


@pytest.mark.parametrize("maxlenratio", [0.0, -4, 0.5])
def test_forward_batch_equals_one_at_a_time(dev, group_a_single, maxlenratio):
    """Searches that stop by end detection, at a forced end after four steps and at half the frames: every ended hypothesis and every
    per-scorer score of every utterance, from one group of eleven."""
    bs, xs, single = group_a_single
    with _precise():
        out = bs.forward_batch(xs, batch=16, maxlenratio=maxlenratio)  # (a batch larger than the list)
    _same_as_single(out, single[maxlenratio])


def test_forward_batch_group_sizes(dev, group_a_single):
    """batch = 1, a one-element list, an empty list and a workspace bound that forces groups of one (several groups of three otherwise);
    on the seven shorter utterances of group A."""
    from auto_avsr_amd import decode_native

    bs, xs, single = group_a_single
    pick = [0, 1, 3, 4, 6, 8, 10]  # 9, 1, 15, 2, 12, 3, 5 frames
    xs, single = [xs[i] for i in pick], {0.0: [single[0.0][i] for i in pick]}
    seen = []
    real = decode_native.NativeBeam.search_group

    def spy(self, group, *a, **k):
        seen.append(len(group))
        return real(self, group, *a, **k)

    decode_native.NativeBeam.search_group = spy
    try:
        with _precise():
            _same_as_single(bs.forward_batch(xs, batch=1), single[0.0])
            assert seen == [1] * len(xs)
            _same_as_single(bs.forward_batch(xs[2:3], batch=8), single[0.0][2:3])
            assert bs.forward_batch([], batch=8) == []
            del seen[:]
            _same_as_single(bs.forward_batch(xs, batch=3), single[0.0])
            assert seen == [3, 3, 1]
            del seen[:]
            _same_as_single(bs.forward_batch(xs, batch=3, max_workspace_bytes=1), single[0.0])
            assert seen == [1] * len(xs)
    finally:
        decode_native.NativeBeam.search_group = real


def test_batch_group_limits(dev, group_a_single):
    """The library refuses groups it has no tables for, with a message: more than 32 utterances, more than 1024 packed rows."""
    import ctypes

    from auto_avsr_amd import _lib

    bs, xs, _ = group_a_single
    sess = bs._native
    assert sess.group_workspace_bytes([5] * 32, 5) > 0
    with pytest.raises(_lib.AvsrLibraryError, match="U <= 32"):
        sess.group_workspace_bytes([5] * 33, 5)
    T = (ctypes.c_int32 * 33)(*[5] * 33)
    p = (ctypes.c_void_p * 33)()
    with pytest.raises(_lib.AvsrLibraryError, match="group too large"):
        _lib.lib().call("avsr_beam_begin_batch", sess.handle, 33, ctypes.cast(p, ctypes.c_void_p), ctypes.cast(T, ctypes.c_void_p),
                        ctypes.cast(p, ctypes.c_void_p), ctypes.cast(T, ctypes.c_void_p), ctypes.cast(p, ctypes.c_void_p), None, 0, 5, None)


# ------------------------------------------------------------------------------------------------------- 3. kernel corners
def test_forward_batch_kernel_corners(dev):
    """Vocabulary 5049 (row pitch 5056), beam 40, FFN 2048 (K slices + row sum), four utterances of 300 / 70 / 5 / 130 frames: 160
    packed rows (more than the 128 the per-utterance tables hold), source attention with 16, 8, 4 and 8 waves in one launch, its
    groups of four rows at utterance boundaries; six steps."""
    bs = _bs(dev, 11, 5049, 40, 0.1, 0.0, linear_units=2048)
    xs = [_enc(dev, 11, T) for T in (300, 70, 5, 130)]
    with _precise():
        out = bs.forward_batch(xs, batch=4, maxlenratio=-6)
        single = [bs(x, maxlenratio=-6) for x in xs]
    assert bs._native
    _same_as_single(out, single)


@pytest.mark.parametrize("beam,lengths,maxlenratio", [(2, (9, 1, 2, 7), 0.0), (5, (9, 1, 2), -1), (4, (2, 9, 1), 0.0)])
def test_forward_batch_edge_cases(dev, beam, lengths, maxlenratio):
    """The cases of test_native_beam_search_edge_cases as members of one group: the smallest beam (2: pre-beam 3), a one-frame and a
    two-frame utterance next to longer ones (they retire after one / two steps), a one-step search (forced end at the first step)."""
    bs = _bs(dev, 3, 30, beam, 0.1, 0.0)
    xs = [_enc(dev, 3, T) for T in lengths]
    with _precise():
        out = bs.forward_batch(xs, batch=len(xs), maxlenratio=maxlenratio)
        single = [bs(x, maxlenratio=maxlenratio) for x in xs]
    _same_as_single(out, single, min_live=1)


# ------------------------------------------------------------------------------------------------------- 4. with a language model
@pytest.mark.parametrize("case", GOLD_LM, ids=lambda c: f"seed{c['seed']}-w{c['lm_weight']}-V{c['odim']}")
def test_forward_batch_with_language_model(dev, case):
    """The cases of golden_lm_v1.pt (built as tests/test_lm_fusion.py builds them), each in a group with three further utterances of other
    lengths: the case's row reproduces the reference's n-best with the LM (tolerances of test_lm_beam_search_vs_reference), the other
    rows equal bs(x)."""
    from auto_avsr_amd.lm import TransformerLM

    E, D, H, FF, NL = case["lm_dims"]
    lm = TransformerLM(case["odim"], embed_unit=E, att_unit=D, head=H, unit=FF, layer=NL)
    lm.load_state_dict(synth_state_dict(lm.state_dict(), case["seed"] + 2))
    bs = _bs(dev, case["seed"], case["odim"], case["beam"], case["ctc_weight"], case["penalty"], lm=lm.to(dev), lm_weight=case["lm_weight"],
             D=case["D"])
    x = (torch.randn(case["T"], case["D"], generator=torch.Generator().manual_seed(500 + case["seed"])) * 1.5).to(dev)
    others = [_enc(dev, case["seed"], T, case["D"]) for T in (case["T"] + 2, 3, 6)]
    xs = [others[0], x, others[1], others[2]]
    with _precise():
        out = bs.forward_batch(xs, batch=4)
        single = [bs(o) for o in others]
    assert bs._native and "lm" in bs.full_scorers
    nbest = out[1]
    assert len(nbest) == case["n_ended"]
    for got, ref in zip(nbest, case["hyps"]):
        d = got.asdict()
        assert d["yseq"] == ref["yseq"]
        assert abs(d["score"] - ref["score"]) < 1e-3 * max(1.0, abs(ref["score"]))
        assert set(d["scores"]) == set(ref["scores"]) and "lm" in ref["scores"]
        for k, v in ref["scores"].items():
            assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), k
    _same_as_single([out[0], out[2], out[3]], single, min_live=1)


# ------------------------------------------------------------------------------------------------------- 5. fallback
def test_forward_batch_falls_back_to_the_python_step(dev):
    """A scorer set NativeBeam.supported refuses (pre-beam 45 >= vocabulary 40: no pre-beam) still returns [bs(x) for x in xs]."""
    from auto_avsr_amd.decode_native import NativeBeam

    bs = _bs(dev, 11, 40, 30, 0.1, 0.0)
    assert not NativeBeam.supported(bs)
    xs = [_enc(dev, 11, T) for T in (4, 2)]
    with _precise():
        out = bs.forward_batch(xs, batch=2, maxlenratio=-2)
        single = [bs(x, maxlenratio=-2) for x in xs]
    assert bs._native is False
    _same_as_single(out, single, min_live=1)


# ------------------------------------------------------------------------------------------------------- 7. on the MI355X
@pytest.mark.gpu
def test_forward_batch_on_the_trained_fixture():
    """The trained fixture of tests/test_wer_trained.py (32 utterances, T = 12 ... 400, beam 40, precise mode), encoded one utterance at
    a time and decoded through groups of eight: the reference's best hypothesis token for token for every utterance, the identical
    total edit distance, worst relative score error < 1e-3 (that test's assertions)."""
    import lightning
    import trained_common as TC

    from auto_avsr_amd import _lib
    from auto_avsr_amd.e2e import E2E

    assert torch.cuda.is_available(), "GPU suite needs a GPU"
    _lib._lib = None
    assert not _lib.lib().is_emulator
    fx = torch.load(TC.FIXTURE, weights_only=False)
    AF.invalidate_weight_cache()
    m = E2E(TC.ODIM, "video", adim=TC.D, aheads=TC.H, eunits=TC.U, elayers=TC.NENC, dunits=TC.U, dlayers=TC.NDEC)
    sd = synth_state_dict(m.state_dict(), TC.SEED)
    sd.update(fx["weights"])
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    bs = lightning.get_beam_search_decoder(m, [str(i) for i in range(TC.ODIM)], beam_size=TC.BEAM)
    AF.set_mode("precise")
    try:
        encs = []
        with torch.no_grad():
            for i, u in enumerate(fx["utts"]):
                enc, _ = m.encoder(m.proj_encoder(m.frontend(TC.video(i, u["T"]).unsqueeze(0).cuda())), None)
                encs.append(enc.squeeze(0).float())
            out = bs.forward_batch(encs, batch=8)
    finally:
        AF.set_mode("bf16")
        AF.invalidate_weight_cache()
    assert bs._native and len(out) == len(fx["utts"]) == 32
    tot, worst = 0, 0.0
    for i, (u, nbest) in enumerate(zip(fx["utts"], out)):
        got, ref = nbest[0].asdict(), u["hyps"][0]
        assert [int(t) for t in got["yseq"]] == ref["yseq"], (i, u["T"], got["yseq"], ref["yseq"])
        worst = max(worst, abs(float(got["score"]) - ref["score"]) / max(1.0, abs(ref["score"])))
        tot += TC.edit_distance(u["label"], [int(t) for t in got["yseq"][1:-1]])
    print(f"\nWER {tot}/{fx['total_length']} (reference {fx['wer']:.4f}); worst relative score error {worst:.2e}")
    assert tot == fx["total_distance"]
    assert worst < 1e-3


@pytest.mark.gpu
def test_eval_decode_batch_writes_the_same_records(tmp_path):
    """eval.py --decode-batch 4 --timestamps on six synthetic utterances writes the JSON lines of a run without --decode-batch."""
    import eval as E

    a, b = str(tmp_path / "one.jsonl"), str(tmp_path / "batch.jsonl")
    try:
        torch.manual_seed(0)  # (no checkpoint: each run builds its model from the generator's state)
        E.cli_main(["--synthetic-utterances", "6", "--timestamps", a])
        torch.manual_seed(0)
        E.cli_main(["--synthetic-utterances", "6", "--timestamps", b, "--decode-batch", "4"])
    finally:  # (cli_main leaves its --numerics mode set)
        AF.set_mode("bf16")
        AF.invalidate_weight_cache()
    ra, rb = [json.loads(l) for l in open(a)], [json.loads(l) for l in open(b)]
    assert len(ra) == len(rb) == 6
    assert ra == rb


def test_eval_decode_batch_usage(capsys):
    """--decode-batch is off by default; with --decode-workers > 1 or --decode-mode rescore it is a usage error with a message."""
    import eval as E

    assert E.parse_args([]).decode_batch == 0 and E.parse_args(["--decode-batch", "8"]).decode_batch == 8
    for extra in (["--decode-workers", "2"], ["--decode-mode", "rescore"]):
        with pytest.raises(SystemExit):
            E.parse_args(["--decode-batch", "4"] + extra)
        assert "--decode-batch" in capsys.readouterr().err
