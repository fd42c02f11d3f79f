"""CTC forced alignment on the device (csrc/ctc_align.hip; ctc.py:95-242) and what is built on it: ops.ctc_align /
functional.ctc_align, CTC.forced_align / forced_align_batch / align, alignment.segments / word_timestamps,
ModelModule.align and `eval.py --timestamps`.  Kernels through the emulator (CPU suite) or on the MI355X (-m gpu).

Path identity against the reference is asserted only on stored inputs whose every trellis decision has a gap >= 1e-3
(tests/golden/make_golden_align.py asserts that condition when it writes them); everywhere else the criterion is the score
of the returned path against the float64 optimum."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from auto_avsr_amd import _lib, alignment, nets, ops  # noqa: E402
from auto_avsr_amd import functional as AF  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "golden_align_v1.pt")


# ------------------------------------------------------------------------------------------------ restatement (float64)
def viterbi64(lp, y, blank=0):
    """Best-path score of the labels y through log-probabilities lp (T, V), float64; -inf if they do not fit."""
    ext = np.full(2 * len(y) + 1, blank, dtype=np.int64)
    ext[1::2] = y
    S = len(ext)
    skip = np.zeros(S, dtype=bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    delta = np.full(S, -np.inf)
    delta[:2] = lp[0, ext[:2]]
    for t in range(1, lp.shape[0]):
        c1 = np.concatenate(([-np.inf], delta[:-1]))
        c2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], delta[:-2])), -np.inf)
        delta = np.maximum(np.maximum(delta, c1), c2) + lp[t, ext]
    return float(delta[-2:].max())


def collapse(ali, blank=0):
    out, prev = [], blank
    for a in ali:
        if a != blank and a != prev:
            out.append(int(a))
        prev = a
    return out


def spacing_f32(x):
    return float(np.spacing(np.float32(abs(x))))


def check_optimal(name, logits, labels, in_lens, ali, score, blank=0, ignore_id=-1, deficit_ref=None):
    """logits (B, T, V) as the kernel saw them (bf16 already rounded), float32/float64 on the host.  Returns the largest deficit."""
    B, T, _ = logits.shape
    lp64 = torch.log_softmax(logits.double(), -1).numpy()
    ali = ali.cpu().numpy()
    score = score.cpu().numpy()
    worst = 0.0
    for b in range(B):
        y = [int(v) for v in labels[b].tolist() if v != ignore_id]
        Tb = int(in_lens[b])
        assert ali.shape[1] == T and (ali[b, Tb:] == ignore_id).all()
        a = ali[b, :Tb]
        assert collapse(a, blank) == y, (name, b)  # (a) a valid alignment of exactly these labels
        opt = viterbi64(lp64[b, :Tb], y, blank)
        mine = float(lp64[b, np.arange(Tb), a].sum())
        deficit = opt - mine
        bound = (deficit_ref[b] if deficit_ref is not None else 0.0) + 8 * spacing_f32(opt)
        print(f"{name} b={b} T={Tb} L={len(y)}: optimum {opt:.4f} deficit {deficit:.3e} (bound {bound:.3e}) "
              f"returned score off by {abs(score[b] - mine):.3e}")
        assert -1e-9 <= deficit <= bound, (name, b, deficit, bound)  # (b) its float64 score is the optimum's
        assert abs(score[b] - mine) <= 1e-3 * abs(mine), (name, b, score[b], mine)  # (c) the returned score is that path's
        worst = max(worst, deficit)
    return worst


def run_align(dev, logits, labels, in_lens, blank=0, ignore_id=-1, dtype=torch.float32):
    """ops.ctc_align on a pitch-padded copy of logits (B, T, V)."""
    B, T, V = logits.shape
    ld = (V + 7) // 8 * 8
    x = torch.zeros(B * T, ld, dtype=dtype)
    x[:, :V] = logits.reshape(B * T, V).to(dtype)
    return ops.ctc_align(x.to(dev), ld, labels.to(dev), in_lens.to(dev), B, T, V, blank=blank, ignore_id=ignore_id)


def identity_ctc(V, dev):
    """nets.CTC whose ctc_lo copies its input: hidden states (.., D = V rounded up to 8) ARE the logits.  With split hi / lo bf16
    planes (precise mode) and inputs of 16 significant bits, as the golden file stores them, the copy is exact."""
    D = (V + 7) // 8 * 8
    ctc = nets.CTC(V, D, 0.0)
    with torch.no_grad():
        ctc.ctc_lo.weight.copy_(torch.eye(V, D))
        ctc.ctc_lo.bias.zero_()
    return ctc.to(dev).eval(), D


def as_hidden(logits, D):
    h = torch.zeros(logits.shape[:-1] + (D,))
    h[..., : logits.shape[-1]] = logits
    return h


# ------------------------------------------------------------------------------------------------ tests
def test_align_matches_reference_paths(dev):
    """Stored cases whose every float64 trellis decision (and the final S-1 / S-2 choice) has a gap >= 1e-3 and on which the
    reference's forced_align and forced_align_batch agree: the alignment equals the reference's element for element through all
    three python entry points, the score is the reference path's float64 score to 1e-3 relative.  Includes a repeated label,
    L = 1, and a ragged batch with label rows padded with -1."""
    gold = torch.load(GOLDEN)
    V = gold["V"]
    AF.invalidate_weight_cache()
    ctc, D = identity_ctc(V, dev)
    with AF.precise(True), torch.no_grad():
        for c in gold["exact"]:
            T, ref, want = c["T"], c["ali"].numpy(), float(c["score"])
            assert c["gap"] >= 1e-3
            logits = c["logits"]  # (T, 1, V)
            h = as_hidden(logits[:, 0], D).to(dev)
            # 1. CTC.forced_align: hidden states (T, D), labels as tensor / numpy / list -> list of T python ints
            for y in (c["y"], c["y"].numpy(), c["y"].tolist()):
                a1 = ctc.forced_align(h, y)
                assert isinstance(a1, list) and len(a1) == T and all(type(v) is int for v in a1)
                assert a1 == ref.tolist(), (T, c["L"])
            assert ctc.forced_align(h.unsqueeze(0), c["y"]) == ref.tolist()
            # 2. CTC.forced_align_batch: time-major LOGITS (T, B, V) -> list of numpy int64 arrays
            a2 = ctc.forced_align_batch(logits.to(dev), c["y"].view(1, -1), torch.tensor([T]))
            assert len(a2) == 1 and isinstance(a2[0], np.ndarray) and a2[0].dtype == np.int64 and a2[0].shape == (T,)
            assert np.array_equal(a2[0], ref)
            # 3. CTC.align: hidden states (B, T, D) -> device tensors
            ali, score = ctc.align(h.unsqueeze(0), torch.tensor([T]), c["y"].view(1, -1))
            assert ali.device.type == dev.type and ali.dtype == torch.int32 and ali.shape == (1, T)
            assert np.array_equal(ali[0].cpu().numpy(), ref)
            print(f"exact T={T} L={c['L']}: score {float(score[0]):.4f} reference path (float64) {want:.4f}")
            assert abs(float(score[0]) - want) <= 1e-3 * abs(want)
        for c in gold["exact_batch"]:
            ilens, ref, Ls = c["ilens"], c["ali"].numpy(), c["Ls"]
            B = len(Ls)
            a2 = ctc.forced_align_batch(c["logits"].to(dev), c["ys"], ilens)
            ali, score = ctc.align(as_hidden(c["logits"].transpose(0, 1), D).to(dev), ilens, c["ys"].to(dev))
            assert ali.shape == (B, c["Tmax"])
            for b in range(B):
                Tb = int(ilens[b])
                assert a2[b].dtype == np.int64 and np.array_equal(a2[b], ref[b, :Tb]), b
                assert np.array_equal(ali[b].cpu().numpy(), ref[b]), b  # (-1 beyond ilens[b] on both sides)
                a1 = ctc.forced_align(as_hidden(c["logits"][:Tb, b], D).to(dev), c["ys"][b, : Ls[b]])
                assert a1 == ref[b, :Tb].tolist(), b
                assert abs(float(score[b]) - float(c["score"][b])) <= 1e-3 * abs(float(c["score"][b]))
    AF.invalidate_weight_cache()


# label widths chosen to hit every states-per-lane instantiation of the trellis kernel (S = 2L + 1 over 64 lanes: 1, 2, 3, 4, 6,
# 8 states per lane), as tests/test_loss_kernels.py::test_ctc; T up to 600 (three 256-frame chunks of the back-trace) and once
# 2048; the real vocabulary (V = 5049 in rows of pitch 5056) once; bf16 logits once
OPT_CASES = [(3, 40, 53, 9, "f32"), (2, 150, 301, 70, "f32"), (2, 12, 20, 1, "f32"), (1, 300, 64, 140, "f32"),
             (2, 90, 64, 40, "f32"), (1, 260, 40, 100, "f32"), (1, 520, 40, 230, "f32"), (1, 600, 53, 90, "f32"),
             (2, 100, 5049, 16, "f32"), (2, 90, 64, 40, "bf16"), (1, 2048, 16, 20, "f32")]


@pytest.mark.parametrize("B,T,V,L,dtype", OPT_CASES)
def test_align_is_optimal(dev, B, T, V, L, dtype):
    """For every utterance: the alignment has length in_lens[b] (ignore_id beyond) and collapses to exactly the labels; its
    score, re-computed in float64 from a float64 log-softmax of the same logits, is within
    deficit_ref + 8 * spacing_f32(|optimum|) of the float64 Viterbi optimum (deficit_ref: the reference forced_align_batch's own
    deficit, 0 for generated inputs; the margin because the kernel keeps the running score in float32 like the reference but sums
    the log-softmax denominator in another order); the returned score equals the re-computed one to 1e-3 relative.

    Largest deficit measured over all cases of this test, test_align_is_optimal_stored and test_align_edges: 7.3e-12 on the
    emulator and 7.3e-12 on the MI355X (the T = 2048 case; every returned path re-scores to the float64 optimum up to the
    rounding of the float64 sums themselves), against bounds of 1.5e-5 .. 3.9e-3."""
    torch.manual_seed(B * 100 + T)
    logits = torch.randn(B, T, V) * 2
    labels = torch.randint(1, V, (B, L))
    if B > 1 and L > 3:
        labels[1, L - 3:] = -1
    if L > 4:
        labels[0, 2] = labels[0, 1]  # repeated label -> mandatory blank
    in_lens = torch.full((B,), T, dtype=torch.int64)
    if B > 1:
        in_lens[1] = max(T - 7, 1)
    if B > 2:
        in_lens[2] = T - 11
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    ali, score = run_align(dev, logits, labels, in_lens, dtype=td)
    seen = logits.to(td).float()  # bf16: the float64 re-scoring starts from the rounded logits
    check_optimal(f"generated B={B} T={T} V={V} L={L} {dtype}", seen, labels, in_lens, ali, score)


def test_align_is_optimal_stored(dev):
    """The same criterion on the stored larger inputs ((T, L) = (300, 140), and (400, 64) with `randn * 4` logits, optimum about
    -2700), with the reference forced_align_batch's own float64 deficit from the golden file as deficit_ref."""
    for c in torch.load(GOLDEN)["optimal"]:
        T = c["T"]
        logits = c["logits"].transpose(0, 1)  # (1, T, V)
        labels, in_lens = c["y"].view(1, -1), torch.tensor([T])
        ali, score = run_align(dev, logits, labels, in_lens)
        check_optimal(f"stored T={T} L={c['L']} scale={c['scale']}", logits, labels, in_lens, ali, score,
                      deficit_ref=[float(c["deficit_ref"])])


def test_align_edges(dev):
    """No labels; labels that do not fit (3 frames for 9 labels; T = L with an adjacent repeat; no frames) next to utterances
    that do; ignore_id between valid ids; a blank id other than 0; Lmax = 256 refused before anything is launched."""
    torch.manual_seed(3)
    B, T, V, Lmax = 5, 12, 20, 9
    logits = torch.randn(B, T, V) * 2
    labels = torch.randint(1, V, (B, Lmax))
    labels[0] = -1  # L = 0
    labels[2] = torch.tensor([4, -1, 7, -1, -1, 7, 2, -1, 9])  # padded "anywhere": y = 4 7 7 2 9
    labels[3, 5:] = -1
    in_lens = torch.tensor([T, 3, T, T - 2, 0])  # row 1: 3 frames, 9 labels; row 4: no frames
    ali, score = run_align(dev, logits, labels, in_lens)
    ali, score = ali.cpu(), score.cpu()
    lp = torch.log_softmax(logits.double(), -1)
    assert (ali[0] == 0).all() and abs(float(score[0]) - float(lp[0, :, 0].sum())) < 1e-4
    for b in (1, 4):
        assert score[b] == float("-inf") and (ali[b] == -1).all()
    keep = [0, 2, 3]
    check_optimal("edges", logits[keep], labels[keep], in_lens[keep], ali[keep], score[keep])
    assert collapse(ali[2].tolist()) == [4, 7, 7, 2, 9]

    # T = L: feasible only without an adjacent repeat, and then without a single blank
    logits = torch.randn(2, 5, V) * 2
    labels = torch.tensor([[3, 3, 4, 5, 6], [3, 4, 5, 6, 7]])
    in_lens = torch.tensor([5, 5])
    ali, score = run_align(dev, logits, labels, in_lens)
    assert score[0].item() == float("-inf") and (ali[0].cpu() == -1).all()
    assert ali[1].cpu().tolist() == [3, 4, 5, 6, 7]
    check_optimal("T=L", logits[1:], labels[1:], in_lens[1:], ali[1:], score[1:])

    # blank = 2, ignore_id = -5
    logits = torch.randn(2, 30, V) * 2
    labels = torch.tensor([[1, 1, 3, 0, -5, 7], [5, -5, -5, 5, 6, 0]])
    in_lens = torch.tensor([30, 21])
    ali, score = run_align(dev, logits, labels, in_lens, blank=2, ignore_id=-5)
    check_optimal("blank=2", logits, labels, in_lens, ali, score, blank=2, ignore_id=-5)

    with pytest.raises(_lib.AvsrLibraryError, match="at most 255 labels"):
        run_align(dev, torch.randn(1, 8, V), torch.randint(1, V, (1, 256)), torch.tensor([8]))

    # functional.ctc_align: [..., :V] view of a pitched buffer, inputs that require grad, no graph
    buf = torch.randn(2, 30, 24).to(dev).requires_grad_()
    a2, s2 = AF.ctc_align(buf[..., :V], labels.to(dev), in_lens.to(dev), blank=2, ignore_id=-5)
    assert not a2.requires_grad and not s2.requires_grad and a2.device.type == dev.type
    check_optimal("functional", buf.detach().cpu()[..., :V], labels, in_lens, a2, s2, blank=2, ignore_id=-5)


def test_word_timestamps():
    toks = ["<blank>", "▁he", "llo", "▁wor", "ld", "▁a", "<eos>"]
    #      frame: 0  1  2  3  4  5  6  7  8  9 10 11 12 13
    ali = [0, 1, 1, 0, 2, 3, 3, 3, 4, 0, 0, 5, 0, 5]
    assert alignment.segments(ali) == [(1, 1, 2), (2, 4, 4), (3, 5, 7), (4, 8, 8), (5, 11, 11), (5, 13, 13)]  # blank-separated repeat: two
    words = alignment.word_timestamps(ali, toks)
    assert [w["word"] for w in words] == ["hello", "world", "a", "a"]
    assert words[0]["start"] == pytest.approx(0.04) and words[0]["end"] == pytest.approx(5 * 0.04)
    assert words[1]["start"] == pytest.approx(5 * 0.04) and words[1]["end"] == pytest.approx(9 * 0.04)
    assert words[2] == {"word": "a", "start": pytest.approx(11 * 0.04), "end": pytest.approx(12 * 0.04)}
    assert words[3]["start"] == pytest.approx(13 * 0.04) and words[3]["end"] == pytest.approx(14 * 0.04)
    assert alignment.word_timestamps(ali, toks, frame_seconds=0.5)[1]["end"] == 4.5
    # tensors and numpy arrays, frames beyond the utterance (ignore_id), a leading piece without the word mark
    assert alignment.segments(torch.tensor([2, 2, 0, 1, -1, -1], dtype=torch.int32)) == [(2, 0, 1), (1, 3, 3)]
    assert [w["word"] for w in alignment.word_timestamps(np.array([2, 2, 0, 1, -1]), toks)] == ["llo", "he"]
    assert alignment.segments([]) == [] and alignment.word_timestamps([], toks) == []
    assert alignment.segments([0, 0, 0]) == [] and alignment.word_timestamps([0, 0], toks) == []


def _tiny_module(dev, odim=30):
    import lightning as LM
    from test_train_eval_loops import small_e2e

    mod = LM.ModelModule.__new__(LM.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.modality = "video"
    mod.model = small_e2e(odim).to(dev).eval()
    # an untrained model decodes "<blank>" or nothing: keep the decoder off the blank id and the CTC head off all-blank paths, so
    # that the hypotheses are six to eight words on as many frames
    with torch.no_grad():
        mod.model.decoder.output_layer.bias[0] = -1000.0
        mod.model.ctc.ctc_lo.bias[0] = -20.0
    AF.invalidate_weight_cache()

    class Text:
        token_list = ["<blank>"] + [f"▁w{i}" for i in range(odim - 2)] + ["<eos>"]

        def post_process(self, ids):
            ids = ids[ids != -1]
            return "".join(self.token_list[int(i)] for i in ids).replace("▁", " ").strip().replace("<eos>", "")

    mod.text_transform = Text()
    mod.token_list = Text.token_list
    return mod, Text


def test_eval_timestamps(dev, tmp_path, monkeypatch):
    """run_test_loop with timestamps=PATH writes one JSON line per utterance whose words concatenate to the hypothesis, with
    non-decreasing times within the utterance's T * 0.04 s; WER and transcripts are those of a run without it, for
    decode_workers 1 and 2; without it ops.ctc_align is never called."""
    import eval as EV
    import lightning as LM
    from datamodule.av_dataset import SyntheticAVDataset

    odim, lengths = 30, [6, 8, 7]
    mod, Text = _tiny_module(dev, odim)
    monkeypatch.setattr(LM, "TextTransform", Text)  # on_test_epoch_start re-creates the transform
    loader = torch.utils.data.DataLoader(SyntheticAVDataset(3, "video", odim=odim, seed=2, lengths=lengths), batch_size=None)
    hyps = []

    def boom(*a, **k):
        raise AssertionError("ctc_align called without --timestamps")

    with monkeypatch.context() as mp:
        mp.setattr(ops, "ctc_align", boom)
        plain = [EV.run_test_loop(mod, loader, dev, decode_workers=w) for w in (1, 2)]
    assert plain[0] == plain[1]
    for w in (1, 2):
        path = tmp_path / f"ts{w}.jsonl"
        seen = []
        wer = EV.run_test_loop(mod, loader, dev, decode_workers=w, timestamps=str(path), log=lambda i, d, n: seen.append((i, d, n)))
        assert wer == plain[0] and len(seen) == 3
        assert mod.timestamp_records is None
        recs = [json.loads(line) for line in open(path, encoding="utf8")]
        assert [r["utt"] for r in recs] == [0, 1, 2]
        hyps.append([r["hyp"] for r in recs])
        for r, T in zip(recs, lengths):
            assert r["words"] and len(r["words"]) >= 3 and r["score"] < 0
            assert " ".join(x["word"] for x in r["words"]) == r["hyp"]
            times = [v for x in r["words"] for v in (x["start"], x["end"])]
            assert times == sorted(times) and times[0] >= 0 and times[-1] <= T * 0.04 + 1e-9
        print(recs)
    assert hyps[0] == hyps[1]
    # the transcripts of the run with the flag are those of the run without it
    mod.on_test_epoch_start()
    with torch.no_grad():
        for sample, h in zip(loader, hyps[0]):
            assert mod._decode(sample["input"].to(dev)) == h
            # ModelModule.align: the same words from a second encoder pass over the sample
            words = mod.align(sample["input"].to(dev), mod._last_decoded[1])
            rec = mod._timestamp_record(*mod._last_decoded, h)
            assert words == rec["words"]
    # an empty hypothesis, or one that does not fit the frames: "words": null
    enc = mod._last_decoded[0]
    assert mod._timestamp_record(enc, torch.tensor([odim - 1]), "") == {"hyp": "", "score": None, "words": None}
    assert mod._timestamp_record(enc[:2], torch.tensor([3, 3, 4, odim - 1]), "x")["words"] is None
    AF.invalidate_weight_cache()
