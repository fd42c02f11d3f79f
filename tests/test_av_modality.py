"""--modality audiovisual end to end: the command lines, the audio-visual items of the datasets and of synthetic.make_batch,
ModelModule around a small E2EAV through eval.py's test loop with every decoding flag, the native beam search on the fused
memory, the two single-modality checkpoints of --pretrained-video-path / --pretrained-audio-path, and the native training loop
(eager everywhere; replayed as a hipGraph on the MI355X).  Small model instances; kernels through the emulator or the MI355X."""
import json
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

from auto_avsr_amd import functional as AF  # noqa: E402

ODIM = 30


def small_av(odim=ODIM):
    from auto_avsr_amd.e2e_av import E2EAV

    torch.manual_seed(0)
    return E2EAV(odim, adim=128, aheads=2, eunits=64, elayers=1, dunits=64, dlayers=1, cnn_module_kernel=7, fusion_hdim=160)


def small_e2e(modality, odim=ODIM, adim=128):
    from auto_avsr_amd.e2e import E2E

    return E2E(odim, modality, adim=adim, aheads=2, eunits=64, elayers=1, dunits=64, dlayers=1, cnn_module_kernel=7)


class _Text:
    token_list = ["<blank>"] + [f"▁w{i}" for i in range(ODIM - 2)] + ["<eos>"]

    def post_process(self, ids):
        ids = ids[ids != -1]
        return "".join(self.token_list[int(i)] for i in ids).replace("▁", " ").strip().replace("<eos>", "")


def _module(model, **args):
    import lightning as LM

    mod = LM.ModelModule.__new__(LM.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.modality = "audiovisual"
    mod.model = model
    mod.text_transform = _Text()
    mod.token_list = _Text.token_list
    if args:
        mod.args = types.SimpleNamespace(**args)
    return mod


# ------------------------------------------------------------------------------------------------ command lines
def test_parse_args_audiovisual():
    import eval as EV
    import train as TR

    assert EV.parse_args(["--modality", "audiovisual"]).modality == "audiovisual"
    assert TR.parse_args(["--modality", "audiovisual", "--synthetic"]).modality == "audiovisual"
    a = EV.parse_args(["--encode-batch", "4", "--modality", "audiovisual", "--pretrained-video-path", "v.pth",
                       "--pretrained-audio-path", "a.pth"])
    assert a.encode_batch == 4 and a.pretrained_video_path == "v.pth" and a.pretrained_audio_path == "a.pth"
    t = TR.parse_args(["--modality", "audiovisual", "--pretrained-audio-path", "a.pth"])
    assert t.pretrained_audio_path == "a.pth" and t.pretrained_video_path is None
    assert EV.parse_args(["--modality", "audiovisual", "--decode-mode", "rescore", "--encode-batch", "2", "--timestamps", "t.jsonl"])
    # the refusals parse_args already had still hold
    for argv in (["--encode-batch", "4", "--modality", "audio"],
                 ["--modality", "audiovisual", "--decode-batch", "2", "--decode-workers", "2"],
                 ["--modality", "audiovisual", "--decode-batch", "2", "--decode-mode", "rescore"],
                 ["--modality", "audiovisual", "--bias-weight", "1.0", "--decode-mode", "rescore"],
                 ["--modality", "audiovisual", "--ngram-weight", "0.5", "--decode-mode", "rescore"],
                 ["--modality", "video", "--pretrained-video-path", "v.pth"],
                 ["--modality", "both"]):
        with pytest.raises(SystemExit):
            EV.parse_args(argv)


# ------------------------------------------------------------------------------------------------ items and batches
def test_synthetic_av_items():
    from datamodule.av_dataset import SyntheticAVDataset, cut_or_pad

    lens = [6, 3]
    ds = SyntheticAVDataset(2, "audiovisual", odim=ODIM, seed=2, lengths=lens)
    for i, t in enumerate(lens):
        item = ds[i]
        assert set(item) == {"video", "audio", "target"}
        assert item["video"].shape == (t, 1, 88, 88) and item["audio"].shape == (640 * t, 1)
        assert item["target"].shape == (max(1, round(t / 6.5)),)
        # the video is the video-only item of the same seed
        assert torch.equal(item["video"], SyntheticAVDataset(2, "video", odim=ODIM, seed=2, lengths=lens)[i]["input"])
    w = torch.arange(5.0).unsqueeze(1)
    assert torch.equal(cut_or_pad(w, 3), w[:3])
    assert torch.equal(cut_or_pad(w, 8)[:5], w) and cut_or_pad(w, 8)[5:].abs().max() == 0 and cut_or_pad(w, 8).shape == (8, 1)


def test_make_batch_audiovisual(dev):
    from auto_avsr_amd.synthetic import make_batch

    lengths = [5, 3, 4]
    for on_device in (False, True):
        (v, a), lens, y, frames = make_batch(lengths, [0, 1, 2], "audiovisual", ODIM, seed=3, device=dev, on_device=on_device)
        assert v.shape == (3, 5, 1, 88, 88) and a.shape == (3, 640 * 5, 1) and frames == 12
        assert v.device.type == a.device.type == dev.type
        assert lens.tolist() == lengths, "lengths in frames"
        xv, lv, yv, _ = make_batch(lengths, [0, 1, 2], "video", ODIM, seed=3, device=dev, on_device=on_device)
        assert torch.equal(y, yv) and torch.equal(lens, lv), "the same lengths and labels"
        for b, t in enumerate(lengths):
            assert v[b, t:].abs().sum() == 0 and a[b, 640 * t:].abs().sum() == 0, "zero padding"
            assert v[b, :t].abs().sum() > 0 and a[b, :640 * t].abs().sum() > 0


# ------------------------------------------------------------------------------------------------ the test loop
def test_eval_loop_audiovisual(dev, tmp_path):
    import eval as EV
    import lightning as LM
    from datamodule.av_dataset import SyntheticAVDataset

    AF.invalidate_weight_cache()
    model = small_av().to(dev).eval()
    loader = torch.utils.data.DataLoader(SyntheticAVDataset(3, "audiovisual", odim=ODIM, seed=2, lengths=[2, 4, 3]), batch_size=None)
    keep, LM.TextTransform = LM.TextTransform, _Text  # on_test_epoch_start re-creates the transform
    runs = {}
    try:
        with AF.precise():
            for name, kw, args in (("plain", {}, {}), ("workers", dict(decode_workers=2), {}), ("batch", dict(decode_batch=2), {}),
                                   ("enc", dict(encode_batch=2), {}), ("rescore", {}, dict(decode_mode="rescore"))):
                mod = _module(model, **args)
                seen = []
                ts = str(tmp_path / (name + ".jsonl"))
                wer = EV.run_test_loop(mod, loader, dev, log=lambda i, d, n: seen.append((i, d, n)), timestamps=ts, **kw)
                with open(ts, encoding="utf8") as f:
                    runs[name] = (seen, wer, [json.loads(line) for line in f])
    finally:
        LM.TextTransform = keep
        AF.invalidate_weight_cache()
    seen, wer, recs = runs["plain"]
    assert len(seen) == 3 and len(recs) == 3 and 0.0 <= wer
    assert seen[-1][2] == sum(max(1, round(t / 6.5)) for t in (2, 4, 3))
    for r in recs:  # --timestamps: one record per utterance, words inside the utterance
        assert set(r) == {"utt", "hyp", "score", "words"}
        for w in r["words"] or []:
            assert 0.0 <= w["start"] <= w["end"] <= 4 * 0.04 + 1e-9
    for name in ("workers", "batch", "enc"):  # the same search, the same (precise) encodings: the same hypotheses
        assert runs[name][0] == seen and runs[name][1] == wer, name
        assert [r["hyp"] for r in runs[name][2]] == [r["hyp"] for r in recs], name
    assert len(runs["rescore"][0]) == 3 and len(runs["rescore"][2]) == 3 and 0.0 <= runs["rescore"][1]


def test_decode_accepts_dict_and_pair(dev):
    from datamodule.av_dataset import SyntheticAVDataset

    AF.invalidate_weight_cache()
    mod = _module(small_av().to(dev).eval())
    item = {k: v.to(dev) for k, v in SyntheticAVDataset(1, "audiovisual", odim=ODIM, seed=5, lengths=[3])[0].items()}
    with AF.precise(), torch.no_grad():
        a = mod(item)
        b = mod((item["video"], item["audio"]))
        ids = mod._last_decoded[1]
        words = mod.align(item, ids)
    AF.invalidate_weight_cache()
    assert a == b
    assert words is None or all(0.0 <= w["start"] <= w["end"] for w in words)


def test_native_search_on_fused_memory_equals_python_step(dev):
    """tests/test_decoding.py::test_native_beam_search_equals_python_step, on the fused memory of the audio-visual model."""
    import lightning as LM
    from auto_avsr_amd import decoding
    from datamodule.av_dataset import SyntheticAVDataset

    AF.invalidate_weight_cache()
    model = small_av().to(dev).eval()
    mod = _module(model)
    item = SyntheticAVDataset(1, "audiovisual", odim=ODIM, seed=4, lengths=[6])[0]
    was = decoding.NATIVE_BEAM
    out = {}
    try:
        with AF.precise(), torch.no_grad():
            mem = mod._encode_one({k: v.to(dev) for k, v in item.items()})
            for native in (True, False):
                decoding.NATIVE_BEAM = native
                bs = LM.get_beam_search_decoder(model, _Text.token_list, beam_size=5)
                out[native] = bs(mem, maxlenratio=-4)
                assert bool(bs._native) == native  # the path asked for is the one that ran
    finally:
        decoding.NATIVE_BEAM = was
        AF.invalidate_weight_cache()
    a, b = out[True], out[False]
    assert len(a) == len(b) and len(a) >= 1
    live = 0
    for x, y in zip(a, b):
        x, y = x.asdict(), y.asdict()
        if y["score"] < -1e8:
            assert x["score"] < -1e8
            continue
        live += 1
        assert x["yseq"] == y["yseq"]
        assert abs(x["score"] - y["score"]) < 1e-3 * max(1.0, abs(y["score"]))
        assert set(x["scores"]) == set(y["scores"])
        for k, v in y["scores"].items():
            assert abs(x["scores"][k] - v) < 1e-3 * max(1.0, abs(v)), k
    assert live >= 3


# ------------------------------------------------------------------------------------------------ checkpoints
def test_pretrained_video_and_audio_paths(tmp_path):
    import lightning as LM

    torch.manual_seed(1)
    v, a = small_e2e("video"), small_e2e("audio")
    vp, ap = str(tmp_path / "v.pth"), str(tmp_path / "a.pth")
    torch.save(v.state_dict(), vp)
    torch.save(a.state_dict(), ap)
    m = small_av()
    fusion = {k: t.clone() for k, t in m.fusion.state_dict().items()}
    LM.load_pretrained(m, types.SimpleNamespace(modality="audiovisual", pretrained_video_path=vp, pretrained_audio_path=ap))
    sd, vs, as_ = m.state_dict(), v.state_dict(), a.state_dict()
    n = 0
    for k, t in vs.items():
        if k.split(".")[0] in ("frontend", "proj_encoder", "encoder", "decoder", "ctc"):
            assert torch.equal(sd[k], t), k  # both given: the heads come from the video checkpoint
            n += 1
    for k, t in as_.items():
        if k.split(".")[0] in ("frontend", "proj_encoder", "encoder"):
            assert torch.equal(sd["aux_" + k], t), k
            n += 1
    assert n > 100
    assert not torch.equal(vs["decoder.embed.0.weight"], as_["decoder.embed.0.weight"])
    assert all(torch.equal(m.fusion.state_dict()[k], t) for k, t in fusion.items())
    # the audio checkpoint alone: its stack, and its heads
    m2 = small_av()
    before = {k: t.clone() for k, t in m2.state_dict().items()}
    LM.load_pretrained(m2, types.SimpleNamespace(modality="audiovisual", pretrained_video_path=None, pretrained_audio_path=ap))
    sd2 = m2.state_dict()
    assert torch.equal(sd2["aux_proj_encoder.weight"], as_["proj_encoder.weight"])
    assert torch.equal(sd2["decoder.embed.0.weight"], as_["decoder.embed.0.weight"])
    assert torch.equal(sd2["proj_encoder.weight"], before["proj_encoder.weight"])
    # a shape mismatch names the key
    torch.save(small_e2e("audio", adim=64).state_dict(), ap)
    with pytest.raises(ValueError, match="proj_encoder|weight"):
        LM.load_pretrained(small_av(), types.SimpleNamespace(modality="audiovisual", pretrained_video_path=None, pretrained_audio_path=ap))


def test_model_module_builds_e2eav(monkeypatch):
    import lightning as LM
    from auto_avsr_amd import e2e_av

    built = {}

    class Stub(torch.nn.Module):
        def __init__(self, odim, ctc_weight=0.1):
            super().__init__()
            built["odim"], built["ctc_weight"] = odim, ctc_weight

    monkeypatch.setattr(e2e_av, "E2EAV", Stub)
    monkeypatch.setattr(LM, "TextTransform", _Text)
    mod = LM.ModelModule(types.SimpleNamespace(modality="audiovisual", ctc_weight=0.3))
    assert isinstance(mod.model, Stub) and built == {"odim": ODIM, "ctc_weight": 0.3}


# ------------------------------------------------------------------------------------------------ training
def _train_args(**kw):
    a = types.SimpleNamespace(modality="audiovisual", max_frames=8, train_num_buckets=4, lr=1e-3, weight_decay=0.03, warmup_epochs=1,
                              max_epochs=50, exp_dir=None, exp_name="run", ckpt_path=None, steps=None, val_batches=1,
                              synthetic_utterances=2, log_every=1)
    a.__dict__.update(kw)
    return a


def _no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def test_native_stepper_audiovisual_repeated_batch(dev):
    """The whole native step (forward, backward, clip, AdamW, schedule) on the (video, audio) pair, the same batch again and again:
    finite losses that do not rise.  On the MI355X the shape is captured on its second visit and replayed from then on."""
    from auto_avsr_amd import train_native as TN
    from auto_avsr_amd.synthetic import make_batch

    AF.invalidate_weight_cache()
    m = _no_dropout(small_av()).to(dev).train()
    gpu = dev.type == "cuda"
    # (the emulator is too slow for more than a few frames; on the GPU the lengths of test_train_eval_loops.py's graph tests)
    x, lens, y, _ = make_batch([12, 14] if gpu else [3, 2], [0, 1], "audiovisual", ODIM, seed=1, device=dev)
    old = AF._save_mode()
    ns = None
    try:
        AF.set_mode("mixed" if gpu else "precise")
        ns = TN.NativeStepper(m, _train_args(no_graph=not gpu), dev, 0, 1, steps_per_epoch=2, log=print)
        losses = []
        for _ in range(5 if gpu else 3):
            out = ns(x, lens, y)
            losses.append(float(out[0]))
        stats = dict(ns.stats)
    finally:
        if ns is not None:
            ns.close()
        AF._restore_mode(old)
        AF.invalidate_weight_cache()
    print("losses", losses, stats)
    assert all(l == l and abs(l) != float("inf") for l in losses)
    assert all(b <= a for a, b in zip(losses, losses[1:])), losses
    if gpu:
        assert stats["captured"] == 1 and stats["replayed"] > 0, stats
    else:
        assert stats["replayed"] == 0 and stats["eager"] == 3


def test_native_fit_audiovisual(dev, monkeypatch):
    """train.py --modality audiovisual --synthetic: the loop's own batch source and validation pass carry the pair."""
    import auto_avsr_amd.synthetic as S
    from auto_avsr_amd import train_native as TN

    monkeypatch.setattr(S, "utterance_lengths", lambda n=6, seed=42, lo=12, hi=400: torch.tensor([3, 4][:n]).numpy())
    AF.invalidate_weight_cache()
    m = _no_dropout(small_av()).to(dev).train()
    logs = []
    with AF.precise(dev.type == "cpu"):
        losses = TN.fit(m, _train_args(max_epochs=2, numerics=None if dev.type == "cpu" else "mixed"), dev, log=logs.append)
    AF.invalidate_weight_cache()
    assert len(losses) == 2 and all(l == l and abs(l) != float("inf") for l in losses)
    assert sum("validation" in s for s in logs) == 2
