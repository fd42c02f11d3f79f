"""Length-exact batched encoder inference (eval.py --encode-batch): the inference conv-module middle with per-utterance lengths
(ops.convmod_dw_eval) against torch, ModelModule.encode_many against the oracle run on every utterance ALONE, and the evaluation
loop / flags around them.  The reference's masked padded forward is NOT what an utterance encodes alone: its depthwise convolution
reads the padded frames (conformer_encoder.py:30-35) -- the encoder test shows that leak on its own inputs."""
import functools
import json
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
from synth import synth_state_dict  # noqa: E402

import avsr_oracle as O  # noqa: E402
from auto_avsr_amd import functional as AF  # noqa: E402
from auto_avsr_amd import nets, ops  # noqa: E402
from auto_avsr_amd.e2e import E2E  # noqa: E402


# ------------------------------------------------------------------------------------------------ 1. the kernel
# C = 72: one full and one ragged 64-channel block; T = 37: one full and one ragged 32-frame time tile;
# lens: full / one past a tile edge / exactly a tile / shorter than K // 2
LENS = (37, 33, 32, 3)


@functools.lru_cache(maxsize=None)
def _kernel_case(K, C=72, B=4, T=37, lens=LENS):
    g = torch.Generator().manual_seed(100 + K + C)
    a = torch.randn(B, T, 2 * C, generator=g)
    w, bias = torch.randn(C, K, generator=g), torch.randn(C, generator=g)
    mean, invstd = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = []
    for b, n in enumerate(lens):  # every utterance alone, fp32
        c = F.conv1d(F.glu(a[b, :n], dim=-1).t().unsqueeze(0), w.unsqueeze(1), bias, padding=K // 2, groups=C)[0].t()
        ref.append(F.silu((c - mean) * invstd * gamma + beta))
    return dict(a=a, w=w, bias=bias, mean=mean, invstd=invstd, gamma=gamma, beta=beta, lens=lens, ref=ref, B=B, T=T, C=C, K=K)


def _run(c, dev, a=None, lens="case", T=None, in_dtype=torch.float32, out_dtype=None):
    a = c["a"] if a is None else a
    T = T or c["T"]
    lens = c["lens"] if isinstance(lens, str) else lens
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    p = [c[k].to(dev) for k in ("mean", "invstd", "gamma", "beta")]
    s = ops.convmod_dw_eval(a.to(in_dtype).contiguous().to(dev), c["w"].to(dev), c["bias"].to(dev), ld, c["B"], T, c["C"], c["K"], *p,
                            out_dtype=out_dtype)
    return s.cpu().view(c["B"], T, c["C"])


@pytest.mark.parametrize("K", [7, 31])
def test_convmod_dw_eval_f32(dev, K):
    c = _kernel_case(K)
    s = _run(c, dev)
    assert s.dtype == torch.float32
    for b, n in enumerate(c["lens"]):
        err = float((s[b, :n] - c["ref"][b]).abs().max())
        print(f"K={K} utt {b} len {n}: max abs error {err:.3e}")
        assert err < 1e-4
        assert n == c["T"] or s[b, n:].abs().max() == 0, "rows at or beyond lens[b] are exactly zero"
    # NaN in the padded rows of a reaches no valid row (select, not multiply by zero), and the padded rows still come out zero
    a_nan = c["a"].clone()
    for b, n in enumerate(c["lens"]):
        a_nan[b, n:] = float("nan")
    assert torch.equal(_run(c, dev, a=a_nan), s)
    # the same utterances padded to T = 70: no frame's arithmetic depends on T
    a70 = torch.randn(c["B"], 70, 2 * c["C"], generator=torch.Generator().manual_seed(3))
    a70[:, :c["T"]] = c["a"]
    s70 = _run(c, dev, a=a70, T=70)
    for b, n in enumerate(c["lens"]):
        assert torch.equal(s70[b, :n], s[b, :n]) and s70[b, n:].abs().max() == 0
    # lens = None is lens = [T] * B
    assert torch.equal(_run(c, dev, lens=None), _run(c, dev, lens=[c["T"]] * c["B"]))


@pytest.mark.parametrize("K", [7, 31])
def test_convmod_dw_eval_f16_out(dev, K):
    """The mixed mode's form: f32 chain, rounded to f16 once on the way out -- the f32 bound plus one f16 rounding."""
    c = _kernel_case(K)
    s = _run(c, dev, out_dtype=torch.float16)
    assert s.dtype == torch.float16
    for b, n in enumerate(c["lens"]):
        ref = c["ref"][b]
        over = (s[b, :n].float() - ref).abs() - (2.0 ** -11 * ref.abs() + 1e-4)
        print(f"K={K} utt {b} len {n}: worst excess over the bound {float(over.max()):.3e}")
        assert over.max() <= 0
        assert n == c["T"] or s[b, n:].abs().max() == 0


@pytest.mark.parametrize("K", [7, 31])
def test_convmod_dw_eval_bf16(dev, K):
    """bf16 -> bf16 against the stand-alone sequence (depthwise convolution with the folded GLU, then BatchNorm + SiLU) run on
    each utterance alone: within one bf16 step of the largest value."""
    c = _kernel_case(K)
    s = _run(c, dev, in_dtype=torch.bfloat16)
    assert s.dtype == torch.bfloat16
    p = [c[k].to(dev) for k in ("mean", "invstd", "gamma", "beta")]
    for b, n in enumerate(c["lens"]):
        ab = c["a"][b, :n].to(torch.bfloat16).contiguous().to(dev)
        cc = ops.dwconv(ab, c["w"].to(dev), c["bias"].to(dev), 1, n, c["C"], K, glu_in=True)
        ref = ops.bn_act_fwd(cc.view(n, c["C"]), None, *p, n, c["C"], 1).cpu().float()
        diff = float((s[b, :n].float() - ref).abs().max())
        print(f"K={K} utt {b} len {n}: max abs difference {diff:.3e} (bound {2.0 ** -7 * float(ref.abs().max()):.3e})")
        assert diff <= 2.0 ** -7 * float(ref.abs().max())
        assert n == c["T"] or s[b, n:].float().abs().max() == 0


def test_convmod_dw_eval_model_width(dev):
    c = _kernel_case(31, C=768, B=2, T=65, lens=(65, 40))
    s = _run(c, dev)
    for b, n in enumerate(c["lens"]):
        assert (s[b, :n] - c["ref"][b]).abs().max() < 1e-4
        assert n == c["T"] or s[b, n:].abs().max() == 0


# ------------------------------------------------------------------------------------------------ 2. the encoder
class _Text:
    def __init__(self, odim):
        self.token_list = ["<blank>"] + [f"▁w{i}" for i in range(odim - 2)] + ["<eos>"]

    def post_process(self, ids):
        ids = ids[ids != -1]
        return "".join(self.token_list[int(i)] for i in ids).replace("▁", " ").strip().replace("<eos>", "")


def _module(model, modality="video"):
    """A ModelModule around `model`, built the way tests/test_train_eval_loops.py::test_eval_wer_loop builds one."""
    import lightning as LM

    odim = model.odim if model is not None else 30
    mod = LM.ModelModule.__new__(LM.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.modality = modality
    mod.model = model
    mod.text_transform = _Text(odim)
    mod.token_list = mod.text_transform.token_list
    return mod


ENC_CASES = {7: (12, 5, 2), 31: (20, 9, 3)}


@functools.lru_cache(maxsize=None)
def _encoder_case(K):
    """Weights, utterances (lengths unsorted) and the oracle's encoding of every utterance alone -- computed once."""
    torch.manual_seed(0)
    m = E2E(40, "video", adim=128, aheads=2, eunits=256, elayers=2, dunits=256, dlayers=2, cnn_module_kernel=K)
    sd = synth_state_dict(m.state_dict(), 11)
    lens = ENC_CASES[K]
    lens = (lens[1], lens[0], lens[2])  # not sorted: encode_many has to restore the order
    g = torch.Generator().manual_seed(50 + K)
    samples = [torch.randn(n, 1, 88, 88, generator=g) for n in lens]
    refs = []
    with torch.no_grad():
        for x in samples:
            h = O.linear(sd, "proj_encoder.", O.video_frontend(sd, "frontend.", x[None], False))
            refs.append(O.conformer_encoder(sd, "encoder.", h, None, 2, False)[0])
    return sd, samples, refs


def _encoder_module(K, dev):
    sd, samples, refs = _encoder_case(K)
    AF.invalidate_weight_cache()
    torch.manual_seed(0)
    m = E2E(40, "video", adim=128, aheads=2, eunits=256, elayers=2, dunits=256, dlayers=2, cnn_module_kernel=K)
    m.load_state_dict(sd, strict=True)
    return _module(m.to(dev).eval()), [s.to(dev) for s in samples], refs


_FULL = {}  # (backend, K) -> encode_many(samples, batch=3) on the CPU: computed once, shared, never changed


def _full_encodings(mod, samples, K, dev):
    key = (dev.type, K)
    if key not in _FULL:
        with AF.precise(), torch.no_grad():
            encs = mod.encode_many(samples, batch=3)
            # each a contiguous tensor of its own, not a view into the padded batch
            assert all(e.is_contiguous() and e.untyped_storage().nbytes() == e.numel() * e.element_size() for e in encs)
            _FULL[key] = [e.cpu() for e in encs]
    return _FULL[key]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("K", [7, 31])
def test_encode_many_vs_oracle(dev, K):
    mod, samples, refs = _encoder_module(K, dev)
    encs = _full_encodings(mod, samples, K, dev)
    with AF.precise(), torch.no_grad():
        # the reference-shaped forward: zero-padded batch, attention key mask, no lengths for the convolution modules
        lens = [s.shape[0] for s in samples]
        x = torch.zeros(3, max(lens), 1, 88, 88, device=dev)
        for b, s in enumerate(samples):
            x[b, :lens[b]] = s
        mask = nets.non_pad_mask_device(torch.tensor(lens).to(dev), max(lens))
        leaky, _ = mod.model.encoder(mod.model.proj_encoder(mod.model.frontend(x)), mask)
    AF.invalidate_weight_cache()
    assert len(encs) == 3
    for i, (e, r) in enumerate(zip(encs, refs)):  # input order, whatever the sort did
        assert e.shape == r.shape
        print(f"K={K} utt {i} len {lens[i]}: rel L2 {_rel(e, r):.3e}")
        assert _rel(e, r) < 1e-3
    short = min(range(3), key=lambda i: lens[i])
    leak = _rel(leaky[short, :lens[short]].cpu(), refs[short])
    print(f"K={K}: masked padded forward without lengths, shortest utterance: rel L2 {leak:.3e}")
    assert leak > 1e-2, "these inputs cannot see the padded-frame leak"


def test_encode_many_grouping(dev):
    mod, samples, refs = _encoder_module(7, dev)
    full = _full_encodings(mod, samples, 7, dev)
    with AF.precise(), torch.no_grad():
        loop = []
        for s in samples:  # the existing per-utterance path (ModelModule._decode / align)
            e, _ = mod.model.encoder(mod.model.proj_encoder(mod.model.frontend(s.unsqueeze(0))), None)
            loop.append(e.squeeze(0))
        one = mod.encode_many(samples, batch=1)
        calls = []
        fe = mod.model.frontend.forward
        mod.model.frontend.forward = lambda x: (calls.append(tuple(x.shape[:2])), fe(x))[1]
        try:
            split = mod.encode_many(samples, batch=3, max_frames=24)  # 24 < 3 * Tmax = 36: {2, 5} and {12}
        finally:
            del mod.model.frontend.forward
    AF.invalidate_weight_cache()
    assert all(torch.equal(a, b) for a, b in zip(one, loop)), "batch=1 is the per-utterance loop, bit for bit"
    assert calls == [(2, 5), (1, 12)]
    for a, b in zip(split, full):
        assert _rel(a.cpu(), b) < 1e-5


# ------------------------------------------------------------------------------------------------ 3. loop and flags
def _loop_setup(dev):
    import lightning as LM
    from datamodule.av_dataset import SyntheticAVDataset

    odim = 30
    AF.invalidate_weight_cache()
    torch.manual_seed(0)
    model = E2E(odim, "video", adim=128, aheads=2, eunits=64, elayers=1, dunits=64, dlayers=1, cnn_module_kernel=7)
    mod = _module(model.to(dev).eval())
    ds = SyntheticAVDataset(3, "video", odim=odim, seed=2, lengths=[6, 8, 7])
    return LM, mod, torch.utils.data.DataLoader(ds, batch_size=None), odim


def test_eval_loop_encode_batch(dev, tmp_path):
    import eval as EV

    LM, mod, loader, odim = _loop_setup(dev)
    keep, LM.TextTransform = LM.TextTransform, lambda: _Text(odim)  # on_test_epoch_start re-creates the transform
    try:
        runs = {}
        for name, kw in (("plain", {}), ("enc", dict(encode_batch=2)), ("enc+workers", dict(encode_batch=2, decode_workers=2))):
            seen = []
            ts = str(tmp_path / (name + ".jsonl"))
            wer = EV.run_test_loop(mod, loader, dev, log=lambda i, d, n: seen.append((i, d, n)), timestamps=ts, **kw)
            with open(ts, encoding="utf8") as f:
                runs[name] = (seen, wer, [json.loads(line) for line in f])
    finally:
        LM.TextTransform = keep
        AF.invalidate_weight_cache()
    seen, wer, recs = runs["plain"]
    assert len(seen) == 3 and len(recs) == 3
    for name in ("enc", "enc+workers"):
        assert runs[name][0] == seen and runs[name][1] == wer, name
        assert [r["utt"] for r in runs[name][2]] == [0, 1, 2]
        assert [r["hyp"] for r in runs[name][2]] == [r["hyp"] for r in recs], name


def test_parse_args_encode_batch():
    import eval as EV

    assert EV.parse_args([]).encode_batch == 0
    assert EV.parse_args(["--encode-batch", "4", "--decode-mode", "rescore", "--decode-workers", "2"]).encode_batch == 4
    assert EV.parse_args(["--encode-batch", "1", "--modality", "audio"]).encode_batch == 1
    with pytest.raises(SystemExit):
        EV.parse_args(["--encode-batch", "-1"])
    with pytest.raises(SystemExit):
        EV.parse_args(["--encode-batch", "4", "--modality", "audio"])


def test_encode_many_refuses_audio():
    mod = _module(None, modality="audio")
    with pytest.raises(NotImplementedError, match="trunk"):
        mod.encode_many([torch.zeros(640, 1), torch.zeros(1280, 1)], batch=2)


def test_padded_lengths_is_evaluation_only(dev):
    conv = nets.ConvolutionModule(64, 7).to(dev).train()
    x = torch.randn(1, 4, 64, device=dev)
    with pytest.raises(AssertionError):
        with AF.padded_lengths([4], conv):
            pass
    with pytest.raises(AssertionError):
        with AF.padded_lengths([4]):
            conv(x)
    assert AF._state.get("pad_lens") is None  # the context is left behind clean
