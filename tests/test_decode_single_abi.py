"""The per-utterance entry points of csrc/decode.hip (avsr_beam_workspace_bytes / _begin / _step / _keep / _fetch_yseq: the binding
INTEGRATION.md documents for a caller that drives the search itself) against the group entry points run with a group of one
(BatchBeamSearch.forward_batch(batch=1)): the same ended hypotheses, and the same [K][8] records at every step, bit for bit.  The
driver below is the only python caller of the per-utterance entry points; the shapes are the smallest at which each piece of a
step can go wrong.  Kernels through the emulator (CPU suite) or on the MI355X (-m gpu)."""
import ctypes
import math

import numpy as np
import pytest
import torch
from test_context_bias import SMALL as BIAS_CASES
from test_context_bias import _case_bs as _bias_bs
from test_context_bias import _enc as _bias_enc
from test_decode_batch import GOLD_LM, GROUP_A, _bs, _enc, _group_bs, _precise, _same_as_single

from synth import synth_state_dict

from auto_avsr_amd import _lib, ops
from auto_avsr_amd.decode_native import NativeBeam, _f32, prepare_ctc, search_maxlen
from auto_avsr_amd.decoding import Hypothesis


def _drive(sess, x, maxlenratio=0.0):
    """One search of x on the session through the per-utterance entry points: the n-best list and the [K][8] records of every step."""
    bs = sess.bs
    dev, T, maxlen = x.device, x.shape[0], search_maxlen(x.shape[0], maxlenratio)
    sess._bind(dev, maxlen + 2)
    L = _lib.lib()
    logp, r_init = prepare_ctc(bs.part_scorers["ctc"], x)
    memory = _f32(x)
    nws = L.call("avsr_beam_workspace_bytes", sess.handle, T, maxlen)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    stream = ops._stream(memory)
    L.call("avsr_beam_begin", sess.handle, memory.data_ptr(), T, logp.data_ptr(), logp.stride(0), r_init.data_ptr(), ws.data_ptr(), nws,
           maxlen, stream)
    pin = dev.type == "cuda"
    host = torch.empty(bs.beam_size * 8, dtype=torch.float32, pin_memory=pin)
    host_np = host.numpy().reshape(-1, 8)
    yseq_host = torch.empty(bs.beam_size * (maxlen + 2), dtype=torch.int64, pin_memory=pin)
    n_out = ctypes.c_int(0)
    n_ptr = ctypes.cast(ctypes.pointer(n_out), ctypes.c_void_p)
    names = ["decoder"] + [k for k in ("lm", "bias", "length_bonus") if k in bs.full_scorers] + ["ctc"]
    col = {"decoder": 3, "ctc": 4, "length_bonus": 5, "lm": 6, "bias": 7}
    eos = bs.eos
    ended, records, best, best_len = [], [], -math.inf, {}

    def fetch():
        ldy, Lc = ctypes.c_int(0), ctypes.c_int(0)
        L.call("avsr_beam_fetch_yseq", sess.handle, yseq_host.data_ptr(), ctypes.cast(ctypes.pointer(ldy), ctypes.c_void_p),
               ctypes.cast(ctypes.pointer(Lc), ctypes.c_void_p), stream)
        return yseq_host.numpy(), ldy.value, Lc.value

    def end(row, ys, forced):
        nonlocal best
        ys = list(ys) + ([eos] if forced else [])
        sc = float(row[2])
        ended.append(Hypothesis(yseq=torch.tensor(ys, dtype=torch.int64), score=sc, scores={k: float(row[col[k]]) for k in names}, states={}))
        best = max(best, sc)
        best_len[len(ys)] = max(best_len.get(len(ys), -math.inf), sc)

    for i in range(maxlen):
        L.call("avsr_beam_step", sess.handle, host.data_ptr(), n_ptr, stream)
        K = n_out.value
        out = host_np[:K]
        records.append(out.copy())
        tok = out[:, 0].astype(np.int64)
        if i == maxlen - 1:  # force an end so that at least one hypothesis finishes (beam_search.py:430-436)
            ys, ldy, Lc = fetch()
            for b in range(K):
                end(out[b], ys[b * ldy: b * ldy + Lc], True)
            n_alive = 0
        else:
            is_eos = tok == eos
            n_alive = K
            if is_eos.any():
                ys, ldy, Lc = fetch()
                for b in np.nonzero(is_eos)[0].tolist():
                    end(out[b], ys[b * ldy: b * ldy + Lc], False)
                keep = np.nonzero(~is_eos)[0].astype(np.int32)
                n_alive = int(keep.shape[0])
                L.call("avsr_beam_keep", sess.handle, keep.ctypes.data, n_alive, stream)
        if maxlenratio == 0.0 and ended and NativeBeam._end_detect(best, best_len, i):
            break
        if n_alive == 0:
            break
    return sorted(ended, key=lambda h: float(h.score), reverse=True), records


def _group_of_one(bs, x, maxlenratio, monkeypatch):
    """forward_batch(batch=1) of x: its n-best list and the records every avsr_beam_step_batch call left in the host buffer."""
    records = []
    L = _lib.lib()
    real = L.call

    def spy(name, *args):
        rc = real(name, *args)
        if name == "avsr_beam_step_batch":  # (handle, host_out, n_out [U], stream): a running utterance gets `beam` records
            rows = (ctypes.c_float * (bs.beam_size * 8)).from_address(int(args[1]))
            records.append(np.ctypeslib.as_array(rows).reshape(-1, 8).copy())
        return rc

    with monkeypatch.context() as mp:
        mp.setattr(L, "call", spy)
        nbest = bs.forward_batch([x], batch=1, maxlenratio=maxlenratio)[0]
    return nbest, records


def _check(bs, x, maxlenratio, monkeypatch, expect_keep=False):
    with _precise():
        want, want_rec = _group_of_one(bs, x, maxlenratio, monkeypatch)
        assert bs._native
        got, got_rec = _drive(bs._native, x, maxlenratio)
    assert len(got) == len(want) >= 1
    _same_as_single([got], [want], min_live=1)
    for a, b in zip(got, want):  # (the ruled-out hypotheses too: same tokens in the same order)
        assert a.yseq.tolist() == b.yseq.tolist()
    assert len(got_rec) == len(want_rec) >= 1
    same = [a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got_rec, want_rec)]
    print(f"\nsteps {len(got_rec)}, ended {len(got)}, records bit-identical at {sum(same)} of {len(same)} steps")
    assert all(same)
    if expect_keep:  # some hypothesis ended before the last step and the search went on: avsr_beam_keep ran
        assert any((r[:, 0] == bs.eos).any() and not (r[:, 0] == bs.eos).all() for r in got_rec[:-1])
    return got


@pytest.mark.parametrize("beam,T,maxlenratio", [(2, 1, 0.0), (2, 9, 0.0), (4, 2, 0.0), (5, 9, -1), (4, 70, -6), (4, 300, -3)])
def test_single_abi_equals_group_of_one(dev, monkeypatch, beam, T, maxlenratio):
    """One frame with the smallest beam (pre-beam 3); nine frames with it (with these weights every hypothesis ends at the forced end
    of the last step: the hypotheses that leave the beam earlier are test_single_abi_keep's); two frames; a forced end at the first
    step; source attention with 8 waves (T = 70) and with 16 (T = 300)."""
    bs = _bs(dev, 3, 30, beam, 0.1, 0.0)
    _check(bs, _enc(dev, 3, T), maxlenratio, monkeypatch)


def test_single_abi_keep(dev, monkeypatch):
    """Group A's search (vocabulary 40, beam 5) on its nine-frame utterance: one hypothesis ends on <eos> at the seventh step and four
    at the eighth, so avsr_beam_keep takes rows off the beam twice and the steps after it run on 4 and on 1 hypotheses."""
    bs = _group_bs(dev, GROUP_A)
    got = _check(bs, _enc(dev, GROUP_A["seed"], 9), 0.0, monkeypatch, expect_keep=True)
    assert len(got) > bs.beam_size


def test_single_abi_with_language_model(dev, monkeypatch):
    """The smallest case of golden_lm_v1.pt: the language model's pass and its column of the records."""
    from auto_avsr_amd.lm import TransformerLM

    case = min(GOLD_LM, key=lambda c: (c["odim"], c["T"], c["beam"], c["lm_weight"]))
    E, D, H, FF, NL = case["lm_dims"]
    lm = TransformerLM(case["odim"], embed_unit=E, att_unit=D, head=H, unit=FF, layer=NL)
    lm.load_state_dict(synth_state_dict(lm.state_dict(), case["seed"] + 2))
    bs = _bs(dev, case["seed"], case["odim"], case["beam"], case["ctc_weight"], case["penalty"], lm=lm.to(dev), lm_weight=case["lm_weight"],
             D=case["D"])
    x = (torch.randn(case["T"], case["D"], generator=torch.Generator().manual_seed(500 + case["seed"])) * 1.5).to(dev)
    got = _check(bs, x, 0.0, monkeypatch)
    assert "lm" in bs.full_scorers and any(h.scores["lm"] != 0 for h in got)


def test_single_abi_with_bias_list(dev, monkeypatch):
    """The smallest case of golden_bias_v1.pt: avsr_beam_begin takes over the list bound by avsr_beam_set_bias; the node and gain
    columns of the selection reach the records."""
    case = BIAS_CASES[0]
    bs = _bias_bs(dev, case)
    got = _check(bs, _bias_enc(case, dev), 0.0, monkeypatch)
    assert bs._native.bias_key is not None and any(h.scores["bias"] != 0 for h in got)


def test_single_abi_session_reuse(dev, monkeypatch):
    """Two searches back to back on one session, the second shorter than the first: avsr_beam_begin carves the workspace anew and
    resets the beam, whatever the session ran before (a group of one between them)."""
    bs = _bs(dev, 3, 30, 4, 0.1, 0.0)
    long, short = _enc(dev, 3, 9), _enc(dev, 3, 2)
    first = _check(bs, long, 0.0, monkeypatch)
    sess = bs._native
    _check(bs, short, 0.0, monkeypatch)
    assert bs._native is sess
    with _precise():
        again, _ = _drive(sess, short, 0.0)
        after, _ = _drive(sess, long, 0.0)
    _same_as_single([after], [first], min_live=1)
    assert [h.yseq.tolist() for h in after] == [h.yseq.tolist() for h in first] and len(again) >= 1
