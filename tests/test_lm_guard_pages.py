"""Out-of-bounds detector (as tests/test_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an access past
either end is a SIGSEGV of a child process) for the entry points language-model fusion adds: `avsr_decode_attention` on its own, and
a whole search with an LM attached whose session workspace -- decoder share, then the LM's caches, activations and log-probabilities,
the last of them ending within the 256 bytes of alignment slack before the guard -- is exactly `avsr_beam_workspace_bytes` long."""
import multiprocessing as mp
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(emu_path, case, q):
    import ctypes
    import mmap

    import torch

    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from auto_avsr_amd import _lib, ops

    _lib._install_for_tests(emu_path)
    libc = ctypes.CDLL(None, use_errno=True)
    PAGE = 4096
    keep = []

    def guarded(t):
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        body = (nbytes + PAGE - 1) // PAGE * PAGE
        m = mmap.mmap(-1, body + 2 * PAGE)
        addr = ctypes.addressof(ctypes.c_char.from_buffer(m))
        for off in (0, PAGE + body):
            assert libc.mprotect(ctypes.c_void_p(addr + off), PAGE, 0) == 0
        start = PAGE + body - nbytes
        start -= start % 16
        buf = (ctypes.c_char * nbytes).from_address(addr + start)
        g = torch.frombuffer(buf, dtype=t.dtype, count=t.numel()).view(t.shape)
        g.copy_(t)
        keep.append((m, buf))
        return g

    torch.manual_seed(3)
    if case[0] == "attention":
        _, n, H, L = case
        D = 64 * H
        qv, kv = guarded(torch.randn(n, D)), guarded(torch.randn(n, L, 2 * D))
        out, anc = guarded(torch.zeros(n, D)), guarded(torch.zeros(n * L, dtype=torch.int32))
        ops.call("avsr_decode_attention", ops._ptr(qv), D, ops._ptr(kv), L * 2 * D, 2 * D, 0, D, n, H, L, ops._ptr(out), D, ops._ptr(anc), None)
        k, v = kv[..., :D].view(n, L, H, 64), kv[..., D:].view(n, L, H, 64)
        p = torch.softmax(torch.einsum("nhd,nlhd->nhl", qv.view(n, H, 64), k) / 8.0, -1)
        ref = torch.einsum("nhl,nlhd->nhd", p, v).reshape(n, D)
        q.put(float((out - ref).abs().max()))
        return
    from synth import synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import nets
    from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus
    from auto_avsr_amd.lm import TransformerLM

    _, odim, T, beam, FF = case
    dec = nets.TransformerDecoder(odim, attention_dim=128, attention_heads=2, linear_units=256, num_blocks=1).eval()
    ctc = nets.CTC(odim, 128, 0.1, reduce=True).eval()
    lm = TransformerLM(odim, embed_unit=32, att_unit=64, head=1, unit=FF, layer=2)
    dec.load_state_dict(synth_state_dict(dec.state_dict(), 1))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), 2))
    lm.load_state_dict(synth_state_dict(lm.state_dict(), 3))
    bs = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights={"decoder": 0.9, "ctc": 0.1, "lm": 0.3, "length_bonus": 0.0},
                         scorers={"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": lm, "length_bonus": LengthBonus(odim)},
                         sos=odim - 1, eos=odim - 1, token_list=None, pre_beam_score_key="decoder")
    empty, seen = torch.empty, []

    def guarded_empty(*a, **k):  # the session workspace (decode_native.NativeBeam.search: the one uint8 allocation)
        t = empty(*a, **k)
        if k.get("dtype") is torch.uint8 and t.dim() == 1 and not k.get("pin_memory"):
            seen.append(t.numel())
            return guarded(t)
        return t

    torch.empty = guarded_empty
    AF.set_precise(True)
    try:
        nbest = bs(torch.randn(T, 128) * 1.5)
    finally:
        torch.empty = empty
        AF.set_precise(False)
    assert bs._native and seen
    q.put(float(len(nbest)))


@pytest.mark.parametrize("case", [("attention", 5, 2, 7), ("attention", 3, 1, 70), ("attention", 2, 1, 300),
                                  ("search", 41, 9, 4, 128), ("search", 45, 12, 5, 1024)], ids=lambda c: "-".join(map(str, c)))
def test_lm_entry_points_stay_inside_their_operands(emu_lib_path, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, case, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    val = q.get(timeout=5)
    if case[0] == "attention":
        assert val < 1e-4
    else:
        assert val >= 1
