"""Out-of-bounds detector (as tests/test_lm_guard_pages.py: the operand ENDS at an unmapped page and BEGINS right after one; an access
past either end is a SIGSEGV of a child process) for the batched beam search: the one uint8 workspace of a group -- tables for U * beam
packed rows, the frames of all utterances behind one another, with a language model its caches and activations at the end -- is exactly
`avsr_beam_batch_workspace_bytes` long."""
import multiprocessing as mp
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(emu_path, with_lm, q):
    import ctypes
    import mmap

    import torch

    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from auto_avsr_amd import _lib

    _lib._install_for_tests(emu_path)
    libc = ctypes.CDLL(None, use_errno=True)
    PAGE = 4096
    keep = []

    def guarded(t):
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
        keep.append((m, buf))
        return g

    from synth import synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import nets
    from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus
    from auto_avsr_amd.lm import TransformerLM

    torch.manual_seed(3)
    odim, beam = 41, 4
    dec = nets.TransformerDecoder(odim, attention_dim=128, attention_heads=2, linear_units=256, num_blocks=1).eval()
    ctc = nets.CTC(odim, 128, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), 1))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), 2))
    lm = None
    if with_lm:
        lm = TransformerLM(odim, embed_unit=32, att_unit=64, head=1, unit=128, layer=2)
        lm.load_state_dict(synth_state_dict(lm.state_dict(), 3))
    bs = BatchBeamSearch(beam_size=beam, vocab_size=odim, weights={"decoder": 0.9, "ctc": 0.1, "lm": 0.3 if with_lm else 0.0, "length_bonus": 0.0},
                         scorers={"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": lm, "length_bonus": LengthBonus(odim)},
                         sos=odim - 1, eos=odim - 1, token_list=None, pre_beam_score_key="decoder")
    empty, seen = torch.empty, []

    def guarded_empty(*a, **k):  # the group's workspace (decode_native.NativeBeam.search_group: the one uint8 allocation)
        t = empty(*a, **k)
        if k.get("dtype") is torch.uint8 and t.dim() == 1 and not k.get("pin_memory"):
            seen.append(t.numel())
            return guarded(t)
        return t

    xs = [torch.randn(T, 128) * 1.5 for T in (9, 1, 12)]
    torch.empty = guarded_empty
    AF.set_precise(True)
    try:
        out = bs.forward_batch(xs, batch=3)
    finally:
        torch.empty = empty
        AF.set_precise(False)
    assert bs._native and ("lm" in bs.full_scorers) == with_lm
    assert seen == [bs._native.group_workspace_bytes([1, 9, 12], 12)]  # (sorted by length: one group, one allocation of that size)
    q.put([len(nbest) for nbest in out])


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
def test_batched_search_stays_inside_its_workspace(emu_lib_path, with_lm):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, with_lm, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    counts = q.get(timeout=5)
    assert len(counts) == 3 and min(counts) >= 1
