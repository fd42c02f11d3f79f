"""Out-of-bounds detector (as tests/test_context_bias_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an
access past either end is a SIGSEGV of a child process) for n-gram shallow fusion: the six tables of the model and a session
workspace that is exactly `avsr_beam_workspace_bytes` / `avsr_beam_batch_workspace_bytes` long -- per-row nodes, sums, the selected
entries' values and nodes and the host copy's source are its last tables -- through one full search and one search of a group, on the
emulator."""
import multiprocessing as mp
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(emu_path, q):
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
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        body = (nbytes + PAGE - 1) // PAGE * PAGE
        m = mmap.mmap(-1, body + 2 * PAGE)
        addr = ctypes.addressof(ctypes.c_char.from_buffer(m))
        for off in (0, PAGE + body):
            assert libc.mprotect(ctypes.c_void_p(addr + off), PAGE, 0) == 0
        start = PAGE + body - nbytes
        start -= start % (16 if t.dtype is torch.uint8 else t.element_size())  # 4-byte tables END at the page: one entry past them faults
        buf = (ctypes.c_char * nbytes).from_address(addr + start)
        g = torch.frombuffer(buf, dtype=t.dtype, count=t.numel()).view(t.shape)
        g.copy_(t)
        keep.append((m, buf))
        return g

    from synth import synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import nets
    from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus
    from auto_avsr_amd.ngram import NgramScorer

    torch.manual_seed(3)
    odim, beam = 41, 4
    dec = nets.TransformerDecoder(odim, attention_dim=128, attention_heads=2, linear_units=256, num_blocks=1).eval()
    ctc = nets.CTC(odim, 128, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), 1))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), 2))

    def search(sc):
        scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "length_bonus": LengthBonus(odim)}
        weights = {"decoder": 0.9, "ctc": 0.1, "length_bonus": 0.0}
        if sc is not None:
            # the tables the session reads: each between two protected pages (tok / logp / next end on the last edge of the last node)
            sc._dev["cpu"] = tuple(guarded(t) for t in sc.device_tables(torch.device("cpu")))
            scorers["ngram"], weights["ngram"] = sc, 0.5
        return BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1, token_list=None,
                               pre_beam_score_key="decoder")

    xs = [torch.randn(T, 128) * 1.5 for T in (9, 3, 12)]
    AF.set_precise(True)
    try:
        first = [int(t) for t in search(None)(xs[0])[0].yseq[1:-1]]
        S, E = odim, odim - 1
        # a 3-gram model around the plain winner: contexts with and without lower-order nodes, the last node's edges end on the
        # largest token (<eos>), unigrams by <unk> fill-in
        a, b, c = first[0], first[1], first[2]
        P = {(E,): -2.0, (a,): -1.0, (b,): -1.5, (S,): -99.0, (S, a): -0.3, (a, b): -0.2, (S, a, b): -0.1, (a, b, c): -0.4, (a, b, E): -0.9}
        B = {(S,): -0.2, (a,): -0.3, (S, a): -0.4, (a, b): -0.6, (b,): -0.1}
        bs = search(NgramScorer(odim, P, B, order=3, unk_logp=-4.0))
        empty, seen = torch.empty, []

        def guarded_empty(*a, **k):  # the session workspace (decode_native: the one uint8 allocation of a search / a group)
            t = empty(*a, **k)
            if k.get("dtype") is torch.uint8 and t.dim() == 1 and not k.get("pin_memory"):
                seen.append(t.numel())
                return guarded(t)
            return t

        torch.empty = guarded_empty
        try:
            nbest = bs(xs[0])
            groups = bs.forward_batch(xs, batch=3)
        finally:
            torch.empty = empty
    finally:
        AF.set_precise(False)
    assert bs._native and bs._native.ngram_key is not None and len(seen) == 2
    assert any(h.scores["ngram"] != 0 for h in nbest)
    q.put(float(len(nbest) + sum(len(g) for g in groups)))


def test_ngram_search_stays_inside_its_tables_and_workspace(emu_lib_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    assert q.get(timeout=5) >= 4
