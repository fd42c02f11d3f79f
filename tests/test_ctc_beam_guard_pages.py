"""Out-of-bounds detector (as tests/test_lm_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an access past
either end is a SIGSEGV of a child process) for the entry points of two-pass decoding: `avsr_ctc_beam_search` with a workspace of
exactly `avsr_ctc_beam_workspace_bytes`, and `avsr_ctc_score` with one of exactly `avsr_ctc_score_workspace_bytes`.  Results must
equal the unguarded run's.  CPU emulator only."""
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

    V, ld, in_lens, W, K, N = case
    B, T = len(in_lens), max(in_lens)
    g0 = torch.Generator().manual_seed(V + T)
    x = torch.randn(B * T, ld, generator=g0) * 3
    x[:, 0] += 6
    x[:, V:] = float("nan")  # the pad columns are never read
    lp = torch.full_like(x, float("nan"))
    lp[:, :V] = torch.log_softmax(x[:, :V], 1)
    lens = torch.tensor(in_lens, dtype=torch.int64)
    labels = torch.randint(1, V, (B, N, 7), generator=g0)
    labels[:, 1, 3:] = -1
    labels[:, 2, :] = -1

    def run(wrap):
        ws_b = ops.call("avsr_ctc_beam_workspace_bytes", B, T, W, K)
        assert ws_b % 4 == 0
        lpw, lw = wrap(lp), wrap(lens)
        ws = wrap(torch.zeros(ws_b // 4, dtype=torch.int32))
        tokens = wrap(torch.zeros(B, N, T, dtype=torch.int32))
        ilens, nv = wrap(torch.zeros(B, N, dtype=torch.int32)), wrap(torch.zeros(B, dtype=torch.int32))
        score, pb, pnb = (wrap(torch.zeros(B, N)) for _ in range(3))
        ops.call("avsr_ctc_beam_search", ops._ptr(lpw), ld, ops._ptr(lw), 0, W, K, N, ops._ptr(tokens), ops._ptr(ilens), ops._ptr(score),
                 ops._ptr(pb), ops._ptr(pnb), ops._ptr(nv), ops._ptr(ws), B, T, V, None)
        sw_b = ops.call("avsr_ctc_score_workspace_bytes", B, N, T, labels.shape[2])
        sws = wrap(torch.zeros(sw_b // 4))
        ll = wrap(torch.zeros(B, N))
        ops.call("avsr_ctc_score", ops._ptr(lpw), ld, ops._ptr(wrap(labels)), N, labels.shape[2], -1, ops._ptr(lw), 0, ops._ptr(ll),
                 ops._ptr(sws), B, T, V, None)
        return [t.clone() for t in (tokens, ilens, nv, score, pb, pnb, ll)]

    plain, guard = run(lambda t: t.contiguous()), run(guarded)
    q.put(bool(all(torch.equal(a, b) for a, b in zip(plain, guard))) and int(plain[2].min()) >= 1)


# (V, pitch, in_lens, beam, topk, nbest): the full vocabulary at its pitch of 5049 rounded up to 8; two utterances of unequal lengths;
# the widest beam and token budget (the 1024-thread block)
@pytest.mark.parametrize("case", [(5049, 5056, (9,), 8, 8, 4), (37, 40, (13, 5), 6, 5, 6), (41, 48, (6, 1), 64, 32, 3)],
                         ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_ctc_beam_entry_points_stay_inside_their_operands(emu_lib_path, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, case, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    assert q.get(timeout=5) is True
