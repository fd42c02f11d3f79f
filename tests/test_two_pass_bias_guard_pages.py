"""Out-of-bounds detector (as tests/test_ctc_beam_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an access
past either end is a SIGSEGV of a child process) for `avsr_ctc_beam_search_bias`: a workspace of exactly
`avsr_ctc_beam_bias_workspace_bytes` and trie tables of exactly n_nodes + 1 / n_edges / n_edges / n_nodes elements.  Results must equal
the unguarded run's.  CPU emulator only."""
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
    from auto_avsr_amd.bias import ContextBiasScorer

    _lib._install_for_tests(emu_path)
    libc = ctypes.CDLL(None, use_errno=True)
    PAGE = 4096
    keep = []

    def guarded(t, align=16):
        t = t.contiguous()
        nbytes = t.numel() * t.element_size()
        body = (nbytes + PAGE - 1) // PAGE * PAGE
        m = mmap.mmap(-1, body + 2 * PAGE)
        addr = ctypes.addressof(ctypes.c_char.from_buffer(m))
        for off in (0, PAGE + body):
            assert libc.mprotect(ctypes.c_void_p(addr + off), PAGE, 0) == 0
        start = PAGE + body - nbytes
        start -= start % align
        buf = (ctypes.c_char * nbytes).from_address(addr + start)
        g = torch.frombuffer(buf, dtype=t.dtype, count=t.numel()).view(t.shape)
        g.copy_(t)
        keep.append((m, buf))
        return g

    V, ld, in_lens, W, K, N, kind = case
    B, T = len(in_lens), max(in_lens)
    g0 = torch.Generator().manual_seed(V + T)
    x = torch.randn(B * T, ld, generator=g0) * 3
    x[:, 0] += 6
    x[:, V:] = float("nan")  # the pad columns are never read
    lp = torch.full_like(x, float("nan"))
    lp[:, :V] = torch.log_softmax(x[:, :V], 1)
    lens = torch.tensor(in_lens, dtype=torch.int64)
    # the list: tokens the frames of utterance 0 offer, so that the search stands below the root and takes rewards back
    top = [[c for c in row if c <= V - 2] for row in torch.topk(lp[: in_lens[0], 1:V], K, dim=1).indices.add(1).tolist()]
    if kind == "one":
        phrases = [[top[0][0], top[1][0], top[2][0]]]
    elif kind == "wide":  # more children of the root than K
        firsts = sorted({c for row in top for c in row})[: 3 * K]
        assert len(firsts) > K
        phrases = [[c, top[(i + 1) % len(top)][0]] for i, c in enumerate(firsts)]
    else:
        phrases = [[top[t][0], top[t + 1][1 % len(top[t + 1])]] for t in range(len(top) - 1)] + [[top[0][0]], [top[0][0], top[1][0], top[2][0]]]
        phrases = [[c for i, c in enumerate(p) if i == 0 or c != p[i - 1]] for p in phrases]
    sc = ContextBiasScorer(phrases, V)
    tabs = [torch.from_numpy(a.copy()) for a in (sc.first, sc.tok, sc.child, sc.unc)]
    assert [t.numel() for t in tabs] == [sc.n_nodes + 1, sc.n_edges, sc.n_edges, sc.n_nodes]

    def run(wrap):
        ws_b = ops.call("avsr_ctc_beam_bias_workspace_bytes", B, T, W, K)
        assert ws_b % 4 == 0
        lpw, lw = wrap(lp), wrap(lens)
        ws = wrap(torch.zeros(ws_b // 4, dtype=torch.int32))
        tokens = wrap(torch.zeros(B, N, T, dtype=torch.int32))
        ilens, nv = wrap(torch.zeros(B, N, dtype=torch.int32)), wrap(torch.zeros(B, dtype=torch.int32))
        score, pb, pnb, bsum = (wrap(torch.zeros(B, N)) for _ in range(4))
        bnode = wrap(torch.zeros(B, N, dtype=torch.int32))
        ops.call("avsr_ctc_beam_search_bias", ops._ptr(lpw), ld, ops._ptr(lw), 0, W, K, N, *[ops._ptr(wrap(t, 4)) for t in tabs], sc.n_nodes,
                 sc.n_edges, 2.0, ops._ptr(tokens), ops._ptr(ilens), ops._ptr(score), ops._ptr(pb), ops._ptr(pnb), ops._ptr(nv),
                 ops._ptr(bsum), ops._ptr(bnode), ops._ptr(ws), B, T, V, None)
        return [t.clone() for t in (tokens, ilens, nv, score, pb, pnb, bsum, bnode)]

    plain, guard = run(lambda t, align=16: t.contiguous()), run(guarded)  # (align 4: an int32 table ends exactly at the page)
    q.put(bool(all(torch.equal(a, b) for a, b in zip(plain, guard))) and int(plain[2].min()) >= 1 and float(plain[6].abs().max()) > 0)


# (V, pitch, in_lens, beam, topk, nbest, list): the full vocabulary at its pitch of 5049 rounded up to 8; the widest beam and token
# budget (the 1024-thread block) with two utterances of unequal lengths; a list of one phrase; a root with more children than topk
@pytest.mark.parametrize("case", [(5049, 5056, (9,), 8, 8, 4, "mixed"), (41, 48, (6, 1), 64, 32, 3, "mixed"),
                                  (37, 40, (13, 5), 6, 5, 6, "one"), (37, 40, (13, 5), 6, 5, 6, "wide")],
                         ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_ctc_beam_bias_entry_point_stays_inside_its_operands(emu_lib_path, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, case, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    assert q.get(timeout=5) is True
