"""Out-of-bounds detector (as tests/test_two_pass_bias_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an
access past either end is a SIGSEGV of a child process) for `avsr_ctc_beam_search_ngram`: a workspace of exactly
`avsr_ctc_beam_ngram_workspace_bytes`, n-gram tables of exactly n_nodes + 1 / n_edges / n_edges / n_edges / n_nodes / n_nodes elements
and, with a list, trie tables of exactly their element counts.  Results must equal the unguarded run's.  CPU emulator only."""
import multiprocessing as mp
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(emu_path, case, q):
    import ctypes
    import mmap
    import random

    import torch

    sys.path.insert(0, os.path.dirname(HERE))
    from auto_avsr_amd import _lib, ops
    from auto_avsr_amd.bias import ContextBiasScorer
    from auto_avsr_amd.ngram import NgramScorer

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

    V, ld, in_lens, W, K, N, kind, with_bias = case
    B, T = len(in_lens), max(in_lens)
    g0 = torch.Generator().manual_seed(V + T)
    x = torch.randn(B * T, ld, generator=g0) * 3
    x[:, 0] += 6
    x[:, V:] = float("nan")  # the pad columns are never read
    lp = torch.full_like(x, float("nan"))
    lp[:, :V] = torch.log_softmax(x[:, :V], 1)
    lens = torch.tensor(in_lens, dtype=torch.int64)
    # the model: n-grams over the tokens the frames of utterance 0 offer, so that the search stands below the root and backs off
    top = torch.topk(lp[: in_lens[0], 1:V], K, dim=1).indices.add(1).tolist()
    rng = random.Random(V)
    P = {(t,): -rng.uniform(2.0, 9.0) for t in range(1, V)}
    Bo = {}
    if kind == "uni":  # one node: the root alone, which is also where every hypothesis starts
        order = 1
    else:
        order = 3
        P[(V,)] = -99.0
        Bo[(V,)] = -0.4
        for t in range(len(top) - 1):
            for _ in range(2 * K):
                g = (rng.choice(top[t]), rng.choice(top[t + 1]), rng.choice(top[min(t + 2, len(top) - 1)]))
                if V - 1 in g[:2]:
                    continue
                for i in (2, 3):
                    P.setdefault(g[:i], -rng.uniform(0.1, 4.0))
                    Bo.setdefault(g[:i - 1], -rng.uniform(0.05, 1.5))
        P.setdefault((V, top[0][0]), -0.2)
    sc = NgramScorer(V, P, Bo, order=order)
    tabs = [torch.from_numpy(a.copy()) for a in (sc.first, sc.tok, sc.logp, sc.next, sc.bow, sc.back)]
    assert [t.numel() for t in tabs] == [sc.n_nodes + 1, sc.n_edges, sc.n_edges, sc.n_edges, sc.n_nodes, sc.n_nodes]
    bias = ContextBiasScorer([[top[0][0], top[1][0], top[2][0]], [top[1][1 % K]], [top[0][0], top[1][1 % K]]], V) if with_bias else None
    btabs = [torch.from_numpy(a.copy()) for a in (bias.first, bias.tok, bias.child, bias.unc)] if bias else [None] * 4

    def run(wrap):
        ws_b = ops.call("avsr_ctc_beam_ngram_workspace_bytes", B, T, W, K, int(with_bias))
        assert ws_b % 4 == 0
        lpw, lw = wrap(lp), wrap(lens)
        ws = wrap(torch.zeros(ws_b // 4, dtype=torch.int32))
        tokens = wrap(torch.zeros(B, N, T, dtype=torch.int32))
        ilens, nv = wrap(torch.zeros(B, N, dtype=torch.int32)), wrap(torch.zeros(B, dtype=torch.int32))
        score, pb, pnb, bsum, nsum = (wrap(torch.zeros(B, N)) for _ in range(5))
        bnode, nnode = (wrap(torch.zeros(B, N, dtype=torch.int32)) for _ in range(2))
        ops.call("avsr_ctc_beam_search_ngram", ops._ptr(lpw), ld, ops._ptr(lw), 0, W, K, N,
                 *[ops._ptr(wrap(t, 4)) if t is not None else None for t in btabs], bias.n_nodes if bias else 0, bias.n_edges if bias else 0,
                 2.0, *[ops._ptr(wrap(t, 4)) for t in tabs], sc.n_nodes, sc.n_edges, int(sc.start_node), V - 1, 0.5, 0.7, ops._ptr(tokens),
                 ops._ptr(ilens), ops._ptr(score), ops._ptr(pb), ops._ptr(pnb), ops._ptr(nv), ops._ptr(bsum), ops._ptr(bnode), ops._ptr(nsum),
                 ops._ptr(nnode), ops._ptr(ws), B, T, V, None)
        return [t.clone() for t in (tokens, ilens, nv, score, pb, pnb, bsum, bnode, nsum, nnode)]

    plain, guard = run(lambda t, align=16: t.contiguous()), run(guarded)  # (align 4: a table ends exactly at the page)
    below = kind == "uni" or int(plain[9].abs().max()) > 0  # a hypothesis of the n-best stands below the root
    q.put(bool(all(torch.equal(a, b) for a, b in zip(plain, guard))) and int(plain[2].min()) >= 1 and float(plain[8].abs().max()) > 0
          and below and (not with_bias or float(plain[6].abs().max()) > 0))


# (V, pitch, in_lens, beam, topk, nbest, model, with a bias list): the full vocabulary at its pitch of 5049 rounded up to 8; the widest
# beam and token budget (the 1024-thread block) with two utterances of unequal lengths; the one-node model; list and model together
@pytest.mark.parametrize("case", [(5049, 5056, (9,), 8, 8, 4, "tri", False), (41, 48, (6, 1), 64, 32, 3, "tri", False),
                                  (37, 40, (13, 5), 6, 5, 6, "uni", False), (37, 40, (13, 5), 6, 5, 6, "tri", True)],
                         ids=lambda c: "-".join(map(str, c)).replace(" ", ""))
def test_ctc_beam_ngram_entry_point_stays_inside_its_operands(emu_lib_path, case):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, case, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    assert q.get(timeout=5) is True
