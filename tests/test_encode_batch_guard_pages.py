"""Out-of-bounds detector (as tests/test_ctc_beam_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an access
past either end is a SIGSEGV of a child process) for `avsr_convmod_dw_eval_fwd`, the inference conv-module middle with per-utterance
lengths: every operand -- the lengths included -- is guarded, in the f32 -> f32 and f32 -> f16 forms.  Results must equal the
unguarded run's.  CPU emulator only."""
import multiprocessing as mp
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(emu_path, out_f16, q):
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

    # the shape of tests/test_encode_batch.py's kernel case: ragged channel block, ragged time tile, a tile that is all padding
    B, T, C, K = 4, 37, 72, 31
    g0 = torch.Generator().manual_seed(7)
    a = torch.randn(B * T, 2 * C, generator=g0)
    w, bias = torch.randn(C, K, generator=g0), torch.randn(C, generator=g0)
    mean, invstd = torch.randn(C, generator=g0), torch.rand(C, generator=g0) + 0.5
    gamma, beta = torch.randn(C, generator=g0), torch.randn(C, generator=g0)
    lens = torch.tensor([37, 33, 32, 3], dtype=torch.int32)
    odt = torch.float16 if out_f16 else torch.float32

    def run(wrap):
        s = wrap(torch.full((B * T, C), float("nan"), dtype=odt))
        ops.call("avsr_convmod_dw_eval_fwd", ops._ptr(wrap(a)), 0, ops._ptr(wrap(w)), ops._ptr(wrap(bias)), ops._ptr(wrap(lens)), B, T, C,
                 K, ops._ptr(wrap(mean)), ops._ptr(wrap(invstd)), ops._ptr(wrap(gamma)), ops._ptr(wrap(beta)), ops._ptr(s),
                 2 if out_f16 else 0, None)
        return s.clone()

    plain, guard = run(lambda t: t.contiguous()), run(guarded)
    q.put(bool(torch.equal(plain, guard)) and bool(torch.isfinite(plain.float()).all()))


@pytest.mark.parametrize("out_f16", [False, True], ids=["f32", "f16"])
def test_convmod_dw_eval_stays_inside_its_operands(emu_lib_path, out_f16):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, out_f16, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    assert q.get(timeout=5) is True
