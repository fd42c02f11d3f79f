"""Out-of-bounds detector (as tests/test_encode_batch_guard_pages.py: operands END at an unmapped page and BEGIN right after one; an
access past either end is a SIGSEGV of a child process) for `avsr_bn_act_lens_fwd`, the length-masked BatchNorm + activation pass of
the audio trunk: every operand -- x, add, the four parameter vectors, the lengths, y -- is guarded, in the f32 and f16 forms.
Results must equal the unguarded run's.  CPU emulator only."""
import multiprocessing as mp
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _child(emu_path, f16, q):
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

    # the shape of tests/test_bn_act_lens.py: 9 vectors per row (rows do not align with the 256-vector blocks), a ragged last block,
    # blocks that are all padding, an empty item, a length beyond Tmax
    N, per, tmax, C = 4, 20, 5, 72
    W = per * tmax
    dtype = torch.float16 if f16 else torch.float32
    g0 = torch.Generator().manual_seed(11)
    x = torch.randn(N, W, C, generator=g0).to(dtype)
    add = torch.randn(N, W, C, generator=g0).to(dtype)
    mean, invstd = torch.randn(C, generator=g0), torch.rand(C, generator=g0) + 0.5
    gamma, beta = torch.randn(C, generator=g0), torch.randn(C, generator=g0)
    lens = torch.tensor([5, 3, 0, 7], dtype=torch.int32)

    def run(wrap, with_add):
        y = wrap(torch.full((N, W, C), float("nan"), dtype=dtype))
        ops.call("avsr_bn_act_lens_fwd", ops._ptr(wrap(x)), ops._ptr(wrap(add)) if with_add else None, 2 if f16 else 0,
                 ops._ptr(wrap(mean)), ops._ptr(wrap(invstd)), ops._ptr(wrap(gamma)), ops._ptr(wrap(beta)), ops._ptr(wrap(lens)),
                 ops._ptr(y), N, W, C, per, 1, None)
        return y.clone()

    ok = True
    for with_add in (False, True):
        plain, guard = run(lambda t: t.contiguous(), with_add), run(guarded, with_add)
        ok = ok and bool(torch.equal(plain, guard)) and bool(torch.isfinite(plain.float()).all())
    q.put(ok)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
def test_bn_act_lens_stays_inside_its_operands(emu_lib_path, f16):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_child, args=(emu_lib_path, f16, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    assert q.get(timeout=5) is True
