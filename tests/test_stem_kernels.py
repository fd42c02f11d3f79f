"""Video-stem kernels of csrc/stem.hip (row-group forward in both arithmetic modes, row-run weight gradient) against torch conv3d in float64
and its autograd, at the smallest geometries at which each mechanism can break:

  (2, 3, 20, 24)  T < 5: every temporal tap is clipped on both sides, and a frame of the other utterance must not leak across the
                  batch edge
  (1, 1, 88, 88)  the real 44 x 44 output: 44 rows (11 groups of 4, a ragged 5.5 blocks of 8), 44 pixels (no multiple of 16 / 32 / 48)
  (3, 2, 88, 88)  several utterances at the real width, more rows / groups than one block's run
  (2, 2, 12, 96)  the widest input: OW = 48, OH = 6 (a group of 4 rows that is half empty, a block of 8 rows that spans two frames)
  (1, 2, 4, 4)    OH = OW = 2: nearly every tap is padding
  (3, 57, 18, 24) 171 frames of 9 x 12 outputs = 513 groups of 4 rows (the third group of a frame holds one row): one more than the
                  512 persistent blocks of the forward and weight-gradient grids, so every block but the last walks TWO groups and
                  the last one -- a ragged run.  The only geometry here at which a block's loop over groups turns: the barrier
                  before a patch is overwritten, group i + 1 requested while group i is staged and multiplied, statistics and
                  weight-gradient accumulators carried from group to group.  Three tiles of 16 pixels: both tile parities work

Tolerances are those of tests/test_conv_kernels.py (test_stem357_dedicated / test_stem357_split_forward), relative to
max(1, |ref|max): 2e-5 for the split forward against f64, 2e-2 for the bf16 forward and the weight gradient against bf16-rounded
operands.  The per-row weight-gradient kernel (avsr_tune knob 28 = 1) is the in-tree reference of the row-run kernel: both round the
same operands to bf16 and differ in summation order only, so against the f64 gradient of the ROUNDED operands (which isolates the
summation error) the new kernel may be at most 2x as far off as the old one."""
import functools
import multiprocessing as mp
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from auto_avsr_amd import ops

HERE = os.path.dirname(os.path.abspath(__file__))
GEOMS = [(2, 3, 20, 24), (1, 1, 88, 88), (3, 2, 88, 88), (2, 2, 12, 96), (1, 2, 4, 4), (3, 57, 18, 24)]
KNOB_OLD = 28  # 1 = the kernels this file's subjects replace


def _nhwc(y):  # (B, C, T, OH, OW) -> (B*T, OH, OW, C)
    return y.permute(0, 2, 3, 4, 1).reshape(y.shape[0] * y.shape[2], y.shape[3], y.shape[4], y.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def _case(geom):
    """Inputs and float64 references of one geometry, computed once and shared (read-only) by every test."""
    B, T, H, W = geom
    g = torch.Generator().manual_seed(1000 * H + 10 * W + B + T)
    x = torch.randn(B, T, H, W, generator=g)
    w = torch.randn(64, 1, 5, 7, 7, generator=g) / 245 ** 0.5
    conv = lambda a, b: F.conv3d(a.unsqueeze(1), b, stride=(1, 2, 2), padding=(2, 3, 3))
    y64 = conv(x.double(), w.double())
    xq, wq = x.bfloat16().double(), w.bfloat16().double().requires_grad_()
    yq = conv(xq, wq)
    dy = torch.randn(yq.shape, generator=g).bfloat16()
    yq.backward(dy.double())
    return {"x": x, "w": w, "y64": _nhwc(y64), "yq": _nhwc(yq.detach()), "dy": _nhwc(dy), "dwq": wq.grad.detach()}


def _err(a, ref):
    return float((a.double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_stem_forward_split_and_bf16(dev, geom):
    c = _case(geom)
    B, T, H, W = geom
    x, w = c["x"].to(dev), c["w"].to(dev)
    y = ops.stem357_fwd_f32s(x, w, B, T, H, W)
    e32 = _err(y, c["y64"])
    yb = ops.stem357_fwd(x, w, B, T, H, W)
    e16 = _err(yb.float(), c["yq"])
    print(f"stem forward {geom}: split vs f64 {e32:.3e} (< 2e-5), bf16 vs rounded operands {e16:.3e} (< 2e-2)")
    assert y.dtype == torch.float32 and y.shape == c["y64"].shape and e32 < 2e-5
    assert yb.dtype == torch.bfloat16 and e16 < 2e-2
    try:  # the per-row kernels: the same products accumulated in the same order
        ops.tune(KNOB_OLD, 1)
        y_old, yb_old = ops.stem357_fwd_f32s(x, w, B, T, H, W), ops.stem357_fwd(x, w, B, T, H, W)
    finally:
        ops.tune(KNOB_OLD, 0)
    assert torch.equal(y, y_old) and torch.equal(yb, yb_old)


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_stem_forward_statistics(dev, geom):
    """want_stats: the same output bit for bit, partial sums that add up to the sums of the output, the same partials every call."""
    c = _case(geom)
    B, T, H, W = geom
    x, w = c["x"].to(dev), c["w"].to(dev)
    y0 = ops.stem357_fwd_f32s(x, w, B, T, H, W)
    y, part = ops.stem357_fwd_f32s(x, w, B, T, H, W, want_stats=True)
    y1, part1 = ops.stem357_fwd_f32s(x, w, B, T, H, W, want_stats=True)
    assert torch.equal(y, y0) and torch.equal(y1, y0) and torch.isfinite(part).all()
    assert torch.equal(part, part1)
    groups = B * T * ((y.shape[1] + 3) // 4)  # one row of partials per persistent block, each with ceil(groups / 512) groups
    per_block = (groups + 511) // 512
    assert part.shape[0] == (groups + per_block - 1) // per_block
    y2 = y.view(-1, 64).double()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    r1, r2 = rel(part[:, 0].sum(0).double(), y2.sum(0)), rel(part[:, 1].sum(0).double(), (y2 * y2).sum(0))
    print(f"stem statistics {geom}: sums {r1:.3e}, sums of squares {r2:.3e} (< 1e-5)")
    assert r1 < 1e-5 and r2 < 1e-5


def _wgrad_both(c, geom, dev, blocks=0):
    B, T, H, W = geom
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    out = []
    try:
        ops.tune(6, blocks)
        for old in (1, 0):
            ops.tune(KNOB_OLD, old)
            out.append(ops.stem357_wgrad(dy, x, B, T, H, W))
        again = ops.stem357_wgrad(dy, x, B, T, H, W)
    finally:
        ops.tune(KNOB_OLD, 0)
        ops.tune(6, 0)
    assert torch.equal(again, out[1])  # ordered partial sums: the same bits every call
    return out


@pytest.mark.parametrize("geom,blocks", [(g, 0) for g in GEOMS] + [((3, 2, 88, 88), 3)], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"blocks{v}")
def test_stem_wgrad_row_runs(dev, geom, blocks):
    """blocks = 3 (knob 6): rows >> blocks, uneven runs (66 groups of 4 rows -> 22 per block; the per-row kernel: 264 rows over 3)."""
    c = _case(geom)
    old, new = _wgrad_both(c, geom, dev, blocks)
    e_old, e_new = _err(old, c["dwq"]), _err(new, c["dwq"])
    print(f"stem wgrad {geom} blocks={blocks}: max error vs f64 on the rounded operands: per-row kernel {e_old:.3e}, row-run kernel {e_new:.3e}")
    assert new.shape == (64, 1, 5, 7, 7) and e_new < 2e-2
    assert e_old < 2e-2
    assert e_new <= 2 * e_old


# ---------------------------------------------------------------- guard pages (CPU emulator only)
def _guard_child(emu_path, geom, q):
    """Every operand of the three entry points lies between two unmapped pages, and the calls are made twice: with each operand
    ENDING at the rear guard (to within the 15 bytes of its 16-byte alignment; its start is then up to a page behind the front
    guard), and with each operand BEGINNING right at the front guard (its end up to a page short of the rear one).  An access
    past the abutted end kills this process: over-reads in the first placement, under-reads (the clamped first column and first
    input row of the staging loads) in the second."""
    import ctypes
    import mmap

    sys.path.insert(0, os.path.dirname(HERE))
    from auto_avsr_amd import _lib

    _lib._install_for_tests(emu_path)
    libc = ctypes.CDLL(None, use_errno=True)
    PAGE = 4096
    keep = []

    front = False

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
        if front:
            start = PAGE
        buf = (ctypes.c_char * nbytes).from_address(addr + start)
        g = torch.frombuffer(buf, dtype=t.dtype, count=t.numel()).view(t.shape)
        g.copy_(t)
        keep.append((m, buf))
        return g

    c = _case(geom)
    B, T, H, W = geom
    P = ops._ptr
    errs = []
    for front in (False, True):
        x, w, dy = guarded(c["x"]), guarded(c["w"]), guarded(c["dy"])
        ws = guarded(torch.zeros(ops.call("avsr_stem357_workspace_bytes"), dtype=torch.uint8))
        yb = guarded(torch.zeros(c["yq"].shape, dtype=torch.bfloat16))
        ops.call("avsr_stem357_fwd", P(x), P(w), P(yb), P(ws), B, T, H, W, None)
        y, y2 = guarded(torch.zeros(c["y64"].shape)), guarded(torch.zeros(c["y64"].shape, dtype=torch.bfloat16))
        part = guarded(torch.zeros(ops.call("avsr_stem357_stat_rows", B, T, H), 2, 64))
        ops.call("avsr_stem357_fwd_f32s_stats", P(x), P(w), P(y), P(y2), P(ws), B, T, H, W, P(part), part.shape[0], None)
        dw = guarded(torch.zeros(64, 1, 5, 7, 7))
        ops.call("avsr_stem357_wgrad", P(dy), P(x), P(dw), P(ws), B, T, H, W, None)
        errs.append((_err(yb.float(), c["yq"]), _err(y, c["y64"]), _err(y2.float(), c["y64"]), _err(dw, c["dwq"])))
    q.put(errs)


@pytest.mark.parametrize("geom", [(1, 1, 88, 88), (2, 3, 20, 24), (3, 57, 18, 24)], ids=lambda g: "x".join(map(str, g)))
def test_stem_entry_points_stay_inside_their_operands(emu_lib_path, geom):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_guard_child, args=(emu_lib_path, geom, q))
    p.start()
    p.join(300)
    assert not p.is_alive(), "child hung"
    assert p.exitcode == 0, f"child died with {p.exitcode} (out-of-bounds access?)"
    for eb, e32, etwin, ew in q.get(timeout=5):
        assert eb < 2e-2 and e32 < 2e-5 and etwin < 2e-2 and ew < 2e-2
