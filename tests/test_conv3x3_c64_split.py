"""conv3x3_c64_split.hip: the patch-staged, weights-in-registers persistent kernel of the 64 -> 64 channel 3x3 / stride-1
split-plane forward convolution (avsr_conv2d_f32s / avsr_conv2d_f32s_stats on a pre-split activation), forced with knob 27 = 2,
against torch conv2d in float64, against the tiled kernel it replaces (knob 27 = 1), and its bf16 twin / BatchNorm statistics."""
import pytest
import torch
import torch.nn.functional as F

from auto_avsr_amd import ops

KNOB = 27
C = 64


def rel(a, b):
    a, b = a.double().flatten().cpu(), b.double().flatten().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def sp(v):  # what the split8 layout keeps of a value: hi + lo bf16
    hi = v.bfloat16().float()
    return hi + (v - hi).bfloat16().float()


# several bands per image, a ragged last band, more tiles than blocks, one tile only, widths that are no multiple of 8, statistics
# groups of more than one tile (tiles of fewer than 128 pixels), >= 1100 images
GEOMS = [(3, 22, 22), (2, 9, 10), (5, 1, 37), (2, 30, 12), (300, 7, 5), (1100, 6, 4), (1, 4, 4)]


@pytest.mark.parametrize("cfg", GEOMS)
def test_conv3x3_c64_split(dev, cfg, monkeypatch):
    N, H, W = cfg
    torch.manual_seed(H * 100 + W)
    made = []

    def make(y):
        t = torch.full(y.shape, float("nan"), dtype=torch.bfloat16, device=y.device)
        made.append(t)
        return t

    monkeypatch.setattr(ops, "TWIN", make)
    x = sp(torch.randn(N, H, W, C) + 0.3)  # exactly representable as hi + lo
    w = sp(torch.randn(C, C, 3, 3) / (C * 9) ** 0.5)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=1, padding=1).permute(0, 2, 3, 1)
    xs = ops.split_pack(x.to(dev))
    wp = ops.conv_weight_permute_split(w.to(dev))
    assert isinstance(xs, ops.Split8) and isinstance(wp, ops.Split8)
    rows = N * H * W

    def run(knob, stats):
        ops.tune(KNOB, knob)
        try:
            part = torch.full((ops.bn_stat_tiles(rows), 2, C), float("nan"), device=dev) if stats else None
            y = ops.conv2d_fwd(xs, wp, N, H, W, C, C, 3, 3, 1, 1, 1, True, stats=part)
        finally:
            ops.tune(KNOB, 0)
        return y, made[-1], part

    y, tw, part = run(2, True)
    y0, tw0, _ = run(2, False)
    yt, twt, _ = run(1, False)
    e_ref, e_tiled = rel(y, ref), rel(y, yt)
    print(f"geometry {cfg}: rel L2 vs float64 {e_ref:.3e}, vs the tiled kernel {e_tiled:.3e}")
    # 1. against float64; 2. against the tiled kernel (another summation order of the same products)
    assert e_ref < 3e-5
    assert rel(yt, ref) < 3e-5 and e_tiled < 1e-6
    # 3. the bf16 twin
    assert torch.equal(tw.view(torch.int16), y.bfloat16().view(torch.int16))
    assert torch.equal(twt.view(torch.int16), yt.bfloat16().view(torch.int16))
    # 4. with statistics == without; every row written; the rows sum to the column sums / sums of squares of y
    assert torch.equal(y, y0) and torch.equal(tw.view(torch.int16), tw0.view(torch.int16))
    assert torch.isfinite(part).all()
    y2 = y.view(rows, C).double()
    e_sum, e_sq = rel(part[:, 0].sum(0).double(), y2.sum(0)), rel(part[:, 1].sum(0).double(), (y2 * y2).sum(0))
    print(f"geometry {cfg}: statistics rel L2 sums {e_sum:.3e}, sums of squares {e_sq:.3e}")
    assert e_sum < 1e-5 and e_sq < 1e-5
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    rm0, rv0 = rm.clone(), rv.clone()
    mean, invstd = ops.bn_finalize_parts(part, rows, C, 1e-5, 0.1, rm, rv)
    mean0, invstd0 = ops.bn_stats_finalize(y.view(rows, C), rows, C, 1e-5, 0.1, rm0, rv0)
    assert rel(mean, mean0) < 1e-5 and rel(invstd, invstd0) < 1e-5 and rel(rm, rm0) < 1e-5 and rel(rv, rv0) < 1e-5
    # 6. no atomics, static tile map: a second call gives the same bits
    y1, tw1, part1 = run(2, True)
    assert torch.equal(y, y1) and torch.equal(tw.view(torch.int16), tw1.view(torch.int16)) and torch.equal(part, part1)


def test_conv3x3_c64_split_dispatch(dev):
    """Knob 27 = 0: small outputs (< 65536 rows) stay on the tiled kernel -- bit-equal to knob 27 = 1."""
    torch.manual_seed(5)
    N, H, W = 3, 8, 8
    xs = ops.split_pack(torch.randn(N, H, W, C).to(dev))
    wp = ops.conv_weight_permute_split((0.1 * torch.randn(C, C, 3, 3)).to(dev))
    y_rule = ops.conv2d_fwd(xs, wp, N, H, W, C, C, 3, 3, 1, 1, 1, True)
    ops.tune(KNOB, 1)
    try:
        y_tiled = ops.conv2d_fwd(xs, wp, N, H, W, C, C, 3, 3, 1, 1, 1, True)
    finally:
        ops.tune(KNOB, 0)
    assert torch.equal(y_rule, y_tiled)
