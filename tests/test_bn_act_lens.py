"""ops.bn_act_lens_fwd (avsr_bn_act_lens_fwd): BatchNorm + activation of a zero-padded batch [N, W, C] with per-item lengths, the
pass that makes the audio front-end's 1-D trunk length-exact under functional.padded_lengths.  Valid rows against the torch fp64
expression at the tolerances this suite already holds ops.bn_act_fwd to -- f32: max abs 1e-4 (test_convmod_kernels.py::
test_batchnorm_train), f16: relative L2 6e-4, a bf16-stored result: relative L2 4e-3 (test_mixed_mode.py, the f16 BatchNorm pass and
its bf16 twin); rows beyond the length exactly zero; NaN in the padded rows reaches nothing; no mask == ops.bn_act_fwd, bit for bit."""
import functools

import pytest
import torch
import torch.nn.functional as F

from auto_avsr_amd import ops

N = 4
LENS = (5, 3, 0, 1)
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _case(C, per, tmax, dtype_name, with_add, act):
    """Operands (rounded to the storage type) and the fp64 reference -- computed once, shared, never changed."""
    dtype = DTYPES[dtype_name]
    W = per * tmax
    g0 = torch.Generator().manual_seed(1000 * C + per + (7 if with_add else 0) + act)
    x = (torch.randn(N, W, C, generator=g0) * 1.7 + 0.6).to(dtype)
    add = torch.randn(N, W, C, generator=g0).to(dtype) if with_add else None
    mean, invstd = torch.randn(C, generator=g0), torch.rand(C, generator=g0) + 0.5
    gamma, beta = torch.rand(C, generator=g0) + 0.5, torch.randn(C, generator=g0) * 0.3
    z = (x.double() - mean.double()) * invstd.double() * gamma.double() + beta.double()
    if with_add:
        z = z + add.double()
    ref = F.silu(z) if act == 1 else z
    return dict(x=x, add=add, p=(mean, invstd, gamma, beta), ref=ref, W=W, C=C, per=per, tmax=tmax, act=act, dtype=dtype)


def _run(c, dev, lens, x=None, add=None):
    x = c["x"] if x is None else x
    add = c["add"] if add is None else add
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int32).to(dev)
    p = [t.to(dev) for t in c["p"]]
    y = ops.bn_act_lens_fwd(x.contiguous().to(dev), None if add is None else add.contiguous().to(dev), *p, ld, c["per"], N, c["W"],
                            c["C"], c["act"])
    assert y.dtype == c["dtype"] and tuple(y.shape) == (N, c["W"], c["C"])
    return y.cpu()


def _check_valid(c, y, n, rows, what):
    if rows == 0:
        return
    got, ref = y[n, :rows].double(), c["ref"][n, :rows]
    if c["dtype"] == torch.float32:
        err = float((got - ref).abs().max())
        print(f"{what} item {n} rows {rows}: max abs error {err:.3e} (bound 1e-4)")
        assert err < 1e-4
    else:
        bound = 6e-4 if c["dtype"] == torch.float16 else 4e-3
        err = float((got - ref).norm() / ref.norm())
        print(f"{what} item {n} rows {rows}: rel L2 {err:.3e} (bound {bound:.0e})")
        assert err < bound


def _check(c, dev, lens):
    y = _run(c, dev, lens)
    valid = [min(c["W"], max(0, n) * c["per"]) for n in lens]
    for n, rows in enumerate(valid):
        _check_valid(c, y, n, rows, "plain")
        assert rows == c["W"] or y[n, rows:].float().abs().max() == 0, "rows beyond the length are exactly zero"
    # NaN in every padded row of x and add: the output stays finite, the valid rows do not move (a select, not a multiplication)
    xn = c["x"].clone()
    an = None if c["add"] is None else c["add"].clone()
    for n, rows in enumerate(valid):
        xn[n, rows:] = float("nan")
        if an is not None:
            an[n, rows:] = float("nan")
    yn = _run(c, dev, lens, x=xn, add=an)
    assert torch.isfinite(yn.float()).all()
    assert torch.equal(yn, y)
    return y


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("with_add,act", [(False, 1), (True, 1), (False, 0), (True, 0)], ids=["silu", "add-silu", "none", "add-none"])
@pytest.mark.parametrize("C", [64, 72])
def test_bn_act_lens(dev, C, with_add, act, dtype):
    """per = 20, Tmax = 5: W * C / 8 = 800 / 900 vectors per item -- several blocks per item, blocks that are all padding, blocks that
    straddle the length, a ragged last block; C = 72: 9 vectors per row (rows do not align with the blocks)."""
    _check(_case(C, 20, 5, dtype, with_add, act), dev, LENS)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_bn_act_lens_stem_rows(dev, dtype):
    """The stem's geometry: 160 rows per frame, Tmax = 2."""
    _check(_case(64, 160, 2, dtype, False, 1), dev, (2, 1, 0, 1))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_bn_act_lens_clamps(dev, dtype):
    """A length above Tmax is Tmax, a negative one is 0."""
    c = _case(72, 20, 5, dtype, True, 1)
    y = _check(c, dev, (9, 3, -2, 5))
    assert torch.equal(y, _run(c, dev, (5, 3, 0, 5)))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("with_add,act", [(False, 1), (True, 1), (True, 0)], ids=["silu", "add-silu", "add-none"])
def test_bn_act_lens_unmasked_is_bn_act_fwd(dev, with_add, act, dtype):
    """lens = None and lens = [Tmax] * N: the parent's expression on every row -- bit-equal to ops.bn_act_fwd."""
    c = _case(72, 20, 5, dtype, with_add, act)
    rows = N * c["W"]
    p = [t.to(dev) for t in c["p"]]
    add = None if c["add"] is None else c["add"].view(rows, c["C"]).to(dev)
    ref = ops.bn_act_fwd(c["x"].view(rows, c["C"]).to(dev), add, *p, rows, c["C"], act).cpu().view(N, c["W"], c["C"])
    assert torch.equal(_run(c, dev, None), ref)
    assert torch.equal(_run(c, dev, (c["tmax"],) * N), ref)
