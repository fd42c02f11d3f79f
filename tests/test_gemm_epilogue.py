"""The shared GEMM epilogue (csrc/gemm_core.h epilogue_lds) against float64, option by option and all together:

    +bias -> act (relu | silu) -> gate (g > 0 ? v * gate_scale : 0) -> dropout(seed + *seed_dev, row * N + col)
          -> * alpha * *alpha_dev -> + resid (f32 | bf16, pitch ldr) -> store (f32 | bf16 | f16, pitch ldc) [+ bf16 twin] [+ column sums]

Every Linear of the model ends in this chain, instantiated once per tile shape (BM, BN, thread count, k groups), each step with a
vector path (full chunk of 8 columns, pitch a multiple of 8) and a scalar path.  The reference is float64 math on the stored
operands with the dropout keep mask REPLAYED outside the GEMM through avsr_scale_dropout (element index row * N + col with the
logical N, whatever the pitches are).  Tolerances are the project's, relative to the largest reference magnitude: 2e-6 for an f32
result of bf16 / f16 stored operands, 2e-5 for split-plane f32 operands, 1e-2 for a bf16 / f16 result, 1e-4 of the largest column
sum for column sums, bit equality wherever two launches run the same tile kernel.

Each test prints its measured errors as `EPI-ERR <family> <quantity> <error> <bound>` lines (pytest -s / -rP shows them)."""
import contextlib
import math

import pytest
import torch

from auto_avsr_amd import _lib, ops

SENT = 7.0  # pad columns of every output start at this value and must still hold it afterwards
SHAPES = [(150, 70, 64), (257, 136, 192)]  # ragged tail chunk + one k-tile + ragged M | full chunks, M past a 256-row tile, ring wraps
PITCHES = ["vector", "scalar"]
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
P_DROP, SEED, STEP = 0.25, 1234, 5

BF16_TILES = [1, 2, 3, 4, 5, 6, 7, 8]
F32S_TILES = [1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, 16]
H16_TILES = [1, 4, 7]
H16X2_TILES = [1, 21, 4, 7, 2, 5, 8, 22, 23]
FAMILIES = ([("bf16", t) for t in BF16_TILES] + [("f32s", t) for t in F32S_TILES] + [("h16", t) for t in H16_TILES]
            + [("h16x2", t) for t in H16X2_TILES]
            + [("gemm", (lay, ft, pr)) for lay in (ops.NT, ops.NN, ops.TN) for ft in (64, 128) for pr in (False, True)])
# what each family's entry point accepts
HAS = {
    "bf16": {"gate", "alpha_dev", "colsum", "resid_bf16"},
    "f32s": {"gate", "alpha_dev", "colsum", "resid_bf16", "twin"},
    "h16": {"resid_bf16", "twin", "c_f16"},
    "h16x2": {"resid_bf16", "twin", "c_f16"},
    "gemm": {"gate", "alpha_dev"},
}


def _fam_id(f):
    name, arg = f
    if name == "gemm":
        return "gemm-%s-%d%s" % (("nt", "nn", "tn")[arg[0]], arg[1], "-precise" if arg[2] else "")
    return f"{name}-t{arg}"


def _pitches(N, variant):
    """vector: every pitch a multiple of 8, different from N and from each other; scalar: no pitch a multiple of 4."""
    if variant == "vector":
        r8 = (N + 7) // 8 * 8
        return dict(ldc=r8 + 8, ldg=r8 + 16, ldr=r8 + 24)
    return dict(ldc=N + 3, ldg=N + 5, ldr=N + 1)


def _pitched(t, ld, dev, fill=SENT):
    """A fresh allocation [rows, ld] holding t in its logical columns."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    buf[:, : t.shape[1]] = t
    return buf.to(dev)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _operands(kind, shape):
    """Stored operands (CPU) and their float64 product, once per (operand kind, shape)."""

    def make():
        M, N, K = shape
        g = torch.Generator().manual_seed(100 * M + {"bf16": 1, "f32": 2, "h16": 3, "h16x2": 4}[kind])
        A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
        if kind == "bf16":
            A, B = A.bfloat16(), B.bfloat16()
            Bd = B.double()
        elif kind == "f32":
            Bd = B.double()
        elif kind == "h16":
            A, B = A.half(), (0.1 * B).half()
            Bd = B.double()
        else:  # two f16 weight planes (csrc/prims.h f2h_lo): hi + lo / 2048 is what the kernel multiplies with
            A, W = A.half(), 0.1 * B
            hi = W.half()
            lo = ((W - hi.float()) * 2048.0).half()
            B = (hi, lo)
            Bd = hi.double() + lo.double() / 2048.0
        return A, B, A.double() @ Bd.t()

    return _cached(("operands", kind, shape), make)


# gate entries that must switch their element off although they are not negative: +0.0 and -0.0 at known positions
def _planted(M, N):
    return [(0, 0, 0.0), (1, 1, -0.0), (M - 1, N - 1, -0.0), (M - 1, N - 2, 0.0), (M // 2, 8, -0.0), (M // 2 + 1, N - 1, 0.0),
            (64, 63, -0.0), (65, 64, 0.0)]


def _epi_inputs(shape):
    def make():
        M, N, _ = shape
        g = torch.Generator().manual_seed(7 * M + N)
        bias, gate, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
        for r, c, z in _planted(M, N):
            gate[r, c] = z
        return bias, gate, resid

    return _cached(("epi", shape), make)


def _keep_mask(dev, M, N, p, seed, step):
    """The keep mask of (seed, step) for an [M, N] result, replayed through avsr_scale_dropout (index row * N + col)."""

    def make():
        sd = torch.tensor([step], dtype=torch.int64, device=dev)
        out = ops.scale_dropout(torch.ones(M * N, device=dev), torch.float32, drop_p=p, seed=seed, seed_dev=sd).cpu()
        kept = out != 0
        assert torch.allclose(out[kept], torch.full((1,), 1.0 / (1.0 - p))), "kept elements carry 1 / (1 - p)"
        return kept.reshape(M, N)

    return _cached(("keep", dev.type, M, N, p, seed, step), make)


def _reference(prod, *, bias=None, act=0, gate=None, gate_scale=1.0, keep=None, p=0.0, alpha=1.0, resid=None):
    """float64 epilogue of the formula in the module docstring; gate / resid are the STORED (possibly bf16) tensors."""
    v = prod.clone()
    if bias is not None:
        v = v + bias.double()
    if act == 1:
        v = torch.relu(v)
    elif act == 2:
        v = v * torch.sigmoid(v)
    if gate is not None:
        v = torch.where(gate.double() > 0, v * gate_scale, torch.zeros_like(v))
    if keep is not None:
        v = v * keep.double() / (1.0 - p)
    v = v * alpha
    if resid is not None:
        v = v + resid.double()
    return v


@contextlib.contextmanager
def _twin_provider():
    """ops.TWIN as functional.set_mode('mixed' / 'hpf') installs it: a bf16 buffer of the result's shape (here sentinel-filled)."""
    made = []

    def make(y):
        t = torch.full(y.shape, SENT, dtype=torch.bfloat16, device=y.device)
        made.append((y, t))
        return t

    saved = ops.TWIN
    ops.TWIN = make
    try:
        yield made
    finally:
        ops.TWIN = saved


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _tol(fam, c_dtype):
    if c_dtype != F32:
        return 1e-2
    name, arg = fam
    return 2e-5 if (name == "f32s" or (name == "gemm" and arg[2])) else 2e-6


def _launch(fam, dev, shape, C, ldc, kw):
    """One launch of `fam` on fresh device copies of the cached operands."""
    name, arg = fam
    M, N, K = shape
    if name == "bf16":
        A, B, _ = _operands("bf16", shape)
        ops.gemm_bf16_nt(A.to(dev), K, B.to(dev), K, M, N, K, C, ldc, tile=arg, **kw)
    elif name == "f32s":
        A, B, _ = _operands("f32", shape)
        ops.gemm_f32s_nt(_pitched(A, K + 8, dev, 0.0), K + 8, B.to(dev), K, M, N, K, C, ldc, tile=arg, **kw)
    elif name == "h16":
        A, B, _ = _operands("h16", shape)
        ops.gemm_h16_nt(A.to(dev), K, B.to(dev), K, M, N, K, C, ldc, tile=arg, **kw)
    elif name == "h16x2":
        A, (hi, lo), _ = _operands("h16x2", shape)
        ops.gemm_h16_nt(A.to(dev), K, hi.to(dev), K, M, N, K, C, ldc, tile=arg, B_lo=lo.to(dev), **kw)
    else:
        layout, force_tile, precise = arg
        A, B, _ = _operands("f32" if precise else "bf16", shape)
        As = A if layout != ops.TN else A.t().contiguous()
        Bs = B if layout == ops.NT else B.t().contiguous()
        lda, ldb = (As.shape[1] + 7) // 8 * 8 + 8, (Bs.shape[1] + 7) // 8 * 8 + 8
        ops.gemm(layout, _pitched(As, lda, dev, 0.0), lda, _pitched(Bs, ldb, dev, 0.0), ldb, M, N, K, C, ldc, precise=precise,
                 force_tile=force_tile, **kw)


def _product(fam, shape):
    name, arg = fam
    kind = {"bf16": "bf16", "f32s": "f32", "h16": "h16", "h16x2": "h16x2"}.get(name) or ("f32" if arg[2] else "bf16")
    return _operands(kind, shape)[2]


def _run(dev, fam, shape, pitch, opts, *, act=0, gate_dtype=F32, resid_dtype=F32, c_dtype=F32, p=P_DROP, seed=SEED, step=STEP,
         gate_scale=1.25, alpha=0.5, alpha_dev=1.5):
    """Launch `fam` with the epilogue options in `opts` (subset of bias gate drop alpha alpha_dev resid colsum twin; act separately),
    check the result, the pad columns, the exactness conditions, the column sums and the twin.  Returns (C logical columns on the
    CPU, reference, keep mask or None, stored gate or None)."""
    name = fam[0]
    M, N, _ = shape
    ld = _pitches(N, pitch)
    bias_c, gate_c, resid_c = _epi_inputs(shape)
    kw, ref_kw = {}, {}
    if act:
        kw["act"] = ref_kw["act"] = act
    if "bias" in opts:
        kw["bias"] = bias_c.to(dev)
        ref_kw["bias"] = bias_c
    gate = None
    if "gate" in opts:
        gate = gate_c.to(gate_dtype)
        kw.update(gate=_pitched(gate, ld["ldg"], dev, 1.0), ldg=ld["ldg"], gate_scale=gate_scale)
        ref_kw.update(gate=gate, gate_scale=gate_scale)
    keep = None
    if "drop" in opts:
        keep = _keep_mask(dev, M, N, p, seed, step)
        kw.update(drop_p=p, seed=seed, seed_dev=torch.tensor([step], dtype=torch.int64, device=dev))
        ref_kw.update(keep=keep, p=p)
    a = 1.0
    if "alpha" in opts:
        kw["alpha"] = a = alpha
    if "alpha_dev" in opts:
        kw["alpha_dev"] = torch.tensor([alpha_dev], device=dev)
        a *= alpha_dev
    ref_kw["alpha"] = a
    resid = None
    if "resid" in opts:
        resid = resid_c.to(resid_dtype)
        kw.update(resid=_pitched(resid, ld["ldr"], dev, 100.0), ldr=ld["ldr"])
        ref_kw["resid"] = resid
    cs = None
    if "colsum" in opts:
        cs = kw["colsum"] = torch.full((N,), 3.0, device=dev)
    if "twin" in opts:
        kw["twin"] = True
    ref = _reference(_product(fam, shape), **ref_kw)
    C = torch.full((M, ld["ldc"]), SENT, dtype=c_dtype, device=dev)
    with _twin_provider() as made:
        _launch(fam, dev, shape, C, ld["ldc"], kw)
    Cc = C.cpu()
    out = Cc[:, :N]
    scale = float(ref.abs().max())
    err = float((out.double() - ref).abs().max()) / scale
    tol = _tol(fam, c_dtype)
    tag = f"{_fam_id(fam)} {shape} {pitch} act={act} opts={'+'.join(sorted(opts))} C={c_dtype}"
    print(f"EPI-ERR {name}{'-precise' if name == 'gemm' and fam[1][2] else ''} C-{str(c_dtype)[6:]} {err:.3e} {tol:g}   [{tag}]")
    assert err < tol, (tag, err, tol)
    assert bool((Cc[:, N:] == SENT).all()), f"{tag}: wrote outside the logical columns of C"
    # exactness: a dropped or gated-off element is alpha * 0 (+ resid), whatever the product was
    off = torch.zeros(M, N, dtype=torch.bool)
    if keep is not None:
        off |= ~keep
    if gate is not None:
        off |= ~(gate.float() > 0)
        for r, c, _ in _planted(M, N):
            assert bool(off[r, c]), "planted +-0.0 gate entries switch their element off"
    if c_dtype == F32 and bool(off.any()):
        if resid is not None:
            assert torch.equal(_bits(out[off]), _bits(resid.float()[off])), f"{tag}: a switched-off element is not resid bit for bit"
        else:
            assert bool((out[off] == 0).all()), f"{tag}: a switched-off element is not 0.0"
    if cs is not None:
        want = ref.sum(0)
        cerr = float((cs.cpu().double() - 3.0 - want).abs().max()) / float(want.abs().max())
        print(f"EPI-ERR {name} colsum {cerr:.3e} 1e-4   [{tag}]")
        assert cerr < 1e-4, (tag, cerr)
    if "twin" in opts and c_dtype != BF16:
        (y, tw), = made
        assert y is C
        twc = tw.cpu()
        assert bool((twc[:, N:] == SENT).all()), f"{tag}: wrote outside the logical columns of the twin"
        if c_dtype == F32:  # the twin is the bf16 rounding of the very values stored
            assert torch.equal(_bits(twc[:, :N]), _bits(out.bfloat16())), f"{tag}: twin != bf16(C)"
        else:  # f16 C: both are roundings of the same f32 value
            terr = float((twc[:, :N].double() - ref).abs().max()) / scale
            assert terr < 1e-2, (tag, terr)
    elif "twin" in opts:
        assert not made, "a bf16 result has no twin"
    return out, ref, keep, gate


def _everything(fam):
    """The options of the everything-on launch that `fam` has."""
    name = fam[0]
    opts = {"bias", "drop", "alpha", "resid"}
    if "gate" in HAS[name]:
        opts |= {"gate", "alpha_dev"}
    if "colsum" in HAS[name]:
        opts.add("colsum")
    if name in ("h16", "h16x2"):
        opts.add("twin")
    return opts


# ---------------------------------------------------------------- (a) everything on, every tile


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fam", FAMILIES, ids=_fam_id)
def test_epilogue_everything_on(dev, fam, shape, pitch):
    """bias + act + gate * 1.25 + dropout 0.25 (seed + device step) + alpha 0.5 * device 1.5 + resid + column sums in ONE launch, per
    tile instantiation; silu and then relu (exact zeros); gate / resid / result dtypes rotate over the cases, and the relu launch
    stores the other result dtype than the silu launch."""
    name = fam[0]
    k = FAMILIES.index(fam) + 3 * SHAPES.index(shape) + 5 * PITCHES.index(pitch)
    for i, act in enumerate((2, 1)):
        kk = k + 4 * i
        c_dtype = F32 if not (kk >> 2) & 1 else (BF16 if (kk & 1 or "c_f16" not in HAS[name]) else F16)
        resid_dtype = BF16 if ((kk >> 1) & 1 and "resid_bf16" in HAS[name]) else F32
        _run(dev, fam, shape, pitch, _everything(fam), act=act, gate_dtype=BF16 if kk & 1 else F32, resid_dtype=resid_dtype,
             c_dtype=c_dtype)


# ---------------------------------------------------------------- (b) each step alone, default tile


ALONE = {
    "gate": dict(opts={"gate"}),
    "dropout": dict(opts={"drop"}),
    "silu": dict(opts=set(), act=2),
    "alpha_dev": dict(opts={"alpha_dev"}),
    "resid_bf16": dict(opts={"resid"}, resid_dtype=BF16),
}
DEFAULT_TILE = [("bf16", 0), ("f32s", 0), ("h16", 0), ("gemm", (ops.NT, 0, False))]
# (avsr_gemm_h16_nt has no gate / alpha_dev argument)
ALONE_CASES = [(f, s) for f in DEFAULT_TILE for s in ALONE if not (f[0] == "h16" and s in ("gate", "alpha_dev"))]


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fam,step_name", ALONE_CASES, ids=lambda v: v if isinstance(v, str) else _fam_id(v))
def test_epilogue_step_alone(dev, fam, step_name, shape, pitch):
    """One epilogue step per launch, so that a failure of the everything-on case names its step."""
    case = dict(ALONE[step_name])
    opts = case.pop("opts")
    if fam[0] == "gemm":
        case.pop("resid_dtype", None)  # avsr_gemm takes an f32 residual only
    _run(dev, fam, shape, pitch, opts, **case)


# ---------------------------------------------------------------- (c) exactness conditions


@pytest.mark.parametrize("with_resid", [True, False], ids=["resid", "noresid"])
@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fam", [("bf16", 0), ("f32s", 0)], ids=_fam_id)
def test_epilogue_exact_zeros(dev, fam, shape, pitch, with_resid):
    """f32 result: a dropped element or one whose gate is <= 0 (+0.0 and -0.0 included) is resid bit for bit, or 0.0 without a
    residual (asserted inside _run); the keep rate is 1 - p within 4 sigma; about half of the gate is positive."""
    M, N, _ = shape
    opts = {"bias", "gate", "drop", "alpha"} | ({"resid"} if with_resid else set())
    out, _, keep, gate = _run(dev, fam, shape, pitch, opts)
    n = M * N
    rate = float(keep.float().mean())
    assert abs(rate - (1 - P_DROP)) < 4 * math.sqrt(P_DROP * (1 - P_DROP) / n), rate
    assert 0.3 < float((gate > 0).float().mean()) < 0.7
    # the planted zeros decide something: at some of them the mask keeps the element and the product is not 0, so that a
    # kernel that let a zero gate pass would store something else than resid / 0.0 there
    live = [(r, c) for r, c, _ in _planted(M, N) if keep[r, c] and _product(fam, shape)[r, c] != 0]
    assert len(live) >= 2
    if not with_resid:
        kept_on = keep & (gate > 0)
        assert bool((out[kept_on] != 0).all()), "only switched-off elements are zero (no activation here)"


# ---------------------------------------------------------------- (d) the device-side step counter


@pytest.mark.parametrize("fam", [("bf16", 0), ("f32s", 0)], ids=_fam_id)
def test_epilogue_seed_dev_contract(dev, fam):
    """(seed, step s) is the generator of (seed + s, step 0) and not that of (seed, step s + 1)."""
    shape, s = SHAPES[0], 9
    M, N, _ = shape
    ldc = N + 3

    def run(seed, step):
        C = torch.full((M, ldc), SENT, device=dev)
        _launch(fam, dev, shape, C, ldc, dict(drop_p=P_DROP, seed=seed, seed_dev=torch.tensor([step], dtype=torch.int64, device=dev)))
        return C.cpu()

    a, b, c = run(SEED, s), run(SEED + s, 0), run(SEED, s + 1)
    assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(a[:, :N] != 0, _keep_mask(dev, M, N, P_DROP, SEED, s))
    both = float(((a[:, :N] != 0) & (c[:, :N] != 0)).float().mean())
    want = (1 - P_DROP) ** 2  # independent masks
    assert abs(both - want) < 4 * math.sqrt(want * (1 - want) / (M * N)), (both, want)


# ---------------------------------------------------------------- (e) / (f) one FFN: forward and backward share a mask


def _ffn(shape):
    """Inputs of one FFN (h W1^T + b1 -> relu -> dropout -> W2^T) and the gradient g of its output, once per shape."""

    def make():
        rows, d_ff, d_in = shape
        d_out = 128
        # The sign of the pre-activation decides relu and with it the gate.  The kernel forms the sum in f32 (2e-6 of the largest
        # magnitude is the project's bound for that), float64 here: draw inputs whose pre-activations all stay clear of zero by
        # that bound, so that both agree on every sign.
        for attempt in range(16):
            g = torch.Generator().manual_seed(1000 * attempt + rows + d_ff)
            h, W1 = torch.randn(rows, d_in, generator=g).bfloat16(), torch.randn(d_ff, d_in, generator=g).bfloat16()
            b1 = torch.randn(d_ff, generator=g)
            W2 = (0.1 * torch.randn(d_out, d_ff, generator=g)).bfloat16()
            gy = torch.randn(rows, d_out, generator=g).bfloat16()
            pre = h.double() @ W1.double().t() + b1.double()
            if float(pre.abs().min()) > 2e-6 * float(pre.abs().max()):
                return h, W1, b1, W2, gy
        raise AssertionError("no draw with every pre-activation clear of zero")

    return _cached(("ffn", shape), make)


def _ffn_reference(dev, shape, p):
    """float64 autograd through dropout_mask * relu(h W1^T + b1) . W2^T with the replayed mask: (keep, u, du, db1), du being the
    gradient of the pre-activation (what the gated GEMM produces) and db1 that of the bias (its column sums)."""

    def make():
        rows, d_ff, _ = shape
        h, W1, b1, W2, gy = _ffn(shape)
        keep = _keep_mask(dev, rows, d_ff, p, SEED, STEP)
        b1d = b1.double().requires_grad_()
        pre = h.double() @ W1.double().t() + b1d
        pre.retain_grad()
        u = keep.double() / (1.0 - p) * torch.relu(pre)
        (u @ W2.double().t()).backward(gy.double())
        return keep, u.detach(), pre.grad.detach(), b1d.grad.detach()

    return _cached(("ffn-ref", dev.type, shape, p), make)


def _ffn_forward(dev, shape, pitch, tile, p=P_DROP):
    rows, d_ff, d_in = shape
    h, W1, b1, _, _ = _ffn(shape)
    ldu = _pitches(d_ff, pitch)["ldc"]
    u = torch.full((rows, ldu), SENT, dtype=BF16, device=dev)
    ops.gemm_bf16_nt(h.to(dev), d_in, W1.to(dev), d_in, rows, d_ff, d_in, u, ldu, bias=b1.to(dev), act=1, drop_p=p, seed=SEED,
                     seed_dev=torch.tensor([STEP], dtype=torch.int64, device=dev), tile=tile)
    return u, ldu


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ffn_forward_backward_share_mask(dev, shape, pitch):
    """u = dropout(relu(h W1^T + b1)) into a pitched bf16 buffer; du = (g W2) gated by u with scale 1 / (1 - p), db1 = its column
    sums: u, du and db1 against float64 autograd with the replayed mask; u == 0 means du == 0 exactly."""
    rows, d_ff, _ = shape
    p = P_DROP
    _, _, _, W2, gy = _ffn(shape)
    d_out = W2.shape[0]
    _, u_ref, du_ref, db1_ref = _ffn_reference(dev, shape, p)
    u, ldu = _ffn_forward(dev, shape, pitch, 0)
    uc = u.cpu()
    assert bool((uc[:, d_ff:] == SENT).all())
    err_u = float((uc[:, :d_ff].double() - u_ref).abs().max() / u_ref.abs().max())
    assert err_u < 1e-2, err_u
    assert torch.equal(uc[:, :d_ff] != 0, u_ref != 0), "forward mask / relu pattern"
    W2T = W2.t().contiguous()  # [d_ff, d_out]
    for c_dtype, tol in ((F32, 2e-6), (BF16, 1e-2)):
        ldd = _pitches(d_ff, pitch)["ldr"]
        du = torch.full((rows, ldd), SENT, dtype=c_dtype, device=dev)
        db1 = torch.zeros(d_ff, device=dev)
        ops.gemm_bf16_nt(gy.to(dev), d_out, W2T.to(dev), d_out, rows, d_ff, d_out, du, ldd, gate=u, ldg=ldu, gate_scale=1.0 / (1.0 - p),
                         colsum=db1)
        duc = du.cpu()
        assert bool((duc[:, d_ff:] == SENT).all())
        err = float((duc[:, :d_ff].double() - du_ref).abs().max() / du_ref.abs().max())
        cerr = float((db1.cpu().double() - db1_ref).abs().max() / db1_ref.abs().max())
        print(f"EPI-ERR bf16 ffn-du-{str(c_dtype)[6:]} {err:.3e} {tol:g}   [{shape} {pitch}]")
        print(f"EPI-ERR bf16 ffn-db1 {cerr:.3e} 1e-4   [{shape} {pitch}]")
        assert err < tol, err
        assert cerr < 1e-4, cerr
        assert bool((duc[:, :d_ff][uc[:, :d_ff] == 0] == 0).all()), "u == 0 must give du == 0 exactly"


@pytest.mark.parametrize("tile", [1, 7])
@pytest.mark.parametrize("split", [1, 2])
def test_ffn_backward_paired_launch(dev, tile, split):
    """The gated data-gradient GEMM (with column sums) and the TN weight gradient g^T u (with colsum_a) as ONE paired launch:
    bit-equal to the two separate launches (same tile kernels), column sums to summation order."""
    shape = SHAPES[1]  # d_ff = 136: the TN kernel needs N % 8 == 0 and a pitch that is a multiple of 8
    rows, d_ff, _ = shape
    p = P_DROP
    _, _, _, W2, gy = _ffn(shape)
    d_out = W2.shape[0]
    u, ldu = _ffn_forward(dev, shape, "vector", tile)
    g, W2T = gy.to(dev), W2.t().contiguous().to(dev)

    def nt(du, db1):
        ops.gemm_bf16_nt(g, d_out, W2T, d_out, rows, d_ff, d_out, du, d_ff + 8, gate=u, ldg=ldu, gate_scale=1.0 / (1.0 - p), colsum=db1,
                         tile=tile)

    def tn(dw, db2):
        ops.gemm_bf16_tn(g, d_out, u, ldu, d_out, d_ff, rows, dw, d_ff, accumulate=split > 1, split_k=split, colsum_a=db2)

    def buffers():
        return (torch.full((rows, d_ff + 8), SENT, dtype=BF16, device=dev), torch.zeros(d_ff, device=dev),
                torch.zeros(d_out, d_ff, device=dev), torch.zeros(d_out, device=dev))

    du0, db10, dw0, db20 = buffers()
    nt(du0, db10)
    tn(dw0, db20)
    du1, db11, dw1, db21 = buffers()
    with ops.paired():
        tn(dw1, db21)
        nt(du1, db11)
    assert torch.equal(_bits(du1.cpu()), _bits(du0.cpu())) and torch.equal(_bits(dw1.cpu()), _bits(dw0.cpu()))
    assert (db11 - db10).abs().max() <= 1e-4 * db10.abs().max()
    assert (db21 - db20).abs().max() <= 1e-4 * db20.abs().max()
    # and both are right: float64 with the replayed mask
    _, _, du_ref, db1_ref = _ffn_reference(dev, shape, p)
    duc = du1.cpu()
    assert float((duc[:, :d_ff].double() - du_ref).abs().max() / du_ref.abs().max()) < 1e-2
    assert bool((duc[:, d_ff:] == SENT).all())
    assert float((db11.cpu().double() - db1_ref).abs().max() / db1_ref.abs().max()) < 1e-4
    dw_ref = gy.double().t() @ u.cpu()[:, :d_ff].double()
    assert float((dw1.cpu().double() - dw_ref).abs().max() / dw_ref.abs().max()) < 2e-6
    want_db2 = gy.double().sum(0)
    assert float((db21.cpu().double() - want_db2).abs().max() / want_db2.abs().max()) < 1e-4


# ---------------------------------------------------------------- (g) the twin


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fam", [("f32s", 0), ("h16", 0), ("h16x2", 0)], ids=_fam_id)
def test_epilogue_twin(dev, fam, shape, pitch):
    """With a TWIN provider installed, C2 is bf16(C) bit for bit in the logical columns and untouched beyond them (asserted in _run)."""
    opts = {"bias", "drop", "alpha", "resid", "twin"}
    _run(dev, fam, shape, pitch, opts, act=2, c_dtype=F32)
    assert ops.TWIN is None


# ---------------------------------------------------------------- accumulating outputs: bias and alpha only


ENTRY = {"gemm": ("gemm", (ops.NT, 0, False)), "gemm_bf16_nt": ("bf16", 0), "gemm_f32s_nt": ("f32s", 0)}


@pytest.mark.parametrize("what", ["resid", "act", "gate", "drop"])
@pytest.mark.parametrize("entry", list(ENTRY))
def test_accumulate_rejects_nonlinear_epilogue(dev, entry, what):
    """An accumulating (split-K / "+=") output applies bias and alpha only: activation, gate, dropout and residual cannot be applied
    to partial sums and are refused at the entry point (host-side argument check, nothing is launched, C stays as it was)."""
    shape = SHAPES[0]
    M, N, _ = shape
    _, gate, resid = _epi_inputs(shape)
    kw = {"resid": dict(resid=resid.to(dev), ldr=N), "act": dict(act=1), "gate": dict(gate=gate.to(dev), ldg=N),
          "drop": dict(drop_p=0.1, seed=3)}[what]
    g = torch.Generator().manual_seed(5)
    C0 = torch.randn(M, N, generator=g)
    C = C0.clone().to(dev)
    with pytest.raises(_lib.AvsrLibraryError, match=rf"\b{entry}: accumulate"):
        _launch(ENTRY[entry], dev, shape, C, N, dict(accumulate=True, **kw))
    assert torch.equal(_bits(C.cpu()), _bits(C0))


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("fam", [("gemm", (ops.NT, 0, False)), ("gemm", (ops.TN, 64, True)), ("bf16", 0), ("bf16", 5), ("f32s", 0)], ids=_fam_id)
def test_accumulate_bias_alpha(dev, fam, split):
    """C += alpha * alpha_dev * (A B^T + bias), one and three k splits (the bias enters once, on the lead split)."""
    shape = SHAPES[1]  # K = 192: three k-tiles
    M, N, _ = shape
    bias, _, _ = _epi_inputs(shape)
    g = torch.Generator().manual_seed(6)
    C0 = torch.randn(M, N + 3, generator=g)
    for with_dev in (False, True):
        C = C0.clone().to(dev)
        kw = dict(bias=bias.to(dev), alpha=0.5, accumulate=True, split_k=split)
        if with_dev:
            kw["alpha_dev"] = torch.tensor([1.5], device=dev)
        _launch(fam, dev, shape, C, N + 3, kw)
        ref = C0[:, :N].double() + (0.75 if with_dev else 0.5) * (_product(fam, shape) + bias.double())
        Cc = C.cpu()
        err = float((Cc[:, :N].double() - ref).abs().max() / ref.abs().max())
        tol = _tol(fam, F32)
        print(f"EPI-ERR {fam[0]} accumulate {err:.3e} {tol:g}   [{_fam_id(fam)} split={split} alpha_dev={with_dev}]")
        assert err < tol, err
        assert torch.equal(_bits(Cc[:, N:]), _bits(C0[:, N:])), "wrote outside the logical columns"
