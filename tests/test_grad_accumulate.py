"""Gradient accumulation in the native training step (Trainer(accumulate_grad_batches=K)): the multi-tensor accumulate kernel
(csrc/optim.hip: avsr_grad_accumulate) against float64, optim.GradAccumulator under a hipGraph, train_native.NativeStepper's open
and closing micro-steps against a manual composition, the loop's step arithmetic, graph replay against eager launches, two ranks
on gloo and train.py's flag.  After the closing micro-step of a window the gradient handed to clip + AdamW is

    G = (sum over ranks and micro-steps of grad loss_{r,k}) / (sum over ranks and micro-steps of B_{r,k})

Error bound of the accumulator, element-wise, from K - 1 f32 additions, one reciprocal and one product (u = 2^-24):
    |acc - G| <= (K + 2) u sum_k |g_k| / sum B"""
import math
import os
import sys
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

U = 2.0 ** -24
SHAPES = [(1,), (7,), (4096,), (4097,), (33, 5), (5049,), (3, 1, 5, 7, 7)]
MISALIGNED = 3  # index into SHAPES of the gradient handed over as a view one float into a larger buffer


def small_e2e(odim=30):
    from auto_avsr_amd.e2e import E2E

    torch.manual_seed(0)
    m = E2E(odim, "video", adim=128, aheads=2, eunits=64, elayers=1, dunits=64, dlayers=1, cnn_module_kernel=7)
    return m


def no_dropout(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    return m


def make_grads(seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, s in enumerate(SHAPES):
        n = math.prod(s)
        if i == MISALIGNED:
            buf = (torch.randn(n + 9, generator=g) * scale).to(dev)
            t = buf[1:1 + n].view(s)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        else:
            t = (torch.randn(s, generator=g) * scale).to(dev)
        out.append(t)
    return out


def check_window(acc, windows, sizes, K, extra=0):
    """acc.grads against sum_k g_k / sum B in float64, within (K + extra + 2) u sum_k |g_k| / sum B."""
    tot = float(sum(sizes))
    for i, a in enumerate(acc.grads):
        ref = sum(gs[i].double().cpu() for gs in windows) / tot
        mag = sum(gs[i].double().cpu().abs() for gs in windows) / tot
        err = (a.double().cpu() - ref).abs()
        bad = err > (K + extra + 2) * U * mag
        assert not bool(bad.any()), (i, SHAPES[i], float(err.max()), float(((K + extra + 2) * U * mag).max()))


@pytest.mark.parametrize("K", [1, 3])
def test_accumulate_kernel_against_f64(dev, K):
    """Two windows of K micro-steps (B = 3, 1, 5) back to back on one accumulator that starts full of NaN: position 0 overwrites,
    later micro-steps add, the closing one adds and divides by the window's total batch size; the window record is (0, 0) after
    each close.  One gradient is a view at a 4-byte offset."""
    from auto_avsr_amd.optim import GradAccumulator

    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SHAPES]
    acc = GradAccumulator(params)
    assert [tuple(g.shape) for g in acc.grads] == SHAPES and all(g.data_ptr() % 16 == 0 for g in acc.grads)
    assert all(g.untyped_storage().data_ptr() == acc.flat.untyped_storage().data_ptr() for g in acc.grads)
    acc.flat.fill_(float("nan"))
    sizes = [3, 1, 5][:K]
    for window in range(2):
        gs = [make_grads(100 * window + k, dev, scale=(3.0, 0.3, 1.0)[k]) for k in range(K)]
        for k in range(K):
            assert acc.position == (k, float(sum(sizes[:k])))
            acc.add(gs[k], sizes[k], close=k == K - 1)
        assert acc.position == (0, 0.0)
        assert all(bool(torch.isfinite(a).all()) for a in acc.grads)
        check_window(acc, gs, sizes, K)


@pytest.mark.gpu
def test_one_open_graph_serves_any_position():
    """ONE captured open add() on static gradient tensors, replayed at position 0 and at position 1 of a window with different
    contents, then an eager close: the f64 combination of the three.  (Whether a micro-step is the first of its window is read
    from the device record, not baked into the launch.)"""
    from auto_avsr_amd.optim import GradAccumulator

    dev = torch.device("cuda:0")
    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SHAPES]
    acc = GradAccumulator(params)
    acc.flat.fill_(float("nan"))
    static = make_grads(7, dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.add(static, 3, close=False)
    torch.cuda.synchronize()
    assert acc.position == (0, 0.0) and acc.captured_tables() == 1  # (a capture runs nothing)
    windows = [make_grads(11, dev, 3.0), make_grads(12, dev, 0.3), make_grads(13, dev)]
    for k in range(2):
        for s, g in zip(static, windows[k]):
            s.copy_(g)
        graph.replay()
        assert acc.position == (k + 1, 3.0 * (k + 1))
    acc.add(windows[2], 5, close=True)
    assert acc.position == (0, 0.0)
    check_window(acc, windows, [3, 3, 5], 3)


def _stepper_args(**kw):
    a = types.SimpleNamespace(lr=1e-3, weight_decay=0.03, warmup_epochs=1, max_epochs=2, accumulate_grad_batches=2, no_graph=True)
    a.__dict__.update(kw)
    return a


def _manual_grads(model, batches):
    """forward_tensors + backward by hand: per batch, the gradient of every parameter in float64 on the host."""
    from auto_avsr_amd import functional as AF

    out = []
    for x, lens, y in batches:
        for p in model.parameters():
            p.grad = None
        AF.new_step()
        AF.refresh_weight_cache()
        model.forward_tensors(x, lens, y)[0].backward()
        out.append([p.grad.detach().double().cpu() for p in model.parameters()])
    for p in model.parameters():
        p.grad = None
    return out


def test_stepper_against_manual_composition(dev):
    """K = 2, two batches of different shape.  The open micro-step leaves every parameter and the step counter alone; after the
    closing one the accumulator holds (g1 + g2) / (B1 + B2) of a by-hand forward / backward on an identically initialised clone,
    and the parameters are those of one FusedAdamW step on that gradient."""
    from synth import synth_batch

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import train_native as TN
    from auto_avsr_amd.optim import FusedAdamW

    batches = [synth_batch("video", 2, 3, 1, 30, seed=3, lengths=[3, 2]), synth_batch("video", 1, 2, 1, 30, seed=4, lengths=[2])]
    batches = [tuple(t.to(dev) for t in b) for b in batches]
    sizes = [b[2].shape[0] for b in batches]
    det = AF.deterministic()
    AF.set_deterministic(True)
    AF.invalidate_weight_cache()
    ns = None
    try:
        with AF.precise(dev.type == "cpu"):
            clone = no_dropout(small_e2e()).to(dev).train()
            manual = _manual_grads(clone, batches)
            AF.invalidate_weight_cache()
            m = no_dropout(small_e2e()).to(dev).train()
            init = [p.detach().clone() for p in m.parameters()]
            ns = TN.NativeStepper(m, _stepper_args(), dev, 0, 1, 4, log=lambda s: None)
            assert ns.opt.warmup_steps == 2 and ns.opt.total_steps == 4  # ceil(4 / 2) optimizer steps per epoch
            ns(*batches[0])
            assert not ns.closed_last and ns.opt.step_count == 0 and ns.acc.position == (1, float(sizes[0]))
            assert all(torch.equal(p.detach(), q) for p, q in zip(m.parameters(), init))
            ns(*batches[1])
            assert ns.closed_last and ns.opt.step_count == 1 and ns.acc.position == (0, 0.0) and ns.micro_steps == 2
            tot = float(sum(sizes))
            ref = [(a + b) / tot for a, b in zip(*manual)]
            for a, r, g1, g2 in zip(ns.acc.grads, ref, *manual):
                err = (a.double().cpu() - r).abs()
                assert not bool((err > 4 * U * (g1.abs() + g2.abs()) / tot).any()), float(err.max())
            AF.invalidate_weight_cache()
            opt = FusedAdamW(clone.parameters(), lr=1e-3, betas=(0.9, 0.98), weight_decay=0.03, max_grad_norm=10.0, warmup_steps=2,
                             total_steps=4)
            for p, r in zip(clone.parameters(), ref):
                p.grad = r.float().to(dev)
            opt.step()
            assert opt.step_count == 1
            for p, q in zip(m.parameters(), clone.parameters()):
                assert (p.detach() - q.detach()).abs().max() <= 2e-6 * max(1.0, float(q.detach().abs().max()))
            assert any(not torch.equal(p.detach(), q) for p, q in zip(m.parameters(), init))
    finally:
        if ns is not None:
            ns.close()
        AF.set_deterministic(det)
        AF.invalidate_weight_cache()


def _loop_args(tmp, **kw):
    a = types.SimpleNamespace(modality="video", max_frames=6, train_num_buckets=4, lr=1e-3, weight_decay=0.03, warmup_epochs=1,
                              max_epochs=2, exp_dir=str(tmp), exp_name="run", ckpt_path=None, steps=None, val_batches=0,
                              synthetic_utterances=5, log_every=1, numerics="precise", synthetic=True)
    a.__dict__.update(kw)
    return a


def test_loop_arithmetic(emu_lib_path, tmp_path, monkeypatch):
    """Three batches per epoch, K = 2, two epochs: windows of 2 + 1 batches (the short one flushed at the epoch's end) = 4 optimizer
    steps; the schedule, --steps and the checkpoint count optimizer steps; accumulate_grad_batches=1 is today's loop bit for bit."""
    import numpy as np

    import auto_avsr_amd.synthetic as S
    from auto_avsr_amd import _lib
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import train_native as TN

    _lib._install_for_tests(emu_lib_path)
    monkeypatch.setattr(S, "utterance_lengths", lambda n=5, seed=42, lo=12, hi=400: np.array([2, 2, 3, 3, 4][:n]))
    made = []

    class Recording(TN.NativeStepper):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(TN, "NativeStepper", Recording)
    dev = torch.device("cpu")

    def run(tag, **kw):
        AF.invalidate_weight_cache()
        m = no_dropout(small_e2e()).train()
        losses = TN.fit(m, _loop_args(tmp_path / tag, **kw), dev, log=lambda s: None)
        return losses, [p.detach().clone() for p in m.parameters()], made[-1]

    try:
        losses, _, ns = run("k2", accumulate_grad_batches=2)
        assert ns.opt.step_count == 4 and len(losses) == 4 and ns.micro_steps == 6
        assert ns.opt.warmup_steps == 1 * 2 and ns.opt.total_steps == 2 * 2
        ck = torch.load(os.path.join(tmp_path, "k2", "run", "last.ckpt"))
        assert ck["global_step"] == 4 and ck["micro_step"] == 6 and ck["epoch"] == 1
        assert int(ck["optimizer"]["state"][0]) == 4
        losses, _, ns = run("k2s3", accumulate_grad_batches=2, steps=3, exp_dir=None)
        assert ns.opt.step_count == 3 and len(losses) == 3 and ns.micro_steps == 5  # 2 + 1 batches of epoch 0, 2 of epoch 1
        # (deterministic: the emulator's worker threads commit atomic sums in a run-dependent order otherwise)
        l1, w1, ns1 = run("k1", accumulate_grad_batches=1, exp_dir=None, steps=2, deterministic=True)
        l0, w0, ns0 = run("plain", exp_dir=None, steps=2, deterministic=True)
        assert ns1.acc is None and ns1.opt.step_count == ns0.opt.step_count == 2 and ns0.opt.warmup_steps == ns1.opt.warmup_steps == 3
        assert l1 == l0 and len(l0) == 2 and all(torch.equal(a, b) for a, b in zip(w1, w0))
    finally:
        _lib._lib = None
        AF.invalidate_weight_cache()


@pytest.mark.gpu
def test_accumulating_fit_graph_replay_equals_eager(tmp_path, monkeypatch):
    """The pattern of test_native_fit_graph_replay_equals_eager with K = 2 and three batches per epoch (windows of 2 + 1: every
    shape turns up as an open and as a closing micro-step): mixed mode, dropout 0.1, six epochs; open and closing graphs are both
    captured and replayed, the eager run replays nothing, and the two runs agree."""
    import numpy as np

    import auto_avsr_amd.synthetic as S
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import train_native as TN

    dev = torch.device("cuda")
    monkeypatch.setattr(S, "utterance_lengths", lambda n=5, seed=42, lo=12, hi=400: np.array([12, 12, 16, 16, 20][:n]))
    runs = {}
    for tag, no_graph in (("eager", True), ("graph", False)):
        AF.invalidate_weight_cache()
        m = small_e2e().to(dev).train()
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.1
        args = _loop_args(tmp_path / tag, max_frames=32, max_epochs=6, numerics="mixed", no_graph=no_graph, exp_dir=None,
                          accumulate_grad_batches=2)
        runs[tag] = (TN.fit(m, args, dev, log=lambda s: None), TN.fit.last_stats,
                     {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items() if v.is_floating_point()})
    (le, se, we), (lg, sg, wg) = runs["eager"], runs["graph"]
    print("stats eager", se, "graph", sg)
    print("losses eager", le, "graph", lg)
    assert se["replayed"] == 0 and se["captured"] == 0 and se["eager"] == 18
    for kind in ("open", "close"):
        assert sg[kind]["captured"] >= 1 and sg[kind]["replayed"] >= 2 * sg[kind]["captured"], sg
    assert sg["open"]["eager"] + sg["open"]["replayed"] == 6 and sg["close"]["eager"] + sg["close"]["replayed"] == 12, sg
    assert len(le) == len(lg) == 12
    for a, b in zip(le, lg):
        assert abs(a - b) <= 5e-3 * abs(a), (le, lg)
    num = sum(float((we[k] - wg[k]).norm() ** 2) for k in we) ** 0.5
    den = sum(float(we[k].norm() ** 2) for k in we) ** 0.5
    assert num <= 3e-2 * den, num / den
    assert AF.mode() == "bf16"
    AF.invalidate_weight_cache()


def _worker_two_ranks(rank, world, port, emu_path, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(HERE, "golden"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from synth import synth_batch

    from auto_avsr_amd import _lib
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd import train_native as TN

    _lib._install_for_tests(emu_path)
    AF.set_precise(True)
    AF.set_deterministic(True)
    K = 2
    shapes = [[(2, [3, 2]), (1, [2])], [(1, [3]), (2, [4, 2])]][rank]  # (B, lengths) per micro-step: ragged across ranks too
    batches = [synth_batch("video", b, max(ls), 1, 30, seed=20 + 2 * rank + k, lengths=ls) for k, (b, ls) in enumerate(shapes)]
    sizes = [float(b[2].shape[0]) for b in batches]
    # this rank's two gradients by hand on a clone, cross-rank BatchNorm as in the step (both ranks move in lockstep)
    AF.set_bn_sync(dist.group.WORLD)
    clone = no_dropout(small_e2e()).train()
    manual = _manual_grads(clone, batches)
    flat = lambda gs: torch.cat([g.flatten() for g in gs])  # noqa: E731
    gsum, gabs = flat(manual[0]) + flat(manual[1]), flat(manual[0]).abs() + flat(manual[1]).abs()
    total = torch.tensor([sum(sizes)], dtype=torch.float64)
    for t in (gsum, gabs, total):
        dist.all_reduce(t)
    AF.invalidate_weight_cache()
    m = no_dropout(small_e2e()).train()
    ns = TN.NativeStepper(m, _stepper_args(accumulate_grad_batches=K), torch.device("cpu"), rank, world, 4, log=lambda s: None)
    n_flat = ns.acc.flat.numel()
    big, orig = [], dist.all_reduce

    def counting(t, *a, **kw):
        if t.numel() >= sum(p.numel() for p in m.parameters()):
            big.append(t.numel())
        return orig(t, *a, **kw)

    dist.all_reduce = counting
    try:
        ns(*batches[0])
        assert big == [] and ns.opt.step_count == 0
        ns(*batches[1])
    finally:
        dist.all_reduce = orig
    assert big == [n_flat], big  # exactly one gradient-sized collective per window
    assert ns.opt.step_count == 1 and ns.acc.position == (0, 0.0)
    got = flat([g.detach().double() for g in ns.acc.grads])
    err = (got - gsum / total).abs()
    bound = (K + world + 2) * U * gabs / total
    assert not bool((err > bound).any()), (float(err.max()), float(bound.max()))
    params = torch.cat([p.detach().flatten() for p in m.parameters()])
    other = [torch.zeros_like(params) for _ in range(world)]
    dist.all_gather(other, params)
    assert torch.isfinite(params).all() and torch.equal(other[0], other[1])
    ns.close()
    assert AF._state["bn_sync"] is None
    if rank == 0:
        open(os.path.join(out_dir, "ok"), "w").write("1")
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_accumulate(emu_lib_path, tmp_path):
    """Two gloo ranks, K = 2: no DDP wrapper -- each rank accumulates its own window, the closing micro-step all-reduces the
    window's batch-size sum (one float), scales by the global total and all-reduces the flat accumulator ONCE.  Each rank's
    accumulator matches the f64 combination of all four local gradients within (K + world + 2) u sum |g| / sum B, and the
    replicas are bit-identical after the optimizer step."""
    port = 39500 + os.getpid() % 2000
    mp.spawn(_worker_two_ranks, args=(2, port, emu_lib_path, str(tmp_path)), nprocs=2, join=True)
    assert os.path.exists(os.path.join(tmp_path, "ok"))


def test_train_py_flag():
    """train.py --accumulate-grad-batches N: Lightning's name, N >= 1."""
    sys.path.insert(0, ROOT)
    import train

    assert train.parse_args([]).accumulate_grad_batches == 1
    assert train.parse_args(["--accumulate-grad-batches", "4"]).accumulate_grad_batches == 4
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit):
            train.parse_args(["--accumulate-grad-batches", bad])


def test_trainer_native_step_refuses_accumulation():
    """--trainer-step native under a Lightning Trainer (ModelModule.on_fit_start builds the NativeStepper there) refuses N > 1:
    nothing tells training_step which batch ends an epoch, so a short last window would never be flushed."""
    sys.path.insert(0, ROOT)
    import lightning as LM
    from auto_avsr_amd import functional as AF

    mod = LM.ModelModule.__new__(LM.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.args = types.SimpleNamespace(trainer_step="native", accumulate_grad_batches=2, numerics="precise")
    mod.native_step, mod._native = True, None
    before = AF.mode()
    try:
        with pytest.raises(ValueError, match="accumulate-grad-batches"):
            mod.on_fit_start()
    finally:
        mod.on_fit_end()
    assert AF.mode() == before
