#!/usr/bin/env python
"""bench.py -- throughput of the auto_avsr training hot path (E2E forward + backward, video modality,
12-layer Conformer / 6-layer decoder, --max-frames 1600 length-bucketed synthetic batches) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

N > 1 is launched by the driver as `python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`
(one rank per GPU, RCCL).  Rank 0 prints ONE JSON line: whole-job real (un-padded) video frames per second.

A plain run does only what that headline figure needs: set-up, warm-up, the timed steps, --dump-outputs, the line.
`--full` adds everything else the benchmark measures or checks, each in runs of its own AFTER the timed steps (N = 1):
`roofline` (dominant kernel family, MFMA bound; + the HBM-bound family), `parity` (error against the reference goldens),
`bf16` / `hpf` (the same workload timed in another numerical mode) and `cpu_baseline` (the oracle timed on the host cores);
N > 1: `config.bucket_overlap` (one more eager step with an event pair around every gradient bucket).
"""
import argparse
import json
import os
import sys
import time

T_START = time.perf_counter()  # (before `import torch`: the set-up figure printed to stderr counts the imports)
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-frames", type=int, default=1600)
    ap.add_argument("--modality", default="video")
    ap.add_argument("--babble", action="store_true",
                    help="audio only: configs[3] as specified -- every timed step starts from RAW waveforms and runs the reference's "
                         "AudioTransform('train') (time mask + babble noise at SNR 0 dB + layer norm) + padding collation on the device")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything besides the headline figure: roofline legs, parity "
                         "blocks against the reference goldens, the bf16 leg (--hpf-leg: the hpf leg too), the CPU baseline; N > 1: the "
                         "per-bucket overlap timing.  Off by default: a plain run sets up, warms up, times the steps and prints its line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the `cpu_baseline` object")
    ap.add_argument("--no-roofline", action="store_true", help="--full without the `roofline*` objects")
    ap.add_argument("--deterministic", action="store_true", help="time the bit-reproducible variant of the step (functional.set_deterministic)")
    ap.add_argument("--precise", action="store_true", help="parity mode (split-bf16 contractions) instead of bf16")
    ap.add_argument("--mode", choices=["bf16", "precise", "hpf", "mixed"], default=None,
                    help="numerical mode of the timed steps (functional.set_mode).  mixed (default): the mode that meets the north "
                         "star's 1e-3 bound on logits / CTC log-probabilities at the lowest cost -- forward contractions on IEEE-half "
                         "operands (encoder, trunk, decoder) or split bf16 planes (stem, projections, CTC head), bf16 backward; "
                         "bf16: bf16 operands everywhere (fastest, logits 7e-3 off the fp32 reference); hpf: every forward "
                         "contraction on split planes; precise: split planes forward and backward")
    ap.add_argument("--no-precise-leg", "--no-bf16-leg", dest="no_second_leg", action="store_true",
                    help="--full without the extra `bf16` object of the JSON line (throughput + parity of the plain bf16 mode on the "
                         "same workload, N = 1 video)")
    ap.add_argument("--hpf-leg", action="store_true",
                    help="--full only: also time the hpf mode (every forward contraction on split planes) -> object `hpf` of the "
                         "JSON line")
    ap.add_argument("--shapes", type=int, default=8,
                    help="distinct length-bucketed batch shapes cycled through (spread over the bucket list; the longest "
                         "bucket, T = 400, is always one of them)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay (N=1)")
    ap.add_argument("--no-optimizer", action="store_true",
                    help="time forward + backward only (default: the full training step incl. clip + AdamW + LR schedule)")
    ap.add_argument("--fixed", choices=["A", "B"], default=None,
                    help="time ONE fixed batch instead of the bucketed workload: the survey's batch A (4 x 400 frames, 64 "
                         "labels) or batch B (16 x 100, 16 labels), SURVEY.md section 8d")
    ap.add_argument("--no-parity", action="store_true", help="--full without the parity blocks (reference goldens at batches A and B)")
    ap.add_argument("--ddp", choices=["auto", "torch", "buckets", "buckets-graph", "buckets-graph1"], default="auto",
                    help="N > 1 gradient exchange.  buckets-graph: this build's bucketed RCCL all-reduce (auto_avsr_amd/ddp.py) with every "
                         "collective of the step issued through RCCL's C API as a plain stream operation (auto_avsr_amd/comm.py) on two "
                         "communicators, the WHOLE data-parallel step captured into hipGraphs (one-rank evidence: 20.1 ms / step against "
                         "31.2 ms for torch DDP's eager step, profiles/r3_dp1_*.json); buckets-graph1: the same on ONE communicator (strict "
                         "issue order); buckets: the same exchange on torch.distributed, eager launches; torch: DistributedDataParallel, "
                         "eager launches.  auto (default): buckets-graph -> buckets-graph1 -> torch, each attempt in fresh worker "
                         "processes under a wall-clock limit (supervise(): a dead-locked collective is a hang, not an exception)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy (rank 0): the loss, "
                         "the optimizer state, the BatchNorm running statistics and a fixed, seeded sample of the updated "
                         "parameters and Adam moments (gradients too when the step runs eagerly), so that two builds can be "
                         "compared output for output on identical inputs")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)  # a rank process started by supervise()
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.hpf_leg and not args.full:
        ap.error("--hpf-leg is one of the extra legs: it needs --full")
    return args


# round 5: the chain STARTS at the order-safe single-communicator mode (the first N > 1 execution of this code is the driver's: a
# hang in the two-communicator mode would burn its limit before anything is measured); `--ddp buckets-graph` / AVSR_DDP opt in
DDP_CHAIN = ["buckets-graph1", "buckets", "torch"]


def supervise(args):
    """N > 1 entry.  This process does not touch a GPU: it runs the rank process(es) of the data-parallel bench as children and
    watches the clock, because the failure mode of a multi-rank collective is a HANG, not an exception -- a communicator whose
    peers disagree on the order of two collectives spins in a kernel forever, and nothing inside that process can recover.

    * launched by `python -m torch.distributed.run ... bench.py --gpus N` (RANK / WORLD_SIZE in the environment, what the driver
      does): one child = this rank's worker;  launched as plain `python bench.py --gpus N`: the N workers of one node, started
      here with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set (127.0.0.1) -- no torchrun needed;
    * attempt k runs the workers in data-parallel mode DDP_CHAIN[k] on its own rendezvous port (MASTER_PORT + 1 + k) with a
      wall-clock limit; a worker that fails or overruns is killed (whole process group) and the next, more conservative mode is
      tried: buckets-graph1 (bucketed exchange + cross-rank BatchNorm on ONE RCCL communicator through the C API, whole step
      replayed as hipGraphs: every collective of a rank in one issue order, which is the same program order on every rank --
      cannot dead-lock on ordering) -> buckets (the same exchange over torch.distributed, eager launches) -> torch
      (DistributedDataParallel + c10d collectives, eager launches).  `--ddp buckets-graph` (two communicators, so that the
      latency-bound BatchNorm collectives do not queue behind 64 MB buckets) is opt-in: it needs two collective kernels
      co-resident, which no hardware run has confirmed.  Every supervisor applies the same limits, so the ranks move on together;
    * rank 0's JSON line (stdout of its worker) is printed once, by this process, after the attempt that succeeded."""
    import signal
    import subprocess

    world_env = "WORLD_SIZE" in os.environ and "RANK" in os.environ
    if world_env:
        assert int(os.environ["WORLD_SIZE"]) == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={os.environ['WORLD_SIZE']}"
        ranks = [int(os.environ["RANK"])]
    else:
        ranks = list(range(args.gpus))
    base_port = int(os.environ.get("MASTER_PORT", "29500"))
    want = os.environ.get("AVSR_DDP") or args.ddp
    chain = DDP_CHAIN if want == "auto" else [want]
    limits = [float(x) for x in os.environ.get("AVSR_BENCH_ATTEMPT_TIMEOUT", "300,240,240").split(",")]
    argv = [a for a in sys.argv[1:] if a != "--worker"]
    live = []

    def reap(signum=None, frame=None):  # the launcher (torchrun, the driver) is taking this supervisor down: take the workers along
        for pr in live:
            if pr.poll() is None:
                try:
                    os.killpg(pr.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
        if signum is not None:
            sys.exit(128 + signum)

    signal.signal(signal.SIGTERM, reap)
    signal.signal(signal.SIGINT, reap)
    for attempt, mode in enumerate(chain):
        limit = limits[min(attempt, len(limits) - 1)]
        procs = []
        for r in ranks:
            env = dict(os.environ, AVSR_DDP=mode, AVSR_BENCH_ATTEMPT=str(attempt), MASTER_PORT=str(base_port + 1 + attempt),
                       MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), WORLD_SIZE=str(args.gpus), RANK=str(r))
            if not world_env:
                env["LOCAL_RANK"] = str(r)
            # (under torchrun the env:// rendezvous would look for the AGENT's store on MASTER_PORT; the workers of an attempt
            # rendezvous among themselves: rank 0's worker serves the store on this attempt's port)
            env["TORCHELASTIC_USE_AGENT_STORE"] = "False"
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv + ["--worker"], env=env,
                                          stdout=subprocess.PIPE if r == 0 else sys.stderr, text=True, start_new_session=True))
        live[:] = procs  # (only rank 0's JSON line reaches this process's stdout; everything else any worker prints goes to stderr)
        t0 = time.time()
        out0, failed = None, None
        try:
            for r, pr in zip(ranks, procs):
                left = max(1.0, limit - (time.time() - t0))
                o, _ = pr.communicate(timeout=left)
                if r == 0:
                    out0 = o
                if pr.returncode != 0 and failed is None:
                    failed = f"rank {r} exited with code {pr.returncode}"
        except subprocess.TimeoutExpired:
            failed = f"no result within {limit:.0f} s (hang guard)"
        if failed is not None:
            for pr in procs:  # the whole process group of every worker: RCCL helper threads / children included
                if pr.poll() is None:
                    try:
                        os.killpg(pr.pid, signal.SIGKILL)
                    except ProcessLookupError:
                        pass
            for pr in procs:
                try:
                    pr.wait(timeout=30)
                except subprocess.TimeoutExpired:
                    pass
            nxt = f"; falling back to --ddp {chain[attempt + 1]}" if attempt + 1 < len(chain) else ""
            print(f"[bench supervisor, ranks {ranks}] attempt {attempt} (--ddp {mode}) failed: {failed}{nxt}", file=sys.stderr, flush=True)
            continue
        if out0 is not None:
            lines = [ln for ln in out0.splitlines() if ln.startswith("{")]
            for ln in out0.splitlines():
                if not ln.startswith("{"):
                    print(ln, file=sys.stderr)
            if lines:
                print(lines[-1], flush=True)
        return 0
    return 1


def cpu_baseline(modality, odim):
    """The oracle (CPU restatement of the reference graph) on a bounded sample of the same workload: one warm-up
    iteration + three timed iterations of forward + backward, min and median reported."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import statistics

    import avsr_oracle as O
    from synth import synth_state_dict

    from auto_avsr_amd.e2e import E2E
    from auto_avsr_amd.synthetic import make_batch

    cores = min(os.cpu_count() or 1, 32)  # ATen's CPU kernels stop scaling (and thrash) far below 256 threads
    torch.set_num_threads(cores)
    tmpl = E2E(odim, modality)
    sd = synth_state_dict(tmpl.state_dict(), 0)
    del tmpl
    sd = {k: (v.requires_grad_() if v.is_floating_point() and "running_" not in k else v) for k, v in sd.items()}
    lengths = [400, 380, 360, 340]  # the survey's batch A, all four utterances (round 4 timed the first two): 1480 real frames per iteration
    x, lens, y, frames = make_batch(lengths, [0, 1, 2, 3], modality, odim, seed=1)
    times = []
    for it in range(3):
        for v in sd.values():
            if v.is_floating_point():
                v.grad = None
        t0 = time.time()
        (loss, *_), _ = O.e2e_forward(sd, x, lens, y, modality=modality)
        loss.backward()
        if it:
            times.append(time.time() - t0)
    med = statistics.median(times)
    return {"value": round(frames / med, 2), "unit": "video-frames/sec", "cores": cores, "kind": "port",
            "value_best": round(frames / min(times), 2),
            "sample": f"fwd+bwd of the fp32 oracle (oracle/avsr_oracle.py, a CPU restatement pinned against the reference: "
                      f"/root/reference does not exist on the GPU box, so the reference E2E itself cannot be timed here) on "
                      f"{cores} threads, SURVEY batch A (B=4 T=400, {frames} real frames per iteration), 1 warm-up + 2 timed "
                      f"iterations: median {med:.2f}s, min {min(times):.2f}s",
            "reference_itself": {"value": 85.5, "unit": "video-frames/sec", "cores": 8,
                                 "note": "the reference's own E2E fwd+bwd on batch A, measured in the survey container "
                                         "(BASELINE.md section 3); not re-measurable on the GPU box"}}


DUMP_SAMPLE = 1 << 20  # elements drawn from the 250M flat parameter vector (4 MB per sampled array)
DUMP_SEED = 20240501


def dump_outputs(out_dir, loss, model, opt, with_grads):
    """--dump-outputs: what the last timed step handed back, as float32 .npy files in out_dir.  loss: the step's loss;
    optimizer_state: [step, lr, grad norm, clip coefficient]; bn_running_stats: every BatchNorm running mean / variance, in
    named_buffers() order; params / exp_avg / exp_avg_sq (/ grads, eager steps only: a replayed graph keeps its gradients in
    its own memory pool): the same DUMP_SAMPLE positions of the flat concatenation of the trainable parameters (model order),
    drawn with a fixed seed, sorted -- every position when the model is smaller than the sample."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    params = [p for p in model.parameters() if p.requires_grad]
    sizes = [p.numel() for p in params]
    total = sum(sizes)
    if total <= DUMP_SAMPLE:
        idx = torch.arange(total)
    else:
        idx = torch.randint(0, total, (DUMP_SAMPLE,), generator=torch.Generator().manual_seed(DUMP_SEED)).sort().values

    def sample(tensors):
        parts, off = [], 0
        for t, n in zip(tensors, sizes):
            lo, hi = torch.searchsorted(idx, torch.tensor([off, off + n])).tolist()
            if hi > lo:
                parts.append(t.detach().reshape(-1)[(idx[lo:hi] - off).to(t.device)].float().cpu())
            off += n
        return torch.cat(parts).numpy()

    arrays = {"loss": np.asarray(float(loss.detach()), dtype=np.float32),
              "bn_running_stats": torch.cat([b.detach().reshape(-1).float().cpu() for n, b in model.named_buffers()
                                             if b.is_floating_point() and "running_" in n]).numpy(),
              "params": sample(params)}
    if opt is not None:
        arrays.update(optimizer_state=opt.state.detach().float().cpu().numpy(), exp_avg=sample(opt.exp_avg),
                      exp_avg_sq=sample(opt.exp_avg_sq))
    if with_grads and all(p.grad is not None for p in params):
        arrays["grads"] = sample([p.grad for p in params])
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.asarray(a, dtype=np.float32))
    print(f"[bench] --dump-outputs: {', '.join(sorted(arrays))} -> {out_dir}", file=sys.stderr, flush=True)


def parity_block(mode):
    """Measured error of THIS run's numerical mode against the reference at the survey's batch A (full-size video model,
    4 x 400 frames) and batch B (16 x 100): the numbers tests/test_bench_parity.py asserts on, read from the committed reference
    goldens (tests/golden/golden_bench_v1.pt + golden_bench_full_v1.pt, generated by tests/golden/make_golden_bench*.py from
    /root/reference).  `dec_logits_full_rel_l2` is the relative L2 error over the WHOLE decoder-logit tensor pred_pad (B, L+1, 5049)
    -- the figure the north star's 1e-3 applies to; `ctc_logits_raw_rel_l2` / `enc_full_rel_l2` are the raw CTC-head logits and the
    encoder output at 8 frames per utterance, all channels, unflattered by any offset (`dec_logits_rel_l2` / `ctc_logp_rel_l2` are
    round 4's 32-column / log-probability figures, kept for continuity: they read 1.5 - 8x lower)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import bench_common as BC

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    gold = torch.load(BC.FIXTURE, weights_only=False)
    keep = ("loss_rel_err", "ctc_rel_err", "att_rel_err", "dec_logits_full_rel_l2", "ctc_logits_raw_rel_l2", "enc_full_rel_l2",
            "dec_logits_rel_l2", "ctc_logp_rel_l2", "acc", "acc_ref", "grad_sample_cos_min", "grad_sample_rel_l2_median",
            "grad_norm_rel_err_median")
    out = {}
    for tag in ("A", "B"):
        case = gold[tag]
        AF.invalidate_weight_cache()
        m = E2E(BC.ODIM, "video")
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        m.load_state_dict(BC.bench_state_dict(m.state_dict(), case["seed"]))
        m = m.cuda().train()
        with AF.numerics(mode):
            r = BC.measure(m, case, torch.device("cuda"))
        AF.invalidate_weight_cache()
        del m
        out[tag] = {k: (float(f"{r[k]:.3g}") if isinstance(r[k], float) else r[k]) for k in keep if k in r}
    out.update(mode={"precise": "precise (split-bf16 forward + backward)", "bf16": "bf16",
                     "hpf": "hpf (split-bf16 forward, bf16 backward)",
                     "mixed": "mixed (forward: encoder / decoder / ResNet stages 3-4 on f16 activations x two-plane f16 weights, "
                              "stem / stages 1-2 / projections / heads on split-bf16 planes; bf16 backward)"}[mode],
               batches="A: 4 x 400 frames, 64 labels; B: 16 x 100 frames, 16 labels; reference goldens", north_star_tol=1e-3)
    return out


def main():
    args = parse()
    if args.gpus > 1 and not args.worker:
        sys.exit(supervise(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    import datetime

    import torch.distributed as dist

    from auto_avsr_amd import _lib, ops
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E
    from auto_avsr_amd.synthetic import bucket_batches, make_batch, rank_batches, utterance_lengths

    # tests/test_ddp_gloo.py::test_bench_main_two_ranks drives THIS main() on two CPU processes (gloo, kernels through the
    # host emulator, a small instance of the same model) so that the N > 1 control flow below -- process-group set-up,
    # cross-rank BatchNorm, DDP wrapping, W / sum(B) rescale, barriers, max-over-ranks timing, rank-0 JSON -- is executed
    # before it ever meets an 8-GPU node.  Never set outside the test suite: the product path requires the MI355X.
    selftest = json.loads(os.environ["AVSR_BENCH_SELFTEST"]) if os.environ.get("AVSR_BENCH_SELFTEST") else None
    if selftest:
        _lib._install_for_tests(selftest["emu"])
        dev = torch.device("cpu")
        torch.set_num_threads(2)
        args.no_graph = args.no_roofline = args.no_cpu_baseline = args.no_parity = True
    else:
        assert torch.cuda.is_available(), "bench.py needs MI355X GPUs (there is no CPU path)"
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
        assert not _lib.lib().is_emulator
    ops.apply_env_tuning()
    if args.deterministic or os.environ.get("AVSR_DETERMINISTIC", "0") == "1":
        from auto_avsr_amd import functional as _AF

        _AF.set_deterministic(True)
    # dp: the data-parallel machinery (process group, cross-rank BatchNorm, gradient exchange, W / sum(B) rescale) is active.
    # AVSR_BENCH_FORCE_DP=1 switches it on for ONE rank (a single-rank RCCL group): the N > 1 code path of this file measured on
    # a one-GPU box (gpurun boxes have one GPU; RCCL refuses two ranks on one device) -- evidence runs only.
    dp = world > 1 or os.environ.get("AVSR_BENCH_FORCE_DP") == "1"
    if dp:
        if world == 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(29600 + os.getpid() % 300))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        # (the rendezvous waits for ranks whose previous attempt is still running into its wall-clock limit: supervise())
        if selftest:
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=900))
        else:
            dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=900))
        AF.set_bn_sync(dist.group.WORLD)
        if selftest and os.environ.get("AVSR_BENCH_TEST_HANG") == (os.environ.get("AVSR_DDP") or args.ddp) and rank == world - 1:
            time.sleep(3600)  # test-suite hook: one rank of this mode never arrives (what a dead-locked collective looks like)
    odim = selftest["odim"] if selftest else 5049
    torch.manual_seed(0)
    model = E2E(odim, args.modality, **(selftest["model"] if selftest else {})).to(dev).train()
    mode = args.mode or ("precise" if args.precise else "mixed")
    AF.set_mode(mode)
    AF.manual_seed(1234 + rank)
    seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    AF.set_seed_tensor(seed_dev)
    class HotPath(torch.nn.Module):
        """forward_tensors()[0] behind nn.Module.__call__ so that DDP's reducer hooks see the step."""

        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x, lens, y):
            return self.m.forward_tensors(x, lens, y)[0]

    hot = HotPath(model)
    opt = None

    def make_optimizer():
        from auto_avsr_amd.optim import FusedAdamW

        return FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.98), weight_decay=0.03, max_grad_norm=10.0,
                          warmup_steps=5 * 1000, total_steps=75 * 1000, cast_weights=True)

    if not args.no_optimizer:
        # the reference's optimisation (lightning.py:48-52, train.py:41): AdamW(1e-3, (0.9, 0.98), wd 0.03), global-norm
        # clip 10, per-step warm-up cosine -- one fused multi-tensor step (auto_avsr_amd/optim.py) that also rewrites the
        # bf16 operand copies of the Linear weights, so the next forward pass needs no separate re-cast of 250M weights
        opt = make_optimizer()
    buckets = comm = comm_grads = None
    if dp and os.environ.get("AVSR_DDP") in ("torch", "buckets", "buckets-graph", "buckets-graph1"):
        args.ddp = os.environ["AVSR_DDP"]  # set by supervise() per attempt (or by hand: AVSR_DDP=torch is the conservative path)
    if dp and args.ddp == "auto":
        args.ddp = DDP_CHAIN[0]  # (a worker started without the supervisor: the head of the chain, the single-communicator mode)
    graph_modes = ("buckets-graph", "buckets-graph1")
    if dp and args.ddp in graph_modes:
        # every collective of the step straight on RCCL's C API (auto_avsr_amd/comm.py): stream operations only, so the capture
        # below has no torch Work objects in it (the process group stays for rendezvous, barriers and the timing).
        # buckets-graph: TWO communicators -- RCCL runs the operations of ONE communicator in issue order even across streams,
        # and the latency-bound BatchNorm collectives on the compute stream must not queue behind 64 MB bucket all-reduces on
        # the side stream.  buckets-graph1: ONE communicator for both (strict issue order = program order on every rank).
        # (CPU self-test: comm.GroupComm, the same interface over gloo, so that this control flow runs in the test suite.)
        if selftest:
            from auto_avsr_amd.comm import GroupComm as Comm
        else:
            from auto_avsr_amd.comm import StreamComm as Comm
        comm = Comm.from_process_group()
        comm_grads = Comm.from_process_group() if args.ddp == "buckets-graph" else comm
        AF.set_bn_sync(dist.group.WORLD, comm=comm)
    if dp and args.ddp == "torch":
        hot = torch.nn.parallel.DistributedDataParallel(hot, device_ids=None if selftest else [local_rank],
                                                        find_unused_parameters=False, broadcast_buffers=False,
                                                        gradient_as_bucket_view=True, bucket_cap_mb=64)
    elif dp:
        # train.py:37 DDPStrategy(find_unused_parameters=False): bucketed gradient all-reduce over RCCL/xGMI, issued by this
        # build's own exchange (auto_avsr_amd/ddp.py) so that the WHOLE data-parallel step -- collectives included -- can be
        # captured into a hipGraph (torch's DDP reducer cannot: tools/rccl_capture_probe.py).
        # 64 MB buckets (AVSR_BUCKET_MB): ring all-reduce over point-to-point xGMI links is per-link bound and wants large
        # messages; the parameter-poor, compute-rich ResNet trunk runs LAST in the backward pass (~5 ms, 45 MB of gradients),
        # so the ~15 encoder/decoder buckets drain underneath it and the exposed tail stays one small bucket.
        # AVSR_GRAD_WIRE=bf16: the buckets travel as bf16 (half the bytes per link; stated in config.grad_wire).
        from auto_avsr_amd.ddp import GradBuckets

        # wire format: f32, the reference's DDP all-reduce (and train.py's default); AVSR_GRAD_WIRE=bf16 opts into half the bytes
        # per xGMI link with bf16 sums across the ranks
        buckets = GradBuckets(model.parameters(), group=dist.group.WORLD, comm=comm_grads, wire=os.environ.get("AVSR_GRAD_WIRE") or "f32")

    if dp and rank == 0:
        print(f"[bench] data-parallel mode: --ddp {args.ddp}" + (" (RCCL C-API communicators, hipGraph replay)" if comm is not None else ""),
              file=sys.stderr, flush=True)
    lengths = utterance_lengths() if not selftest else __import__("numpy").array(selftest["lengths"])
    batches = rank_batches(bucket_batches(lengths, args.max_frames, 400 if not selftest else 4), rank, world, seed=0)
    if args.fixed:  # SURVEY.md section 8d fixed-shape lines
        lengths = [400, 380, 360, 340] if args.fixed == "A" else [100] * 16
        batches = [list(range(len(lengths)))]
        args.shapes = 1
    n_need = args.warmup + args.steps
    # `--shapes` batches spread over the bucket list (short/wide ... long/narrow) are kept resident and cycled, the
    # way a bucketed sampler revisits its (B, T, L) shapes; every step still runs a full fwd+bwd on its batch.
    nshape = max(1, min(args.shapes, len(batches)))
    by_len = sorted(batches, key=lambda b: max(int(lengths[i]) for i in b))  # short / wide ... long / narrow
    picks = [by_len[(2 * j + 1) * len(by_len) // (2 * nshape)] for j in range(nshape)]
    if nshape > 1:
        picks[-1] = by_len[-1]  # the T = 400 bucket of the survey's batch A geometry
    pool = [make_batch(lengths, b, args.modality, odim, seed=j, device=dev) for j, b in enumerate(picks)]
    if args.fixed == "A":  # labels capped at the survey's L = 64
        pool = [(x, lens, y[:, :, :64].contiguous(), fr) for (x, lens, y, fr) in pool]
    data = [pool[i % nshape] for i in range(max(n_need, nshape))]  # (the capture loop below visits every shape once)
    raw = babble = None
    if args.babble:
        # configs[3]: raw 16 kHz waveforms resident in HBM (what load_audio hands over, already uploaded); the babble recording
        # is data the repository does not hold -- a synthetic 60 s coloured-noise stand-in of the same rate.  The reference's
        # AddNoise(snr_target=0) falls back to its random level list (0 is falsy, transforms.py:71); the level is pinned here.
        assert args.modality == "audio", "--babble is the audio front-end path"
        from auto_avsr_amd import transforms as TR

        g = torch.Generator().manual_seed(5)
        noise = torch.randn(1, 16000 * 60, generator=g)
        noise = (noise + torch.roll(noise, 1, 1) + torch.roll(noise, 2, 1)) / 3
        babble = TR.AddNoise(noise=noise.to(dev))
        babble.snr_levels = [0]
        raw = [[0.1 * torch.randn(int(n), generator=g).to(dev) for n in lens.tolist()] for (_, lens, _, _) in pool]
    use_graph = not args.no_graph and (not dp or args.ddp in ("buckets-graph", "buckets-graph1"))
    st = {"opt": opt}
    all_params = list(model.parameters())

    def clear_grads():  # Module.zero_grad walks the module tree (2 ms of host time per step); this is the same effect
        for p in all_params:
            p.grad = None

    def eager_step(x, lens, y):
        clear_grads()  # (the gradients of a replayed step live in the graph's memory pool: never accumulate into them)
        if buckets is not None:
            buckets.begin_step()  # the bucket gathers are issued on THIS stream (ddp.py: no foreign-stream launches)
        AF.new_step()
        seed_dev.add_(1)
        AF.refresh_weight_cache()  # an optimizer step would change the weights: pay the bf16 re-casts every step
        loss = hot(x, lens, y)
        if dp:
            # loss rescale of lightning.py:88-90: loss *= world / sum of batch sizes (all-gather of B)
            bs = torch.full((1,), float(x.shape[0]), device=dev)
            allb = torch.empty(world, device=dev)
            if comm is not None:
                comm.all_gather(allb, bs)
            else:
                dist.all_gather_into_tensor(allb, bs)
            loss = loss * (world / allb.sum())
        loss.backward()
        if buckets is not None:
            buckets.finish()  # the compute stream waits for the bucket all-reduces issued during the backward pass
        if st["opt"] is not None:
            st["opt"].step()
        if buckets is not None and not buckets.rebuilt and not (dev.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            # after the FIRST step (always an eager one): re-bucket the parameters in the order their gradients arrived, so that
            # every bucket leaves as soon as its layers are done (ddp.GradBuckets.rebuild_by_arrival; every rank, same order)
            clear_grads()
            buckets.rebuild_by_arrival()
        return (loss,)

    # One hipGraph per batch shape (auto_avsr_amd/graph_step.py -- the same class train.py's native driver steps through): the
    # ~850 kernel launches of a step (N > 1: + the RCCL collectives) are replayed by the GPU front-end instead of being issued one
    # by one from Python (HIP graphs, not a tracing compiler).  The benchmark captures a shape on first sight, after one eager
    # warm-up step on a side stream (set-up, outside the timed region).
    from auto_avsr_amd.graph_step import StepGraphs

    def warm(x, lens, y):
        eager_step(x, lens, y)
        clear_grads()
        AF.refresh_weight_cache()  # builds the multi-tensor cast table (H2D copy) outside the capture

    def capture_failed(e):
        print(f"[bench rank {rank}] hipGraph capture of the data-parallel step failed ({type(e).__name__}: "
              f"{str(e)[:200]}); continuing with eager launches", file=sys.stderr, flush=True)
        clear_grads()
        if buckets is not None:
            buckets.abort_step()

    # (N > 1: the process group's watchdog thread queries events while this thread captures -> thread-local capture mode; a
    # failed capture is fatal at N = 1 and a fall-back to eager launches at N > 1)
    stepper = StepGraphs(eager_step, enabled=use_graph, capture_after=0, warm=warm, thread_local=dp,
                         on_fail=capture_failed if dp else None, max_graphs=max(64, nshape))

    def step(i):
        x, lens, y, _ = data[i]
        if raw is not None:
            # inside the timed step: per-utterance mask / noise-offset draws on the host, ONE device launch for the batch; the
            # result overwrites the step's input tensor
            xb, _ = TR.audio_batch(raw[i % nshape], "train", babble)
            x.copy_(xb)
        return stepper(x, lens, y)[0]

    sync = (lambda: None) if selftest else torch.cuda.synchronize

    def timed_run(n_warm, n_end):
        """Captures (set-up, not steps), n_warm untimed steps, then steps [n_warm, n_end) between barrier + synchronize."""
        if stepper.enabled:
            for j in range(nshape):
                step(j)
        for i in range(n_warm):
            step(i)
        sync()
        if world > 1:
            dist.barrier()
        t0 = time.perf_counter()
        last = None
        for i in range(n_warm, n_end):
            last = step(i)
        sync()
        if world > 1:
            dist.barrier()
        return time.perf_counter() - t0, last

    t_setup = time.perf_counter()
    dt, last_loss = timed_run(args.warmup, n_need)
    if rank == 0:
        print(f"[bench] outside the timed steps: imports + model + batches {t_setup - T_START:.1f} s, captures + warm-up "
              f"{time.perf_counter() - t_setup - dt:.1f} s", file=sys.stderr, flush=True)
    final_loss = float(last_loss.detach())  # after the timed region: the last step's loss (a replayed graph's static output)
    assert final_loss == final_loss and abs(final_loss) < 1e30, f"non-finite loss after the timed steps: {final_loss}"
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_loss, model, st["opt"], with_grads=not stepper.enabled)
    # (only the steps that were timed: `data` holds at least one entry per batch shape, which may be more than the steps)
    frames = sum(d[3] for d in data[args.warmup:n_need])
    padded = sum(d[0].shape[0] * d[0].shape[1] for d in data[args.warmup:n_need]) // (640 if args.modality == "audio" else 1)
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    ftot = torch.tensor([float(frames), float(padded)], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(ftot)
    dt = float(tmax)
    out = {
        "metric": ("video-frames/sec/node (25fps 88x88" if args.modality == "video" else "audio-frames/sec/node (640 samples of 16 kHz wav per frame")
                  + f", max-frames={args.max_frames}), E2E " + ("fwd+bwd" if args.no_optimizer else "training step (fwd+bwd+clip+AdamW)"),
        "value": round(float(ftot[0]) / dt, 2),
        "unit": "video-frames/sec" if args.modality == "video" else "audio-frames/sec",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(dt / args.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": {"bf16": "bf16", "precise": "f32 (split-bf16 MFMA)", "hpf": "f32 forward (split-bf16 MFMA) / bf16 backward",
                  "mixed": "f16 activations x " + ", ".join(
                      f"{fmt} weights ({', '.join(k for k, v in sorted(AF.MIXED_POLICY.items()) if v == fmt)})"
                      for fmt in ("f16x2", "f16") if fmt in AF.MIXED_POLICY.values())
                           + " + split-bf16 (everything else) forward / bf16 backward"}[mode],
        "data": "synthetic",
        "config": {"workload": ("configs[1]: modality=video vsr_trlrs3_base" if args.modality == "video" else
                                "configs[3] single-GPU leg: modality=audio asr_trlrs3_base (a frame = 640 samples)")
                               + " (12-layer Conformer + 6-layer decoder, 250M), "
                               + (f"FIXED batch {args.fixed} of SURVEY 8d" if args.fixed else "length-bucketed batches")
                               + f", max-frames={args.max_frames} (real frames), fwd+bwd"
                               + ("" if args.no_optimizer else " + global-norm clip 10 + AdamW(1e-3, .9/.98, wd .03) + warm-up cosine + bf16 weight re-cast")
                               + ((", DDP grad all-reduce + SyncBN over RCCL" if args.ddp == "torch" else
                                   ", bucketed RCCL gradient all-reduce overlapped with backward (auto_avsr_amd.ddp) + SyncBN"
                                   + (", every collective a stream operation on RCCL's C API (auto_avsr_amd.comm)" if (comm is not None and not selftest) else "")) if dp else "")
                               + (" [AVSR_BENCH_FORCE_DP: data-parallel machinery on ONE rank]" if dp and world == 1 else "")
                               + (", every step from RAW waveforms: AudioTransform('train') with babble noise at SNR 0 dB + collation "
                                  "on the device inside the timed region" if args.babble else "")
                               + (f", hipGraph replay, {nshape} batch shapes cycled" if stepper.enabled else f", eager launches, {nshape} batch shapes cycled"),
                   "padded_frames_per_sec": round(float(ftot[1]) / dt, 2), "final_loss": round(final_loss, 4),
                   "batch_shapes": sorted({(int(d[0].shape[0]), int(d[0].shape[1]) // (640 if args.modality == "audio" else 1),
                                            int(d[2].shape[2])) for d in data}),
                   "deterministic": bool(AF.deterministic()),
                   "all_hot_path_compute": "libavsr_hip.so (hand-written HIP, gfx950)"},
    }
    if dp:
        out["config"].update(ddp_mode=args.ddp, attempt=int(os.environ.get("AVSR_BENCH_ATTEMPT", "0")),
                             rccl_ranks=(comm.ranks() if comm is not None else dist.get_world_size()),
                             communicators=(0 if comm is None else (1 if comm_grads is comm else 2)),
                             grad_wire=(buckets.wire if buckets is not None else "f32"),
                             bucket_mb=(round(buckets.flat[0].numel() * 4 / 2 ** 20, 1) if buckets is not None else 64))
    if args.full and dp and buckets is not None and buckets.comm is not None and not selftest:
        # one more step, eager, with an event pair around every bucket's exchange (EVERY rank runs it: the collectives need their
        # peers): when does each bucket leave, how long does it travel, and how long does the compute stream stand at the join
        # after the backward pass -- the part of the gradient exchange the backward pass did not hide
        torch.cuda.synchronize()
        buckets.time_next_step()
        eager_step(*data[args.warmup][:3])
        torch.cuda.synchronize()
        rep = buckets.timing_report()
        if rep is not None:
            out["config"]["bucket_overlap"] = rep
    # everything from here to the JSON line is --full: measurements and checks besides the headline figure, in runs of their own
    extras = args.full and rank == 0 and not dp
    if extras and not args.no_roofline:
        # (N > 1: an extra rank-0-only step would dead-lock the DDP / BatchNorm collectives; the kernels are the same)
        fwd, hbm, pair = roofline(model, data[args.warmup], ops)
        # `roofline` = the dominant kernel family BY TIME of the replayed step: the paired backward launches when they outweigh the
        # forward entry points (they do: ~4.0 vs ~3.1 ms); the other one is reported beside it
        if pair is not None and pair["total_ms"] >= fwd.get("total_ms", 0.0):
            out["roofline"], out["roofline_fwd"] = pair, fwd
        else:
            out["roofline"] = fwd
            if pair is not None:
                out["roofline_pair"] = pair
        if hbm is not None:
            out["roofline_hbm"] = hbm
    if extras and not args.no_parity and args.modality == "video":
        out["parity"] = parity_block(mode)
    def second_leg(leg_mode, description):
        """The SAME workload and step timed in another numerical mode (fewer steps, same protocol) + its parity block."""
        AF.set_mode(leg_mode)
        AF.invalidate_weight_cache()
        stepper.reset()
        model.zero_grad(set_to_none=True)
        st["opt"] = make_optimizer()
        n_w, n_t = min(args.warmup, 2), min(args.steps, 8)
        dt_p, loss_p = timed_run(n_w, n_w + n_t)
        fr_p = sum(d[3] for d in data[n_w:n_w + n_t])
        lp = float(loss_p.detach())
        assert lp == lp and abs(lp) < 1e30, f"non-finite loss in the {leg_mode} leg: {lp}"
        stepper.reset()
        res = {"mode": description, "ms_per_step": round(dt_p / n_t * 1e3, 3), "value": round(fr_p / dt_p, 2),
               "unit": "video-frames/sec", "steps": n_t, "warmup": n_w,
               "vs_headline_step": round((dt_p / n_t) / (dt / args.steps), 3),
               "parity": None if args.no_parity else parity_block(leg_mode)}
        AF.set_mode(mode)
        AF.invalidate_weight_cache()
        return res

    legs_ok = extras and args.modality == "video" and not args.no_optimizer and not selftest
    if legs_ok and mode != "bf16" and not args.no_second_leg:
        # the fastest arithmetic of this build, for comparison: bf16 operands in every contraction (8 significant bits: decoder
        # logits 7e-3 / CTC log-probabilities 4e-3 off the fp32 reference -- outside the north star's 1e-3 bound)
        out["bf16"] = second_leg("bf16", "bf16 operands in every forward and backward contraction (does NOT meet the 1e-3 bound on "
                                         "logits: see its parity block)")
    if legs_ok and mode != "hpf" and args.hpf_leg:
        out["hpf"] = second_leg("hpf", "forward on split hi/lo bf16 planes everywhere (3 MFMAs per product, f32 activations), backward "
                                       "+ optimizer as the bf16 step")
    if extras and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(args.modality, odim)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dp:
        for c in {id(c): c for c in (comm, comm_grads) if c is not None}.values():
            c.close()
        dist.destroy_process_group()


# entry points that launch the SAME kernel template on another operand format are one roofline family: the LDS-DMA NT tile kernel
# (csrc/gemm_fast_kernel.h) runs bf16 operands behind avsr_gemm_bf16_nt and f16 operands behind avsr_gemm_h16_nt (mixed mode forward)
SAME_KERNEL = {"avsr_gemm_h16_nt": "avsr_gemm_bf16_nt", "avsr_conv2d_h16": "avsr_conv2d_bf16"}
BN_FAMILY = ("avsr_bn_stats", "avsr_bn_stats_finalize", "avsr_bn_act_fwd", "avsr_bn_bwd_reduce", "avsr_bn_bwd_apply",
             "avsr_bn_act_pool_fwd", "avsr_bn_pool_bwd_reduce", "avsr_bn_pool_bwd_apply", "avsr_bn_small_fwd", "avsr_bn_small_bwd",
             "avsr_bn_act_fwd2", "avsr_bn_act_fwd_h16", "avsr_bn_small_fwd2", "avsr_bn_small_fwd_h16")
# C-ABI entry point -> the kernel names it launches, as rocprofv3 prints them (profiles/*_hbm_traffic.json keys)
KERNELS_OF = {"avsr_gemm_bf16_nt": r"^gemm_fast_kernel<\d+, \d+, \d+, 0,", "avsr_conv2d_bf16": r"^(gemm_fast_kernel<\d+, \d+, \d+, [12],|conv3x3_c64_kernel|conv_patch_kernel)",
              "avsr_conv3x3_wgrad_bf16": r"^(conv3x3_wgrad_kernel|wgrad_reduce_kernel)", "avsr_gemm_bf16_tn": r"^gemm_tn_fast_kernel",
              "bn": r"^bn_(colreduce|bwd_apply|act_fwd|partial_finalize|partial_sum|act_pool3?_fwd|pool_bwd_reduce|pool3?_bwd_apply|stats|small_fwd|small_bwd)"}


def counter_traffic(pattern):
    """HBM-side bytes per launch (FETCH_SIZE + WRITE_SIZE, calibrated) of the kernels matching `pattern`, from the committed
    summary of the two rocprofv3 --pmc passes over one eager step of this workload (tools/pmc_step.py, tools/pmc_report.py ->
    profiles/r6_hbm_traffic.json, taken on the SAME batch shape the roofline legs re-issue their launches on; tools/r6_pmc.sh is the recipe; the round-5 summary is the fall-back).  PMC counters cannot be read from inside this process; the
    passes are separate runs, as the profiling guide prescribes.  None when the summary is absent."""
    import re

    path = os.path.join(ROOT, "profiles", "r6_hbm_traffic.json")  # (tools/r6_pmc.sh)
    if not os.path.exists(path):
        path = os.path.join(ROOT, "profiles", "r5_hbm_traffic.json")
    if not os.path.exists(path):
        return None, None
    tr = json.load(open(path))
    n = rd = wr = 0.0
    for name, k in tr["kernels"].items():
        if re.search(pattern, name):
            n += k["calls"]
            rd += k["rd_bytes"]
            wr += k["wr_bytes"]
    if n == 0:
        return None, None
    return round((rd + wr) / n), f"profiles/{os.path.basename(path)} ({tr.get('shape', '')}): {int(n)} launches, read {rd / 1e6:.0f} MB + written {wr / 1e6:.0f} MB"


def roofline(model, batch, ops):
    """Dominant MFMA-bound kernel family and dominant HBM-bound family (BatchNorm passes) of one training step.
    Pass 1 brackets every C-ABI launch with HIP events on the launch stream and ranks the entry points by time.
    Pass 2 records the argument tuples of the families of interest during one more step and re-issues exactly those
    launches back to back between ONE pair of events: the per-launch duration then carries the launch boundary
    (~1 us) but not the ~3 us an event pair adds around a 10-20 us kernel, and agrees with the rocprofv3 kernel-trace
    averages in profiles/.  achieved = algorithmic FLOP (bytes) of those launches / that time."""
    from auto_avsr_amd import _lib

    x, lens, y, _ = batch
    ops.PROFILE = []
    loss, *_ = model.forward_tensors(x, lens, y)
    loss.backward()
    torch.cuda.synchronize()
    rec, ops.PROFILE = ops.PROFILE, None
    model.zero_grad(set_to_none=True)
    fam = {}
    for name, e0, e1, flops, nbytes in rec:
        name = SAME_KERNEL.get(name, name)
        t = e0.elapsed_time(e1) * 1e-3
        f = fam.setdefault(name, [0.0, 0.0, 0])
        f[0] += t
        f[1] += flops
        f[2] += 1
    tot = sum(v[0] for v in fam.values())
    name = max(fam, key=lambda k: fam[k][0])
    t_ev, _, n = fam[name]
    # pass 2: the same launches, back to back (buffers of the recorded step may have been recycled by the allocator --
    # irrelevant for timing, and nothing of the model is used afterwards)
    members = tuple(k for k, v in SAME_KERNEL.items() if v == name) + (name,)
    ops.RECORD = (members + BN_FAMILY, [])
    loss, *_ = model.forward_tensors(x, lens, y)
    loss.backward()
    torch.cuda.synchronize()
    rec2, ops.RECORD = ops.RECORD[1], None
    lib = _lib.lib()

    def replay(calls, reps=3):
        for nm, a, *_ in calls:  # warm
            lib.call(nm, *a)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for nm, a, *_ in calls:
                lib.call(nm, *a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    # (the launches of this family that are STAND-ALONE in the replayed step: the data-gradient NT calls issued inside a paired()
    # block leave as part of gemm_pair_kernel there and are reported by the `pair` object below)
    calls = [c for c in rec2 if c[0] in members and not c[4]]
    t = replay(calls)
    fl = sum(c[2] for c in calls)
    peak = 2500.0
    ach = fl / t / 1e12 if t > 0 else 0.0
    traffic, src = counter_traffic(KERNELS_OF.get(name, "^$"))  # (the pattern of the bf16 entry point matches the f16 instantiations too)
    algo = sum(c[3] for c in calls) / max(len(calls), 1)
    main = {"bound": "mfma", "kernel": " + ".join(reversed(members)), "launches": len(calls), "avg_us": round(t / max(len(calls), 1) * 1e6, 2),
            "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic,
            "traffic_unit": "HBM-side bytes per launch (FETCH_SIZE + WRITE_SIZE, calibrated)", "traffic_source": src,
            "algorithmic_bytes_per_launch": round(algo),
            "avg_us_event_bracketed": round(t_ev / n * 1e6, 2),
            "event_bracketed_sum_ms": round(tot * 1e3, 3),  # (sum over launches INCLUDING ~3 us of event-pair overhead each: not kernel time)
            "share_of_kernel_time": round(t_ev / tot, 3),
            "families_ms": {k: round(v[0] * 1e3, 3) for k, v in sorted(fam.items(), key=lambda kv: -kv[1][0])[:8]}}
    # The largest line of the step by time is not an entry point of its own: every Linear backward issues its data-gradient (NT)
    # and weight-gradient (TN) contraction between avsr_gemm_pair_begin / _end and they leave as ONE launch (gemm_pair_kernel).
    # Pairing is off while the per-launch hooks above are installed, so the pairs are recorded in a pass of their own (ops.PAIR_RECORD:
    # the calls inside every paired block) and re-issued back to back as pairs.
    ops.PAIR_RECORD = []
    loss, *_ = model.forward_tensors(x, lens, y)
    loss.backward()
    torch.cuda.synchronize()
    pairs, ops.PAIR_RECORD = ops.PAIR_RECORD, None
    model.zero_grad(set_to_none=True)
    pair = None
    if pairs:
        def replay_pairs(reps=3):
            def once():
                for blk in pairs:
                    lib.call("avsr_gemm_pair_begin")
                    for nm, a, _f, _b in blk:
                        lib.call(nm, *a)
                    lib.call("avsr_gemm_pair_end")
            once()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                once()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps

        tp = replay_pairs()
        flp = sum(c[2] for blk in pairs for c in blk)
        algp = sum(c[3] for blk in pairs for c in blk) / len(pairs)
        traffic_p, src_p = counter_traffic(r"^gemm_pair_kernel")
        achp = flp / tp / 1e12 if tp > 0 else 0.0
        pair = {"bound": "mfma", "kernel": "gemm_pair_kernel (avsr_gemm_pair_begin / _end: the data-gradient NT tiles and the weight-gradient TN "
                                           "tiles of one Linear backward in ONE grid)",
                "launches": len(pairs), "avg_us": round(tp / len(pairs) * 1e6, 2), "total_ms": round(tp * 1e3, 3),
                "achieved": round(achp, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achp / peak, 4), "traffic": traffic_p,
                "traffic_unit": "HBM-side bytes per launch (FETCH_SIZE + WRITE_SIZE, calibrated)", "traffic_source": src_p,
                "algorithmic_bytes_per_launch": round(algp)}
    main["total_ms"] = round(t * 1e3, 3)
    bn = [c for c in rec2 if c[0] in BN_FAMILY]
    hbm = None
    if bn:
        tb = replay(bn)
        nb = sum(c[3] for c in bn)
        traffic_b, src_b = counter_traffic(KERNELS_OF["bn"])
        n_kern = None
        hbm = {"bound": "hbm", "kernel": "BatchNorm passes (avsr_bn_*: statistics, apply + SiLU (+ residual), backward reduce / apply)",
               "launches": len(bn), "avg_us": round(tb / len(bn) * 1e6, 2), "achieved": round(nb / tb / 1e9, 1), "peak": 8000.0,
               "unit": "GB/s", "frac": round(nb / tb / 8e12, 4), "algorithmic_bytes_per_launch": round(nb / len(bn)),
               "traffic": traffic_b, "traffic_unit": "HBM-side bytes per KERNEL launch (an entry point may launch two)",
               "traffic_source": src_b,
               "share_of_kernel_time": round(sum(fam[k][0] for k in fam if k in BN_FAMILY) / tot, 3)}
    return main, hbm, pair


if __name__ == "__main__":
    main()
