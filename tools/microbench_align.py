"""CTC forced alignment (csrc/ctc_align.hip) at the shapes a user aligns: graph-replayed time of one avsr_ctc_align call next to
avsr_ctc_loss without the gradient on the same input (same emissions, same chain length: alpha and beta run side by side there)
as a yardstick, at the real vocabulary (V = 5049 in rows of pitch 5056).  Times are device events around REPS replays of a
captured hipGraph, the median of ROUNDS such windows; the two calls alternate window by window.  Prints one JSON line.
GPU box:  python tools/microbench_align.py   (output kept in profiles/align_microbench.txt)"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch

from auto_avsr_amd import ops

V, LD = 5049, 5056
REPS, ROUNDS = 1000, 7
if "--reps" in sys.argv:  # a short run under a kernel trace
    REPS, ROUNDS = int(sys.argv[sys.argv.index("--reps") + 1]), 2
dev = torch.device("cuda:0")


def graph_of(fn):
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):  # warm-up: code objects, the allocator
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = fn()
    torch.cuda.synchronize()
    return g, out


def window_us(g):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        g.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("microbench_align.py needs an MI355X")
    rows = []
    for B, T, L in ((4, 400, 64), (16, 100, 16), (1, 400, 64)):
        g = torch.Generator().manual_seed(B * 1000 + T)
        logits = torch.zeros(B * T, LD)
        logits[:, :V] = torch.randn(B * T, V, generator=g) * 2
        logits = logits.to(dev)
        labels = torch.randint(1, V, (B, L), generator=g).to(dev)
        in_lens = torch.full((B,), T, dtype=torch.int64, device=dev)
        g_align, (ali, score) = graph_of(lambda: ops.ctc_align(logits, LD, labels, in_lens, B, T, V))
        g_loss, (nll, _) = graph_of(lambda: ops.ctc_loss(logits, LD, labels, in_lens, B, T, V, want_grad=False))
        for gr in (g_align, g_loss):
            window_us(gr)
        t_align, t_loss = [], []
        for _ in range(ROUNDS):
            t_align.append(window_us(g_align))
            t_loss.append(window_us(g_loss))
        # the replayed call still computes what the eager one does: a valid alignment whose score is below the total likelihood
        assert bool(((ali != 0).sum(1) >= L).all()) and bool((score <= -nll + 1e-3 * nll.abs()).all())
        rows.append({"B": B, "T": T, "L": L, "align_us": round(statistics.median(t_align), 2),
                     "align_us_min_max": [round(min(t_align), 2), round(max(t_align), 2)],
                     "ctc_loss_nograd_us": round(statistics.median(t_loss), 2),
                     "ctc_loss_nograd_us_min_max": [round(min(t_loss), 2), round(max(t_loss), 2)]})
    print(json.dumps({"bench": "ctc_align", "V": V, "ld": LD, "reps_per_window": REPS, "windows": ROUNDS,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
