"""Golden vectors for CTC forced alignment: runs the REFERENCE `CTC.forced_align` (float64 python loop) and
`CTC.forced_align_batch` (float32 numpy loop) of espnet/nets/pytorch_backend/ctc.py and saves inputs and results (tensors only).

Two groups:
  exact    inputs for which path identity is a sound criterion: this script ASSERTS that every predecessor decision of the
           float64 Viterbi trellis (every reachable cell with two or more finite candidates) and the final choice between the
           last two states have a gap >= 1e-3, that |best score| < 600 (float32 spacing 6e-5, 16 times below the gap), and that
           the reference's two implementations return the same path.  Seeds are searched from the given start; the logits
           are `randn * 2` rounded to 16 significant bits (hi + lo bf16), so that a split-plane `ctc_lo` with an identity weight
           reproduces them exactly.  (The reference's forced_align lets state 0 be entered from the LAST state -- its
           `logdelta[t - 1, s - 1]` wraps around at s = 0 -- which utterances with many more frames than labels hit; such seeds
           fail the agreement check and are passed over, and the ragged batch keeps T close to L for that reason.)
  optimal  larger inputs where near-ties make the path implementation-dependent: the float64 optimum and the deficit of the
           reference's float32 `forced_align_batch` path against it (re-scored in float64) are stored instead of a path.

Run on the build machine only, with the reference checkout given explicitly:
    python tests/golden/make_golden_align.py <path to the reference checkout>   ->  tests/golden/golden_align_v1.pt"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
V = 53
GAP = 1e-3


def round16(x):
    """x rounded to hi + lo bf16 planes (16 significant bits)."""
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def trellis64(lp, y, blank=0):
    """float64 Viterbi over log-probabilities lp (T, V): best score, path of token ids, smallest decision gap."""
    ext = [blank]
    for t in y:
        ext += [int(t), blank]
    T, S = lp.shape[0], len(ext)
    delta = np.full((T, S), -np.inf)
    back = np.zeros((T, S), dtype=np.int64)
    delta[0, 0] = lp[0, ext[0]]
    if S > 1:
        delta[0, 1] = lp[0, ext[1]]
    gap = np.inf
    for t in range(1, T):
        for s in range(S):
            cand = [delta[t - 1, s]]
            if s >= 1:
                cand.append(delta[t - 1, s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                cand.append(delta[t - 1, s - 2])
            k = int(np.argmax(cand))
            if np.isfinite(cand[k]):
                fin = sorted((c for c in cand if np.isfinite(c)), reverse=True)
                if len(fin) > 1:
                    gap = min(gap, fin[0] - fin[1])
                delta[t, s] = cand[k] + lp[t, ext[s]]
                back[t, s] = k
    ends = [delta[T - 1, S - 1]] + ([delta[T - 1, S - 2]] if S > 1 else [])
    k = int(np.argmax(ends))
    if len(ends) > 1 and np.isfinite(ends[1 - k]):
        gap = min(gap, ends[k] - ends[1 - k])
    s = S - 1 - k
    path = np.zeros(T, dtype=np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = ext[s]
        s -= back[t, s]
    return float(ends[k]), path, float(gap)


def rescore64(lp, path):
    return float(sum(lp[t, int(p)] for t, p in enumerate(path)))


def make_ctc(CTC):
    ctc = CTC(V, V, 0.0)
    with torch.no_grad():
        ctc.ctc_lo.weight.copy_(torch.eye(V))
        ctc.ctc_lo.bias.zero_()
    return ctc.eval()


def draw(seed, T, L, scale=2.0, rounded=True):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, 1, V, generator=g) * scale
    y = torch.randint(1, V, (L,), generator=g)
    if L > 2:
        y[2] = y[1]  # repeated label -> mandatory blank
    return (round16(logits) if rounded else logits), y


def exact_case(ctc, T, L, seed0, tries=64):
    for seed in range(seed0, seed0 + tries):
        logits, y = draw(seed, T, L)
        lp64 = torch.log_softmax(logits[:, 0].double(), -1).numpy()
        best, path, gap = trellis64(lp64, y.tolist())
        if gap < GAP or abs(best) >= 600:
            continue
        with torch.no_grad():
            a1 = np.asarray(ctc.forced_align(logits[:, 0], y.numpy()), dtype=np.int64)
            a2 = ctc.forced_align_batch(logits, y.view(1, -1), torch.tensor([T]))[0]
        if not (np.array_equal(a1, a2) and np.array_equal(a1, path)):
            continue
        assert gap >= GAP and abs(best) < 600 and np.array_equal(a1, a2)
        print(f"exact  T={T} L={L} seed={seed} gap={gap:.3e} best={best:.3f}")
        return dict(T=T, L=L, seed=seed, logits=logits, y=y, ali=torch.from_numpy(a1), score=torch.tensor(best, dtype=torch.float64), gap=gap)
    raise SystemExit(f"no seed in [{seed0}, {seed0 + tries}) qualifies for T={T} L={L}")


def exact_batch(ctc, Tmax, ilens, Ls, seed0, tries=256):
    """A ragged batch (lengths and label counts differ, label rows padded with -1) every utterance of which qualifies."""
    B, Lmax = len(ilens), max(Ls)
    for seed in range(seed0, seed0 + tries):
        g = torch.Generator().manual_seed(seed)
        logits = round16(torch.randn(Tmax, B, V, generator=g) * 2)
        ys = torch.full((B, Lmax), -1, dtype=torch.int64)
        for b, L in enumerate(Ls):
            ys[b, :L] = torch.randint(1, V, (L,), generator=g)
            if L > 2:
                ys[b, 2] = ys[b, 1]
        with torch.no_grad():
            batch = ctc.forced_align_batch(logits, ys, torch.tensor(ilens))
        ok, scores, gaps = True, [], []
        for b in range(B):
            y = ys[b, : Ls[b]]
            lp64 = torch.log_softmax(logits[: ilens[b], b].double(), -1).numpy()
            best, path, gap = trellis64(lp64, y.tolist())
            with torch.no_grad():
                a1 = np.asarray(ctc.forced_align(logits[: ilens[b], b], y.numpy()), dtype=np.int64)
            ok = ok and gap >= GAP and abs(best) < 600 and np.array_equal(a1, batch[b]) and np.array_equal(a1, path)
            scores.append(best)
            gaps.append(gap)
        if not ok:
            continue
        print(f"exact  batch Tmax={Tmax} ilens={ilens} Ls={Ls} seed={seed} gaps={['%.2e' % x for x in gaps]}")
        ali = torch.full((B, Tmax), -1, dtype=torch.int64)
        for b in range(B):
            ali[b, : ilens[b]] = torch.from_numpy(batch[b])
        return dict(Tmax=Tmax, ilens=torch.tensor(ilens), Ls=Ls, seed=seed, logits=logits, ys=ys, ali=ali,
                    score=torch.tensor(scores, dtype=torch.float64), gap=min(gaps))
    raise SystemExit("no seed qualifies for the ragged batch")


def optimal_case(ctc, T, L, seed, scale):
    """The deficit of the reference's float32 batch path against the float64 optimum, on unrounded logits."""
    logits, y = draw(seed, T, L, scale, rounded=False)
    lp64 = torch.log_softmax(logits[:, 0].double(), -1).numpy()
    best, _, gap = trellis64(lp64, y.tolist())
    with torch.no_grad():
        a2 = ctc.forced_align_batch(logits, y.view(1, -1), torch.tensor([T]))[0]
    deficit = best - rescore64(lp64, a2)
    assert deficit >= -1e-9
    print(f"optimal T={T} L={L} seed={seed} scale={scale} optimum={best:.3f} gap={gap:.2e} reference deficit={deficit:.3e}")
    return dict(T=T, L=L, seed=seed, scale=scale, logits=logits, y=y, optimum=torch.tensor(best, dtype=torch.float64),
                deficit_ref=max(deficit, 0.0))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from espnet.nets.pytorch_backend.ctc import CTC  # noqa: E402  (the reference's)

    ctc = make_ctc(CTC)
    out = {
        "V": V,
        "exact": [exact_case(ctc, 40, 9, 0), exact_case(ctc, 90, 40, 0), exact_case(ctc, 150, 40, 0), exact_case(ctc, 12, 1, 0)],
        "exact_batch": [exact_batch(ctc, 40, [40, 33, 6], [16, 12, 1], 0)],
        "optimal": [optimal_case(ctc, 300, 140, 1, 2.0), optimal_case(ctc, 400, 64, 3, 4.0)],
    }
    path = os.path.join(HERE, "golden_align_v1.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")
