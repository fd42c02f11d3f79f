"""CTC prefix beam search on the device (csrc/ctc_beam.hip: avsr_ctc_beam_search) and the exact CTC score of n hypotheses against
one copy of the posteriors (avsr_ctc_score).

The search is checked FRAME BY FRAME, never end to end: the launch leaves the beam after every frame and the frame's token set in
its workspace; a float64 restatement of one step of the search (`_step64`) is run from the kernel's own previous beam and token
set, and the kernel's next beam must be a valid top-W of those candidates with the right masses.  (Whole-search identity against
an oracle is not a criterion: beyond toy sizes the gap at the beam's cut falls below any f32 tolerance somewhere along T frames.)

Tolerance of a mass s: 1e-5 * max(1, |s|) + 1e-5 -- a frame update is at most W + 2 f32 operations per value (W <= 64), each
6e-8 relative: 66 * 6e-8 = 4e-6."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from auto_avsr_amd import functional as AF
from auto_avsr_amd import nets, ops

NEG = float("-inf")


def _tol(s):
    return 1e-5 * max(1.0, abs(s)) + 1e-5


def _lae(a, b):
    return float(np.logaddexp(a, b))


def _step64(beam, toks, row, blank):
    """One frame of the prefix beam search in float64: beam [(prefix, pb, pnb)], the frame's non-blank tokens, its log-posterior row
    -> {prefix: [pb', pnb']} of every candidate (contributions that denote the same prefix merged)."""
    cand = {}

    def add(p, which, v):
        e = cand.setdefault(p, [NEG, NEG])
        e[which] = _lae(e[which], v)

    for p, pb, pnb in beam:
        s, e = _lae(pb, pnb), (p[-1] if p else None)
        add(p, 0, s + row[blank])
        for c in toks:
            if c != e:
                add(p + (c,), 1, s + row[c])
            else:
                add(p, 1, pnb + row[c])
                if pb > NEG:
                    add(p + (c,), 1, pb + row[c])
    return cand


def _search(dev, logits, in_lens, W, K, nbest=None):
    lp = AF.log_softmax(logits.to(dev))
    res = AF.ctc_beam_search(lp, torch.as_tensor(in_lens), blank=0, beam=W, topk=K, nbest=nbest)
    return lp, res


def _logits(B, T, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, V, generator=g) * 3
    x[..., 0] += 6
    return x


def _ctc_ll64(lp64, y, T):
    """log P_ctc(y | lp[:T]) in float64 through torch's CTC loss."""
    if len(y) == 0:
        return float(lp64[:T, 0].sum())
    if len(y) > T:
        return NEG
    nll = F.ctc_loss(lp64[:T].unsqueeze(1), torch.tensor([list(y)]), torch.tensor([T]), torch.tensor([len(y)]), blank=0,
                     reduction="none", zero_infinity=False)
    v = -float(nll[0])
    return NEG if math.isinf(v) else v


# ---------------------------------------------------------------------------------------------------- test 1: no pruning
def test_without_pruning_every_prefix_carries_its_ctc_likelihood(dev):
    T, V = 4, 3
    lp, res = _search(dev, _logits(1, T, V, 0), [T], W=64, K=2)
    assert int(res["n_valid"][0]) == 15
    lp64 = lp[0].cpu().double()
    score, lens, toks = res["score"][0].cpu().double(), res["lens"][0].cpu(), res["tokens"][0].cpu()
    assert abs(float(torch.logsumexp(score[:15], 0))) < 1e-5
    seen, worst = set(), 0.0
    for r in range(15):
        y = tuple(toks[r, : int(lens[r])].tolist())
        seen.add(y)
        ref = _ctc_ll64(lp64, y, T)
        worst = max(worst, abs(float(score[r]) - ref) / _tol(ref))
        assert abs(float(score[r]) - ref) <= _tol(ref), (y, float(score[r]), ref)
        assert abs(_lae(float(res["pb"][0, r]), float(res["pnb"][0, r])) - float(score[r])) <= _tol(ref)
    assert len(seen) == 15 and () in seen
    print(f"no pruning: worst |score - log P_ctc| = {worst:.3f} of the tolerance")


# ---------------------------------------------------------------------------------------------------- test 2: frame by frame
def _check_frames(lp, res, in_lens, W, K):
    trace, topk = ops.ctc_beam_trace(res, in_lens)
    worst = 0.0
    for b, Tb in enumerate(in_lens):
        rows = lp[b].cpu().double().numpy()
        Tb = min(Tb, rows.shape[0])
        assert len(trace[b]) == Tb
        beam = [((), 0.0, NEG)]
        for t in range(Tb):
            row, toks = rows[t], topk[b][t]
            # (a) the token set is a valid top-K of the row by value
            assert len(set(toks)) == K and 0 not in toks and all(0 < c < len(row) for c in toks)
            rest = np.delete(row, [0] + toks)
            assert rest.size == 0 or rest.max() <= min(row[c] for c in toks), (b, t)
            cand = _step64(beam, toks, row, 0)
            tot = {p: _lae(v[0], v[1]) for p, v in cand.items()}
            live = [p for p in cand if tot[p] > NEG]
            new = trace[b][t]
            # (d) min(W, #candidates) entries, all prefixes distinct
            assert len(new) == min(W, len(live)), (b, t, len(new), len(live))
            kept = [p for p, _, _ in new]
            assert len(set(kept)) == len(kept), (b, t)
            # (b) every kept entry is a candidate with the candidate's masses
            for p, pb, pnb in new:
                assert p in cand, (b, t, p)
                s = tot[p]
                err = abs(_lae(pb, pnb) - s)
                worst = max(worst, err / _tol(s))
                assert err <= _tol(s), (b, t, p, pb, pnb, cand[p])
                for got, ref in ((pb, cand[p][0]), (pnb, cand[p][1])):
                    if ref >= s - 20:
                        assert abs(got - ref) <= _tol(s), (b, t, p, got, ref)
            # (c) no candidate outside the beam exceeds the smallest kept total by more than the tolerance
            floor = min(tot[p] for p in kept)
            out = [tot[p] for p in live if p not in set(kept)]
            assert not out or max(out) <= floor + _tol(floor), (b, t, max(out), floor)
            beam = new
    return worst


@pytest.mark.parametrize("T,V,W,K", [(12, 20, 4, 4), (40, 64, 8, 8), (37, 5049, 16, 16), (400, 5049, 16, 8), (8, 40, 64, 32)])
def test_every_frame_is_a_valid_step_from_the_kernels_own_beam(dev, T, V, W, K):
    lp, res = _search(dev, _logits(1, T, V, T + V), [T], W, K)
    if V == 5049:
        assert lp.stride(-2) == 5056
    worst = _check_frames(lp, res, [T], W, K)
    print(f"T={T} V={V} W={W} K={K}: worst mass error {worst:.3f} of the tolerance")


def test_every_frame_of_a_batch_of_unequal_lengths(dev):
    in_lens = [400, 37, 1]
    lp, res = _search(dev, _logits(3, 400, 5049, 7), in_lens, 16, 8)
    assert lp.stride(-2) == 5056
    worst = _check_frames(lp, res, in_lens, 16, 8)
    print(f"B=3 in_lens={in_lens}: worst mass error {worst:.3f} of the tolerance")


# ---------------------------------------------------------------------------------------------------- test 3: the n-best
def test_nbest_is_the_last_beam_sorted(dev):
    in_lens, T, V, W, K, N = [23, 1, 0, 9], 23, 31, 8, 6, 5
    lp, res = _search(dev, _logits(4, T, V, 11), in_lens, W, K, nbest=N)
    trace, _ = ops.ctc_beam_trace(res, in_lens)
    toks, lens, nv = res["tokens"].cpu(), res["lens"].cpu(), res["n_valid"].cpu()
    score, pb, pnb = res["score"].cpu(), res["pb"].cpu(), res["pnb"].cpu()
    assert toks.shape == (4, N, T)
    for b, Tb in enumerate(in_lens):
        last = trace[b][-1] if Tb > 0 else [((), 0.0, NEG)]
        last = sorted(last, key=lambda e: -_lae(e[1], e[2]))
        assert int(nv[b]) == min(N, len(last))
        for r in range(N):
            if r >= int(nv[b]):
                assert int(lens[b, r]) == 0 and float(score[b, r]) == NEG and (toks[b, r] == -1).all()
                continue
            p, rpb, rpnb = last[r]
            assert tuple(toks[b, r, : int(lens[b, r])].tolist()) == p and int(lens[b, r]) == len(p)
            assert (toks[b, r, len(p):] == -1).all()
            assert float(pb[b, r]) == rpb and float(pnb[b, r]) == rpnb
            assert abs(float(score[b, r]) - _lae(rpb, rpnb)) <= _tol(float(score[b, r]))
    # T = 1: blank and the K tokens; in_lens = 0: the empty hypothesis with score 0
    assert int(nv[1]) == min(N, K + 1) and sorted(int(x) for x in lens[1, : int(nv[1])]) == [0] + [1] * (int(nv[1]) - 1)
    assert int(nv[2]) == 1 and int(lens[2, 0]) == 0 and float(score[2, 0]) == 0.0


def test_ctc_head_method_is_the_search_over_its_log_softmax(dev):
    torch.manual_seed(5)
    ctc = nets.CTC(29, 16, 0.0).eval().to(dev)
    hs, hlens = torch.randn(2, 14, 16).to(dev) * 2, torch.tensor([14, 9])
    with torch.no_grad():
        got = ctc.prefix_beam_search(hs, hlens, beam=6, topk=5, nbest=4)
        lp = ctc.log_softmax(hs)
        want = AF.ctc_beam_search(lp, hlens, blank=0, beam=6, topk=5, nbest=4)
    for k in ("tokens", "lens", "score", "pb", "pnb", "n_valid"):
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    assert got["tokens"].shape == (2, 4, 14)


def test_rejects_what_the_kernel_cannot_hold(dev):
    lp = AF.log_softmax(_logits(1, 4, 5, 0).to(dev))
    for kw in (dict(beam=1, topk=2), dict(beam=65, topk=2), dict(beam=4, topk=5), dict(beam=4, topk=0), dict(beam=4, topk=2, nbest=5)):
        with pytest.raises(Exception):
            AF.ctc_beam_search(lp, torch.tensor([4]), **kw)


# ---------------------------------------------------------------------------------------------------- test 4: exact CTC score
def test_ctc_score_against_float64_ctc_loss(dev):
    B, T, V, N = 2, 30, 41, 6
    in_lens = [30, 11]
    lp = AF.log_softmax(_logits(B, T, V, 3).to(dev))
    g = torch.Generator().manual_seed(1)
    labels = torch.full((B, N, T + 2), -1, dtype=torch.int64)
    seqs = []
    for b, Tb in enumerate(in_lens):
        rep = torch.randint(1, V, (5,), generator=g).tolist()
        rep[2] = rep[1]  # a repeated token: a blank must separate the two
        full = torch.randint(1, V, (Tb,), generator=g).tolist()
        for i in range(1, Tb):  # L = T fits only without repeats
            if full[i] == full[i - 1]:
                full[i] = full[i] % (V - 1) + 1
        row = [[], rep, full, torch.randint(1, V, (Tb + 1,), generator=g).tolist(),
               torch.randint(1, V, (3,), generator=g).tolist(), [7]]
        seqs.append(row)
        for i, y in enumerate(row):
            labels[b, i, : len(y)] = torch.tensor(y, dtype=torch.int64)
    got = AF.ctc_score(lp, labels.to(dev), torch.tensor(in_lens)).cpu()
    assert got.shape == (B, N)
    finite = []
    for b, Tb in enumerate(in_lens):
        lp64 = lp[b].cpu().double()
        for i, y in enumerate(seqs[b]):
            ref = _ctc_ll64(lp64, y, Tb)
            if ref == NEG:
                assert float(got[b, i]) == NEG, (b, i)
            else:
                finite.append((float(got[b, i]), ref))
        assert float(got[b, 3]) == NEG  # L > T
        assert abs(float(got[b, 0]) - float(lp64[:Tb, 0].sum())) < 2e-3 * max(1.0, abs(float(lp64[:Tb, 0].sum())))
    assert len(finite) == B * 5
    scale = max(1.0, max(abs(r) for _, r in finite))  # (tolerance of test_loss_kernels.py::test_ctc)
    worst = max(abs(a - r) for a, r in finite)
    print(f"ctc_score: worst |loglik - ref| = {worst:.2e} (bound {2e-3 * scale:.2e})")
    assert worst < 2e-3 * scale
