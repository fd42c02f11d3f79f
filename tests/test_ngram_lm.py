"""Back-off n-gram language model (ARPA) shallow fusion in the beam search: the loader and the flattened model of
auto_avsr_amd/ngram.py, the lookup kernel alone (`avsr_ngram_score` against the scorer's own numpy step, bit for bit, and against a
float64 dict recursion of the definition), the model inside the one-call-per-step session of csrc/decode.hip (avsr_beam_set_ngram) and
in the python-issued step -- against golden vectors of the reference's BatchBeamSearch with an independent dict-recursion partial
scorer (tests/golden/make_golden_ngram.py) --, in forward_many / forward_batch, across a change of the model between utterances, in a
session without a model, and through get_beam_search_decoder / eval.py.  Kernels through the emulator (CPU suite) or on the MI355X
(-m gpu)."""
import ctypes
import math
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
from synth import synth_state_dict  # noqa: E402

from auto_avsr_amd import functional as AF  # noqa: E402
from auto_avsr_amd import nets  # noqa: E402
from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "golden_ngram_v1.pt"), weights_only=False)["cases"]
GOLD_LM = torch.load(os.path.join(HERE, "golden", "golden_lm_v1.pt"), weights_only=False)["cases"]
_ID = lambda c: f"seed{c['seed']}-w{c['ngram_weight']}"  # noqa: E731
LN10 = math.log(10.0)


class _precise:
    def __enter__(self):
        AF.set_precise(True)

    def __exit__(self, *a):
        AF.set_precise(False)


def _scorer(*a, **k):
    from auto_avsr_amd.ngram import NgramScorer

    return NgramScorer(*a, **k)


def _case_model(case):
    return _scorer(case["odim"], case["probs"], case["backoffs"], order=case["order"])


def _bs(dev, seed, odim, beam, ctc_weight, penalty, ngram=None, ngram_weight=0.0, bias=None, bias_weight=0.0, lm=None, lm_weight=0.0,
        ngram_first=False, slot=True, D=128):
    torch.manual_seed(0)
    dec = nets.TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = nets.CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    dec, ctc = dec.to(dev), ctc.to(dev)
    scorers = {"decoder": dec}
    if ngram_first:
        scorers["ngram"] = ngram
    scorers.update({"ctc": CTCPrefixScorer(ctc, odim - 1), "lm": lm, "bias": bias, "length_bonus": LengthBonus(odim)})
    weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": lm_weight, "bias": bias_weight, "length_bonus": penalty}
    if slot:
        scorers.setdefault("ngram", ngram)
        weights["ngram"] = ngram_weight
    return BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                           token_list=[str(i) for i in range(odim)], pre_beam_score_key="decoder")


def _case_bs(dev, case, **kw):
    if "ngram" not in kw:
        kw["ngram"] = _case_model(case)
    kw.setdefault("ngram_weight", case["ngram_weight"])
    return _bs(dev, case["seed"], case["odim"], case["beam"], case["ctc_weight"], case["penalty"], **kw)


def _enc(case, dev, T=None, seed=None):
    g = torch.Generator().manual_seed(500 + case["seed"] if seed is None else seed)
    return (torch.randn(T or case["T"], case["D"], generator=g) * 1.5).to(dev)


def _run(bs, x, native, maxlenratio=0.0):
    from auto_avsr_amd import decoding

    was = decoding.NATIVE_BEAM
    decoding.NATIVE_BEAM = native
    try:
        with _precise():
            nbest = bs(x, maxlenratio=maxlenratio)
    finally:
        decoding.NATIVE_BEAM = was
    assert bool(bs._native) == native  # the path asked for is the one that ran
    return nbest


# ------------------------------------------------------------------------------------------------------- 1. the loader
def _arpa(tmp_path, name, sections, counts=None):
    """sections: {order: [(log10 p, words, log10 back-off or None)]}"""
    lines = ["", "\\data\\"] + [f"ngram {k}={len(v) if counts is None else counts[k]}" for k, v in sorted(sections.items())] + [""]
    for k, rows in sorted(sections.items()):
        lines.append(f"\\{k}-grams:")
        lines += ["\t".join([repr(p), " ".join(w)] + ([repr(b)] if b is not None else [])) for p, w, b in rows]
        lines.append("")
    lines.append("\\end\\")
    path = tmp_path / name
    path.write_text("\n".join(lines) + "\n")
    return str(path)


V0 = 8
TOKS = ["<blank>", "▁a", "▁b", "c", "d", "e", "f", "<eos>"]
UNI_IDS = [(-1.0, ("<s>",), -0.5), (-0.9, ("</s>",), None)] + [(-0.1 * t - 0.5, (str(t),), -0.25 * t) for t in range(1, V0 - 1)]


def test_arpa_orders_ids_pieces_and_conversion(tmp_path):
    from auto_avsr_amd.ngram import NgramScorer
    from espnet.nets.scorers.ngram import NgramScorer as Shim

    assert Shim is NgramScorer
    f32 = lambda x: np.float32(x * LN10)  # noqa: E731
    # order 1, token ids: one node, the root's edges are the tokens 1 .. V - 1 in order (<s> predicts nothing)
    sc = NgramScorer.from_arpa(_arpa(tmp_path, "o1.arpa", {1: UNI_IDS}), TOKS)
    assert (sc.order, sc.n_nodes, sc.n_edges, sc.start_node) == (1, 1, V0 - 1, 0)
    assert sc.tok.tolist() == list(range(1, V0)) and sc.logp.dtype == np.float32 and sc.bow.dtype == np.float32
    assert sc.logp[2] == f32(-0.8) and sc.logp[V0 - 2] == f32(-0.9) and sc.step(0, 3) == (f32(-0.8), 0)
    # order 2, ids: every unigram is a context; <s> is where a hypothesis starts
    bi = [(-0.3, ("<s>", "2"), None), (-0.2, ("2", "3"), None), (-0.7, ("2", "</s>"), None), (-0.4, ("3", "3"), None)]
    sc = NgramScorer.from_arpa(_arpa(tmp_path, "o2.arpa", {1: UNI_IDS, 2: bi}), TOKS)
    assert (sc.order, sc.n_nodes, sc.n_edges) == (2, 1 + V0, V0 - 1 + 4)
    assert sc.contexts[sc.start_node] == (V0,) and sc.bow[sc.start_node] == f32(-0.5)
    s2 = sc.contexts.index((2,))
    assert sc.step(sc.start_node, 2) == (f32(-0.3), s2) and sc.step(s2, V0 - 1)[0] == f32(-0.7)
    r, nx = sc.step(s2, 4)  # backs off: bow(2) + p(4)
    assert r == np.float32(f32(-0.5) + f32(-0.9)) and nx == sc.contexts.index((4,))
    assert sc.step(s2, 0) == (np.float32(0.0), s2)  # the blank
    # order 3, piece strings
    uni = [(-1.0, ("<s>",), -0.5), (-0.9, ("</s>",), None)] + [(-0.1 * t - 0.5, (TOKS[t],), -0.25 * t) for t in range(1, V0 - 1)]
    bi = [(-0.3, ("<s>", "▁a"), -0.2), (-0.2, ("▁a", "c"), -0.1), (-0.6, ("c", "d"), None)]
    tri = [(-0.05, ("<s>", "▁a", "c"), None), (-0.15, ("▁a", "c", "</s>"), None)]
    sc = NgramScorer.from_arpa(_arpa(tmp_path, "o3.arpa", {1: uni, 2: bi, 3: tri}), TOKS)
    assert sc.order == 3 and (V0, 1) in sc.contexts and (1, 3) in sc.contexts
    total, s = sc.walk([1, 3, V0 - 1])
    assert total == np.float32(np.float32(f32(-0.3) + f32(-0.05)) + f32(-0.15))
    total, s = sc.walk([1, 3, 4])  # (a, c) has no entry on d: bow(a c) + p(d | c)
    assert s == sc.contexts.index((3, 4)) and sc.step(sc.contexts.index((1, 3)), 4)[0] == np.float32(f32(-0.1) + f32(-0.6))
    with pytest.raises(ValueError, match="token list"):
        NgramScorer.from_arpa(_arpa(tmp_path, "bad.arpa", {1: uni + [(-1.0, ("zzz",), None)]}), TOKS)


def test_arpa_unk_fill_in_and_empty_highest_order(tmp_path):
    from auto_avsr_amd.ngram import NgramScorer

    uni = [(-1.0, ("<s>",), -0.5), (-0.9, ("</s>",), None), (-2.5, ("<unk>",), -0.3), (-0.4, ("2",), -0.2), (-0.6, ("5",), None)]
    bi = [(-0.3, ("2", "5"), None), (-0.1, ("<unk>", "5"), None)]
    sc = NgramScorer.from_arpa(_arpa(tmp_path, "unk.arpa", {1: uni, 2: bi, 3: []}, counts={1: 5, 2: 2, 3: 0}), TOKS)
    assert sc.order == 3  # the header's order, although the section is empty: bigrams are contexts and keep their back-offs
    assert sc.tok[: sc.first[1]].tolist() == list(range(1, V0))
    unk = np.float32(-2.5 * LN10)
    for t in (1, 3, 4, 6):
        assert sc.step(0, t) == (unk, 0)  # <unk>'s log-probability, no context of its own (back-off 0)
    assert (3,) not in sc.contexts and (2,) in sc.contexts and (2, 5) in sc.contexts
    assert sc.n_nodes == 1 + 4 + 1  # <s>, </s>, 2, 5; (2, 5): the n-grams with <unk> are dropped
    r, nx = sc.step(sc.contexts.index((2,)), 3)
    assert r == np.float32(np.float32(-0.2 * LN10) + unk) and nx == 0


def test_arpa_closure_errors(tmp_path):
    from auto_avsr_amd.ngram import NgramScorer

    with pytest.raises(ValueError, match="prefix"):
        NgramScorer.from_arpa(_arpa(tmp_path, "a.arpa", {1: UNI_IDS, 2: [(-0.3, ("2", "3"), None)], 3: [(-0.1, ("3", "2", "3"), None)]}), TOKS)
    with pytest.raises(ValueError, match="</s>"):
        NgramScorer.from_arpa(_arpa(tmp_path, "b.arpa", {1: [u for u in UNI_IDS if u[1] != ("</s>",)]}), TOKS)
    with pytest.raises(ValueError, match="<unk>"):
        NgramScorer.from_arpa(_arpa(tmp_path, "c.arpa", {1: [u for u in UNI_IDS if u[1] != ("4",)]}), TOKS)
    with pytest.raises(ValueError):
        NgramScorer.from_arpa(_arpa(tmp_path, "d.arpa", {1: UNI_IDS + [(-1.0, (str(V0 + 3),), None)]}), TOKS)
    (tmp_path / "e.arpa").write_text("not an arpa file\n")
    with pytest.raises(ValueError):
        NgramScorer.from_arpa(str(tmp_path / "e.arpa"), TOKS)


# ------------------------------------------------------------------------------------------------------- 2. the kernel alone
class _Def:
    """The definition of the issue as a float64 recursion over two dicts: shares nothing with auto_avsr_amd/ngram.py."""

    def __init__(self, P, B, V, N, unk=None):
        self.P, self.B, self.V, self.N, self.unk = P, B, V, N, unk

    def p(self, v, h):
        g = tuple(h) + (v,)
        if g in self.P:
            return float(self.P[g])
        if not h:
            return float(self.unk)
        return float(self.B.get(tuple(h), 0.0)) + self.p(v, h[1:])

    def total(self, tokens):
        hist, total = [self.V], 0.0
        for v in tokens:
            if v != 0:
                total += self.p(v, tuple(hist[-(self.N - 1):]) if self.N > 1 else ())
                hist.append(v)
        return total


def _kernel(dev, sc, nodes, cand, eos, n_nodes=None):
    from auto_avsr_amd import ops

    tabs = sc.device_tables(dev)
    node_t = torch.tensor(nodes, dtype=torch.int32, device=dev)
    cand_t = torch.tensor(cand, dtype=torch.int64, device=dev).contiguous()
    n, S = cand_t.shape
    score = torch.full((n, S + 1), 77.0, dtype=torch.float32, device=dev)
    nxt = torch.full((n, S + 1), -7, dtype=torch.int32, device=dev)
    ops.call("avsr_ngram_score", *[ops._ptr(t) for t in tabs], sc.n_nodes if n_nodes is None else n_nodes, sc.n_edges, ops._ptr(node_t),
             ops._ptr(cand_t), n, S, eos, 0, ops._ptr(score), ops._ptr(nxt), ops._stream(score))
    return score.cpu(), nxt.cpu()


def _check_kernel(dev, sc, ref, nodes, cand):
    V = sc.n_vocab
    score, nxt = _kernel(dev, sc, nodes, cand, V - 1)
    cols = np.asarray([list(r) + [V - 1] for r in cand], dtype=np.int64)
    es, en = sc.lookup(np.repeat(np.asarray(nodes)[:, None], cols.shape[1], 1), cols)
    assert torch.equal(score, torch.from_numpy(es)) and torch.equal(nxt, torch.from_numpy(en.astype(np.int32)))  # bit for bit
    for r, s in enumerate(nodes):
        for c, v in enumerate(cols[r].tolist()):
            want = 0.0 if v == 0 else ref.p(v, sc.contexts[s])
            assert abs(float(score[r, c]) - want) <= 1e-5 * max(1.0, abs(want)), (s, v)
            if v == 0:
                assert int(nxt[r, c]) == s
    return score, nxt


V1 = 50
S1, E1 = V1, V1 - 1
_UNI = {(t,): -1.0 - 0.01 * t for t in range(1, V1)}
TRIES = {
    # name: (P beyond the unigrams, B, order)
    "unigram-only": ({}, {}, 1),
    "1-2-3-children": ({(5, 10): -0.5, (6, 20): -0.4, (6, 30): -0.6, (7, 3): -0.2, (7, 11): -0.3, (7, 33): -0.7},
                       {(5,): -0.11, (6,): -0.22, (7,): -0.33}, 2),
    "edge-tokens": ({(1, V1 - 2): -0.5, (V1 - 2, 1): -0.4, (1, 1): -0.3, (V1 - 2, V1 - 2): -0.2, (1, V1 - 2, 1): -0.1},
                    {(1,): -0.5, (V1 - 2,): -0.25, (1, V1 - 2): -0.125}, 3),
    "eos-entries": ({(5, E1): -0.3, (5, 6): -0.4, (5, 6, E1): -0.05, (6, E1): -0.9}, {(5,): -0.1, (6,): -0.2, (5, 6): -0.3}, 3),
    "start": ({(S1,): -99.0, (S1, 5): -0.2, (S1, 5, 6): -0.1, (5, 6): -0.7}, {(S1,): -0.4, (S1, 5): -0.3, (5,): -0.2, (5, 6): -0.1}, 3),
}


@pytest.mark.parametrize("name", list(TRIES))
def test_ngram_score_kernel_small_models(dev, name):
    """Every node as a row, EVERY token of the vocabulary as a candidate column (each child's token, tokens below the first and above
    the last child, 1 and V - 2, the blank, <eos> in a candidate column) plus the extra <eos> column."""
    P, B, N = TRIES[name]
    P = {**_UNI, **P}
    sc = _scorer(V1, P, B, order=N)
    ref = _Def(P, B, V1, N)
    if name == "unigram-only":
        assert (sc.n_nodes, sc.n_edges) == (1, V1 - 1)
    if name == "1-2-3-children":
        assert [int(sc.first[s + 1] - sc.first[s]) for s in (sc.contexts.index((5,)), sc.contexts.index((6,)), sc.contexts.index((7,)))] == [1, 2, 3]
    if name == "start":
        assert sc.contexts[sc.start_node] == (S1,) and S1 not in sc.tok.tolist()
    else:
        assert sc.start_node == 0
    nodes = list(range(sc.n_nodes))
    score, nxt = _check_kernel(dev, sc, ref, nodes, [list(range(V1))] * len(nodes))
    assert torch.equal(score[:, V1 - 1], score[:, V1]) and torch.equal(nxt[:, V1 - 1], nxt[:, V1])
    rng = random.Random(1)
    alphabet = sorted({t for g in P if len(g) > 1 for t in g if t < V1} | {0, 2, E1})
    for _ in range(100):
        seq = [rng.choice(alphabet) for _ in range(rng.randint(1, 9))]
        got = float(sc.walk(seq)[0])
        assert abs(got - ref.total(seq)) <= 1e-5 * max(1.0, abs(got)), seq


def test_ngram_score_kernel_back_skips_a_level_and_next_is_a_shorter_suffix(dev):
    """<unk> fill-in makes unigrams that are no contexts: the node (5, 6) has no node (6,) to fall back to, so `back` goes straight to
    the root; the trigram (5, 6, 7) leads to (7,) because (6, 7) is no node, and (5, 6, 8) to the root."""
    unk = -3.0
    P = {(E1,): -1.5, (5,): -1.0, (7,): -1.2, (5, 6): -0.4, (5, 6, 7): -0.1, (5, 6, 8): -0.2, (7, 9): -0.3}
    B = {(5,): -0.5, (7,): -0.6, (5, 6): -0.7}
    sc = _scorer(V1, P, B, order=3, unk_logp=unk)
    ref = _Def(P, B, V1, 3, unk=unk)
    s56, s7 = sc.contexts.index((5, 6)), sc.contexts.index((7,))
    assert (6,) not in sc.contexts and int(sc.back[s56]) == 0
    assert sc.step(s56, 7)[1] == s7 and sc.step(s56, 8)[1] == 0 and sc.step(s7, 9)[1] == sc.contexts.index((7, 9))
    r, nx = sc.step(s56, 9)  # bow(5 6), then the root at once: the level of (6,) carries back-off 0 and no entries
    assert r == np.float32(np.float32(-0.7) + np.float32(unk)) and nx == 0
    _check_kernel(dev, sc, ref, list(range(sc.n_nodes)), [list(range(V1))] * sc.n_nodes)
    seq = [5, 6, 7, 9, 5, 6, 8, 3, E1]
    assert abs(float(sc.walk(seq)[0]) - ref.total(seq)) < 1e-4


def _random_model(V, n_bi, n_tri, seed):
    rng = random.Random(seed)
    P = {(t,): -rng.uniform(2.0, 9.0) for t in range(1, V)}
    P[(V,)] = -99.0
    B = {(V,): -rng.uniform(0.1, 1.0)}
    heads = list(range(1, V - 1)) + [V]
    bis = set()
    while len(bis) < n_bi:
        bis.add((rng.choice(heads), rng.randint(1, V - 1)))
    bis = sorted(bis)
    for g in bis:
        P[g] = -rng.uniform(0.1, 6.0)
    inner = [g for g in bis if g[1] != V - 1]
    tris = set()
    while len(tris) < n_tri:
        tris.add(rng.choice(inner) + (rng.randint(1, V - 1),))
    for g in tris:
        P[g] = -rng.uniform(0.1, 5.0)
        B[g[:2]] = -rng.uniform(0.05, 2.0)
    for g in bis:
        B.setdefault((g[0],), -rng.uniform(0.05, 2.0))
    return P, B


_LARGE = {}


def _large():
    if not _LARGE:
        P, B = _random_model(5049, 65000, 130000, 5)
        _LARGE["m"] = (_scorer(5049, P, B, order=3), _Def(P, B, 5049, 3))
    return _LARGE["m"]


def test_ngram_score_kernel_large_model(dev):
    """A random 3-gram model over the full vocabulary of 5 049 with about 2 * 10^5 n-grams; 64 rows x 60 candidates drawn from the
    row's own children, the children of the node it backs off to, and the whole vocabulary."""
    V, rng = 5049, random.Random(6)
    sc, ref = _large()
    assert sc.n_edges >= 195000 and sc.order == 3 and sc.start_node != 0
    deep = [s for s in range(sc.n_nodes) if len(sc.contexts[s]) == 2 and sc.first[s + 1] > sc.first[s]]
    mid = [s for s in range(sc.n_nodes) if len(sc.contexts[s]) == 1 and sc.first[s + 1] > sc.first[s]]
    nodes = [0, sc.start_node] + [rng.choice(deep) for _ in range(40)] + [rng.choice(mid) for _ in range(22)]
    cand = []
    for s in nodes:
        own = sc.tok[sc.first[s]: sc.first[s + 1]].tolist()
        b = int(sc.back[s])
        lower = sc.tok[sc.first[b]: sc.first[b + 1]].tolist()
        row = [rng.choice(own) for _ in range(20)] + [rng.choice(lower) for _ in range(20)] + [rng.randint(0, V - 1) for _ in range(18)] + [0, V - 1]
        rng.shuffle(row)
        cand.append(row)
    score, nxt = _check_kernel(dev, sc, ref, nodes, cand)
    assert int((nxt > 0).sum()) > 1000 and int((score == 0).sum()) >= 64
    for _ in range(20):
        g = rng.choice(deep)
        seq = list(sc.contexts[g]) + [rng.randint(1, V - 2) for _ in range(4)] + [V - 1]
        seq = [t for t in seq if t != V]
        got = float(sc.walk(seq)[0])
        assert abs(got - ref.total(seq)) <= 1e-5 * max(1.0, abs(got))


def test_ngram_score_without_a_model_and_oversized_tables(dev):
    from auto_avsr_amd import _lib

    sc = _scorer(V1, _UNI, {}, order=1)
    score, nxt = _kernel(dev, sc, [0, 0], [[1, 2, 3], [0, 4, V1 - 1]], V1 - 1, n_nodes=0)
    assert int(score.abs().max()) == 0 and int(nxt.abs().max()) == 0
    for nn, ne in (((1 << 26) + 1, 5), (5, (1 << 27) + 1), (-1, 5)):
        sc2 = _scorer(V1, _UNI, {}, order=1)
        sc2.n_edges = ne
        with pytest.raises(_lib.AvsrLibraryError, match="nodes or edges"):
            _kernel(dev, sc2, [0], [[1]], V1 - 1, n_nodes=nn)


# ------------------------------------------------------------------------------------------------------- 3. against the reference
def _check_vs_reference(nbest, case):
    assert len(nbest) == case["n_ended"]
    assert len(case["hyps"]) == 4
    for got, ref in zip(nbest, case["hyps"]):
        d = got.asdict()
        assert d["yseq"] == ref["yseq"]
        print(d["score"], ref["score"], d["scores"], ref["scores"])
        assert abs(d["score"] - ref["score"]) < 1e-3 * max(1.0, abs(ref["score"]))
        assert set(d["scores"]) == set(ref["scores"]) and "ngram" in ref["scores"]
        for k, v in ref["scores"].items():
            assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), k
        assert d["scores"]["ngram"] != 0.0


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("case", GOLD, ids=_ID)
def test_ngram_beam_search_vs_reference(dev, case, native):
    """Same weights, same encoder output, same model: the n-best token sequences equal the reference's, total within 1e-3, per-scorer
    scores within 2e-3 (the tolerances of test_context_bias and test_lm_fusion for the same comparison) -- for the one-call-per-step
    search and for the python-issued step.  The last case has the full vocabulary of 5 049."""
    assert case["odim"] < 100 or case["odim"] == 5049
    assert case["T"] <= 12 and 4 <= case["beam"] <= 6
    _check_vs_reference(_run(_case_bs(dev, case), _enc(case, dev), native), case)


# ------------------------------------------------------------------------------------------------------- 4. native against python step
def _same(a, b, keys, tol=1e-3, min_live=3):
    assert len(a) == len(b) and len(a) >= 1
    live = 0
    for x, y in zip(a, b):
        x, y = x.asdict(), y.asdict()
        if y["score"] < -1e8:  # ruled out by the CTC scorer (LOGZERO): these tie and are ordered arbitrarily by any top-k
            assert x["score"] < -1e8
            continue
        live += 1
        assert x["yseq"] == y["yseq"]
        assert abs(x["score"] - y["score"]) < tol * max(1.0, abs(y["score"]))
        assert set(x["scores"]) == set(y["scores"]) == keys
        for k, v in y["scores"].items():
            assert abs(x["scores"][k] - v) < tol * max(1.0, abs(v)), k
        assert x["scores"]["ngram"] == y["scores"]["ngram"]  # the same f32 additions in the same order
    assert live >= min_live
    assert any(h.scores["ngram"] != 0 for h in a)


@pytest.mark.parametrize("maxlenratio", [0.0, -4, 0.5])
def test_ngram_native_beam_search_equals_python_step(dev, maxlenratio):
    """Every ended hypothesis and every per-scorer score, with the end-detection rule, a forced end after four steps and a length cap."""
    case = GOLD[3]
    x = _enc(case, dev)
    _same(_run(_case_bs(dev, case), x, True, maxlenratio), _run(_case_bs(dev, case), x, False, maxlenratio),
          {"decoder", "ctc", "ngram", "length_bonus"})


def test_ngram_with_bias_native_equals_python_step(dev):
    from auto_avsr_amd.bias import ContextBiasScorer

    case = GOLD[4]
    ys = case["hyps"][1]["yseq"]
    mk = lambda: _case_bs(dev, case, bias=ContextBiasScorer([ys[2:4], ys[5:8], [ys[4]]], case["odim"]), bias_weight=0.6)  # noqa: E731
    x = _enc(case, dev)
    a, b = _run(mk(), x, True), _run(mk(), x, False)
    _same(a, b, {"decoder", "ctc", "ngram", "bias"})
    assert any(h.scores["bias"] != 0 for h in a)


def test_ngram_with_lm_native_equals_python_step(dev):
    """The n-gram next to the LM fixture's language model: decoder, lm, ctc, ngram in one search."""
    from auto_avsr_amd.lm import TransformerLM

    lc = GOLD_LM[4]
    E, D, H, FF, NL = lc["lm_dims"]
    lm = TransformerLM(lc["odim"], embed_unit=E, att_unit=D, head=H, unit=FF, layer=NL)
    lm.load_state_dict(synth_state_dict(lm.state_dict(), lc["seed"] + 2))
    lm = lm.to(dev)
    case = next(c for c in GOLD if c["seed"] == lc["seed"] and c["odim"] == lc["odim"])
    x = _enc(case, dev)
    mk = lambda: _case_bs(dev, case, lm=lm, lm_weight=lc["lm_weight"])  # noqa: E731
    a, b = _run(mk(), x, True, -8), _run(mk(), x, False, -8)  # (a forced end after eight steps: the python-issued LM step is slow on the emulator)
    _same(a, b, {"decoder", "ctc", "lm", "ngram"} | ({"length_bonus"} if case["penalty"] else set()))


# ------------------------------------------------------------------------------------------------------- 5. forward_many / forward_batch
def _same_lists(many, single, tol=1e-4):
    assert len(many) == len(single)
    for a, b in zip(many, single):
        assert len(a) == len(b) and len(a) >= 1
        for x, y in zip(a, b):
            x, y = x.asdict(), y.asdict()
            if y["score"] < -1e8:
                assert x["score"] < -1e8
                continue
            assert x["yseq"] == y["yseq"] and abs(x["score"] - y["score"]) < tol * max(1.0, abs(y["score"]))
            assert set(x["scores"]) == set(y["scores"])
            for k, v in y["scores"].items():
                assert abs(x["scores"][k] - v) < tol * max(1.0, abs(v)), k
            assert x["scores"]["ngram"] == y["scores"]["ngram"]


_FIVE = {}


@pytest.fixture
def five(dev):
    """Five utterances (T = 5, 9, 7, 12, 8) and their one-at-a-time results, computed once per backend."""
    key = str(dev)
    if key not in _FIVE:
        case = dict(GOLD[2], beam=6)
        bs = _case_bs(dev, case)
        g = torch.Generator().manual_seed(77)
        xs = [(torch.randn(T, case["D"], generator=g) * 1.5).to(dev) for T in (5, 9, 7, 12, 8)]
        with _precise():
            single = [bs(x) for x in xs]
        assert bs._native and any(h.scores["ngram"] != 0 for nb in single for h in nb)
        _FIVE[key] = (bs, xs, single)
    return _FIVE[key]


def test_ngram_forward_many_equals_one_at_a_time(dev, five):
    """Five utterances through three concurrent sessions, every one of which got the tables."""
    bs, xs, single = five
    with _precise():
        many = bs.forward_many(xs, workers=3)
    assert bs._native and len(bs._native_pool) == 3 and all(s.ngram_key is not None for s in bs._native_pool)
    _same_lists(many, single)


@pytest.mark.parametrize("batch", [1, 2, 4])
def test_ngram_forward_batch_equals_one_at_a_time(dev, five, batch):
    """Groups of 1, 2 and 4 utterances: beams shrink when hypotheses end and utterances retire while others go on -- the compaction
    moves node and sum with the rows, and the sums come back in the packed order of the records."""
    bs, xs, single = five
    with _precise():
        out = bs.forward_batch(xs, batch=batch)
    assert bs._native and bs._native.ngram_key is not None
    _same_lists(out, single)


# ------------------------------------------------------------------------------------------------------- 6. a new model between utterances
def test_set_model_between_utterances(dev):
    case, other = GOLD[0], GOLD[1]
    sc = _case_model(case)
    bs = _case_bs(dev, case, ngram=sc)
    x1, x2 = _enc(case, dev), _enc(case, dev, T=11, seed=31)
    _check_vs_reference(_run(bs, x1, True), case)
    handle, key = bs._native.handle, bs._native.key
    P2 = {g: v * 0.5 for g, v in other["probs"].items()}
    sc.set_model(P2, other["backoffs"], order=other["order"])
    got = _run(bs, x2, True)
    assert bs._native.handle == handle and bs._native.key == key  # the session was not rebuilt
    fresh = _run(_case_bs(dev, case, ngram=_scorer(case["odim"], P2, other["backoffs"], order=other["order"])), x2, True)
    _same_lists([got], [fresh], tol=1e-6)  # (the same launches on the same inputs)
    assert any(h.scores["ngram"] != 0 for h in got)
    # and back: the first utterance's golden result again
    sc.set_model(case["probs"], case["backoffs"], order=case["order"])
    _check_vs_reference(_run(bs, x1, True), case)
    assert bs._native.handle == handle
    # the scorer taken out of the search object: the session's model is detached with it, the search is the one without the slot
    for d in (bs.scorers, bs.part_scorers):
        del d["ngram"]
    got = _run(bs, x2, True)
    assert bs._native.handle == handle and bs._native.ngram_key is None
    plain = _run(_case_bs(dev, case, ngram=None, slot=False), x2, True)
    assert len(got) == len(plain)
    for a, b in zip(got, plain):
        assert a.asdict() == b.asdict()


def test_native_beam_supported_with_ngram(dev):
    from auto_avsr_amd.decode_native import NativeBeam

    case = GOLD[0]
    assert NativeBeam.supported(_case_bs(dev, case))
    assert set(_case_bs(dev, case).part_scorers) == {"ctc", "ngram"}

    class Other(CTCPrefixScorer):  # a foreign partial scorer in the ngram slot
        def __init__(self):
            pass

    assert not NativeBeam.supported(_case_bs(dev, case, ngram=Other()))
    assert not NativeBeam.supported(_case_bs(dev, case, ngram=_scorer(case["odim"] + 1, case["probs"], case["backoffs"], order=3, unk_logp=-5.0)))
    first = _case_bs(dev, case, ngram_first=True)
    assert list(first.part_scorers) == ["ngram", "ctc"] and not NativeBeam.supported(first)
    # a search the session does not take falls back to the python step, with the results of the native one
    x = _enc(case, dev)
    with _precise():
        nbest = first(x)
    assert first._native is False
    ok = _run(_case_bs(dev, case), x, True)
    assert len(nbest) == len(ok)
    for a, b in zip(nbest, ok):
        a, b = a.asdict(), b.asdict()
        assert a["yseq"] == b["yseq"] and abs(a["score"] - b["score"]) < 1e-3 * max(1.0, abs(b["score"]))
        assert a["scores"]["ngram"] == b["scores"]["ngram"]


def test_set_ngram_refuses_oversized_tables(dev):
    from auto_avsr_amd import _lib
    from auto_avsr_amd.decode_native import NativeBeam

    case = GOLD[0]
    bs = _case_bs(dev, case)
    nb = NativeBeam(bs)
    nb._bind(dev, case["T"] + 2)
    L = _lib.lib()
    tabs = bs.part_scorers["ngram"].device_tables(dev)
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    for nn, ne, st, w, msg in (((1 << 26) + 1, 5, 0, 0.5, "nodes or edges"), (5, (1 << 27) + 1, 0, 0.5, "nodes or edges"), (-1, 5, 0, 0.5, "nodes or edges"),
                               (5, 5, 5, 0.5, "start node"), (5, 5, 0, float("inf"), "finite"), (5, 5, 0, float("nan"), "finite")):
        with pytest.raises(_lib.AvsrLibraryError, match=msg):
            L.call("avsr_beam_set_ngram", nb.handle, vp((ctypes.c_int32 * 3)(nn, ne, st)), vp((ctypes.c_float * 1)(w)), *[t.data_ptr() for t in tabs])
    with _precise():
        _check_vs_reference(nb.search(_enc(case, dev)), case)  # the refused calls left the session's model alone


# ------------------------------------------------------------------------------------------------------- 7. without a model
def test_no_ngram_leaves_sizes_and_results_alone(dev):
    """A session whose model was removed (avsr_beam_set_ngram with zero nodes) reports, from both entry points, the sizes of a session
    that never saw the call; with a model it asks for seven [rows] tables more.  The search of a session that had a model and lost it
    is, bit for bit, the search built without the slot."""
    from auto_avsr_amd import _lib
    from auto_avsr_amd.decode_native import NativeBeam

    case = GOLD[2]
    never = NativeBeam(_case_bs(dev, case, ngram=None, slot=False))
    bs = _case_bs(dev, case)
    with_model = NativeBeam(bs)
    never._bind(dev, 64)
    with_model._bind(dev, 64)
    assert never.ngram_key is None and with_model.ngram_key is not None
    L = _lib.lib()

    def sizes(nb):
        out = []
        for T, Lmax in ((1, 1), (23, 23), (37, 50)):
            out.append(L.call("avsr_beam_workspace_bytes", nb.handle, T, Lmax))
            out.append(nb.group_workspace_bytes([T, 5, 2 * T], Lmax))
        return out

    base, more = sizes(never), sizes(with_model)
    assert all(m > b for m, b in zip(more, base)) and all(m - b <= 7 * 256 + 3 * case["beam"] * 7 * 4 for m, b in zip(more, base))
    x = _enc(case, dev)
    with _precise():
        with_nbest = with_model.search(x)
    for d in (bs.scorers, bs.part_scorers):
        del d["ngram"]
    with_model._bind(dev, 64)
    assert with_model.ngram_key is None and sizes(with_model) == base
    with _precise():
        a, b = with_model.search(x), never.search(x)
    assert len(a) == len(b) >= 1 and [h.asdict() for h in a] == [h.asdict() for h in b]  # bit-equal, no "ngram" key
    assert [h.asdict()["yseq"] for h in with_nbest] != [h.asdict()["yseq"] for h in a] or with_nbest[0].score != a[0].score
    n = ctypes.c_int(-1)
    buf = (ctypes.c_float * 64)()
    L.call("avsr_beam_ngram_sums", with_model.handle, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ctypes.pointer(n), ctypes.c_void_p))
    assert n.value == 0


# ------------------------------------------------------------------------------------------------------- 8. wiring
def _small_e2e(odim, dev):
    from auto_avsr_amd.e2e import E2E

    return E2E(odim, "video", adim=128, aheads=2, eunits=256, elayers=1, dunits=256, dlayers=1, cnn_module_kernel=7).to(dev).eval()


def _ids_arpa(tmp_path, odim, name="lm.arpa"):
    uni = [(-1.0, ("<s>",), -0.5), (-1.2, ("</s>",), None), (-2.0, ("<unk>",), None)] + [(-0.02 * t - 0.8, (str(t),), -0.01 * t) for t in range(1, odim - 1, 2)]
    bi = [(-0.3, ("<s>", "3"), -0.1), (-0.2, ("3", "5"), -0.2), (-0.4, ("5", "</s>"), None), (-0.5, ("7", "9"), None)]
    tri = [(-0.1, ("<s>", "3", "5"), None), (-0.2, ("3", "5", "7"), None)]
    return _arpa(tmp_path, name, {1: uni, 2: bi, 3: tri})


def test_get_beam_search_decoder_with_ngram(dev, tmp_path):
    import lightning
    from auto_avsr_amd.ngram import NgramScorer

    odim = 40
    m = _small_e2e(odim, dev)
    toks = [str(i) for i in range(odim)]
    path = _ids_arpa(tmp_path, odim)
    bs = lightning.get_beam_search_decoder(m, toks, beam_size=3)
    assert "ngram" not in bs.scorers and set(bs.scorers) == {"decoder", "ctc"}
    with pytest.warns(UserWarning, match="without an n-gram weight"):
        bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, ngram=path, ngram_weight=0.0)
    assert "ngram" not in bs.scorers
    with pytest.warns(UserWarning, match="without an n-gram model"):
        bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, ngram_weight=0.4)
    assert "ngram" not in bs.scorers
    bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, ngram=path, ngram_weight=0.4, penalty=0.5)
    sc = bs.part_scorers["ngram"]
    assert isinstance(sc, NgramScorer) and sc.order == 3 and bs.weights["ngram"] == 0.4 and list(bs.part_scorers) == ["ctc", "ngram"]
    bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, ngram=sc, ngram_weight=0.4)
    assert bs.part_scorers["ngram"] is sc
    with pytest.raises(ValueError, match="vocabulary"):
        lightning.get_beam_search_decoder(m, toks + ["x"], beam_size=3, ngram=sc, ngram_weight=0.4)
    with pytest.raises(TypeError):
        lightning.get_beam_search_decoder(m, toks, beam_size=3, ngram=3.5, ngram_weight=0.4)
    with pytest.raises(NotImplementedError, match="n-gram"):
        lightning.get_two_pass_decoder(m, toks, ngram=path, ngram_weight=0.4)
    AF.invalidate_weight_cache()


def test_eval_flags_run_the_test_loop_with_ngram(dev, tmp_path, monkeypatch):
    """eval.py --ngram-path PATH --ngram-weight W: the flags reach ModelModule, whose test loop builds the native search with the model
    -- one at a time, with two workers, and in groups (--decode-batch); they combine with the other decoding flags and are refused
    together with --decode-mode rescore."""
    import eval as EV
    import lightning as LM
    from auto_avsr_amd.ngram import NgramScorer
    from datamodule.av_dataset import SyntheticAVDataset

    odim = 70  # (above the pre-beam of 60 at the loop's beam of 40)
    path = _ids_arpa(tmp_path, odim)
    args = EV.parse_args(["--ngram-path", path, "--ngram-weight", "0.4", "--synthetic-utterances", "2"])
    assert (args.ngram_path, args.ngram_weight) == (path, 0.4)
    plain = EV.parse_args([])
    assert (plain.ngram_path, plain.ngram_weight) == (None, 0.0)
    for extra in (["--decode-workers", "2"], ["--decode-batch", "2"], ["--encode-batch", "2"], ["--lm-path", "x.pt", "--lm-weight", "0.3"],
                  ["--bias-list", "b.txt", "--bias-weight", "1.0"], ["--timestamps", "t.jsonl"]):
        EV.parse_args(["--ngram-path", path, "--ngram-weight", "0.4"] + extra)
    for bad in (["--ngram-path", path, "--ngram-weight", "0.4"], ["--ngram-weight", "0.4"], ["--ngram-path", path]):
        with pytest.raises(SystemExit):
            EV.parse_args(bad + ["--decode-mode", "rescore"])

    class Text:
        token_list = ["<blank>"] + [f"▁w{i}" for i in range(odim - 2)] + ["<eos>"]
        spm = None

        def post_process(self, ids):
            ids = ids[ids != -1]
            return "".join(self.token_list[int(i)] for i in ids).replace("▁", " ").strip().replace("<eos>", "")

    mod = LM.ModelModule.__new__(LM.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.args = args
    mod.modality = "video"
    mod.model = _small_e2e(odim, dev)
    with torch.no_grad():  # (an untrained model would decode nothing: keep it off the blank)
        mod.model.decoder.output_layer.bias[0] = -1000.0
        mod.model.ctc.ctc_lo.bias[0] = -20.0
    AF.invalidate_weight_cache()
    mod.text_transform, mod.token_list = Text(), Text.token_list
    monkeypatch.setattr(LM, "TextTransform", Text)
    loader = torch.utils.data.DataLoader(SyntheticAVDataset(args.synthetic_utterances, "video", odim=odim, seed=2, lengths=[6, 8]), batch_size=None)
    wer = EV.run_test_loop(mod, loader, dev)
    sc = mod.beam_search.part_scorers["ngram"]
    assert isinstance(sc, NgramScorer) and sc.n_vocab == odim and mod.beam_search.weights["ngram"] == 0.4
    assert mod.beam_search._native and mod.beam_search._native.ngram_key is not None  # the loop ran the native step with the model bound
    wer2 = EV.run_test_loop(mod, loader, dev, decode_workers=2)
    assert wer2 == wer and mod.beam_search.part_scorers["ngram"] is sc  # read once
    assert mod.beam_search._native and len(mod.beam_search._native_pool) == 2
    assert EV.run_test_loop(mod, loader, dev, decode_batch=2) == wer
    mod.args = plain
    assert "ngram" not in mod._make_beam_search().scorers
    AF.invalidate_weight_cache()
