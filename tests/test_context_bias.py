"""Contextual biasing (phrase boosting) in the beam search: the trie scorer of auto_avsr_amd/bias.py alone (`avsr_bias_score`
against a python walk), inside the one-call-per-step session of csrc/decode.hip (avsr_beam_set_bias) and in the python-issued step --
against golden vectors of the reference's BatchBeamSearch with an independent dict-trie scorer (tests/golden/make_golden_bias.py) --
in forward_many / forward_batch, across a change of the list between utterances, and through get_beam_search_decoder / eval.py.
Kernels through the emulator (CPU suite) or on the MI355X (-m gpu)."""
import ctypes
import os
import random
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
from synth import synth_state_dict  # noqa: E402

from auto_avsr_amd import functional as AF  # noqa: E402
from auto_avsr_amd import nets  # noqa: E402
from auto_avsr_amd.decoding import BatchBeamSearch, CTCPrefixScorer, LengthBonus  # noqa: E402

GOLD = torch.load(os.path.join(HERE, "golden", "golden_bias_v1.pt"), weights_only=False)["cases"]
GOLD_LM = torch.load(os.path.join(HERE, "golden", "golden_lm_v1.pt"), weights_only=False)["cases"]
GROUP_A = torch.load(os.path.join(HERE, "golden", "golden_decode_batch_v1.pt"), weights_only=False)["groups"][0]
_ID = lambda c: f"seed{c['seed']}-w{c['bias_weight']}"  # noqa: E731
SMALL = [c for c in GOLD if c["odim"] < 1000]


class _precise:
    def __enter__(self):
        AF.set_precise(True)

    def __exit__(self, *a):
        AF.set_precise(False)


def _bias(phrases, odim):
    from auto_avsr_amd.bias import ContextBiasScorer

    return ContextBiasScorer(phrases, odim)


def _bs(dev, seed, odim, beam, ctc_weight, penalty, bias=None, bias_weight=0.0, lm=None, lm_weight=0.0, pre_beam_score_key="decoder", D=128):
    torch.manual_seed(0)
    dec = nets.TransformerDecoder(odim, attention_dim=D, attention_heads=2, linear_units=256, num_blocks=2).eval()
    ctc = nets.CTC(odim, D, 0.1, reduce=True).eval()
    dec.load_state_dict(synth_state_dict(dec.state_dict(), seed))
    ctc.load_state_dict(synth_state_dict(ctc.state_dict(), seed + 1))
    dec, ctc = dec.to(dev), ctc.to(dev)
    scorers = {"decoder": dec, "ctc": CTCPrefixScorer(ctc, odim - 1), "lm": lm, "bias": bias, "length_bonus": LengthBonus(odim)}
    weights = {"decoder": 1.0 - ctc_weight, "ctc": ctc_weight, "lm": lm_weight, "bias": bias_weight, "length_bonus": penalty}
    return BatchBeamSearch(beam_size=beam, vocab_size=odim, weights=weights, scorers=scorers, sos=odim - 1, eos=odim - 1,
                           token_list=[str(i) for i in range(odim)], pre_beam_score_key=pre_beam_score_key)


def _case_bs(dev, case, **kw):
    kw.setdefault("bias", _bias(case["phrases"], case["odim"]))
    kw.setdefault("bias_weight", case["bias_weight"])
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


# ------------------------------------------------------------------------------------------------------- 1. the kernel alone
class _Walker:
    """The semantics of the issue on nested dicts, nodes named by their path: shares nothing with auto_avsr_amd/bias.py."""

    def __init__(self, phrases):
        self.root = {}
        for ph in phrases:
            d = self.root
            for t in ph:
                d = d.setdefault(t, {})
            d[None] = True

    def total(self, tokens):
        d, unc, total = self.root, 0, 0
        for t in tokens:
            if t in d:
                d, unc, g = d[t], unc + 1, 1
            else:
                g = -unc
                if t in self.root:
                    d, unc, g = self.root[t], 1, g + 1
                else:
                    d, unc = self.root, 0
            if None in d:
                unc = 0
                if len(d) == 1:
                    d = self.root
            total += g
        return total


def _kernel(dev, sc, nodes, cand, eos):
    from auto_avsr_amd import ops

    first, tok, child, unc = sc.device_tables(dev)
    node_t = torch.tensor(nodes, dtype=torch.int32, device=dev)
    cand_t = torch.tensor(cand, dtype=torch.int64, device=dev).contiguous()
    n, S = cand_t.shape
    gain = torch.full((n, S + 1), 77.0, dtype=torch.float32, device=dev)
    nxt = torch.full((n, S + 1), -7, dtype=torch.int32, device=dev)
    ops.call("avsr_bias_score", ops._ptr(first), ops._ptr(tok), ops._ptr(child), ops._ptr(unc), sc.n_nodes, sc.n_edges, ops._ptr(node_t),
             ops._ptr(cand_t), n, S, eos, ops._ptr(gain), ops._ptr(nxt), ops._stream(gain))
    return gain.cpu(), nxt.cpu()


def _expect(sc, nodes, cand, eos):
    g = torch.empty(len(nodes), len(cand[0]) + 1)
    nx = torch.empty(len(nodes), len(cand[0]) + 1, dtype=torch.int32)
    for r, s in enumerate(nodes):
        for c, v in enumerate(list(cand[r]) + [eos]):
            g[r, c], nx[r, c] = sc.step(s, v)
    return g, nx


V1 = 50
TRIES = {
    "empty": [],
    "root-fanout-1": [[7, 8, 9]],
    "1-2-3-children": [[5, 10], [5, 20, 3], [5, 20, 30], [5, 30, 11], [5, 30, 22], [5, 30, 33], [9, 1], [9, V1 - 2]],
    "edge-tokens": [[1], [V1 - 2], [1, V1 - 2, 1], [V1 - 2, 1]],
    "prefix-short-first": [[4, 5], [4, 5, 6, 7]],
    "prefix-long-first": [[4, 5, 6, 7], [4, 5]],
    "duplicate": [[3, 4, 5], [3, 4, 5], [3, 4]],
    "one-token": [[12], [13, 14]],
}


@pytest.mark.parametrize("name", list(TRIES))
def test_bias_score_kernel_small_tries(dev, name):
    """Every node of the trie as a row, EVERY token of the vocabulary as a candidate column (each child's token, tokens below the
    first and above the last child, 1 and V - 2, blank, and <eos> in a candidate column) plus the extra <eos> column: gains and next
    nodes equal the host walk exactly; the host walk's sums equal an independent dict-trie walk on random token strings."""
    sc = _bias(TRIES[name], V1)
    if name == "empty":
        assert (sc.n_nodes, sc.n_edges) == (1, 0)
    if name.startswith("prefix"):
        assert sc.n_nodes == 5 and int(sc.unc[2]) == 0 and sc.child.tolist().count(0) == 1  # [4, 5] is an end node with a child
    if name == "duplicate":
        assert sc.n_nodes == 4 and sc.phrases == [(3, 4), (3, 4, 5)]
    nodes = list(range(sc.n_nodes))
    cand = [list(range(V1))] * len(nodes)
    gain, nxt = _kernel(dev, sc, nodes, cand, V1 - 1)
    eg, en = _expect(sc, nodes, cand, V1 - 1)
    assert torch.equal(gain, eg) and torch.equal(nxt, en)
    assert torch.equal(gain[:, V1 - 1], gain[:, V1]) and torch.equal(gain[:, V1], -torch.from_numpy(sc.unc).float())  # <eos>: rule 2, to the root
    assert int(nxt[:, V1].abs().max()) == 0
    rng, w = random.Random(1), _Walker(TRIES[name])
    alphabet = sorted({t for ph in TRIES[name] for t in ph} | {2, V1 - 1})
    for _ in range(200):
        seq = [rng.choice(alphabet) for _ in range(rng.randint(1, 9))]
        assert sc.walk(seq)[0] == w.total(seq), seq


def test_bias_score_kernel_large_trie(dev):
    """A random trie of more than 10 000 nodes with a root fan-out above 1 000 (binary searches of ~10 steps at the root), 64 rows x 60
    candidates drawn from the row's own children, the root's children and the whole vocabulary."""
    V, rng = 5049, random.Random(5)
    heads = rng.sample(range(1, V - 1), 1500)
    phrases = [[rng.choice(heads)] + [rng.randint(1, V - 2) for _ in range(rng.randint(1, 4))] for _ in range(6000)]
    sc = _bias(phrases, V)
    assert sc.n_nodes >= 10000 and int(sc.first[1]) >= 1000
    inner = [s for s in range(sc.n_nodes) if sc.first[s + 1] > sc.first[s]]
    nodes = [0, 0] + [rng.choice(inner) for _ in range(62)]
    roots = sc.tok[: sc.first[1]].tolist()
    cand = []
    for s in nodes:
        own = sc.tok[sc.first[s]: sc.first[s + 1]].tolist()
        row = [rng.choice(own) for _ in range(20)] + [rng.choice(roots) for _ in range(20)] + [rng.randint(0, V - 1) for _ in range(18)] + [0, V - 1]
        rng.shuffle(row)
        cand.append(row)
    gain, nxt = _kernel(dev, sc, nodes, cand, V - 1)
    eg, en = _expect(sc, nodes, cand, V - 1)
    assert torch.equal(gain, eg) and torch.equal(nxt, en)
    assert int((gain == 1).sum()) > 600 and int((gain < 0).sum()) > 100 and int((nxt > 0).sum()) > 600
    w = _Walker(phrases)
    for ph in phrases[:200]:
        seq = ph + [rng.choice(roots), V - 1]
        assert sc.walk(seq)[0] == w.total(seq)


# ------------------------------------------------------------------------------------------------------- 2. against the reference
def _check_vs_reference(nbest, case):
    assert len(nbest) == case["n_ended"]
    assert len(case["hyps"]) == 4
    for got, ref in zip(nbest, case["hyps"]):
        d = got.asdict()
        assert d["yseq"] == ref["yseq"]
        print(d["score"], ref["score"], d["scores"], ref["scores"])
        assert abs(d["score"] - ref["score"]) < 1e-3 * max(1.0, abs(ref["score"]))
        assert set(d["scores"]) == set(ref["scores"]) and "bias" in ref["scores"]
        for k, v in ref["scores"].items():
            assert abs(d["scores"][k] - v) < 2e-3 * max(1.0, abs(v)), k
        assert d["scores"]["bias"] == ref["scores"]["bias"]  # a sum of small integers: exact


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("case", GOLD, ids=_ID)
def test_bias_beam_search_vs_reference(dev, case, native):
    """Same weights, same encoder output, same phrases: the n-best token sequences equal the reference's, total within 1e-3, per-scorer
    scores within 2e-3 (the tolerances of test_lm_fusion for the same comparison), the bias sums exactly -- for the one-call-per-step
    search and for the python-issued step.  The last case has the full vocabulary of 5 049."""
    _check_vs_reference(_run(_case_bs(dev, case), _enc(case, dev), native), case)


# ------------------------------------------------------------------------------------------------------- 3. native against python step
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
        assert x["scores"]["bias"] == y["scores"]["bias"]
    assert live >= min_live


@pytest.mark.parametrize("maxlenratio", [0.0, -4, 0.5])
def test_bias_native_beam_search_equals_python_step(dev, maxlenratio):
    """Every ended hypothesis and every per-scorer score, with the end-detection rule, a forced end after four steps and a length cap."""
    case = GOLD[3]
    x = _enc(case, dev)
    _same(_run(_case_bs(dev, case), x, True, maxlenratio), _run(_case_bs(dev, case), x, False, maxlenratio),
          {"decoder", "ctc", "bias", "length_bonus"})


def test_bias_with_lm_native_equals_python_step(dev):
    """The bias next to the LM fixture's language model: decoder, lm, bias, ctc in one search (the order of additions in the selection)."""
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
    _same(a, b, {"decoder", "ctc", "lm", "bias"})
    assert any(h.scores["bias"] != 0 for h in a)


# ------------------------------------------------------------------------------------------------------- 4. forward_many / forward_batch
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
            assert x["scores"]["bias"] == y["scores"]["bias"]


def test_bias_forward_many_equals_one_at_a_time(dev):
    """Five utterances through three concurrent sessions, every one of which got the list."""
    case = dict(GOLD[2], beam=6)
    bs = _case_bs(dev, case)
    g = torch.Generator().manual_seed(77)
    xs = [(torch.randn(T, case["D"], generator=g) * 1.5).to(dev) for T in (5, 9, 7, 12, 8)]
    with _precise():
        many = bs.forward_many(xs, workers=3)
        assert bs._native and len(bs._native_pool) == 3 and all(s.bias_key is not None for s in bs._native_pool)
        single = [bs(x) for x in xs]
    _same_lists(many, single)
    assert any(h.scores["bias"] != 0 for nb in single for h in nb)


_GROUP = {}


@pytest.fixture
def group_single(dev):
    """Six utterances of group A of the batched-search fixture (1 .. 36 frames, three of which end on <eos> before their last step) with
    a list cut out of their own unbiased hypotheses; the one-at-a-time results, computed once per backend."""
    key = str(dev)
    if key not in _GROUP:
        g = GROUP_A
        pick = [1, 4, 0, 3, 2, 10]  # 1, 2, 9, 15, 36, 5 frames
        xs = [(torch.randn(T, 128, generator=torch.Generator().manual_seed(7000 + 100 * g["seed"] + T)) * 1.5).to(dev)
              for T in (g["lengths"][i] for i in pick)]
        phrases = []
        for u in (g["utts"][i] for i in pick):
            for h in u["hyps"][:2]:
                ys = h["yseq"][1:-1]
                phrases += [ys[i: i + 3] for i in range(0, max(0, len(ys) - 2), 5)] + [ys[:1]]
        phrases = [p for p in phrases if p and all(1 <= t <= g["odim"] - 2 for t in p)]
        bs = _bs(dev, g["seed"], g["odim"], g["beam"], g["ctc_weight"], g["penalty"], bias=_bias(phrases, g["odim"]), bias_weight=0.7)
        with _precise():
            single = [bs(x) for x in xs]
        _GROUP[key] = (bs, xs, single)
    return _GROUP[key]


@pytest.mark.parametrize("batch", [1, 2, 4])
def test_bias_forward_batch_equals_one_at_a_time(dev, group_single, batch):
    """Groups of 1, 2 and 4 utterances: beams shrink when hypotheses end and utterances retire while others go on -- the compaction moves
    node and sum with the rows."""
    bs, xs, single = group_single
    assert min(x.shape[0] for x in xs) == 1 and max(x.shape[0] for x in xs) == 36
    assert any(len(nb[0].yseq) - 2 < x.shape[0] for nb, x in zip(single, xs))  # some end before their last frame
    assert any(h.scores["bias"] != 0 for nb in single for h in nb)
    with _precise():
        out = bs.forward_batch(xs, batch=batch)
    assert bs._native
    _same_lists(out, single)


# ------------------------------------------------------------------------------------------------------- 5. a new list between utterances
def test_set_phrases_between_utterances(dev):
    case = GOLD[0]
    other = GOLD[1]["hyps"][1]["yseq"]
    second = [other[2:5], other[6:8], [other[9]]]
    sc = _bias(case["phrases"], case["odim"])
    bs = _case_bs(dev, case, bias=sc)
    x1, x2 = _enc(case, dev), _enc(case, dev, T=11, seed=31)
    _check_vs_reference(_run(bs, x1, True), case)
    handle, key = bs._native.handle, bs._native.key
    sc.set_phrases(second)
    got = _run(bs, x2, True)
    assert bs._native.handle == handle and bs._native.key == key  # the session was not rebuilt
    fresh = _run(_case_bs(dev, case, bias=_bias(second, case["odim"])), x2, True)
    _same_lists([got], [fresh], tol=1e-6)  # (the same launches on the same inputs)
    assert any(h.scores["bias"] != 0 for h in got)
    # an emptied list: the search without the scorer, apart from the extra key
    sc.set_phrases([])
    got = _run(bs, x2, True)
    assert bs._native.handle == handle
    plain = _run(_case_bs(dev, case, bias=None, bias_weight=0.0), x2, True)
    assert len(got) == len(plain)
    for a, b in zip(got, plain):
        a, b = a.asdict(), b.asdict()
        assert a["scores"].pop("bias") == 0.0 and a["yseq"] == b["yseq"] and set(a["scores"]) == set(b["scores"])
        assert abs(a["score"] - b["score"]) <= 1e-6 * max(1.0, abs(b["score"]))
        assert all(abs(a["scores"][k] - v) <= 1e-6 * max(1.0, abs(v)) for k, v in b["scores"].items())
    # and back: the first utterance's golden result again
    sc.set_phrases(case["phrases"])
    _check_vs_reference(_run(bs, x1, True), case)
    assert bs._native.handle == handle
    # the scorer taken out of the search object afterwards: the session's list is detached with it
    for d in (bs.scorers, bs.full_scorers):
        del d["bias"]
    got = _run(bs, x2, True)
    assert bs._native.handle == handle and bs._native.bias_key is None
    assert len(got) == len(plain)
    for a, b in zip(got, plain):
        a, b = a.asdict(), b.asdict()
        assert a["yseq"] == b["yseq"] and set(a["scores"]) == set(b["scores"])
        assert abs(a["score"] - b["score"]) <= 1e-6 * max(1.0, abs(b["score"]))


# ------------------------------------------------------------------------------------------------------- 6. eligibility
def test_native_beam_supported_with_bias(dev):
    from auto_avsr_amd.bias import ContextBiasScorer
    from auto_avsr_amd.decode_native import NativeBeam

    case = GOLD[0]
    assert NativeBeam.supported(_case_bs(dev, case))
    assert not NativeBeam.supported(_case_bs(dev, case, pre_beam_score_key="full"))

    class Other(LengthBonus):  # a foreign full scorer in the bias slot
        pass

    assert not NativeBeam.supported(_case_bs(dev, case, bias=Other(case["odim"])))
    x = _enc(case, dev)
    bs = _case_bs(dev, case, bias=Other(case["odim"]))
    with _precise():
        nbest = bs(x)
    assert bs._native is False and len(nbest) >= 1 and "bias" in nbest[0].scores
    bs = _case_bs(dev, case, pre_beam_score_key="full")
    with _precise():
        nbest = bs(x)
    assert bs._native is False and len(nbest) >= 1
    V = case["odim"]
    for bad in ([[3, 0, 4]], [[V - 1]], [[5], [6, V - 1]], [[V]], [[-1]], [[]]):
        with pytest.raises(ValueError):
            ContextBiasScorer(bad, V)
    from espnet.nets.scorers.context_bias import ContextBiasScorer as Shim

    assert Shim is ContextBiasScorer


def test_set_bias_refuses_oversized_tables(dev):
    from auto_avsr_amd import _lib
    from auto_avsr_amd.decode_native import NativeBeam

    case = GOLD[0]
    bs = _case_bs(dev, case)
    nb = NativeBeam(bs)
    nb._bind(dev, case["T"] + 2)
    L = _lib.lib()
    tabs = bs.full_scorers["bias"].device_tables(dev)
    fcfg = (ctypes.c_float * 1)(0.5)
    for nn, ne in (((1 << 24) + 1, 5), (5, (1 << 24) + 1), (-1, 5)):
        cfg = (ctypes.c_int32 * 2)(nn, ne)
        with pytest.raises(_lib.AvsrLibraryError, match="nodes or edges"):
            L.call("avsr_beam_set_bias", nb.handle, ctypes.cast(cfg, ctypes.c_void_p), ctypes.cast(fcfg, ctypes.c_void_p), *[t.data_ptr() for t in tabs])
    with _precise():
        _check_vs_reference(nb.search(_enc(case, dev)), case)  # the refused calls left the session's list alone


# ------------------------------------------------------------------------------------------------------- 7. wiring
def _small_e2e(odim, dev):
    from auto_avsr_amd.e2e import E2E

    return E2E(odim, "video", adim=128, aheads=2, eunits=256, elayers=1, dunits=256, dlayers=1, cnn_module_kernel=7).to(dev).eval()


def test_get_beam_search_decoder_with_bias(dev):
    import lightning
    from auto_avsr_amd.bias import ContextBiasScorer

    odim = 40
    m = _small_e2e(odim, dev)
    toks = [str(i) for i in range(odim)]
    for kw in (dict(), dict(bias_phrases=[[3, 4]], bias_weight=0.0)):
        bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, **kw)
        assert "bias" not in bs.full_scorers and set(bs.scorers) == {"decoder", "ctc"}
    with pytest.warns(UserWarning, match="without a bias list"):
        bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, bias_weight=0.8)
    assert "bias" not in bs.full_scorers
    bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, bias_phrases=[[3, 4], [5]], bias_weight=0.8, penalty=0.5)
    assert isinstance(bs.full_scorers["bias"], ContextBiasScorer) and bs.weights["bias"] == 0.8
    assert list(bs.full_scorers) == ["decoder", "bias", "length_bonus"]  # after `lm`, before `length_bonus`
    sc = ContextBiasScorer([], odim)
    bs = lightning.get_beam_search_decoder(m, toks, beam_size=3, bias_phrases=sc, bias_weight=0.8)
    assert bs.full_scorers["bias"] is sc
    with pytest.raises(ValueError):
        lightning.get_beam_search_decoder(m, toks, beam_size=3, bias_phrases=[[odim - 1]], bias_weight=0.8)
    with pytest.raises(ValueError):
        lightning.get_beam_search_decoder(m, toks + ["x"], beam_size=3, bias_phrases=sc, bias_weight=0.8)
    AF.invalidate_weight_cache()


def test_eval_flags_run_the_test_loop_with_bias(dev, tmp_path, monkeypatch):
    """eval.py --bias-list PATH --bias-weight W: the flags reach ModelModule, whose test loop builds the native search with the list --
    one at a time, with two workers and --timestamps, and in groups (--decode-batch); a list of integer lines needs no tokenizer file,
    a text line without one is a clear error, and the flags are refused together with --decode-mode rescore."""
    import json

    import eval as EV
    import lightning as LM
    from auto_avsr_amd.bias import ContextBiasScorer
    from datamodule.av_dataset import SyntheticAVDataset

    odim = 70  # (above the pre-beam of 60 at the loop's beam of 40)
    path = tmp_path / "bias.txt"
    path.write_text("3 4 5\n\n17\n  8 9\n")
    args = EV.parse_args(["--bias-list", str(path), "--bias-weight", "1.5", "--synthetic-utterances", "2"])
    assert (args.bias_list, args.bias_weight) == (str(path), 1.5)
    plain = EV.parse_args([])
    assert (plain.bias_list, plain.bias_weight) == (None, 0.0)
    for extra in (["--decode-workers", "2"], ["--decode-batch", "2"], ["--lm-path", "x.pt", "--lm-weight", "0.3"], ["--timestamps", "t.jsonl"]):
        EV.parse_args(["--bias-list", str(path), "--bias-weight", "1.5"] + extra)
    with pytest.raises(SystemExit):
        EV.parse_args(["--bias-list", str(path), "--bias-weight", "1.5", "--decode-mode", "rescore"])
    assert LM.read_bias_list(str(path)) == [[3, 4, 5], [17], [8, 9]]
    text = tmp_path / "text.txt"
    text.write_text("3 4\nhello world\n")

    class Text:
        token_list = ["<blank>"] + [f"▁w{i}" for i in range(odim - 2)] + ["<eos>"]
        spm = None  # the SentencePiece model file is missing

        def post_process(self, ids):
            ids = ids[ids != -1]
            return "".join(self.token_list[int(i)] for i in ids).replace("▁", " ").strip().replace("<eos>", "")

    with pytest.raises(FileNotFoundError, match="SentencePiece"):
        LM.read_bias_list(str(text), Text())

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
    sc = mod.beam_search.full_scorers["bias"]
    assert isinstance(sc, ContextBiasScorer) and sc.phrases == [(3, 4, 5), (8, 9), (17,)] and mod.beam_search.weights["bias"] == 1.5
    assert mod.beam_search._native  # the loop ran the native step with the list attached
    wer2 = EV.run_test_loop(mod, loader, dev, decode_workers=2, timestamps=str(tmp_path / "ts.jsonl"))
    assert wer2 == wer and mod.beam_search.full_scorers["bias"] is sc  # read once
    assert mod.beam_search._native and len(mod.beam_search._native_pool) == 2
    assert len([json.loads(line) for line in open(tmp_path / "ts.jsonl", encoding="utf8")]) == 2
    assert EV.run_test_loop(mod, loader, dev, decode_batch=2) == wer
    # per-utterance lists in user code
    mod.set_bias([[5, 6]])
    assert sc.phrases == [(5, 6)] and mod.beam_search.full_scorers["bias"] is sc
    # without the flags: no bias in the search, and set_bias says so
    # half of the flags: a list without a weight is not read and says so; a weight without a list builds the empty scorer and says so
    mod.args = EV.parse_args(["--bias-list", str(path)])
    with pytest.warns(UserWarning, match="without a bias weight"):
        assert "bias" not in mod._make_beam_search().full_scorers
    mod.args = EV.parse_args(["--bias-weight", "1.0"])
    with pytest.warns(UserWarning, match="without a bias list"):
        empty = mod._make_beam_search().full_scorers["bias"]
    assert empty.phrases == [] and empty is not sc
    mod.args = plain
    assert "bias" not in mod._make_beam_search().full_scorers
    with pytest.raises(ValueError):
        mod.set_bias([[5]])
    AF.invalidate_weight_cache()


# ------------------------------------------------------------------------------------------------------- 8. without a list
def test_no_bias_list_leaves_the_workspace_sizes_alone(dev):
    """A session whose list was emptied (avsr_beam_set_bias with zero nodes) reports, from both entry points, the sizes of a session that
    never saw the call; with a list the session asks for five [rows] tables more, and not a byte beyond what it carves (guard-page test)."""
    from auto_avsr_amd import _lib
    from auto_avsr_amd.decode_native import NativeBeam

    case = GOLD[2]
    never = NativeBeam(_case_bs(dev, case, bias=None, bias_weight=0.0))
    sc = _bias(case["phrases"], case["odim"])
    with_list = NativeBeam(_case_bs(dev, case, bias=sc))
    never._bind(dev, 64)
    with_list._bind(dev, 64)
    assert never.bias_key is None and with_list.bias_key is not None
    L = _lib.lib()

    def sizes(nb):
        out = []
        for T, Lmax in ((1, 1), (23, 23), (37, 50)):
            out.append(L.call("avsr_beam_workspace_bytes", nb.handle, T, Lmax))
            out.append(nb.group_workspace_bytes([T, 5, 2 * T], Lmax))
        return out

    base, more = sizes(never), sizes(with_list)
    assert all(m > b for m, b in zip(more, base)) and all(m - b <= 5 * 256 + 3 * case["beam"] * 5 * 4 for m, b in zip(more, base))
    sc.set_phrases([])
    with_list._bind(dev, 64)
    assert sizes(with_list) == base
