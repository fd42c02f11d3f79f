"""Two-pass decoding (not in the reference): a time-synchronous CTC prefix beam search on the device proposes an n-best
(csrc/ctc_beam.hip, one launch for a whole batch of utterances), then ONE teacher-forced pass of the attention decoder -- and of the
language model, when there is one -- over all of them rescores it under the objective of the reference's hybrid search:

    score(y) = (1 - ctc_weight) * sum_{i <= L+1} log p_dec(y_i | sos, y_<i)  +  ctc_weight * log P_ctc(y | x)
               + lm_weight * sum_{i <= L+1} log p_lm(y_i | sos, y_<i)  +  penalty * (L + 1),        y_{L+1} = <eos>
               + bias_weight * (gains of auto_avsr_amd/bias.py along y_1 .. y_{L+1})

which is exactly what the reference's BatchBeamSearch stores for a hypothesis that ended with a scored <eos> (its `scores`: the
teacher-forced decoder sum, the exact CTC log-likelihood, len(y) + 1 for the length bonus; tests/test_two_pass.py pins this on the
golden searches).  The first-pass score only selects the n-best; the CTC term of the final score is the exact likelihood
(avsr_ctc_score: all hypotheses of an utterance against one copy of its posteriors).  The label-synchronous search is a chain of
maxlen dependent decoder steps per utterance; here the only chain is the T frames inside one kernel.

Contextual biasing (`scorers["bias"]`, a ContextBiasScorer, with `weights["bias"]`): the first pass ranks its prefixes by CTC total +
weight * (gains so far), which pulls the expected phrases into the beam (a boosted token still has to be among the frame's `topk`
tokens), and the objective carries the bias term of the label-synchronous search; the term of the n-best comes back from the first
pass itself.  The scorer is read at every call: `set_phrases` between utterances needs no rebuild.

Back-off n-gram model (`scorers["ngram"]`, an NgramScorer, with `weights["ngram"]`; `set_ngram` swaps it between calls): the first pass
ranks its prefixes by CTC total (+ bias) + weight * G(prefix) + len_bonus * len(prefix), G the model's running sum of
log-probabilities -- the time-synchronous search of every CTC + n-gram decoder, with its per-token bonus against the deletions a sum of
negative terms favours --, and the objective carries

               + ngram_weight * sum_{i <= L+1} log p_ng(y_i | y_<i)

which is what the hybrid search stores in scores["ngram"] for a hypothesis that ended with a scored <eos>.  The term of the n-best
comes back from the first pass (bit for bit the host walk); `rescore` walks sequences given from outside on the host.  len_bonus only
steers the first pass: it is no term of the objective (`length_bonus` is)."""
from typing import List

import torch

from . import functional as AF
from . import nets, ops
from .decoding import Hypothesis


class TwoPassDecoder:
    """A plain object (it owns no parameters: the scorers stay where they are).  Drop-in for BatchBeamSearch where it is called
    (`__call__(enc)`, `forward_many(encs)`): the same scorer / weight dictionaries as lightning.get_beam_search_decoder builds -- `decoder` (TransformerDecoder), `ctc` (the CTC head or its CTCPrefixScorer),
    optional `lm` (TransformerLM), optional `bias` (ContextBiasScorer), optional `ngram` (NgramScorer), optional `length_bonus` (only its weight is used) -- and lists of decoding.Hypothesis, best first,
    with yseq = [sos, y..., eos] and one `scores` entry per scorer of non-zero weight."""

    def __init__(self, scorers, weights, sos, eos, token_list=None, beam_size=16, topk=16, nbest=None, blank=0, ignore_id=-1,
                 len_bonus=0.0):
        self.weights = {k: float(v) for k, v in weights.items()}
        self.scorers = {k: v for k, v in scorers.items() if v is not None and self.weights.get(k, 0.0) != 0.0}
        ctc = scorers.get("ctc")
        if ctc is None or scorers.get("decoder") is None:
            raise ValueError("two-pass decoding needs the `ctc` head (first pass) and the `decoder` (second pass)")
        self.ctc = getattr(ctc, "ctc", ctc)  # (CTCPrefixScorer wraps the head)
        self.decoder = scorers["decoder"]
        self.lm = self.scorers.get("lm")
        self.bias = self.scorers.get("bias")
        if self.lm is not None and not hasattr(self.lm, "att_unit"):
            raise TypeError("lm: an auto_avsr_amd.lm.TransformerLM")
        self.sos, self.eos, self.blank, self.ignore_id = int(sos), int(eos), int(blank), int(ignore_id)
        self.token_list = token_list
        self.n_vocab = self.ctc.ctc_lo.out_features
        if self.bias is not None:  # contextual biasing: this build's trie scorer, nothing else in that slot
            from .bias import ContextBiasScorer

            if not isinstance(self.bias, ContextBiasScorer) or self.bias.n_vocab != self.n_vocab:
                raise TypeError(f"bias: an auto_avsr_amd.bias.ContextBiasScorer over the CTC head's vocabulary ({self.n_vocab})")
        self.ngram, self.len_bonus = None, 0.0
        self.set_ngram(self.scorers.get("ngram"), self.weights.get("ngram", 0.0), len_bonus)
        self.beam_size, self.topk = int(beam_size), min(int(topk), self.n_vocab - 1)
        self.nbest = self.beam_size if nbest is None else int(nbest)
        self.last_first_pass = None  # the first pass' result of the latest call (tools / tests)

    def set_ngram(self, scorer, weight, len_bonus=None):
        """Set, replace or (scorer None or weight 0) remove the n-gram model; len_bonus None keeps the bonus it has.  Takes effect at
        the next call: nothing is cached here."""
        from .ngram import NgramScorer

        weight = float(weight)
        lb = self.len_bonus if len_bonus is None else float(len_bonus)
        if scorer is None or weight == 0.0:
            self.ngram, self.len_bonus = None, lb
            self.scorers.pop("ngram", None)
            self.weights["ngram"] = 0.0
            return
        if not isinstance(scorer, NgramScorer) or scorer.n_vocab != self.n_vocab:
            raise TypeError(f"ngram: an auto_avsr_amd.ngram.NgramScorer over the CTC head's vocabulary ({self.n_vocab})")
        if self.blank != 0 or self.eos != self.n_vocab - 1:
            raise ValueError("ngram: the model's tables need blank == 0 and eos == n_vocab - 1")
        self.ngram, self.len_bonus = scorer, lb
        self.scorers["ngram"] = scorer
        self.weights["ngram"] = weight

    # ------------------------------------------------------------------------------------------------ pieces
    def _posteriors(self, encs):
        dev = encs[0].device
        hlens = torch.tensor([e.shape[0] for e in encs], dtype=torch.int64, device=dev)
        memory = encs[0].unsqueeze(0) if len(encs) == 1 else nets.pad_list(list(encs), 0.0)
        return memory, hlens, self.ctc.log_softmax(memory)

    def first_pass(self, lp, hlens):
        """The n-best prefixes per utterance as label rows padded with ignore_id: (labels int64 [B, N, Lmax], n_valid list)."""
        res = AF.ctc_beam_search(lp, hlens, blank=self.blank, beam=self.beam_size, topk=self.topk, nbest=self.nbest, bias=self.bias,
                                 bias_weight=self.weights.get("bias", 0.0), ngram=self.ngram, ngram_weight=self.weights.get("ngram", 0.0),
                                 len_bonus=self.len_bonus if self.ngram is not None else 0.0)
        self.last_first_pass = res
        Lmax = max(1, int(res["lens"].max()))
        return res["tokens"][:, :, :Lmax].to(torch.int64).contiguous(), res["n_valid"].tolist()

    def _token_sums(self, logits, ys_out):
        """sum over the positions of every row of log softmax(logits)[target] -- csrc/loss.hip's cross-entropy kernel without
        smoothing (ignored targets give 0): logits [R, L, V] f32, ys_out [R, L] -> [R]."""
        R, L, V = logits.shape
        pit = AF._pitched_2d(logits, R * L, V)
        if pit is None:
            pit = (logits.reshape(R * L, V).contiguous(), V)
        nll, _, _ = ops.ce_smooth(pit[0], pit[1], ys_out.reshape(-1).contiguous(), V, 0.0, want_grad=False, ignore_id=self.ignore_id)
        return -nll.view(R, L).sum(1)

    def _bias_sums(self, labels):
        """The bias term of labels [B, N, Lmax] on the host: the gains along each row and of its <eos>."""
        rows = []
        for row in labels.reshape(-1, labels.shape[-1]).tolist():
            g, s = self.bias.walk([t for t in row if t != self.ignore_id])
            rows.append(float(g + self.bias.step(s, self.eos)[0]))
        return torch.tensor(rows, dtype=torch.float32).view(labels.shape[:2]).to(labels.device)

    def _ngram_sums(self, labels):
        """The n-gram term of labels [B, N, Lmax] on the host: the model's f32 walk along each row and its <eos>."""
        rows = [float(self.ngram.walk([t for t in row if t != self.ignore_id] + [self.eos])[0])
                for row in labels.reshape(-1, labels.shape[-1]).tolist()]
        return torch.tensor(rows, dtype=torch.float32).view(labels.shape[:2]).to(labels.device)

    def score_labels(self, memory, hlens, lp, labels, bias_sum=None, ngram_sum=None):
        """The terms of the objective for labels [B, N, Lmax] (padded with ignore_id) of the utterances memory [B, T, D]: a dict of
        [B, N] tensors -- `score` and one entry per scorer of non-zero weight.  bias_sum [B, N]: the bias term where the first pass
        already has it; None: walked on the host.  ngram_sum [B, N]: the same for the n-gram term."""
        B, N, Lmax = labels.shape
        dev = memory.device
        out = {}
        if self.weights.get("ctc", 0.0) != 0.0:
            out["ctc"] = AF.ctc_score(lp, labels, hlens, blank=self.blank, ignore_id=self.ignore_id)
        ys_in, ys_out, mask, _ = ops.prepare_targets(labels.view(B * N, Lmax), self.sos, self.eos, self.ignore_id)
        n_tok = (ys_out != self.ignore_id).sum(1).view(B, N).to(torch.float32)  # len(y) + 1
        if self.weights.get("decoder", 0.0) != 0.0:
            mem = memory if N == 1 else memory.repeat_interleave(N, 0)
            same = bool((hlens == memory.shape[1]).all())
            mem_mask = None if same else nets.non_pad_mask_device(hlens.repeat_interleave(N), memory.shape[1])
            pred, _ = self.decoder(ys_in, mask, mem, mem_mask)
            out["decoder"] = self._token_sums(pred[..., : self.n_vocab], ys_out).view(B, N)
        if self.lm is not None:
            out["lm"] = self._token_sums(self.lm(ys_in)[..., : self.n_vocab], ys_out).view(B, N)
        if self.weights.get("length_bonus", 0.0) != 0.0:
            out["length_bonus"] = n_tok
        if self.bias is not None:
            out["bias"] = self._bias_sums(labels) if bias_sum is None else bias_sum.to(torch.float32)
        if self.ngram is not None:
            out["ngram"] = self._ngram_sums(labels) if ngram_sum is None else ngram_sum.to(torch.float32)
        total = torch.zeros(B, N, dtype=torch.float32, device=dev)
        for k in ("decoder", "lm", "bias", "ngram", "length_bonus", "ctc"):
            if k in out:
                total = total + self.weights[k] * out[k]
        out["score"] = total
        return out

    def _hypotheses(self, labels, terms, b, n):
        hyps = []
        sc = {k: v[b].tolist() for k, v in terms.items()}
        for r in range(n):
            y = [t for t in labels[b, r].tolist() if t != self.ignore_id]
            hyps.append(Hypothesis(yseq=torch.tensor([self.sos] + y + [self.eos], dtype=torch.int64), score=sc["score"][r],
                                   scores={k: v[r] for k, v in sc.items() if k != "score"}, states={}))
        return sorted(hyps, key=lambda h: float(h.score), reverse=True)

    # ------------------------------------------------------------------------------------------------ public
    @torch.no_grad()
    def rescore(self, enc, yseqs):
        """Hypotheses of one utterance (enc [T, D]) for given token sequences -- each with or without its [sos ... eos] frame --
        in the order given (not sorted)."""
        ys = []
        for y in yseqs:
            y = [int(t) for t in (y.tolist() if torch.is_tensor(y) else y)]
            if len(y) >= 2 and y[0] == self.sos and y[-1] == self.eos:
                y = y[1:-1]
            ys.append(y)
        Lmax = max(1, max(len(y) for y in ys))
        labels = torch.full((1, len(ys), Lmax), self.ignore_id, dtype=torch.int64)
        for i, y in enumerate(ys):
            labels[0, i, : len(y)] = torch.tensor(y, dtype=torch.int64)
        labels = labels.to(enc.device)
        memory, hlens, lp = self._posteriors([enc])
        terms = self.score_labels(memory, hlens, lp, labels)
        sc = {k: v[0].tolist() for k, v in terms.items()}
        return [Hypothesis(yseq=torch.tensor([self.sos] + y + [self.eos], dtype=torch.int64), score=sc["score"][i],
                           scores={k: v[i] for k, v in sc.items() if k != "score"}, states={}) for i, y in enumerate(ys)]

    @torch.no_grad()
    def forward_many(self, xs, workers=None, maxlenratio=0.0, minlenratio=0.0) -> List[List[Hypothesis]]:
        """Encoder outputs (T_i, D) of several utterances -> their sorted hypotheses: ONE first-pass launch over the padded batch,
        ONE decoder (+ LM) pass over all B * N hypotheses.  (workers / maxlenratio / minlenratio: BatchBeamSearch's signature;
        there is nothing for them to control here.)"""
        xs = list(xs)
        if not xs:
            return []
        memory, hlens, lp = self._posteriors(xs)
        labels, n_valid = self.first_pass(lp, hlens)
        terms = self.score_labels(memory, hlens, lp, labels, bias_sum=self.last_first_pass["bias_sum"] if self.bias is not None else None,
                                  ngram_sum=self.last_first_pass["ngram_sum"] if self.ngram is not None else None)
        labels = labels.cpu()
        terms = {k: v.cpu() for k, v in terms.items()}
        return [self._hypotheses(labels, terms, b, max(1, int(n_valid[b]))) for b in range(len(xs))]

    def __call__(self, x, maxlenratio=0.0, minlenratio=0.0) -> List[Hypothesis]:
        """x: encoder output of one utterance (T, D).  Returns the rescored n-best, best first."""
        return self.forward_many([x])[0]

    forward = __call__
