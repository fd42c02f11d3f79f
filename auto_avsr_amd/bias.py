"""Contextual biasing (phrase boosting, "hot words") as a scorer of the beam search: `ContextBiasScorer(phrases, n_vocab)` in the
`bias` slot of `scorers`, weight `weights["bias"]` in log units per matched token.

Semantics.  The phrases (non-empty token-id sequences, every id in [1, n_vocab - 2]: neither blank 0 nor <sos> = <eos> =
n_vocab - 1; duplicates collapse) form a trie, node 0 the root; a node where a phrase ends is an END node.  unc(s), the
uncommitted part of a match, is the number of edges from s up to its nearest end ancestor-or-self, or up to the root if there is
none.  A hypothesis carries one node s (the root after <sos>); extending it by token v gains g(s, v) and moves to a next node:

  1. s has a child c on v: g = +1, next = c;
  2. otherwise g = -unc(s) -- the reward of the abandoned partial match is taken back -- and the match restarts from the root:
     if the root has a child c on v, g += 1 and next = c, else next = root;
  3. a next node that is an end node without children becomes the root (its reward stays).

<eos> is never in the trie, so a finished hypothesis keeps rewards only for phrases (or end-node prefixes of longer phrases) it
completed.  There are NO failure links: after a mismatch only the current token is retried from the root, a suffix of the abandoned
match that is itself a prefix of a phrase is not picked up.  The scorer's score for v is g(s, v); `Hypothesis.scores["bias"]` is the
running sum of g, a small integer, exact in f32.

It is a full scorer (it enters the weighted sum before the partial scorers) but never the pre-beam key: a boosted token still has
to be among the `pre_beam_size` candidates of the pre-beam scorer to be extended at all.

The flattened trie (int32: CSR `first` [n_nodes + 1], `tok` [n_edges] ascending within a node, `child` [n_edges] with rule 3
folded in, `unc` [n_nodes]) is what csrc/decode.hip reads (avsr_beam_set_bias, avsr_bias_score); `batch_score` below is the host
form for the python-issued step and for any foreign search."""
import numpy as np
import torch

from .scorer_interface import BatchScorerInterface


class ContextBiasScorer(BatchScorerInterface):
    def __init__(self, phrases, n_vocab: int):
        self.n_vocab = int(n_vocab)
        self.version = 0
        self._dev = {}
        self.set_phrases(phrases)

    # ------------------------------------------------------------------------------------------------ the trie
    def set_phrases(self, phrases):
        """Replace the list (an empty one is legal and scores 0 everywhere).  Bumps `version`, which is what makes a native
        session take the new tables at its next utterance."""
        V = self.n_vocab
        kids, end = [{}], [False]  # per node: {token: child}, phrase ends here
        norm = []
        for ph in phrases or []:
            ph = [int(t) for t in ph]
            if not ph:
                raise ValueError("bias phrase: empty")
            if any(t < 1 or t > V - 2 for t in ph):
                raise ValueError(f"bias phrase {ph}: token ids must lie in [1, {V - 2}] (not blank 0, not <sos>/<eos> {V - 1})")
            norm.append(tuple(ph))
        for ph in norm:
            s = 0
            for t in ph:
                c = kids[s].get(t)
                if c is None:
                    c = len(kids)
                    kids[s][t] = c
                    kids.append({})
                    end.append(False)
                s = c
            end[s] = True
        n = len(kids)
        unc = np.zeros(n, dtype=np.int32)
        first = np.zeros(n + 1, dtype=np.int32)
        tok, child = [], []
        order = [0]  # parents before children
        for s in order:
            order.extend(kids[s].values())
        for s in order:
            for c in kids[s].values():
                unc[c] = 0 if end[c] else unc[s] + 1
        for s in range(n):
            for t in sorted(kids[s]):
                c = kids[s][t]
                tok.append(t)
                child.append(0 if (end[c] and not kids[c]) else c)  # rule 3
            first[s + 1] = len(tok)
        self.phrases = sorted(set(norm))
        self.first, self.unc = first, unc
        self.tok, self.child = np.asarray(tok, dtype=np.int32), np.asarray(child, dtype=np.int32)
        self.n_nodes, self.n_edges = n, len(tok)
        self._next = [{t: (0 if (end[c] and not kids[c]) else c) for t, c in k.items()} for k in kids]
        self.version += 1
        self._dev = {}
        return self

    def step(self, s: int, v: int):
        """(gain, next node) of extending a hypothesis at node s by token v."""
        c = self._next[s].get(v)
        if c is not None:
            return 1, c
        g = -int(self.unc[s])
        c = self._next[0].get(v) if s != 0 else None
        return (g, 0) if c is None else (g + 1, c)

    def walk(self, tokens):
        """(running sum of gains, node) after the tokens (without the leading <sos>) from the root."""
        total, s = 0, 0
        for v in tokens:
            g, s = self.step(s, int(v))
            total += g
        return total, s

    def device_tables(self, device):
        """(first, tok, child, unc) as int32 tensors on `device`, uploaded once per list and device (tables of length 0 are padded to
        one element so that they have an address)."""
        key = str(device)
        got = self._dev.get(key)
        if got is None:
            pad = lambda a: torch.from_numpy(a if a.size else np.zeros(1, dtype=np.int32)).to(device)  # noqa: E731
            got = self._dev[key] = (pad(self.first), pad(self.tok), pad(self.child), pad(self.unc))
        return got

    # ------------------------------------------------------------------------------------------------ scorer API
    def _row(self, s: int):
        row = np.full(self.n_vocab, float(-int(self.unc[s])), dtype=np.float32)
        if s != 0:
            row[self.tok[self.first[0]: self.first[1]]] += 1.0
        row[self.tok[self.first[s]: self.first[s + 1]]] = 1.0
        return row

    def init_state(self, x):
        return None

    def batch_init_state(self, x):
        return None

    def score(self, y, state, x):
        """The reference's single-hypothesis contract: state = the node of y[:-1] (None: the prefix is walked from the root)."""
        y = y.tolist()
        s = self.walk(y[1:])[1] if state is None else self.step(int(state), y[-1])[1]
        row = torch.from_numpy(self._row(s))
        return (row if x is None else row.to(x.device)), s

    def batch_score(self, ys, states, xs):
        """Dense gains [n, n_vocab] of every next token and the state = the node the WHOLE prefix ys[b] reaches, so that a search
        which selects states by parent index gets the parent's node.  Two state contracts, told apart by the elements' type: this
        build's BatchBeamSearch passes back [nodes [n]] (one batched tensor), the reference's a list of per-hypothesis states (None
        before the first token, else the int `select_state` took out of the previous result)."""
        n = ys.shape[0]
        rows = ys.tolist()
        batched = states is not None and len(states) == 1 and torch.is_tensor(states[0]) and states[0].dim() == 1
        if states is None or (not batched and states[0] is None):
            nodes = [self.walk(r[1:])[1] for r in rows]
        else:
            prev = states[0].tolist() if batched else [int(s) for s in states]
            nodes = [self.step(prev[b], rows[b][-1])[1] for b in range(n)]
        dev = ys.device
        gains = torch.from_numpy(np.stack([self._row(s) for s in nodes])).to(dev)
        if batched or states is None:
            return gains, [torch.tensor(nodes, dtype=torch.int64, device=dev)]
        return gains, nodes
