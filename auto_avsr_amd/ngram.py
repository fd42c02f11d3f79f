"""Back-off n-gram language model (ARPA) as a PARTIAL scorer of the beam search: `NgramScorer` in the `ngram` slot of `scorers`,
weight `weights["ngram"]` (ESPnet's scorers["ngram"] / ngram_weight: the model scores the pre-beam candidates only).

Model.  P maps an n-gram (a tuple of token ids) to its log-probability, B an n-gram of order < N to its back-off weight, both natural
logarithms in f32.  </s> is the search's <eos> (n_vocab - 1) as a predicted token, <s> exists only as context and has the pseudo id
n_vocab.  The definition every lookup is held to is plain ARPA back-off:

    p(v | h) = P[h + v]                          if that entry exists,
             = B.get(h, 0) + p(v | h[1:])        otherwise,           h = the last N - 1 tokens of <s> + prefix.

Closure, checked when a model is set (ValueError): every n-gram's prefix (the n-gram without its last word) is present one order
lower; </s> has a unigram; a token id in [1, n_vocab - 2] without a unigram takes <unk>'s log-probability (back-off 0), and without
an <unk> that is an error.  So the recursion always ends at a unigram.

Flattened form (what csrc/decode.hip reads: avsr_beam_set_ngram, avsr_ngram_score).  A node is a context = an n-gram of order < N,
node 0 the empty one, nodes ordered by (order, tokens).  CSR `first` [n_nodes + 1]; `tok` [n_edges] ascending within a node; `logp`
[n_edges] f32; `next` [n_edges] = node of the longest suffix of (context + token), cut to N - 1 tokens, that is a node; `bow`
[n_nodes] f32; `back` [n_nodes] = node of the longest PROPER suffix of the context that is a node (0 if none).  Contexts that are no
nodes carry back-off 0 and no entries, so skipping them is exact.  Entries that predict <s> are never looked up and are left out, so
the root's edges are exactly the tokens 1 .. n_vocab - 1 in order.

Lookup of token v at node s, the order of the f32 additions fixed: walk s, back[s], ... until a node has an edge e on v (the root
always has one); if the first node has it the result is logp[e], otherwise r = bow[s0]; r += bow[s1]; ...; r += logp[e].  The next
node is next[e].  The blank (id 0) scores 0 and keeps the node.  The host lookups below run in numpy f32 in that order, so that
`Hypothesis.scores["ngram"]` of the python-issued step equals the device's bit for bit."""
import math
import re

import numpy as np
import torch

from .scorer_interface import BatchPartialScorerInterface

_SPECIAL = ("<s>", "</s>", "<unk>")


def read_arpa(path):
    """(order, {n-gram of words: (log10 p, log10 back-off or None)}) of an ARPA text file: the \\data\\ counts, the \\N-grams:
    sections, \\end\\.  The order is the highest one the header declares (its section may be empty)."""
    order, grams, sec, seen_data = 0, {}, None, False
    with open(path, encoding="utf8") as f:
        for raw in f:
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                seen_data, sec = True, 0
                continue
            if line == "\\end\\":
                break
            m = re.fullmatch(r"\\(\d+)-grams:", line)
            if m:
                sec = int(m.group(1))
                order = max(order, sec)
                continue
            if sec == 0:
                m = re.fullmatch(r"ngram\s+(\d+)\s*=\s*(\d+)", line)
                if m:
                    order = max(order, int(m.group(1)))
                continue
            if sec is None:
                continue  # (text before \data\)
            parts = line.split()
            if len(parts) not in (sec + 1, sec + 2):
                raise ValueError(f"{path}: bad line in the {sec}-grams: {line!r}")
            words = tuple(parts[1: 1 + sec])
            grams[words] = (float(parts[0]), float(parts[sec + 1]) if len(parts) == sec + 2 else None)
    if not seen_data or order < 1:
        raise ValueError(f"{path}: not an ARPA file (no \\data\\ section)")
    return order, grams


class NgramScorer(BatchPartialScorerInterface):
    def __init__(self, n_vocab: int, probs, backoffs=None, order=None, unk_logp=None):
        """probs {tuple of ids: ln p}, backoffs {tuple of ids: ln back-off}; <s> = n_vocab, </s> = n_vocab - 1; order: N (default the
        longest n-gram); unk_logp: ln p(<unk>) for tokens without a unigram, None = the model has no <unk>."""
        self.n_vocab = int(n_vocab)
        self.blank = 0
        self.version = 0
        self._dev = {}
        self.set_model(probs, backoffs, order, unk_logp)

    @classmethod
    def from_arpa(cls, path, token_list):
        """Words map to ids through `token_list` (piece string -> index); if every word other than <s>, </s>, <unk> is a decimal
        integer the words ARE token ids.  log10 -> ln once: np.float32(x * ln 10)."""
        V = len(token_list)
        order, grams = read_arpa(path)
        words = {w for g in grams for w in g if w not in _SPECIAL}
        ids = all(re.fullmatch(r"\d+", w) for w in words)
        index = {} if ids else {p: i for i, p in enumerate(token_list)}
        ln10 = math.log(10.0)

        def wid(w):
            if w == "<s>":
                return V
            if w == "</s>":
                return V - 1
            if w == "<unk>":
                return index.get(w)  # (a piece of the token list, or a word no hypothesis can hold)
            if ids:
                return int(w)
            if w not in index:
                raise ValueError(f"{path}: word {w!r} is not in the token list")
            return index[w]

        probs, backoffs, unk = {}, {}, None
        for g, (p, b) in grams.items():
            if g == ("<unk>",):
                unk = np.float32(p * ln10)
            key = tuple(wid(w) for w in g)
            if any(t is None for t in key):
                continue
            probs[key] = np.float32(p * ln10)
            if b is not None:
                backoffs[key] = np.float32(b * ln10)
        return cls(V, probs, backoffs, order=order, unk_logp=unk)

    # ------------------------------------------------------------------------------------------------ the tables
    def set_model(self, probs, backoffs=None, order=None, unk_logp=None):
        """Replace the model.  Bumps `version`, which is what makes a native session take the new tables at its next utterance."""
        V = self.n_vocab
        P = {tuple(int(t) for t in k): np.float32(v) for k, v in probs.items()}
        B = {tuple(int(t) for t in k): np.float32(v) for k, v in (backoffs or {}).items()}
        N = int(order) if order is not None else max([len(k) for k in P] + [1])
        if not 1 <= N <= 16:
            raise ValueError(f"n-gram order {N}: the device lookup walks at most 16 back-off levels (AVSR_NGRAM_MAX_ORDER)")
        for k in P:
            if not 1 <= len(k) <= N:
                raise ValueError(f"n-gram {k}: order outside [1, {N}]")
            if any(t < 1 or t > V for t in k):
                raise ValueError(f"n-gram {k}: token ids must lie in [1, {V - 1}] (</s> = {V - 1}; <s> = {V} as context)")
            if len(k) > 1 and k[:-1] not in P:
                raise ValueError(f"n-gram {k}: its prefix {k[:-1]} is missing from the {len(k) - 1}-grams")
        if (V - 1,) not in P:
            raise ValueError("the model has no unigram for </s>")
        real = set(P)  # (the fill-ins below are entries of the root only: contexts that are no nodes)
        for t in range(1, V - 1):
            if (t,) not in P:
                if unk_logp is None:
                    raise ValueError(f"token {t} has no unigram and the model has no <unk>")
                P[(t,)] = np.float32(unk_logp)
        ctxs = sorted((k for k in real if len(k) < N), key=lambda k: (len(k), k))
        node = {(): 0}
        for k in ctxs:
            node[k] = len(node)
        n = len(node)

        def suffix_node(k):  # node of the longest suffix of k that is a node
            for i in range(len(k) + 1):
                s = node.get(k[i:])
                if s is not None:
                    return s
            return 0

        bow, back = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32)
        for k, s in node.items():
            bow[s] = B.get(k, np.float32(0.0))
            back[s] = suffix_node(k[1:]) if k else 0
        rows = [[] for _ in range(n)]
        for k, p in P.items():
            if k[-1] == V:  # predicts <s>: never looked up
                continue
            s = node.get(k[:-1])
            if s is None:  # (order-N entry whose context has no entry of its own: excluded by the prefix check)
                raise ValueError(f"n-gram {k}: its prefix is missing")
            rows[s].append((k[-1], p, suffix_node(k[-(N - 1):] if N > 1 else ())))
        first = np.zeros(n + 1, dtype=np.int32)
        tok, logp, nxt = [], [], []
        for s, row in enumerate(rows):
            row.sort()
            tok += [r[0] for r in row]
            logp += [r[1] for r in row]
            nxt += [r[2] for r in row]
            first[s + 1] = len(tok)
        self.order, self.n_nodes, self.n_edges = N, n, len(tok)
        self.first, self.bow, self.back = first, bow, back
        self.tok, self.logp, self.next = np.asarray(tok, dtype=np.int32), np.asarray(logp, dtype=np.float32), np.asarray(nxt, dtype=np.int32)
        self.contexts = [()] + ctxs  # node -> its n-gram
        self.start_node = node.get((V,), 0)
        # edge (s, v) <-> key s * (V + 1) + v: ascending over the whole edge list, one searchsorted finds any edge
        self._keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(first)) * (V + 1) + self.tok
        self.version += 1
        self._dev = {}
        return self

    def device_tables(self, device):
        """(first, tok, logp, next, bow, back) on `device`, uploaded once per model and device."""
        key = str(device)
        got = self._dev.get(key)
        if got is None:
            got = self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.first, self.tok, self.logp, self.next, self.bow, self.back))
        return got

    # ------------------------------------------------------------------------------------------------ lookups (numpy f32)
    def lookup(self, nodes, toks):
        """(log-probabilities f32, next nodes) of extending hypotheses at `nodes` by `toks` (arrays of one shape)."""
        nodes, toks = np.asarray(nodes, dtype=np.int64), np.asarray(toks, dtype=np.int64)
        shape = nodes.shape
        s, v = nodes.reshape(-1).copy(), toks.reshape(-1)
        res, nxt = np.zeros(s.size, dtype=np.float32), s.copy()
        acc, fresh = np.zeros(s.size, dtype=np.float32), np.ones(s.size, dtype=bool)
        todo = v != self.blank
        for _ in range(self.order):
            if not todo.any():
                break
            idx = np.nonzero(todo)[0]
            key = s[idx] * (self.n_vocab + 1) + v[idx]
            e = np.minimum(np.searchsorted(self._keys, key), self.n_edges - 1)
            hit = self._keys[e] == key
            h, m = idx[hit], idx[~hit]
            lp = self.logp[e[hit]]
            res[h] = np.where(fresh[h], lp, acc[h] + lp)  # f32 + f32
            nxt[h] = self.next[e[hit]]
            acc[m] = np.where(fresh[m], self.bow[s[m]], acc[m] + self.bow[s[m]])
            fresh[m] = False
            if (s[m] == 0).any():
                raise ValueError("n-gram lookup: a token without a unigram (ids must lie in [0, n_vocab - 1])")
            s[m] = self.back[s[m]]
            todo[h] = False
        return res.reshape(shape), nxt.reshape(shape)

    def step(self, s: int, v: int):
        """(log-probability f32, next node) of extending a hypothesis at node s by token v."""
        r, nx = self.lookup([s], [v])
        return r[0], int(nx[0])

    def walk(self, tokens):
        """(running f32 sum, node) after the tokens (without the leading <sos>) from the start node."""
        total, s = np.float32(0.0), self.start_node
        for v in tokens:
            r, s = self.step(s, int(v))
            total = np.float32(total + r)
        return total, s

    # ------------------------------------------------------------------------------------------------ scorer API
    def init_state(self, x):
        return None

    def batch_init_state(self, x):
        return None

    def _node_of(self, state, y):
        return self.walk(y[1:])[1] if state is None else int(state)

    def score_partial(self, y, next_tokens, state, x):
        """The reference's single-hypothesis contract: state = the node of y (None: the prefix is walked from the start node)."""
        s = self._node_of(state, y.tolist())
        ids = next_tokens.tolist()
        r, _ = self.lookup([s] * len(ids), ids)
        out = torch.from_numpy(r)
        return (out if x is None else out.to(x.device)), s

    def select_state(self, state, i, new_id=None):
        """Per-hypothesis contracts: of a list of nodes hypothesis i's (moved along new_id when given); of one node (score_partial's
        state) the node reached on token i."""
        if state is None:
            return None
        if isinstance(state, (list, tuple)):
            s = state[i]
            return s if new_id is None or s is None else self.step(int(s), int(new_id))[1]
        return self.step(int(state), int(i))[1]

    def batch_score_partial(self, ys, part_ids, states, x=None):
        """[n, n_vocab] f32: the lookup value at the candidates `part_ids` [n, S] and at the <eos> column whether or not the pre-beam
        kept it (CTCPrefixScorer gives <eos> its full score outside the candidates too), 0 elsewhere.  The state is the node the
        prefix ys[b] stands at.  Two contracts, told apart by the elements' type: this build's BatchBeamSearch passes [nodes [n]] (one
        batched tensor; None before the first token) and moves it with `select_states`; the reference's a list of per-hypothesis
        nodes (None before the first token) it moves with `select_state(state, i, new_id)`."""
        n = ys.shape[0]
        batched = states is not None and len(states) == 1 and torch.is_tensor(states[0]) and states[0].dim() == 1
        if batched:
            nodes = states[0].tolist()
        else:
            rows = ys.tolist()
            nodes = [self._node_of(None if states is None else states[b], rows[b]) for b in range(n)]
        ids = part_ids.detach().cpu().numpy().astype(np.int64)
        eos = np.full((n, 1), self.n_vocab - 1, dtype=np.int64)
        cols = np.concatenate([ids, eos], 1)
        r, _ = self.lookup(np.repeat(np.asarray(nodes, dtype=np.int64)[:, None], cols.shape[1], 1), cols)
        out = np.zeros((n, self.n_vocab), dtype=np.float32)
        np.put_along_axis(out, cols, r, 1)
        out[:, self.blank] = 0.0
        dev = ys.device
        scores = torch.from_numpy(out).to(dev)
        if batched or states is None:
            return scores, [torch.tensor(nodes, dtype=torch.int64, device=dev)]
        return scores, nodes

    def select_states(self, state, prev, tok):
        """This build's contract: nodes of the new beam, hypothesis prev[j] extended by tok[j]."""
        nodes = state[0][prev].tolist()
        _, nx = self.lookup(nodes, tok.tolist())
        return [torch.as_tensor(nx, dtype=torch.int64, device=state[0].device)]

    @staticmethod
    def keep_states(state, keep):
        return None if state is None else [state[0][keep]]
