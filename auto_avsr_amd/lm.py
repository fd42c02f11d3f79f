"""Transformer language model for shallow fusion in the beam search (the `scorers["lm"]` / `weights["lm"]` slot of the
reference's `get_beam_search_decoder`, lightning.py:126-158).

The reference ships no LM class; architecture and ``state_dict`` keys are those of ESPnet's
``espnet.nets.pytorch_backend.lm.transformer.TransformerLM`` (pre-norm), the format the LM checkpoints of this model family
were released in:

    embed.weight [V][E]
    encoder.embed.0 Linear E -> D, encoder.embed.1 LayerNorm (eps 1e-12), Dropout, ReLU, PositionalEncoding (x * sqrt(D) + pe)
    encoder.encoders.i: norm1, self_attn.linear_{q,k,v,out}, norm2, feed_forward.w_{1,2}
                        x += attn(LN1(x)) under the causal mask;  x += W2 relu(W1 LN2(x))
    encoder.after_norm
    decoder Linear D -> V, log_softmax

Inference only.  Three ways in:
  * ``forward(ys)``: teacher-forced next-token log-probabilities [B][L][V] (the kernels of the decoder's training path);
  * the scorer API (``score`` / ``batch_score`` / ``forward_one_step``) with a per-hypothesis K / V cache: a step projects ONE
    position per hypothesis and attends to the cached keys / values (csrc/decode.hip: avsr_decode_attention) -- the python-issued
    step of decoding.BatchBeamSearch;
  * inside the one-call-per-step search (decode_native.NativeBeam binds the weights to `avsr_beam_attach_lm`)."""
import json

import torch
from torch import nn

from . import functional as AF
from . import ops
from .nets import LayerNorm, MultiHeadedAttention, PositionalEncoding, PositionwiseFeedForward, subsequent_mask
from .scorer_interface import BatchScorerInterface


class _LMEncoderLayer(nn.Module):
    """encoder_layer.py (pre-norm, no concat): parameters only, the arithmetic is issued by TransformerLM."""

    def __init__(self, size, heads, units):
        super().__init__()
        self.self_attn = MultiHeadedAttention(heads, size, 0.0)
        self.feed_forward = PositionwiseFeedForward(size, units, 0.0)
        self.norm1 = LayerNorm(size)
        self.norm2 = LayerNorm(size)


class _LMEncoder(nn.Module):
    def __init__(self, idim, size, heads, units, layers):
        super().__init__()
        self.embed = nn.Sequential(nn.Linear(idim, size), LayerNorm(size), nn.Dropout(0.0), nn.ReLU(), PositionalEncoding(size, 0.0))
        self.encoders = nn.ModuleList(_LMEncoderLayer(size, heads, units) for _ in range(layers))
        self.after_norm = LayerNorm(size)


class TransformerLM(BatchScorerInterface, nn.Module):
    def __init__(self, n_vocab, *, embed_unit=128, att_unit=512, head=8, unit=2048, layer=16):
        super().__init__()
        if att_unit % head:
            raise ValueError("att_unit must be a multiple of head")
        self.n_vocab, self.embed_unit, self.att_unit, self.head, self.unit, self.layer = n_vocab, embed_unit, att_unit, head, unit, layer
        self.embed = nn.Embedding(n_vocab, embed_unit)
        self.encoder = _LMEncoder(embed_unit, att_unit, head, unit, layer)
        self.decoder = nn.Linear(att_unit, n_vocab)
        self._derived = None
        self.eval()

    # ------------------------------------------------------------------------------------------------ loading
    @classmethod
    def from_files(cls, n_vocab, path, conf=None, device=None):
        """path: a state dict saved with torch.save (optionally under ESPnet's `predictor.` prefix); conf: a dict or the path of a
        JSON file with layer / unit / att_unit / head / embed_unit (ESPnet's rnnlm_conf; other entries are ignored)."""
        if isinstance(conf, str):
            with open(conf, encoding="utf8") as f:
                conf = json.load(f)
        conf = dict(conf or {})
        names = {"layer": "layer", "unit": "unit", "att_unit": "att_unit", "att-unit": "att_unit", "head": "head",
                 "embed_unit": "embed_unit", "embed-unit": "embed_unit"}
        kw = {names[k]: int(v) for k, v in conf.items() if k in names and v is not None}
        lm = cls(n_vocab, **kw)
        sd = torch.load(path, map_location="cpu")
        if isinstance(sd.get("model"), dict):  # (a trainer snapshot: the weights sit under "model")
            sd = sd["model"]
        lm.load_state_dict(sd)
        return lm.to(device) if device is not None else lm

    def load_state_dict(self, state_dict, strict=True):
        sd = {(k[len("predictor."):] if k.startswith("predictor.") else k): v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("TransformerLM is inference-only (training a language model is outside this build)")
        return super().train(False)

    # ------------------------------------------------------------------------------------------------ derived weights
    def derived(self):
        """Tensors computed from the parameters, rebuilt when a parameter changes: the input table [V][D] = embed followed by
        encoder.embed.0 (a token's input row is a gather, not a contraction) and the stacked Q / K / V projections per layer."""
        params = list(self.parameters())
        key = (AF.weight_generation(),) + tuple((p.data_ptr(), p._version) for p in params)
        if self._derived is None or self._derived[0] != key:
            lin = self.encoder.embed[0]
            with torch.no_grad(), AF.precise():
                table = AF.linear(self.embed.weight.detach().float(), lin.weight, lin.bias, out_dtype=torch.float32).contiguous()
                qkv = []
                for e in self.encoder.encoders:
                    sa = e.self_attn
                    qkv.append((torch.cat([sa.linear_q.weight, sa.linear_k.weight, sa.linear_v.weight], 0).detach().float().contiguous(),
                                torch.cat([sa.linear_q.bias, sa.linear_k.bias, sa.linear_v.bias], 0).detach().float().contiguous()))
            self._derived = (key, table, qkv)
        return self._derived

    def _input(self, ys, first_pos):
        """ys [B][L] tokens at positions first_pos .. first_pos + L - 1 -> [B][L][D] f32."""
        _, table, _ = self.derived()
        ln, pos = self.encoder.embed[1], self.encoder.embed[4]
        x = AF.layer_norm(table[ys], ln.weight, ln.bias, ln.eps)
        pe = pos.table(first_pos + ys.shape[1], ys.device)[first_pos:]
        return torch.relu(x).mul_(pos.xscale).add_(pe)

    def _head(self, x):
        an = self.encoder.after_norm
        y = AF.layer_norm(x, an.weight, an.bias, an.eps)
        y = AF.linear(y, self.decoder.weight, self.decoder.bias, out_dtype=torch.float32, pad_out=True)
        return AF.log_softmax(y)

    # ------------------------------------------------------------------------------------------------ teacher-forced pass
    @torch.no_grad()
    def forward(self, ys):
        """ys [B][L] int64 -> log p(next token | ys[:, :t + 1]) for every t: [B][L][V] f32."""
        x = self._input(ys, 0)
        mask = subsequent_mask(ys.shape[1], device=ys.device).unsqueeze(0).expand(ys.shape[0], -1, -1)
        for e in self.encoder.encoders:
            sa, ff = e.self_attn, e.feed_forward
            x = AF.mha_sublayer(x, None, None, mask, e.norm1.weight, e.norm1.bias, *sa._params(), None, None, None, sa.h, 0.0, 0.0,
                                e.norm1.eps)
            x = AF.ffn_sublayer(x, e.norm2.weight, e.norm2.bias, ff.w_1.weight, ff.w_1.bias, ff.w_2.weight, ff.w_2.bias, 1.0, 0.0,
                                e.norm2.eps)
        return self._head(x)

    # ------------------------------------------------------------------------------------------------ incremental pass
    @torch.no_grad()
    def forward_one_step(self, tgt, tgt_mask=None, memory=None, memory_mask=None, cache=None):
        """Log-probabilities of the token after tgt [n][L] + the new cache.  cache: per layer the keys | values [n][L - 1][2 D] of
        the positions already scored (None: everything is computed here, position by position).  The signature is the decoder's
        (transformer_decoder.py:226-258), which is what decoding.BatchBeamSearch calls on a full scorer that has it; mask and
        memory are not used (one query row sees every cached position)."""
        n, L = tgt.shape
        if cache is None or cache[0] is None:
            cache = [None] * self.layer
            for t in range(1, L):  # a prefix without a state (not what a search does: it starts from <sos>)
                _, cache = self._one_position(tgt[:, :t], cache)
        assert all(c is None for c in cache) if L == 1 else cache[0].shape[:2] == (n, L - 1)
        return self._one_position(tgt, cache)

    def _one_position(self, tgt, cache):
        n, L = tgt.shape
        D, H = self.att_unit, self.head
        if D != 64 * H:
            raise NotImplementedError("the cached step runs on csrc/decode.hip's attention: heads of 64 (att_unit = 64 * head)")
        _, _, qkv_w = self.derived()
        x = self._input(tgt[:, -1:], L - 1).reshape(n, D)
        new_cache = []
        anc = torch.empty(n * L, dtype=torch.int32, device=tgt.device)
        for e, (wqkv, bqkv), c in zip(self.encoder.encoders, qkv_w, cache):
            ff = e.feed_forward
            h = AF.layer_norm(x, e.norm1.weight, e.norm1.bias, e.norm1.eps)
            qkv = AF.linear(h, wqkv, bqkv, out_dtype=torch.float32)
            kv = qkv[:, D:].unsqueeze(1)
            c = (kv if c is None else torch.cat([c, kv], 1)).contiguous()
            q = qkv[:, :D].contiguous()
            att = torch.empty(n, D, dtype=torch.float32, device=tgt.device)
            ops.call("avsr_decode_attention", ops._ptr(q), D, ops._ptr(c), L * 2 * D, 2 * D, 0, D, n, H, L, ops._ptr(att), D, ops._ptr(anc),
                     ops._stream(q))
            x = x + AF.linear(att, e.self_attn.linear_out.weight, e.self_attn.linear_out.bias, out_dtype=torch.float32)
            x = AF.ffn_sublayer(x.unsqueeze(1), e.norm2.weight, e.norm2.bias, ff.w_1.weight, ff.w_1.bias, ff.w_2.weight, ff.w_2.bias, 1.0,
                                0.0, e.norm2.eps).reshape(n, D)
            new_cache.append(c)
        return self._head(x), new_cache

    # ------------------------------------------------------------------------------------------------ scorer API
    def score(self, y, state, x):
        logp, state = self.forward_one_step(y.unsqueeze(0), cache=None if state is None else [c.unsqueeze(0) for c in state])
        return logp.squeeze(0), [c.squeeze(0) for c in state]

    def batch_score(self, ys, states, xs):
        """The reference's contract (scorer_interface.py:82-125): `states` is a list with one state per hypothesis (None before
        the first token, else the per-layer [L - 1][2 D] caches `select_state` took out of the previous result)."""
        n = len(ys)
        if states is None or states[0] is None:
            batch = None
        elif torch.is_tensor(states[0]):  # already batched per layer
            batch = list(states)
        else:
            batch = [torch.stack([states[b][i] for b in range(n)]) for i in range(self.layer)]
        logp, new = self.forward_one_step(ys, cache=batch)
        return logp, [[new[i][b] for i in range(self.layer)] for b in range(n)]

    def native_ok(self, odim):
        """What csrc/decode.hip's session takes (avsr_beam_attach_lm): heads of 64, block sizes its linear kernel instantiates."""
        from .decode_native import skinny_len_ok

        D, H, FF = self.att_unit, self.head, self.unit
        return self.n_vocab == odim and D == 64 * H and skinny_len_ok(D, False) and skinny_len_ok(FF, True)
