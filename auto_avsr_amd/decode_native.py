"""Host side of csrc/decode.hip: the hybrid CTC / attention beam search with ONE library call per decoding step.

`NativeBeam.search` is what `decoding.BatchBeamSearch.forward` runs when the scorers are the ones the reference wires
(lightning.py:126-158: this build's TransformerDecoder, CTCPrefixScorer, optionally LengthBonus, pre-beam on the decoder
scores): same search (batch_beam_search.py:208-349 over beam_search.py:330-457), same hypotheses, with the per-step work --
decoder pass on the new position over cached K / V, pre-beam, CTC prefix scores, top-k, beam re-ordering -- issued from C++
(`avsr_beam_step_batch`) instead of ~120 python-issued launches.  There is ONE host loop, `NativeBeam.search_group`, for a group
of U utterances whose running hypotheses share every step; `search` is the group of one.  The loop only looks at the 1 KB per
utterance the step copies back (tokens, parents, scores), collects ended hypotheses and applies the end-detection rule.  Any
other scorer configuration keeps the python step of decoding.py."""
import collections
import contextlib
import ctypes
import math
import threading

import numpy as np
import torch

from . import _lib, ops

MAX_BEAM = 128
MAX_GROUP, MAX_GROUP_ROWS = 32, 1024  # csrc/decode.hip: utterances of a group, packed rows (U * beam) of a group


def search_maxlen(T, maxlenratio):
    """Steps a search of a T-frame utterance takes at the most (beam_search.py:349-354)."""
    if maxlenratio == 0:
        return T
    if maxlenratio < 0:
        return -1 * int(maxlenratio)
    return max(1, int(maxlenratio * T))


# A scorer whose device tables a session takes (NativeBeam._bind_tables): the dict of the search that holds it, the entry point that
# binds its tables, cfg of a scorer as that entry point reads it (fcfg is the weight alone), the cfg that detaches, the number of tables
_TableScorer = collections.namedtuple("_TableScorer", "scorers entry cfg cfg_detached n_tables")
_TABLE_SCORERS = {
    "bias": _TableScorer("full_scorers", "avsr_beam_set_bias", lambda sc: (sc.n_nodes if sc.n_edges else 0, sc.n_edges), (0, 0), 4),
    "ngram": _TableScorer("part_scorers", "avsr_beam_set_ngram", lambda sc: (sc.n_nodes, sc.n_edges, sc.start_node), (0, 0, 0), 6),
}


def skinny_len_ok(K, sliced_ok):
    """Contraction lengths the linear kernel of a decoding step takes (csrc/decode.hip skinny_slices): K = 64 * nw * Z with nw an
    instantiated block size (waves of 64 columns of K) and, where the call site allows K slices, Z <= 8."""
    def block_ok(nw):
        return 1 <= nw <= 12 and (nw <= 4 or nw % 2 == 0)

    return K >= 64 and K % 64 == 0 and any(K % (64 * z) == 0 and block_ok(K // (64 * z)) for z in range(1, 9 if sliced_ok else 2))


def _f32(t):
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


class NativeBeam:
    """One session object per BatchBeamSearch: weights are re-bound when any decoder parameter changes."""

    def __init__(self, bs):
        self.bs = bs
        self.handle = 0
        self.lib = None  # the library object that made `handle` (a session is destroyed by the library that created it)
        self.key = None
        self.keep_alive = []
        self.bias_key = self.bias_keep = self.ngram_key = self.ngram_keep = None  # what _bind_tables sent to the session

    def __del__(self):
        try:
            if self.handle:
                self.lib.call("avsr_beam_destroy", self.handle)
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------ eligibility
    @staticmethod
    def supported(bs):
        from .decoding import CTCPrefixScorer, LengthBonus
        from .nets import TransformerDecoder

        full, part = bs.full_scorers, bs.part_scorers
        if set(part) not in ({"ctc"}, {"ctc", "ngram"}) or not isinstance(part["ctc"], CTCPrefixScorer):
            return False
        if "ngram" in part:  # n-gram shallow fusion: this build's back-off scorer over the search's vocabulary, nothing else in that slot
            from .ngram import NgramScorer

            if not isinstance(part["ngram"], NgramScorer) or part["ngram"].n_vocab != bs.n_vocab:
                return False
            # the selection adds the CTC term, then the n-gram's: the python step adds the partial scorers in their listed order
            if list(part) != ["ctc", "ngram"]:
                return False
        if "decoder" not in full or not isinstance(full["decoder"], TransformerDecoder):
            return False
        if set(full) - {"decoder", "length_bonus", "lm", "bias"}:
            return False
        if "bias" in full:  # contextual biasing: this build's trie scorer, nothing else in that slot
            from .bias import ContextBiasScorer

            if not isinstance(full["bias"], ContextBiasScorer) or full["bias"].n_vocab != bs.n_vocab:
                return False
            # as with a language model: the step's pre-beam ranks the decoder's log-probabilities alone
            if bs.pre_beam_score_key != "decoder":
                return False
        if "lm" in full:  # shallow fusion: this build's TransformerLM in a geometry the session takes, nothing else
            from .lm import TransformerLM

            if not isinstance(full["lm"], TransformerLM) or not full["lm"].native_ok(bs.n_vocab):
                return False
            # the step's pre-beam ranks the decoder's log-probabilities alone: with a language model "full" (decoder + LM) is another
            # candidate set (without one the length bonus is a per-row constant and the two keys select alike)
            if bs.pre_beam_score_key != "decoder":
                return False
        if "length_bonus" in full and not isinstance(full["length_bonus"], LengthBonus):
            return False
        if not bs.do_pre_beam or bs.pre_beam_score_key not in ("decoder", "full") or bs.weights["decoder"] <= 0:
            return False
        dec = full["decoder"]
        lay = dec.decoders[0]
        D, H = lay.size, lay.self_attn.h
        FF = lay.feed_forward.w_1.out_features
        if dec.output_layer is None or not dec.normalize_before or D != 64 * H or FF % 64:
            return False
        if not skinny_len_ok(D, False) or not skinny_len_ok(FF, True):
            return False
        beam, S = bs.beam_size, bs.pre_beam_size
        return 2 <= beam <= MAX_BEAM and beam <= S - 1 and beam * (S + 1) <= 8192

    # ------------------------------------------------------------------------------------------------ weights
    def _bind(self, dev, min_pos):
        bs = self.bs
        dec = bs.full_scorers["decoder"]
        lm = bs.full_scorers.get("lm")
        params = list(dec.parameters()) + (list(lm.parameters()) if lm is not None else [])
        pos = dec.embed[1]
        pe = _f32(pos.table(max(pos.pe.size(1), min_pos), dev))
        if lm is not None:
            lm_pos = lm.encoder.embed[4]
            lm_pe = _f32(lm_pos.table(max(lm_pos.pe.size(1), min_pos), dev))
        # (FusedAdamW updates parameters through raw pointers without bumping `_version`: the optimizer-step generation of the
        # weight caches is part of the key, so the stacked copies below are rebuilt after native training steps too)
        from . import functional as AF

        key = (str(dev), pe.data_ptr(), pe.shape[0], AF.weight_generation()) + tuple((p.data_ptr(), p._version) for p in params)
        if lm is not None:
            key += (lm_pe.data_ptr(), lm_pe.shape[0], float(bs.weights["lm"]))
        if key == self.key:
            for kind in _TABLE_SCORERS:
                self._bind_tables(kind, dev)
            return
        L = _lib.lib()
        if self.handle:
            self.lib.call("avsr_beam_destroy", self.handle)
            self.handle = 0
        lay0 = dec.decoders[0]
        D, H, FF = lay0.size, lay0.self_attn.h, lay0.feed_forward.w_1.out_features
        emb = dec.embed[0]
        V = dec.output_layer.out_features
        shared = getattr(bs, "_native_weights", None)  # the stacked / f32 weight tensors: one set for all sessions of this search
        if shared is not None and shared[0] == key:
            keep = shared[1]
        else:
            keep = [_f32(emb.weight), pe]
            for d in dec.decoders:
                sa, ca, ff = d.self_attn, d.src_attn, d.feed_forward
                keep += [_f32(d.norm1.weight), _f32(d.norm1.bias),
                         torch.cat([_f32(sa.linear_q.weight), _f32(sa.linear_k.weight), _f32(sa.linear_v.weight)], 0).contiguous(),
                         torch.cat([_f32(sa.linear_q.bias), _f32(sa.linear_k.bias), _f32(sa.linear_v.bias)], 0).contiguous(),
                         _f32(sa.linear_out.weight), _f32(sa.linear_out.bias),
                         _f32(d.norm2.weight), _f32(d.norm2.bias), _f32(ca.linear_q.weight), _f32(ca.linear_q.bias),
                         torch.cat([_f32(ca.linear_k.weight), _f32(ca.linear_v.weight)], 0).contiguous(),
                         torch.cat([_f32(ca.linear_k.bias), _f32(ca.linear_v.bias)], 0).contiguous(),
                         _f32(ca.linear_out.weight), _f32(ca.linear_out.bias),
                         _f32(d.norm3.weight), _f32(d.norm3.bias), _f32(ff.w_1.weight), _f32(ff.w_1.bias), _f32(ff.w_2.weight),
                         _f32(ff.w_2.bias)]
            keep += [_f32(dec.after_norm.weight), _f32(dec.after_norm.bias), _f32(dec.output_layer.weight), _f32(dec.output_layer.bias)]
            if lm is not None:  # (after the decoder's pointers: avsr_beam_attach_lm's list)
                keep += self._lm_weights(lm, lm_pe)
            bs._native_weights = (key, keep)
        assert all(t.device == keep[0].device for t in keep)
        n_dec = 2 + 20 * len(dec.decoders) + 4
        keep_lm, keep_dec = keep[n_dec:], keep[:n_dec]
        has_len = int("length_bonus" in bs.full_scorers)
        cfg = (ctypes.c_int32 * 12)(D, H, FF, V, len(dec.decoders), bs.beam_size, bs.pre_beam_size, bs.sos, bs.eos,
                                    bs.part_scorers["ctc"].blank, has_len, pe.shape[0])
        fcfg = (ctypes.c_float * 5)(bs.weights["decoder"], bs.weights["ctc"], bs.weights.get("length_bonus", 0.0) if has_len else 0.0,
                                    pos.xscale, dec.decoders[0].norm1.eps)
        ptrs = (ctypes.c_void_p * len(keep_dec))(*[t.data_ptr() for t in keep_dec])
        h = L.call("avsr_beam_create", ctypes.cast(cfg, ctypes.c_void_p), ctypes.cast(fcfg, ctypes.c_void_p),
                   ctypes.cast(ptrs, ctypes.c_void_p), len(keep_dec))
        if not h:
            raise _lib.AvsrLibraryError("avsr_beam_create: " + L.cdll.avsr_last_error().decode())
        if lm is not None:
            lcfg = (ctypes.c_int32 * 6)(lm.att_unit, lm.head, lm.unit, lm.layer, lm.n_vocab, lm_pe.shape[0])
            lfcfg = (ctypes.c_float * 3)(bs.weights["lm"], lm_pos.xscale, lm.encoder.encoders[0].norm1.eps)
            lptrs = (ctypes.c_void_p * len(keep_lm))(*[t.data_ptr() for t in keep_lm])
            try:
                L.call("avsr_beam_attach_lm", h, ctypes.cast(lcfg, ctypes.c_void_p), ctypes.cast(lfcfg, ctypes.c_void_p),
                       ctypes.cast(lptrs, ctypes.c_void_p), len(keep_lm))
            except Exception:
                L.call("avsr_beam_destroy", h)
                raise
        self.handle, self.lib, self.key, self.keep_alive = h, L, key, keep
        self.V, self.pe_rows = V, pe.shape[0]
        self.group_host = self.group_yseq_host = None  # pinned result buffers of search_group, sized by the largest group so far
        for kind in _TABLE_SCORERS:  # (a new session has nothing bound)
            setattr(self, kind + "_key", None)
            self._bind_tables(kind, dev)

    def _bind_tables(self, kind, dev):
        """The device tables of scorers[kind] -- the bias list (avsr_beam_set_bias) or the n-gram model (avsr_beam_set_ngram): re-sent
        when the scorer's version or its weight changed, or the session is new -- never a reason to rebuild the session; detached when
        the scorer left the search after its tables were bound.  Takes effect at the next avsr_beam_begin / _begin_batch."""
        kd = _TABLE_SCORERS[kind]
        sc = getattr(self.bs, kd.scorers).get(kind)
        bound = getattr(self, kind + "_key")
        if sc is None:
            if bound is None:
                return
            key, tabs, cfg, weight, ptrs = None, None, kd.cfg_detached, 0.0, [None] * kd.n_tables
        else:
            key = (id(sc), sc.version, float(self.bs.weights[kind]), str(dev))
            if key == bound:
                return
            tabs = sc.device_tables(dev)
            cfg, weight, ptrs = kd.cfg(sc), self.bs.weights[kind], [t.data_ptr() for t in tabs]
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
        self.lib.call(kd.entry, self.handle, vp((ctypes.c_int32 * len(cfg))(*cfg)), vp((ctypes.c_float * 1)(weight)), *ptrs)
        setattr(self, kind + "_key", key)
        setattr(self, kind + "_keep", tabs)  # (the tables stay alive as long as the session may read them)

    @staticmethod
    def _lm_weights(lm, lm_pe):
        _, table, qkv = lm.derived()
        ln = lm.encoder.embed[1]
        out = [table, _f32(ln.weight), _f32(ln.bias), lm_pe]
        for e, (wqkv, bqkv) in zip(lm.encoder.encoders, qkv):
            sa, ff = e.self_attn, e.feed_forward
            out += [_f32(e.norm1.weight), _f32(e.norm1.bias), wqkv, bqkv, _f32(sa.linear_out.weight), _f32(sa.linear_out.bias),
                    _f32(e.norm2.weight), _f32(e.norm2.bias), _f32(ff.w_1.weight), _f32(ff.w_1.bias), _f32(ff.w_2.weight), _f32(ff.w_2.bias)]
        an = lm.encoder.after_norm
        return out + [_f32(an.weight), _f32(an.bias), _f32(lm.decoder.weight), _f32(lm.decoder.bias)]

    # ------------------------------------------------------------------------------------------------ the search
    @torch.no_grad()
    def search(self, x, maxlenratio=0.0, minlenratio=0.0, ctc_state=None):
        """One utterance: a group of one.  ctc_state: (log-posteriors [T][ld], empty-prefix state [T][2]) from `prepare_ctc` when the
        caller computed them (search_many)."""
        if ctc_state is None:
            ctc_state = prepare_ctc(self.bs.part_scorers["ctc"], x)
        return self.search_group([x], [ctc_state], maxlenratio, minlenratio)[0]

    # ------------------------------------------------------------------------------------------------ a group of utterances
    def group_workspace_bytes(self, Ts, Lmax):
        """Bytes `search_group` allocates for utterances of Ts frames and at most Lmax steps (after `_bind`)."""
        arr = (ctypes.c_int32 * len(Ts))(*Ts)
        n = _lib.lib().call("avsr_beam_batch_workspace_bytes", self.handle, len(Ts), ctypes.cast(arr, ctypes.c_void_p), Lmax)
        if n <= 0:
            raise _lib.AvsrLibraryError("avsr_beam_batch_workspace_bytes: " + _lib.lib().cdll.avsr_last_error().decode())
        return n

    @torch.no_grad()
    def search_group(self, xs, pre, maxlenratio=0.0, minlenratio=0.0):
        """The searches of U utterances with ONE library call per step (avsr_beam_step_batch): every utterance has its own maxlen,
        takes its forced end there, collects its own <eos> hypotheses, stops by its own end detection, and is retired (n_keep = 0)
        while the others go on.  pre[u] = prepare_ctc of xs[u].  Returns one n-best list per utterance."""
        from .decoding import Hypothesis

        bs = self.bs
        U, dev = len(xs), xs[0].device
        Ts = [int(x.shape[0]) for x in xs]
        maxlens = [search_maxlen(T, maxlenratio) for T in Ts]
        Lmax = max(maxlens)
        self._bind(dev, Lmax + 2)
        L = _lib.lib()
        mems = [_f32(x) for x in xs]
        nws = self.group_workspace_bytes(Ts, Lmax)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        stream = ops._stream(mems[0])
        i32, ptr = ctypes.c_int32 * U, ctypes.c_void_p * U
        vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
        L.call("avsr_beam_begin_batch", self.handle, U, vp(ptr(*[m.data_ptr() for m in mems])), vp(i32(*Ts)),
               vp(ptr(*[p[0].data_ptr() for p in pre])), vp(i32(*[p[0].stride(0) for p in pre])), vp(ptr(*[p[1].data_ptr() for p in pre])),
               ws.data_ptr(), nws, Lmax, stream)
        rows = U * bs.beam_size
        pin = dev.type == "cuda"
        host = self.group_host
        if host is None or host.shape[0] < rows * 8:
            host = self.group_host = torch.empty(rows * 8, dtype=torch.float32, pin_memory=pin)
        host_np = host.numpy().reshape(-1, 8)
        yseq_host = self.group_yseq_host
        if yseq_host is None or yseq_host.shape[0] < rows * (Lmax + 2):
            yseq_host = self.group_yseq_host = torch.empty(rows * (Lmax + 2), dtype=torch.int64, pin_memory=pin)
        n_out, c_ldy, c_L = i32(), ctypes.c_int(0), ctypes.c_int(0)
        host_ptr, n_ptr = host.data_ptr(), vp(n_out)  # (what a step passes, formed once)
        yseq_np, yseq_ptr, ldy_ptr, Lc_ptr = yseq_host.numpy(), yseq_host.data_ptr(), vp(ctypes.pointer(c_ldy)), vp(ctypes.pointer(c_L))
        names = ["decoder"] + [k for k in ("lm", "bias", "length_bonus") if k in bs.full_scorers] + ["ctc"]
        col = {"decoder": 3, "ctc": 4, "length_bonus": 5, "lm": 6, "bias": 7}
        # the n-gram sums of a step's records are not a column of them (the records stay [K][8]): avsr_beam_ngram_sums, packed alike
        ngram = "ngram" in bs.part_scorers
        ng_np = np.zeros(rows, dtype=np.float32)
        ng_ptr, ng_n = ng_np.ctypes.data, ctypes.c_int(0)
        ng_n_ptr = vp(ctypes.pointer(ng_n))
        eos = bs.eos
        ended = [[] for _ in range(U)]
        best = [-math.inf] * U
        best_len = [{} for _ in range(U)]
        running = [True] * U

        def end(u, r, ys, forced):
            row = host_np[r]
            ys = list(ys) + ([eos] if forced else [])
            sc = float(row[2])
            scores = {k: float(row[col[k]]) for k in names}
            if ngram:
                scores["ngram"] = float(ng_np[r])
            ended[u].append(Hypothesis(yseq=torch.tensor(ys, dtype=torch.int64), score=sc, scores=scores, states={}))
            best[u] = max(best[u], sc)
            best_len[u][len(ys)] = max(best_len[u].get(len(ys), -math.inf), sc)

        def fetch():
            L.call("avsr_beam_fetch_yseq_batch", self.handle, yseq_ptr, ldy_ptr, Lc_ptr, stream)
            if ngram:  # (a host copy the step made: no device work)
                L.call("avsr_beam_ngram_sums", self.handle, ng_ptr, ng_n_ptr)
            return yseq_np, c_ldy.value, c_L.value

        for i in range(Lmax):
            L.call("avsr_beam_step_batch", self.handle, host_ptr, n_ptr, stream)
            fetched = None
            alive_of, changed, off = [()] * U, False, 0  # per utterance the rows that stay on its beam (the keep list is formed when one leaves)
            for u in range(U):
                K = n_out[u]
                if not running[u]:
                    continue
                out = host_np[off: off + K]
                if i == maxlens[u] - 1:  # this utterance's forced end (beam_search.py:430-436)
                    fetched = fetched or fetch()
                    ys, ldy, Lc = fetched
                    for b in range(K):
                        end(u, off + b, ys[(off + b) * ldy: (off + b) * ldy + Lc], True)
                    alive = ()
                else:
                    is_eos = out[:, 0] == eos
                    alive = range(K)
                    if is_eos.any():
                        fetched = fetched or fetch()
                        ys, ldy, Lc = fetched
                        for b in np.nonzero(is_eos)[0].tolist():
                            end(u, off + b, ys[(off + b) * ldy: (off + b) * ldy + Lc], False)
                        alive = np.nonzero(~is_eos)[0].tolist()
                if maxlenratio == 0.0 and ended[u] and self._end_detect(best[u], best_len[u], i):
                    alive = ()
                if not alive:
                    running[u] = False
                changed = changed or len(alive) != K
                alive_of[u] = alive
                off += K
            if not any(running):
                break
            if changed:
                keep, n_keep = [b for a in alive_of for b in a], [len(a) for a in alive_of]
                L.call("avsr_beam_keep_batch", self.handle, vp((ctypes.c_int32 * max(1, len(keep)))(*keep)), vp(i32(*n_keep)), stream)
        results = []
        for u in range(U):
            nbest = sorted(ended[u], key=lambda h: float(h.score), reverse=True)
            if not nbest and minlenratio >= 0.1:  # (beam_search.py:448-456: the retry is a search of its own)
                nbest = self.search(xs[u], maxlenratio, max(0.0, minlenratio - 0.1), ctc_state=pre[u])
            results.append(nbest)
        return results

    @staticmethod
    def _end_detect(best, best_len, i, M=3, D_end=math.log(1 * math.exp(-10))):
        """decoding.end_detect (e2e_asr_common.py:17-47) on the running maxima instead of the list of dicts."""
        count = 0
        for m in range(M):
            s = best_len.get(i - m)
            if s is not None and s - best < D_end:
                count += 1
        return count == M


def prepare_ctc(ctc_scorer, x):
    """CTC log-posteriors [T][ld] of one utterance and the state of the empty prefix [T][2] (scorers/ctc.py:87-99)."""
    r0, _ = ctc_scorer.batch_init_state(x)
    return ctc_scorer.logp, r0.reshape(x.shape[0], 2).contiguous()


def search_many(bs, xs, workers=4, maxlenratio=0.0, minlenratio=0.0):
    """Beam searches of several utterances AT ONCE: `workers` host threads, each with its own session (beam state, workspace,
    pinned result buffer) and its own stream.  A decoding step is 52 dependent launches of 24 - 316 blocks that are bound by
    launch / memory latency, not by the machine: steps of different utterances overlap on the GPU, and the library call
    releases the GIL while it issues the launches and waits for the step's result.  Results are those of `bs(x)` per utterance
    (each search is the same sequence of launches on its own state).  The CTC posteriors are computed here, on the caller's
    thread: the kernels' python glue (functional.py mode state, weight caches) is not re-entrant."""
    if not xs:
        return []
    dev = xs[0].device
    cuda = dev.type == "cuda"
    ctc = bs.part_scorers["ctc"]
    pre = [prepare_ctc(ctc, x) for x in xs]
    maxpos = max(search_maxlen(int(x.shape[0]), maxlenratio) for x in xs) + 2
    workers = max(1, min(workers, len(xs)))
    pool = getattr(bs, "_native_pool", None)
    if pool is None or len(pool) < workers:
        pool = bs._native_pool = (pool or []) + [NativeBeam(bs) for _ in range(workers - len(pool or []))]
    for sess in pool[:workers]:
        sess._bind(dev, maxpos)  # (on this thread: binding extends the decoder's position table)
    streams = [torch.cuda.Stream(device=dev) for _ in range(workers)] if cuda else [None] * workers
    if cuda:
        for st in streams:
            st.wait_stream(torch.cuda.current_stream(dev))  # encoder outputs / posteriors were produced on the caller's stream
    results, errors, it, lock = [None] * len(xs), [], iter(range(len(xs))), threading.Lock()

    def work(w):
        ctx = torch.cuda.stream(streams[w]) if cuda else contextlib.nullcontext()
        try:
            with ctx, torch.no_grad():
                while True:
                    with lock:
                        i = next(it, None)
                    if i is None or errors:
                        break
                    results[i] = pool[w].search(xs[i], maxlenratio, minlenratio, ctc_state=pre[i])
        except BaseException as e:  # noqa: BLE001 -- re-raised on the caller's thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,), daemon=True) for w in range(workers)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if cuda:
        for st in streams:
            torch.cuda.current_stream(dev).wait_stream(st)
    if errors:
        raise errors[0]
    return results


def search_batch(bs, xs, max_batch=8, max_workspace_bytes=8 << 30, maxlenratio=0.0, minlenratio=0.0):
    """Beam searches of several utterances with ONE decoding step per GROUP of utterances (avsr_beam_step_batch): the U x beam running
    hypotheses of a group go through the same ~60 launches, every weight is read once per step instead of once per step and
    utterance.  Returns [bs(x) for x in xs] in input order (a row's arithmetic does not depend on what else is in its group).

    Utterances are sorted by length and cut into consecutive groups of at most `max_batch` (and at most 32 utterances / 1024
    packed rows, the library's limits); a group takes as many steps as its longest member.  A group is shrunk, never below one
    utterance, until its workspace fits `max_workspace_bytes`.  The workspace of a group (avsr_beam_batch_workspace_bytes) is, with
    R = U * beam rows, F = the frames of all its utterances, D / FF / V the decoder's widths and S the pre-beam size, in bytes
        layers * (Lmax * R * 3 D + F * 2 D) * 4              self-attention caches [Lmax][R][3 D], memory K / V [F][2 D]
      + 2 * (R * (Lmax + 2) * 12 + 2 * F * beam * 4)         two beam states: tokens, ancestry, CTC state [F][2][beam]
      + 2 * F * beam * S * 4                                 CTC forward variables of every candidate
      + R * (14 D + FF + 2 V + 3 S) * 4                      activations, K-slice partial sums, logits, log-probabilities, candidates
    plus, with a language model of width D' / FF' and `lm_layers` layers,
        lm_layers * Lmax * R * 3 D' * 4 + R * (11 D' + FF' + 2 V) * 4.
    (per-row scalars and the 256-byte alignment of every table left out).  The cache term dominates: 1.18 GB per layer for U = 8, beam 40, D = 768, Lmax = 400."""
    xs = list(xs)
    if not xs:
        return []
    dev = xs[0].device
    ctc = bs.part_scorers["ctc"]
    sess = bs._native
    maxpos = max(search_maxlen(int(x.shape[0]), maxlenratio) for x in xs) + 2
    sess._bind(dev, maxpos)
    cap = max(1, min(int(max_batch), MAX_GROUP, MAX_GROUP_ROWS // bs.beam_size))
    order = sorted(range(len(xs)), key=lambda i: int(xs[i].shape[0]))
    results = [None] * len(xs)
    at = 0
    while at < len(order):
        idx = order[at: at + cap]
        while len(idx) > 1:
            Ts = [int(xs[i].shape[0]) for i in idx]
            if sess.group_workspace_bytes(Ts, max(search_maxlen(T, maxlenratio) for T in Ts)) <= max_workspace_bytes:
                break
            idx = idx[:-1]
        group = [xs[i] for i in idx]
        pre = [prepare_ctc(ctc, x) for x in group]
        for i, nbest in zip(idx, sess.search_group(group, pre, maxlenratio, minlenratio)):
            results[i] = nbest
        at += len(idx)
    return results
