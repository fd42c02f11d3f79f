"""Decode throughput of the evaluation path (lightning.ModelModule.forward -- front-end, encoder, hybrid CTC /
attention BatchBeamSearch with beam 40) on the MI355X: utterances/s and ms per emitted token for T = 100 and T = 400 frames,
bf16 and precise numerical modes.  Weights: tests/golden/synth.py (the decode goldens' generator), so the search runs a
realistic number of steps instead of collapsing on an untrained model's first <eos>.
    python tools/bench_decode.py [--reps 3] > profiles/r3_decode_throughput.json
The reference's own CPU figure for the same loop: 2.12 s for one 4 s utterance (T = 100)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--beam", type=int, default=40)
    ap.add_argument("--many", type=int, default=16, help="utterances of the concurrent-decoding rows (BatchBeamSearch.forward_many)")
    ap.add_argument("--lm", action="store_true",
                    help="shallow fusion rows instead of the default ones: a Transformer LM of 16 layers x 512 (8 heads, FF 2048, E 128, synthetic "
                         "weights), lm_weight 0.3 -- native step, python-issued step with the "
                         "cached TransformerLM, python-issued step with a plain-torch LM as a foreign scorer (what a build without the LM slot "
                         "can do)")
    ap.add_argument("--two-pass", action="store_true",
                    help="two-pass decoding rows instead of the default ones: CTC prefix beam search on the device + one teacher-forced "
                         "rescoring pass (auto_avsr_amd/two_pass.py) beside the native one-call search at --beam, on the same encoder "
                         "outputs -- per phase at one utterance, and utterances/s at 1, 8 and 32 utterances per launch")
    ap.add_argument("--two-pass-sweep", action="store_true",
                    help="(beam, topk) sweep of two-pass decoding on the trained fixture of tests/test_wer_trained.py: WER, containment of "
                         "the reference's best hypothesis in the n-best, share of utterances whose winner scores at least the reference's")
    ap.add_argument("--two-pass-once", type=int, default=0, metavar="T",
                    help="one warm-up and one two-pass decode of a T-frame utterance and nothing else (the program of a kernel-trace run)")
    ap.add_argument("--batch", action="store_true",
                    help="batched native search rows instead of the default ones: 16 utterances of T = 100 and of T = 400 frames through "
                         "BatchBeamSearch.forward_batch in groups of 1, 4, 8 and 16 beside one search at a time and forward_many(workers=4), "
                         "alternated, on the same encoder outputs (precise mode; python tools/bench_decode.py --batch > profiles/batch_decode.json)")
    ap.add_argument("--bias", action="store_true",
                    help="contextual-biasing rows instead of the default ones: a list of 1 000 random phrases of 2 - 5 tokens, weight 1.0 -- the "
                         "native step without and with the list, alternated in the same run, and the python-issued step with the list "
                         "(precise mode; python tools/bench_decode.py --bias > profiles/context_bias_decode.json).  With --two-pass: two-pass "
                         "decoding without and with the same list, alternated -- first pass and whole decode "
                         "(python tools/bench_decode.py --two-pass --bias > profiles/two_pass_bias_decode.json)")
    ap.add_argument("--ngram", action="store_true",
                    help="n-gram shallow-fusion rows instead of the default ones: a random 3-gram back-off model of about 10^6 n-grams, weight "
                         "0.3 -- the native step without and with it, and the python-issued step with it, sides alternated "
                         "(precise mode; python tools/bench_decode.py --ngram > profiles/ngram_decode.json).  With --two-pass: two-pass decoding "
                         "without and with the same model inside the first pass, alternated -- first pass and whole decode "
                         "(python tools/bench_decode.py --two-pass --ngram --reps 30 > profiles/two_pass_ngram_decode.json).  With "
                         "--two-pass-sweep: the trained fixture's sweep, then with a 3-gram estimated from the fixture's own transcripts "
                         "(python tools/bench_decode.py --two-pass-sweep --ngram > profiles/two_pass_ngram_sweep.json)")
    ap.add_argument("--encode", action="store_true",
                    help="encoder-only rows instead of the default ones: 16 utterances around T = 100 and around T = 400 frames (lengths spread "
                         "+-20 %) through ModelModule.encode_many one at a time and in zero-padded groups of 4, 8 and 16, alternated, precise "
                         "and mixed modes, then a whole --decode-mode rescore decode without and with encode_batch 16 "
                         "(python tools/bench_decode.py --encode > profiles/encode_batch.json).  With --modality audiovisual: the same for "
                         "the audio-visual model (both front-ends, both encoders, the fusion head), groups of 4 and 8, whole decode with "
                         "encode_batch 8 (python tools/bench_decode.py --encode --modality audiovisual > profiles/encode_batch_av.json)")
    ap.add_argument("--modality", choices=["video", "audiovisual"], default="video", help="--encode: the model whose encoder side is timed")
    ap.add_argument("--bias-weight", type=float, default=1.0, help="--two-pass --bias: the weight of the list")
    ap.add_argument("--rescore-beam", type=int, default=16)
    ap.add_argument("--rescore-topk", type=int, default=16)
    ap.add_argument("--modes", type=str, default="precise", help="--two-pass: comma-separated numerical modes (eval.py decodes in precise)")
    args = ap.parse_args()
    if args.encode:
        return main_encode(args)
    if args.lm:
        return main_lm(args)
    if args.two_pass_sweep:
        return main_two_pass_sweep(args)
    if args.batch:
        return main_batch(args)
    if args.bias and args.two_pass:
        return main_two_pass_bias(args)
    if args.bias:
        return main_bias(args)
    if args.ngram and args.two_pass:
        return main_two_pass_ngram(args)
    if args.ngram:
        return main_ngram(args)
    if args.two_pass or args.two_pass_once:
        return main_two_pass(args)
    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    dev = torch.device("cuda:0")
    m = E2E(5049, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    bs = lightning.get_beam_search_decoder(m, [str(i) for i in range(5049)], beam_size=args.beam)
    rows = []
    from auto_avsr_amd import decoding

    for mode, native in (("mixed", True), ("bf16", True), ("precise", True), ("bf16", False), ("precise", False)):
        AF.set_mode(mode)
        AF.invalidate_weight_cache()
        decoding.NATIVE_BEAM = native  # True: one library call per step (csrc/decode.hip); False: the python-issued step
        bs._native = None
        for T in (100, 400):
            x, _, _ = synth_batch("video", 1, T, 3, 5049, seed=T, lengths=[T])
            x = x.to(dev)
            t_enc, t_dec, steps = [], [], 0
            for rep in range(args.reps + 1):
                with torch.no_grad():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    feats = m.proj_encoder(m.frontend(x))
                    enc, _ = m.encoder(feats, None)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    nbest = bs(enc.squeeze(0).float())
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                if rep:  # first repetition = warm-up
                    t_enc.append(t1 - t0)
                    t_dec.append(t2 - t1)
                steps = max(len(h.asdict()["yseq"]) for h in nbest) - 1 if nbest else 0
            enc_ms, dec_ms = min(t_enc) * 1e3, min(t_dec) * 1e3
            assert bool(bs._native) == native
            rows.append({"mode": mode, "step": "native (avsr_beam_step)" if native else "python-issued", "T_frames": T, "beam": args.beam, "encoder_ms": round(enc_ms, 2), "beam_search_ms": round(dec_ms, 2),
                         "longest_hypothesis_tokens": steps, "ms_per_token": round(dec_ms / max(steps, 1), 3),
                         "utterances_per_sec": round(1e3 / (enc_ms + dec_ms), 3)})
            rows[-1]["best_yseq_head"] = nbest[0].asdict()["yseq"][:12] if nbest else []
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    # several utterances in flight: forward_many with 1, 2, 4, 8 workers over `--many` utterances of T = 100 (encoder outputs ready)
    AF.set_mode("mixed")
    AF.invalidate_weight_cache()
    decoding.NATIVE_BEAM = True
    bs._native = None
    encs = []
    with torch.no_grad():
        for i in range(args.many):
            x, _, _ = synth_batch("video", 1, 100, 3, 5049, seed=1000 + i, lengths=[100])
            feats = m.proj_encoder(m.frontend(x.to(dev)))
            encs.append(m.encoder(feats, None)[0].squeeze(0).float())
        ref = None
        for workers in (1, 2, 4, 8):
            best = None
            for rep in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = bs.forward_many(encs, workers=workers)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None or dt < best else best
            ys = [r[0].asdict()["yseq"] for r in res]
            ref = ys if ref is None else ref
            rows.append({"mode": "mixed", "step": f"native, {workers} searches in flight (forward_many)", "T_frames": 100, "beam": args.beam,
                         "utterances": args.many, "beam_search_ms_total": round(best * 1e3, 1),
                         "utterances_per_sec_search_only": round(args.many / best, 2), "same_best_hypotheses_as_1_worker": ys == ref})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    decoding.NATIVE_BEAM = True
    print(json.dumps({"metric": "decode throughput, video E2E 250M, hybrid CTC/attention beam search (lightning.py:54-64,126-158)",
                      "reference_cpu": "2.12 s per 4 s utterance (T = 100), 8 host cores, BASELINE.md section 2",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


class PlainTorchLM:
    """The LM of auto_avsr_amd.lm.TransformerLM in plain torch, without a cache, as a FOREIGN full scorer: the only way to fuse a
    language model without the `lm` slot -- the search then runs the python-issued step and the LM re-runs the whole prefix of every
    hypothesis at every step."""

    def __init__(self, lm):
        self.sd = {k: v.detach().float() for k, v in lm.state_dict().items()}
        self.D, self.H, self.nl = lm.att_unit, lm.head, lm.layer
        self.pos = lm.encoder.embed[4]

    @torch.no_grad()
    def batch_score(self, ys, states, xs):
        F, sd, D, H = torch.nn.functional, self.sd, self.D, self.H
        n, L = ys.shape
        x = F.linear(F.embedding(ys, sd["embed.weight"]), sd["encoder.embed.0.weight"], sd["encoder.embed.0.bias"])
        x = F.layer_norm(x, (D,), sd["encoder.embed.1.weight"], sd["encoder.embed.1.bias"], 1e-12)
        x = torch.relu(x) * self.pos.xscale + self.pos.table(L, ys.device)
        mask = torch.ones(L, L, dtype=torch.bool, device=ys.device).tril()
        for i in range(self.nl):
            p = f"encoder.encoders.{i}."
            h = F.layer_norm(x, (D,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-12)
            q, k, v = (F.linear(h, sd[p + f"self_attn.linear_{c}.weight"], sd[p + f"self_attn.linear_{c}.bias"]).view(n, L, H, D // H).transpose(1, 2)
                       for c in "qkv")
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(n, L, D)
            x = x + F.linear(a, sd[p + "self_attn.linear_out.weight"], sd[p + "self_attn.linear_out.bias"])
            h = F.layer_norm(x, (D,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-12)
            h = torch.relu(F.linear(h, sd[p + "feed_forward.w_1.weight"], sd[p + "feed_forward.w_1.bias"]))
            x = x + F.linear(h, sd[p + "feed_forward.w_2.weight"], sd[p + "feed_forward.w_2.bias"])
        y = F.layer_norm(x[:, -1], (D,), sd["encoder.after_norm.weight"], sd["encoder.after_norm.bias"], 1e-12)
        return torch.log_softmax(F.linear(y, sd["decoder.weight"], sd["decoder.bias"]), -1), None


def main_lm(args):
    import statistics

    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import decoding
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E
    from auto_avsr_amd.lm import TransformerLM

    dev = torch.device("cuda:0")
    m = E2E(5049, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    lm = TransformerLM(5049, embed_unit=128, att_unit=512, head=8, unit=2048, layer=16)
    lm.load_state_dict(synth_state_dict(lm.state_dict(), 4))
    lm = lm.to(dev)
    toks = [str(i) for i in range(5049)]
    w_lm = 0.3

    def make(side):
        bs = lightning.get_beam_search_decoder(m, toks, rnnlm=lm, lm_weight=w_lm, beam_size=args.beam)
        if side == "foreign":  # the same weights behind a scorer the library does not know
            bs.scorers["lm"] = bs.full_scorers["lm"] = PlainTorchLM(lm)
        return bs

    sides = {"native": ("native step (avsr_beam_step with the LM attached)", True),
             "python": ("python-issued step, cached TransformerLM", False),
             "foreign": ("python-issued step, plain-torch LM as a foreign scorer (no cache): the build without the lm slot", False)}
    searches = {k: make(k) for k in sides}
    rows = []
    for mode in ("precise", "bf16"):
        AF.set_mode(mode)
        AF.invalidate_weight_cache()
        for T in (100, 400):
            x, _, _ = synth_batch("video", 1, T, 3, 5049, seed=T, lengths=[T])
            with torch.no_grad():
                enc = m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float()
            times, out = {k: [] for k in sides}, {}
            for rep in range(args.reps + 1):  # first repetition = warm-up; the sides alternate within a repetition
                for k, (_, native) in sides.items():
                    decoding.NATIVE_BEAM = native
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    with torch.no_grad():
                        nbest = searches[k](enc)
                    torch.cuda.synchronize()
                    if rep:
                        times[k].append((time.perf_counter() - t0) * 1e3)
                    out[k] = nbest
                    assert bool(searches[k]._native) == native
            for k, (label, _) in sides.items():
                steps = max(len(h.asdict()["yseq"]) for h in out[k]) - 1
                med = statistics.median(times[k])
                rows.append({"mode": mode, "step": label, "side": k, "T_frames": T, "beam": args.beam, "lm": "16 x 512, 8 heads, FF 2048, E 128",
                             "lm_weight": w_lm, "beam_search_ms_median": round(med, 2), "beam_search_ms_min": round(min(times[k]), 2),
                             "beam_search_ms_max": round(max(times[k]), 2), "repetitions": len(times[k]), "longest_hypothesis_tokens": steps,
                             "ms_per_token": round(med / max(steps, 1), 3),
                             "same_best_hypothesis_as_native": out[k][0].asdict()["yseq"] == out["native"][0].asdict()["yseq"]})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            base = next(r for r in rows[-3:] if r["side"] == "foreign")["ms_per_token"]
            for r in rows[-3:]:
                r["speedup_over_foreign_scorer"] = round(base / r["ms_per_token"], 2)
    # several utterances in flight with an LM: forward_many at 4 workers
    AF.set_mode("mixed")
    AF.invalidate_weight_cache()
    decoding.NATIVE_BEAM = True
    encs = []
    with torch.no_grad():
        for i in range(args.many):
            x, _, _ = synth_batch("video", 1, 100, 3, 5049, seed=1000 + i, lengths=[100])
            encs.append(m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float())
    ref = None
    t_many = {"native": []}
    for rep in range(args.reps + 1):
        for k in t_many:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = searches[k].forward_many(encs, workers=4)
            torch.cuda.synchronize()
            if rep:
                t_many[k].append((time.perf_counter() - t0) * 1e3)
            ys = [r[0].asdict()["yseq"] for r in res]
            ref = ys if ref is None else ref
            assert ys == ref
    for k, ts in t_many.items():
        rows.append({"mode": "mixed", "step": sides[k][0] + ", 4 searches in flight (forward_many)", "side": k, "T_frames": 100, "beam": args.beam,
                     "utterances": args.many, "beam_search_ms_total_median": round(statistics.median(ts), 1),
                     "beam_search_ms_total_min": round(min(ts), 1), "beam_search_ms_total_max": round(max(ts), 1),
                     "utterances_per_sec_search_only": round(args.many / (statistics.median(ts) / 1e3), 2)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    print(json.dumps({"metric": "beam search with Transformer-LM shallow fusion, video E2E 250M decoder + 16 x 512 LM, beam search only (encoder output ready)",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def _timed(fn, reps):
    """Median / min / max wall time in ms of fn() between device synchronisations, after one warm-up call."""
    import statistics

    ts, out = [], None
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        if rep:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}, out


def main_two_pass(args):
    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import decoding
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    dev = torch.device("cuda:0")
    m = E2E(5049, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    toks = [str(i) for i in range(5049)]
    bs = lightning.get_beam_search_decoder(m, toks, beam_size=args.beam)
    tp = lightning.get_two_pass_decoder(m, toks, beam_size=args.rescore_beam, topk=args.rescore_topk)
    decoding.NATIVE_BEAM = True

    def encode(T, seed):
        x, _, _ = synth_batch("video", 1, T, 3, 5049, seed=seed, lengths=[T])
        with torch.no_grad():
            return m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float()

    if args.two_pass_once:
        AF.set_mode("precise")
        enc = encode(args.two_pass_once, args.two_pass_once)
        for _ in range(2):
            with torch.no_grad():
                nbest = tp(enc)
            torch.cuda.synchronize()
        print(json.dumps({"T_frames": args.two_pass_once, "hypotheses": len(nbest), "best_tokens": len(nbest[0].yseq) - 2}))
        return
    rows = []
    for mode in args.modes.split(","):
        AF.set_mode(mode)
        AF.invalidate_weight_cache()
        bs._native = None
        for T in (100, 400):
            enc = encode(T, T)
            t_native, nbest = _timed(lambda: bs(enc), args.reps)
            assert bs._native
            steps = max(len(h.asdict()["yseq"]) for h in nbest) - 1
            # the phases of one two-pass decode, each between synchronisations
            t_post, (memory, hlens, lp) = _timed(lambda: tp._posteriors([enc]), args.reps)
            t_first, (labels, n_valid) = _timed(lambda: tp.first_pass(lp, hlens), args.reps)
            t_ctc, _ = _timed(lambda: AF.ctc_score(lp, labels, hlens), args.reps)
            t_all, _ = _timed(lambda: tp.score_labels(memory, hlens, lp, labels), args.reps)
            t_total, two = _timed(lambda: tp(enc), args.reps)
            rows.append({"mode": mode, "T_frames": T, "utterances_per_launch": 1, "native_search": {"beam": args.beam, "ms": t_native, "longest_hypothesis_tokens": steps,
                                                                                                   "ms_per_token": round(t_native["median"] / max(steps, 1), 3)},
                         "two_pass": {"beam": tp.beam_size, "topk": tp.topk, "nbest": tp.nbest, "n_valid": int(n_valid[0]), "longest_label_row": int(labels.shape[2]),
                                      "ctc_posteriors_ms": t_post, "first_pass_ms": t_first, "ctc_score_ms": t_ctc,
                                      "rescoring_ms_decoder_plus_ctc_score": t_all, "whole_decode_ms": t_total},
                         "speedup_whole_decode_over_native_search": round(t_native["median"] / t_total["median"], 2),
                         "same_best_hypothesis": two[0].asdict()["yseq"] == nbest[0].asdict()["yseq"],
                         "two_pass_best_score": round(float(two[0].score), 4), "native_best_score": round(float(nbest[0].score), 4)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            for B in (8, 32):
                encs = [enc] + [encode(T, 1000 + i) for i in range(B - 1)]
                t_many, res = _timed(lambda: tp.forward_many(encs), max(1, args.reps - 1))
                t_nat, _ = _timed(lambda: bs.forward_many(encs, workers=4), 1) if B == 8 else (None, None)
                rows.append({"mode": mode, "T_frames": T, "utterances_per_launch": B, "two_pass_ms_total": t_many,
                             "two_pass_utterances_per_sec": round(B / (t_many["median"] / 1e3), 2),
                             "two_pass_utterances_per_sec_at_1": round(1e3 / t_total["median"], 2),
                             "native_search_4_in_flight_ms_total": t_nat,
                             "native_utterances_per_sec_4_in_flight": None if t_nat is None else round(B / (t_nat["median"] / 1e3), 2),
                             "first_equals_single": res[0][0].asdict()["yseq"] == two[0].asdict()["yseq"]})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
                del encs
    AF.set_mode("bf16")
    print(json.dumps({"metric": "two-pass decoding (CTC prefix beam search on the device + teacher-forced rescoring) against the native one-call "
                                "hybrid search, video E2E 250M, vocabulary 5049, search only (encoder output ready)",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def main_encode(args):
    """Encoder side of evaluation alone: front-end -> proj_encoder -> 12 Conformer layers, one utterance at a time (B = 1, unpadded)
    against length-exact zero-padded groups (ModelModule.encode_many); the sides alternate inside every repetition."""
    import statistics

    import lightning
    from synth import synth_state_dict

    from auto_avsr_amd import decoding
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    dev = torch.device("cuda:0")
    av = args.modality == "audiovisual"
    if av:
        from auto_avsr_amd.e2e_av import E2EAV

        m = E2EAV(5049)
    else:
        m = E2E(5049, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    toks = [str(i) for i in range(5049)]

    class Text:
        token_list = toks

        def post_process(self, ids):
            return " ".join(str(int(i)) for i in ids if int(i) != -1)

    mod = lightning.ModelModule.__new__(lightning.ModelModule)
    torch.nn.Module.__init__(mod)
    mod.modality, mod.model, mod.text_transform, mod.token_list = args.modality, m, Text(), toks
    mod.args = argparse.Namespace(decode_mode="rescore", rescore_beam=args.rescore_beam, rescore_topk=args.rescore_topk)
    decoding.NATIVE_BEAM = True
    N = 16

    def utterances(T):
        g = torch.Generator().manual_seed(T)
        lens = [round(T * (0.8 + 0.4 * i / (N - 1))) for i in range(N)]  # T - 20 % .. T + 20 %
        lens = [lens[i] for i in torch.randperm(N, generator=g).tolist()]
        videos = [torch.randn(n, 1, 88, 88, generator=g).to(dev) for n in lens]
        if not av:
            return lens, videos
        return lens, [(v, torch.randn(640 * n, 1, generator=g).to(dev)) for v, n in zip(videos, lens)]  # (unit-variance noise)

    def groups_of(lens, batch, max_frames=1600):  # the groups encode_many forms (sizes only)
        sizes, cur = [], 0
        for n in sorted(lens):
            if cur and (cur == batch or (cur + 1) * n > max_frames):
                sizes.append(cur)
                cur = 0
            cur += 1
        return sizes + [cur]

    def stats(ts):
        return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rows = []
    sides = (1, 4, 8) if av else (1, 4, 8, 16)
    top = sides[-1]
    for mode in ("precise", "mixed"):
        AF.set_mode(mode)
        AF.invalidate_weight_cache()
        for T in (100, 400):
            lens, samples = utterances(T)
            ts = {b: [] for b in sides}
            worst = {b: 0.0 for b in sides}
            for rep in range(args.reps + 1):
                base = None
                for b in sides:  # alternated: every repetition visits every side
                    t, encs = timed(lambda: mod.encode_many(samples, batch=b))
                    if rep:
                        ts[b].append(t)
                        continue
                    if b == 1:  # warm-up repetition: the sides must agree
                        base = [e.double() for e in encs]
                    else:
                        worst[b] = max(float((e.double() - r).norm() / r.norm()) for e, r in zip(encs, base))
                        assert worst[b] < 1e-3, (mode, T, b, worst[b])
            for b in sides:
                rows.append({"what": "encoder only", "mode": mode, "T_frames_nominal": T, "lengths_min_max": [min(lens), max(lens)],
                             "utterances": N, "encode_batch": b, "groups": [1] * N if b == 1 else groups_of(lens, b),
                             "ms_for_all": stats(ts[b]),
                             "utterances_per_sec": {k: round(N / (v / 1e3), 2) for k, v in
                                                    (("median", statistics.median(ts[b])), ("min", max(ts[b])), ("max", min(ts[b])))},
                             "speedup_over_one_at_a_time_medians": round(statistics.median(ts[1]) / statistics.median(ts[b]), 3),
                             "max_rel_l2_against_one_at_a_time": None if b == 1 else float(f"{worst[b]:.3g}")})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            del samples
    # the whole decode of eval.py --decode-mode rescore (precise): ModelModule.decode_many without and with encode_batch 16
    AF.set_mode("precise")
    AF.invalidate_weight_cache()
    mod.beam_search = mod._make_beam_search()
    for T in (100, 400):
        lens, samples = utterances(T)
        ts, hyps = {0: [], top: []}, {}
        for rep in range(args.reps + 1):
            for eb in (0, top):
                t, out = timed(lambda: mod.decode_many(samples, workers=1, encode_batch=eb))
                if rep:
                    ts[eb].append(t)
                else:
                    hyps[eb] = out
        for eb in (0, top):
            rows.append({"what": "whole decode, --decode-mode rescore", "mode": "precise", "T_frames_nominal": T, "utterances": N,
                         "encode_batch": eb, "rescore_beam": args.rescore_beam, "rescore_topk": args.rescore_topk, "ms_for_all": stats(ts[eb]),
                         "utterances_per_sec_median": round(N / (statistics.median(ts[eb]) / 1e3), 2),
                         "speedup_over_encode_batch_0_medians": round(statistics.median(ts[0]) / statistics.median(ts[eb]), 3),
                         "hypotheses_equal_encode_batch_0": sum(a == b for a, b in zip(hyps[eb], hyps[0]))})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        del samples
    AF.set_mode("bf16")
    what = ("encoder side of evaluation (two front-ends + proj_encoders + 2 x 12 Conformer layers + fusion head)" if av else
            "encoder side of evaluation (front-end + proj_encoder + 12 Conformer layers)")
    print(json.dumps({"metric": what + " alone: one utterance at a time "
                                "(B = 1, unpadded) against length-exact zero-padded groups (ModelModule.encode_many, max_frames 1600), "
                                + ("audio-visual E2EAV" if av else "video E2E 250M") +
                                f"; then the whole two-pass decode without and with encode_batch {top}",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights; 16 utterances per row, lengths spread +-20 % around T",
                      "timing": f"wall time between device synchronisations; sides alternated inside each of {args.reps} repetitions after one "
                                "warm-up repetition; median [min, max]",
                      "rows": rows}, indent=1))


def main_batch(args):
    import statistics

    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import decoding
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py --batch needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    m = E2E(5049, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    bs = lightning.get_beam_search_decoder(m, [str(i) for i in range(5049)], beam_size=args.beam)
    decoding.NATIVE_BEAM = True
    AF.set_mode("precise")
    N, groups, big = 16, (1, 4, 8, 16), 64 << 30
    rows = []
    for T in (100, 400):
        encs = []
        with torch.no_grad():
            for i in range(N):
                x, _, _ = synth_batch("video", 1, T, 3, 5049, seed=T if i == 0 else 1000 + i, lengths=[T])
                encs.append(m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float())
        sides = {"one_at_a_time": lambda: [bs(e) for e in encs], "forward_many_workers_4": lambda: bs.forward_many(encs, workers=4)}
        for U in groups:
            sides[f"forward_batch_{U}"] = lambda U=U: bs.forward_batch(encs, batch=U, max_workspace_bytes=big)
        # before anything is timed (this is also every side's warm-up): the batched best hypotheses are the one-at-a-time ones
        with torch.no_grad():
            warm = {k: f() for k, f in sides.items()}
        torch.cuda.synchronize()
        assert bs._native
        best = [nb[0].asdict()["yseq"] for nb in warm["one_at_a_time"]]
        for k, res in warm.items():
            assert [nb[0].asdict()["yseq"] for nb in res] == best, f"{k}: best hypotheses differ from the one-at-a-time search (T = {T})"
        ts = {k: [] for k in sides}
        for _ in range(args.reps):  # the sides alternate within a repetition
            for k, f in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    f()
                torch.cuda.synchronize()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        steps = max(len(y) for y in best) - 1
        Ts = [T] * N
        row = {"T_frames": T, "utterances": N, "beam": args.beam, "mode": "precise", "longest_best_hypothesis_tokens": steps, "sides": {}}
        for k, v in ts.items():
            med = statistics.median(v)
            row["sides"][k] = {"ms_total": {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2)},
                               "utterances_per_sec": {"median": round(N / (med / 1e3), 2), "min": round(N / (max(v) / 1e3), 2),
                                                      "max": round(N / (min(v) / 1e3), 2)}}
        for U in groups:
            row["sides"][f"forward_batch_{U}"]["workspace_bytes_per_group"] = bs._native.group_workspace_bytes(Ts[:U], T)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del encs, warm
    AF.set_mode("bf16")
    print(json.dumps({"metric": "batched native hybrid CTC / attention beam search (one decoding step per group of U utterances) beside one search "
                                "at a time and four sessions in flight, video E2E 250M, vocabulary 5049, search only (encoder outputs ready), wall "
                                "clock between synchronisations, one warm-up then the sides alternated",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def main_bias(args):
    import random
    import statistics

    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import decoding
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py --bias needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    V = 5049
    m = E2E(V, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    toks = [str(i) for i in range(V)]
    rng = random.Random(11)
    phrases = [[rng.randint(1, V - 2) for _ in range(rng.randint(2, 5))] for _ in range(1000)]
    w_bias = 1.0
    AF.set_mode("precise")
    rows = []
    for T in (100, 400):
        x, _, _ = synth_batch("video", 1, T, 3, V, seed=T, lengths=[T])
        with torch.no_grad():
            enc = m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float()
        plain = lightning.get_beam_search_decoder(m, toks, beam_size=args.beam)
        decoding.NATIVE_BEAM = True
        with torch.no_grad():
            first = plain(enc)[0].asdict()["yseq"][1:-1]
        # random phrases never meet a hypothesis: a few cut out of the unbiased winner make the list matter (the rest is its bulk)
        hot = [first[i: i + 3] for i in range(0, max(1, len(first) - 3), 7)]
        hot = [p for p in hot if p and all(1 <= t <= V - 2 for t in p)]
        with_list = {"native_bias": lightning.get_beam_search_decoder(m, toks, beam_size=args.beam, bias_phrases=phrases + hot, bias_weight=w_bias),
                     "python_bias": lightning.get_beam_search_decoder(m, toks, beam_size=args.beam, bias_phrases=phrases + hot, bias_weight=w_bias)}
        sides = {"native_no_list": (plain, True), "native_bias": (with_list["native_bias"], True), "python_bias": (with_list["python_bias"], False)}
        times, out = {k: [] for k in sides}, {}
        for rep_ in range(args.reps + 1):  # first repetition = warm-up; the sides alternate within a repetition
            for k, (bs, native) in sides.items():
                decoding.NATIVE_BEAM = native
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    out[k] = bs(enc)
                torch.cuda.synchronize()
                if rep_:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                assert bool(bs._native) == native
        sc = with_list["native_bias"].full_scorers["bias"]
        row = {"T_frames": T, "beam": args.beam, "mode": "precise", "vocabulary": V, "bias_weight": w_bias, "phrases": len(sc.phrases),
               "trie_nodes": sc.n_nodes, "trie_edges": sc.n_edges, "root_fan_out": int(sc.first[1]), "repetitions": args.reps, "sides": {}}
        for k in sides:
            steps = max(len(h.asdict()["yseq"]) for h in out[k]) - 1
            med = statistics.median(times[k])
            row["sides"][k] = {"beam_search_ms": {"median": round(med, 2), "min": round(min(times[k]), 2), "max": round(max(times[k]), 2)},
                               "longest_hypothesis_tokens": steps, "ms_per_token": round(med / max(steps, 1), 4),
                               "best_bias_sum": out[k][0].asdict()["scores"].get("bias")}
        a, b = row["sides"]["native_no_list"]["ms_per_token"], row["sides"]["native_bias"]["ms_per_token"]
        row["list_cost_ms_per_token"] = round(b - a, 4)
        row["list_cost_relative"] = round(b / a - 1.0, 4)
        row["native_and_python_step_agree_on_best"] = out["native_bias"][0].asdict()["yseq"] == out["python_bias"][0].asdict()["yseq"]
        row["list_changes_best"] = out["native_bias"][0].asdict()["yseq"] != out["native_no_list"][0].asdict()["yseq"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    decoding.NATIVE_BEAM = True
    print(json.dumps({"metric": "contextual biasing in the hybrid CTC / attention beam search: native one-call step without and with a list of "
                                "1 000 random 2 - 5-token phrases (plus a few cut out of the unbiased winner), and the python-issued step with it; video "
                                "E2E 250M decoder, search only (encoder output ready), wall clock between synchronisations, one warm-up then "
                                "the sides alternated",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def main_ngram(args):
    import random
    import statistics

    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import decoding
    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E
    from auto_avsr_amd.ngram import NgramScorer

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py --ngram needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    V = 5049
    m = E2E(V, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    toks = [str(i) for i in range(V)]
    w_ngram = 0.3
    AF.set_mode("precise")
    rows = []
    for T in (100, 400):
        x, _, _ = synth_batch("video", 1, T, 3, V, seed=T, lengths=[T])
        with torch.no_grad():
            enc = m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float()
        plain = lightning.get_beam_search_decoder(m, toks, beam_size=args.beam)
        decoding.NATIVE_BEAM = True
        with torch.no_grad():
            first = plain(enc)[0].asdict()["yseq"][1:-1]
        # a random 3-gram model of about 10^6 n-grams; random contexts never meet a hypothesis, so the winner's own n-grams are part of
        # it: the search then stands at bigram contexts and backs off from them (the rest is the model's bulk)
        rng = random.Random(11)
        P = {(t,): -rng.uniform(2.0, 9.0) for t in range(1, V)}
        P[(V,)] = -99.0
        B = {(V,): -0.5}
        seq = [V] + first + [V - 1]
        bis = {tuple(seq[i: i + 2]) for i in range(len(seq) - 1)}
        while len(bis) < 330000:
            bis.add((rng.randint(1, V - 2), rng.randint(1, V - 1)))
        bis = sorted(bis)
        inner = [g for g in bis if g[1] != V - 1]
        tris = {tuple(seq[i: i + 3]) for i in range(len(seq) - 2)}
        while len(tris) < 665000:
            tris.add(rng.choice(inner) + (rng.randint(1, V - 1),))
        for g in bis:
            P[g] = -rng.uniform(0.1, 6.0)
            B.setdefault((g[0],), -rng.uniform(0.05, 2.0))
        for g in tris:
            P[g] = -rng.uniform(0.1, 5.0)
            B.setdefault(g[:2], -rng.uniform(0.05, 2.0))
        sc = NgramScorer(V, P, B, order=3)
        mk = lambda: lightning.get_beam_search_decoder(m, toks, beam_size=args.beam, ngram=sc, ngram_weight=w_ngram)  # noqa: E731
        sides = {"native_no_model": (plain, True), "native_ngram": (mk(), True), "python_ngram": (mk(), False)}
        times, out = {k: [] for k in sides}, {}
        for rep_ in range(args.reps + 1):  # first repetition = warm-up; the sides alternate within a repetition
            for k, (bs, native) in sides.items():
                decoding.NATIVE_BEAM = native
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.no_grad():
                    out[k] = bs(enc)
                torch.cuda.synchronize()
                if rep_:
                    times[k].append((time.perf_counter() - t0) * 1e3)
                assert bool(bs._native) == native
        row = {"T_frames": T, "beam": args.beam, "mode": "precise", "vocabulary": V, "ngram_weight": w_ngram, "order": sc.order,
               "ngrams": len(P), "nodes": sc.n_nodes, "edges": sc.n_edges, "lookup_placement": "inside the selection block",
               "repetitions": args.reps, "sides": {}}
        for k in sides:
            steps = max(len(h.asdict()["yseq"]) for h in out[k]) - 1
            med = statistics.median(times[k])
            row["sides"][k] = {"beam_search_ms": {"median": round(med, 2), "min": round(min(times[k]), 2), "max": round(max(times[k]), 2)},
                               "longest_hypothesis_tokens": steps, "ms_per_token": round(med / max(steps, 1), 4),
                               "best_ngram_sum": out[k][0].asdict()["scores"].get("ngram")}
        a, b = row["sides"]["native_no_model"]["ms_per_token"], row["sides"]["native_ngram"]["ms_per_token"]
        row["model_cost_ms_per_token"] = round(b - a, 4)
        row["model_cost_relative"] = round(b / a - 1.0, 4)
        row["native_and_python_step_agree_on_best"] = out["native_ngram"][0].asdict()["yseq"] == out["python_ngram"][0].asdict()["yseq"]
        row["native_and_python_ngram_sums_bit_equal"] = (out["native_ngram"][0].asdict()["scores"]["ngram"]
                                                         == out["python_ngram"][0].asdict()["scores"]["ngram"])
        row["model_changes_best"] = out["native_ngram"][0].asdict()["yseq"] != out["native_no_model"][0].asdict()["yseq"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    decoding.NATIVE_BEAM = True
    print(json.dumps({"metric": "n-gram shallow fusion in the hybrid CTC / attention beam search: native one-call step without and with a random "
                                "3-gram back-off model of about 10^6 n-grams (plus the n-grams of the model-free winner), and the python-issued "
                                "step with it; video E2E 250M decoder, search only (encoder output ready), wall clock between synchronisations, "
                                "one warm-up then the sides alternated",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def main_two_pass_bias(args):
    import random
    import statistics

    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py --two-pass --bias needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    V = 5049
    m = E2E(V, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    toks = [str(i) for i in range(V)]
    rng = random.Random(11)
    phrases = [[rng.randint(1, V - 2) for _ in range(rng.randint(2, 5))] for _ in range(1000)]
    w_bias = args.bias_weight
    AF.set_mode("precise")
    rows = []
    for T in (100, 400):
        x, _, _ = synth_batch("video", 1, T, 3, V, seed=T, lengths=[T])
        with torch.no_grad():
            enc = m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float()
        plain = lightning.get_two_pass_decoder(m, toks, beam_size=args.rescore_beam, topk=args.rescore_topk)
        with torch.no_grad():
            first = plain(enc)[0].asdict()["yseq"][1:-1]
        # random phrases never meet a hypothesis: a few cut out of the unbiased winner make the list matter (the rest is its bulk)
        hot = [first[i: i + 3] for i in range(0, max(1, len(first) - 3), 7)]
        hot = [p for p in hot if p and all(1 <= t <= V - 2 for t in p)]
        sides = {"no_list": plain, "with_list": lightning.get_two_pass_decoder(m, toks, beam_size=args.rescore_beam, topk=args.rescore_topk,
                                                                               bias_phrases=phrases + hot, bias_weight=w_bias)}
        with torch.no_grad():
            _, hlens, lp = plain._posteriors([enc])
        times, out, rows_of, failed = {k: {"first_pass": [], "whole_decode": []} for k in sides}, {}, {}, {}
        for rep_ in range(args.reps + 1):  # first repetition = warm-up; the sides alternate within a repetition
            for k, tp in sides.items():
                for what, fn in (("first_pass", lambda: tp.first_pass(lp, hlens)), ("whole_decode", lambda: tp(enc))):
                    if (k, what) in failed:
                        continue
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    try:
                        with torch.no_grad():
                            res = fn()
                    except RuntimeError as e:  # (the rescoring pass takes label rows of at most 255 tokens)
                        failed[(k, what)] = str(e)
                        continue
                    torch.cuda.synchronize()
                    if rep_:
                        times[k][what].append((time.perf_counter() - t0) * 1e3)
                    if what == "first_pass":
                        rows_of[k] = int(res[0].shape[2])
                    else:
                        out[k] = res
        sc = sides["with_list"].bias
        row = {"T_frames": T, "beam": args.rescore_beam, "topk": args.rescore_topk, "mode": "precise", "vocabulary": V, "bias_weight": w_bias,
               "phrases": len(sc.phrases), "trie_nodes": sc.n_nodes, "trie_edges": sc.n_edges, "root_fan_out": int(sc.first[1]),
               "repetitions": args.reps, "sides": {}}
        for k in sides:
            row["sides"][k] = {what + "_ms": None if (k, what) in failed else
                               {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
                               for what, ts in times[k].items()}
            row["sides"][k]["longest_label_row"] = rows_of[k]
            row["sides"][k]["best_bias_sum"] = out[k][0].asdict()["scores"].get("bias") if k in out else None
            for what in ("first_pass", "whole_decode"):
                if (k, what) in failed:
                    row["sides"][k][what + "_error"] = failed[(k, what)]
        for what in ("first_pass", "whole_decode"):
            if any((k, what) in failed for k in sides):
                continue
            a, b = (row["sides"][k][what + "_ms"]["median"] for k in ("no_list", "with_list"))
            row[f"list_cost_{what}_ms"] = round(b - a, 3)
            row[f"list_cost_{what}_relative"] = round(b / a - 1.0, 4)
        if len(out) == 2:
            row["list_changes_best"] = out["with_list"][0].asdict()["yseq"] != out["no_list"][0].asdict()["yseq"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    print(json.dumps({"metric": "contextual biasing in two-pass decoding: CTC prefix beam search on the device (first pass) and the whole decode "
                                "(posteriors + first pass + teacher-forced rescoring) without and with a list of 1 000 random 2 - 5-token "
                                "phrases (plus a few cut out of the unbiased winner); video E2E 250M, one utterance per launch, encoder output "
                                "ready, wall clock between synchronisations, one warm-up then the sides alternated",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def main_two_pass_ngram(args):
    import random
    import statistics

    import lightning
    from synth import synth_batch, synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E
    from auto_avsr_amd.ngram import NgramScorer

    if not torch.cuda.is_available():
        raise SystemExit("bench_decode.py --two-pass --ngram needs an MI355X: there is nothing to time without one")
    dev = torch.device("cuda:0")
    V = 5049
    m = E2E(V, "video")
    m.load_state_dict(synth_state_dict(m.state_dict(), 3))
    m = m.to(dev).eval()
    toks = [str(i) for i in range(V)]
    w_ngram, len_bonus = 0.3, 0.5
    AF.set_mode("precise")
    mk = lambda: lightning.get_two_pass_decoder(m, toks, beam_size=args.rescore_beam, topk=args.rescore_topk)  # noqa: E731
    plain = mk()
    encs, firsts = {}, {}
    for T in (100, 400):
        x, _, _ = synth_batch("video", 1, T, 3, V, seed=T, lengths=[T])
        with torch.no_grad():
            encs[T] = m.encoder(m.proj_encoder(m.frontend(x.to(dev))), None)[0].squeeze(0).float()
            _, hlens, lp = plain._posteriors([encs[T]])
            plain.first_pass(lp, hlens)
        res = plain.last_first_pass
        firsts[T] = res["tokens"][0, 0, : int(res["lens"][0, 0])].tolist()
    # the random 3-gram model of --ngram (about 10^6 n-grams); random contexts never meet a hypothesis, so the n-grams of the model-free
    # first-pass winners are part of it: the search then stands at bigram contexts and backs off from them (the rest is the model's bulk)
    rng = random.Random(11)
    P = {(t,): -rng.uniform(2.0, 9.0) for t in range(1, V)}
    P[(V,)] = -99.0
    B = {(V,): -0.5}
    seqs = [[V] + [t for t in f if t != V - 1] + [V - 1] for f in firsts.values()]
    bis = {tuple(q[i: i + 2]) for q in seqs for i in range(len(q) - 1)}
    while len(bis) < 330000:
        bis.add((rng.randint(1, V - 2), rng.randint(1, V - 1)))
    bis = sorted(bis)
    inner = [g for g in bis if g[1] != V - 1]
    tris = {tuple(q[i: i + 3]) for q in seqs for i in range(len(q) - 2)}
    while len(tris) < 665000:
        tris.add(rng.choice(inner) + (rng.randint(1, V - 1),))
    for g in bis:
        P[g] = -rng.uniform(0.1, 6.0)
        B.setdefault((g[0],), -rng.uniform(0.05, 2.0))
    for g in tris:
        P[g] = -rng.uniform(0.1, 5.0)
        B.setdefault(g[:2], -rng.uniform(0.05, 2.0))
    sc = NgramScorer(V, P, B, order=3)
    fused = mk()
    fused.set_ngram(sc, w_ngram, len_bonus=len_bonus)
    sides = {"no_model": plain, "with_model": fused}
    rows = []
    for T in (100, 400):
        enc = encs[T]
        with torch.no_grad():
            _, hlens, lp = plain._posteriors([enc])
        times, out, rows_of, failed = {k: {"first_pass": [], "whole_decode": []} for k in sides}, {}, {}, {}
        for rep_ in range(args.reps + 1):  # first repetition = warm-up; the sides alternate within a repetition
            for k, tp in sides.items():
                for what, fn in (("first_pass", lambda: tp.first_pass(lp, hlens)), ("whole_decode", lambda: tp(enc))):
                    if (k, what) in failed:
                        continue
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    try:
                        with torch.no_grad():
                            res = fn()
                    except RuntimeError as e:  # (the rescoring pass takes label rows of at most 255 tokens)
                        failed[(k, what)] = str(e)
                        continue
                    torch.cuda.synchronize()
                    if rep_:
                        times[k][what].append((time.perf_counter() - t0) * 1e3)
                    if what == "first_pass":
                        rows_of[k] = int(res[0].shape[2])
                    else:
                        out[k] = res
        fp = fused.last_first_pass
        row = {"T_frames": T, "beam": args.rescore_beam, "topk": args.rescore_topk, "mode": "precise", "vocabulary": V, "ngram_weight": w_ngram,
               "len_bonus": len_bonus, "order": sc.order, "ngrams": len(P), "nodes": sc.n_nodes, "edges": sc.n_edges,
               "winner_lookup": "(G', next) of every extension kept in LDS for the frame's winners (no bias list: 65 120 bytes of LDS)", "repetitions": args.reps,
               "nbest_rows_below_the_root": int((fp["ngram_node"][0] != 0).sum()), "sides": {}}
        for k in sides:
            row["sides"][k] = {what + "_ms": None if (k, what) in failed else
                               {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
                               for what, ts in times[k].items()}
            row["sides"][k]["longest_label_row"] = rows_of[k]
            row["sides"][k]["best_ngram_sum"] = out[k][0].asdict()["scores"].get("ngram") if k in out else None
            for what in ("first_pass", "whole_decode"):
                if (k, what) in failed:
                    row["sides"][k][what + "_error"] = failed[(k, what)]
        for what in ("first_pass", "whole_decode"):
            if any((k, what) in failed for k in sides):
                continue
            a, b = (row["sides"][k][what + "_ms"]["median"] for k in ("no_model", "with_model"))
            row[f"model_cost_{what}_ms"] = round(b - a, 3)
            row[f"model_cost_{what}_relative"] = round(b / a - 1.0, 4)
        if len(out) == 2:
            row["model_changes_best"] = out["with_model"][0].asdict()["yseq"] != out["no_model"][0].asdict()["yseq"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    print(json.dumps({"metric": "back-off n-gram model in two-pass decoding: CTC prefix beam search on the device (first pass) and the whole "
                                "decode (posteriors + first pass + teacher-forced rescoring) without and with a random 3-gram model of about "
                                "10^6 n-grams (plus the n-grams of the model-free first-pass winners); video E2E 250M, one utterance per "
                                "launch, encoder output ready, wall clock between synchronisations, one warm-up then the sides alternated",
                      "data": "synthetic input, synthetic (tests/golden/synth.py) weights", "rows": rows}))


def _fixture_trigram(labels, V):
    """A 3-gram estimated on the host from token-id transcripts: absolute discounting (0.5) with back-off to the lower order, add-0.1
    unigrams over the whole vocabulary.  {n-gram: ln p}, {context: ln back-off}; <s> = V, </s> = V - 1."""
    import math
    from collections import Counter, defaultdict

    D = 0.5
    uni, ctx = Counter(), {2: defaultdict(Counter), 3: defaultdict(Counter)}
    for y in labels:
        q = [V] + [int(t) for t in y] + [V - 1]
        uni.update(q[1:])
        for n in (2, 3):
            for i in range(len(q) - n + 1):
                ctx[n][tuple(q[i: i + n - 1])][q[i + n - 1]] += 1
    total = sum(uni.values()) + 0.1 * (V - 1)
    P = {(t,): math.log((uni.get(t, 0) + 0.1) / total) for t in range(1, V)}
    P[(V,)] = -99.0
    B = {}
    for n in (2, 3):
        for h, nxt in ctx[n].items():
            if n == 3 and h not in P:  # (its own context must be an entry one order lower)
                continue
            c = sum(nxt.values())
            for w, k in nxt.items():
                P[h + (w,)] = math.log((k - D) / c)
            B[h] = math.log(D * len(nxt) / c)
    return P, B


def main_two_pass_sweep(args):
    import lightning
    import trained_common as TC
    from synth import synth_state_dict

    from auto_avsr_amd import functional as AF
    from auto_avsr_amd.e2e import E2E

    fx = torch.load(TC.FIXTURE, weights_only=False)
    m = E2E(TC.ODIM, "video", adim=TC.D, aheads=TC.H, eunits=TC.U, elayers=TC.NENC, dunits=TC.U, dlayers=TC.NDEC)
    sd = synth_state_dict(m.state_dict(), TC.SEED)
    sd.update(fx["weights"])
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    toks = [str(i) for i in range(TC.ODIM)]
    AF.set_mode("precise")
    encs = []
    with torch.no_grad():
        for i, u in enumerate(fx["utts"]):
            encs.append(m.encoder(m.proj_encoder(m.frontend(TC.video(i, u["T"]).unsqueeze(0).cuda())), None)[0].squeeze(0).float())
    rows = []
    for W, K in ((8, 8), (16, 8), (16, 16), (32, 16)):
        tp = lightning.get_two_pass_decoder(m, toks, beam_size=W, topk=K)
        dist, contained, natural, ge, same = 0, 0, 0, 0, 0
        t0 = time.perf_counter()
        with torch.no_grad():
            out = tp.forward_many(encs)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for u, nbest in zip(fx["utts"], out):
            got, ref = nbest[0].asdict(), u["hyps"][0]
            dist += TC.edit_distance(u["label"], [int(t) for t in got["yseq"][1:-1]])
            natural += len(ref["yseq"]) - 2 < u["T"]
            contained += any(h.yseq.tolist() == ref["yseq"] for h in nbest)
            ge += got["score"] >= ref["score"] - 1e-3 * max(1.0, abs(ref["score"]))
            same += got["yseq"] == ref["yseq"]
        n = len(fx["utts"])
        rows.append({"beam": W, "topk": K, "nbest": W, "wer": round(dist / fx["total_length"], 4), "reference_search_wer": round(fx["wer"], 4),
                     "utterances": n, "reference_best_natural_ended": natural, "reference_best_in_nbest": contained,
                     "winner_scores_at_least_reference_best": ge, "winner_is_reference_best": same,
                     "one_launch_ms_all_utterances_incl_first_call_overheads": round(dt * 1e3, 1)})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    if args.ngram:  # --two-pass-sweep --ngram: the same sweep with an IN-DOMAIN 3-gram (estimated from the fixture's own transcripts)
        from auto_avsr_amd.ngram import NgramScorer

        P, B = _fixture_trigram([u["label"] for u in fx["utts"]], TC.ODIM)
        sc = NgramScorer(TC.ODIM, P, B, order=3)
        for W, K in ((16, 16), (32, 16)):
            for w, lb in ((0.0, 0.0), (0.3, 0.0), (0.3, 0.5), (0.5, 1.0), (1.0, 1.0), (1.0, 2.0)):
                tp = lightning.get_two_pass_decoder(m, toks, beam_size=W, topk=K)
                tp.set_ngram(sc if w else None, w, len_bonus=lb if w else 0.0)
                with torch.no_grad():
                    out = tp.forward_many(encs)
                dist, dist_first, contained = 0, 0, 0
                fp = tp.last_first_pass
                for b, (u, nbest) in enumerate(zip(fx["utts"], out)):
                    dist += TC.edit_distance(u["label"], [int(t) for t in nbest[0].asdict()["yseq"][1:-1]])
                    dist_first += TC.edit_distance(u["label"], fp["tokens"][b, 0, : int(fp["lens"][b, 0])].tolist())
                    contained += any(h.yseq.tolist() == u["hyps"][0]["yseq"] for h in nbest)
                rows.append({"beam": W, "topk": K, "nbest": W, "ngram_weight": w, "len_bonus": lb if w else 0.0,
                             "model": "3-gram estimated from the fixture's own reference transcripts (in-domain: a sanity ceiling)" if w else None,
                             "nodes": sc.n_nodes if w else 0, "edges": sc.n_edges if w else 0, "wer": round(dist / fx["total_length"], 4),
                             "first_pass_best_wer": round(dist_first / fx["total_length"], 4), "reference_search_wer": round(fx["wer"], 4),
                             "utterances": len(fx["utts"]), "reference_best_in_nbest": contained})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    AF.set_mode("bf16")
    print(json.dumps({"metric": "two-pass decoding on the trained fixture (32 utterances, T = 12 ... 400, reference search: beam 40)", "rows": rows}))


if __name__ == "__main__":
    main()
