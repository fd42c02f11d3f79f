"""Evaluation entry point with the reference's command line (eval.py:25-79): loads a checkpoint into ModelModule and
runs the WER loop -- hybrid CTC / attention beam search per utterance (auto_avsr_amd/decoding.py), word-level edit
distance against the reference transcript, WER = total distance / total words (lightning.py:69-84,116-123).

With pytorch_lightning installed the loop is driven by `Trainer.test(model, datamodule)` exactly as in the reference.
Without it (this image) the same three hooks -- on_test_epoch_start / test_step / on_test_epoch_end -- are called
directly over `DataModule.test_dataloader()`.  `--root-dir` selects the reference's on-disk test set; without it the
loader yields `--synthetic-utterances` LRS3-shaped synthetic utterances (plumbing check: random targets, so the WER of an
untrained model is ~1; BASELINE.json configs[0])."""
import logging
from argparse import ArgumentParser


def parse_args(argv=None):
    p = ArgumentParser()
    p.add_argument("--modality", type=str, default="video", choices=["audio", "video", "audiovisual"])
    p.add_argument("--root-dir", type=str, default=None)
    p.add_argument("--test-file", default="lrs3_test_transcript_lengths_seg16s.csv", type=str)
    p.add_argument("--pretrained-model-path", type=str, default=None)
    p.add_argument("--pretrained-video-path", type=str, default=None,
                   help="--modality audiovisual: a video checkpoint whose frontend / proj_encoder / encoder (and heads) initialise the video stack")
    p.add_argument("--pretrained-audio-path", type=str, default=None,
                   help="--modality audiovisual: an audio checkpoint whose frontend / proj_encoder / encoder initialise the audio stack "
                        "(aux_*); its heads are used only without --pretrained-video-path")
    p.add_argument("--decode-snr-target", type=float, default=999999)
    p.add_argument("--debug", action="store_true")
    # extras of this build (not in the reference)
    p.add_argument("--synthetic-utterances", type=int, default=0,
                   help="decode this many synthetic utterances instead of a dataset (default when --root-dir is absent: 4)")
    p.add_argument("--max-test-frames", type=int, default=100, help="length cap of the synthetic utterances")
    p.add_argument("--numerics", choices=["precise", "mixed", "bf16"], default="precise",
                   help="arithmetic of the decoding forward pass: precise (split hi / lo bf16 planes -- hypotheses equal an fp32 run "
                        "of the reference; the default) or bf16 (faster on long utterances)")
    p.add_argument("--decode-workers", type=int, default=1,
                   help="beam searches in flight at once (host threads + streams, one decoding session each); 1 = the reference's "
                        "one-utterance-at-a-time loop")
    p.add_argument("--decode-batch", type=int, default=0, metavar="N",
                   help="decode groups of up to N utterances of similar length with ONE decoding step per group (the batched native "
                        "beam search; utterances are taken in windows of 4 N); 0 = off.  Not with --decode-workers > 1 or "
                        "--decode-mode rescore")
    p.add_argument("--encode-batch", type=int, default=0, metavar="N",
                   help="run front-end and encoder on zero-padded groups of up to N utterances of similar length (length-exact: the "
                        "convolution modules convolve over each utterance's own frames, so the encoder outputs are those of the "
                        "one-at-a-time loop; utterances are taken in windows of 4 N); 0 = off.  Video and audiovisual (inside a "
                        "group the audio trunk zeroes its activations beyond each utterance's length); not audio alone.  Combines "
                        "with every other decoding flag")
    p.add_argument("--timestamps", type=str, default=None, metavar="PATH",
                   help="write one JSON line per utterance with the word timestamps of its hypothesis (CTC forced alignment on the "
                        "device, 40 ms per encoder frame): {utt, hyp, score, words: [{word, start, end}] or null}")
    p.add_argument("--lm-path", type=str, default=None,
                   help="state dict of a Transformer language model (ESPnet TransformerLM layout) for shallow fusion in the beam search")
    p.add_argument("--lm-conf", type=str, default=None,
                   help="JSON file with the language model's layer / unit / att_unit / head / embed_unit (default: 16 / 2048 / 512 / 8 / 128)")
    p.add_argument("--lm-weight", type=float, default=0.0, help="weight of the language model's log-probabilities (0: no fusion)")
    p.add_argument("--bias-list", type=str, default=None, metavar="PATH",
                   help="contextual biasing: a file with one expected phrase per line -- a line of integers is token ids, any other line "
                        "is text (tokenised with the SentencePiece model); a boosted token must still be among the decoder's pre-beam candidates")
    p.add_argument("--bias-weight", type=float, default=0.0, help="reward per matched token of a bias phrase, in log units (0: no biasing)")
    p.add_argument("--ngram-path", type=str, default=None, metavar="PATH",
                   help="n-gram shallow fusion: a back-off n-gram language model as an ARPA text file over the token list's pieces (or over "
                        "token ids, if every word is an integer); it scores the decoder's pre-beam candidates")
    p.add_argument("--ngram-weight", type=float, default=0.0, help="weight of the n-gram model's log-probabilities (0: not used)")
    p.add_argument("--decode-mode", choices=["search", "rescore"], default="search",
                   help="search: the reference's label-synchronous hybrid CTC / attention beam search (default).  rescore: two-pass "
                        "decoding -- a CTC prefix beam search on the device, then one teacher-forced decoder (+ LM) pass over its n-best")
    p.add_argument("--rescore-beam", type=int, default=16, help="--decode-mode rescore: beam (and n-best) of the first pass, 2 .. 64")
    p.add_argument("--rescore-topk", type=int, default=16, help="--decode-mode rescore: non-blank tokens considered per frame, 1 .. 32")
    args = p.parse_args(argv)
    if args.decode_batch < 0:
        p.error("--decode-batch must be >= 0")
    if args.encode_batch < 0:
        p.error("--encode-batch must be >= 0")
    if args.encode_batch > 1 and args.modality == "audio":
        p.error("--encode-batch is for video and audiovisual: the audio front-end's 1-D ResNet trunk is length-aware by now (it is what "
                "audiovisual grouping runs on), but the audio-only refusal is pinned by tests; lifting it is a follow-up")
    if (args.pretrained_video_path or args.pretrained_audio_path) and args.modality != "audiovisual":
        p.error("--pretrained-video-path / --pretrained-audio-path initialise the two stacks of --modality audiovisual")
    if args.decode_batch > 1 and args.decode_workers > 1:
        p.error("--decode-batch and --decode-workers > 1 are two ways of decoding several utterances at once: choose one")
    if args.decode_batch > 1 and args.decode_mode == "rescore":
        p.error("--decode-batch groups the steps of the label-synchronous search: it does not apply to --decode-mode rescore")
    if (args.bias_list or args.bias_weight) and args.decode_mode == "rescore":
        p.error("--bias-list / --bias-weight bias the label-synchronous search: they do not apply to --decode-mode rescore")
    if (args.ngram_path or args.ngram_weight) and args.decode_mode == "rescore":
        p.error("--ngram-path / --ngram-weight fuse the model into the label-synchronous search: they do not apply to --decode-mode rescore")
    return args


def run_test_loop(module, loader, device, log=None, decode_workers=1, timestamps=None, decode_batch=0, encode_batch=0):
    """Trainer.test without Lightning: the module's own hooks over the loader (lightning.py:69-84,116-123).  decode_workers > 1:
    utterances are taken in groups whose beam searches run concurrently (ModelModule.decode_many); same transcripts, same WER.
    decode_batch > 1: utterances are taken in windows of 4 * decode_batch whose searches share their decoding steps in groups of
    at most decode_batch utterances of similar length; same transcripts, same WER.
    encode_batch > 1: the grouped branch as well (windows of 4 * the largest of the three); front-end and encoder run on zero-padded
    groups of at most encode_batch utterances (ModelModule.encode_many), the searches as the other two arguments say.
    timestamps: path of a JSON-lines file that receives, per utterance, the word timestamps of its hypothesis (CTC forced
    alignment on the encoder output the decoding already computed); without it nothing is aligned."""
    import json

    import torch

    from lightning import compute_word_level_distance

    module.on_test_epoch_start()
    records = [] if timestamps else None
    module.timestamp_records = records  # test_step appends to it
    with torch.no_grad():
        if decode_workers <= 1 and decode_batch <= 1 and encode_batch <= 1:
            for i, sample in enumerate(loader):
                sample = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sample.items()}
                module.test_step(sample, i)
                if log is not None:
                    log(i, module.total_edit_distance, module.total_length)
        else:
            group, done = [], 0

            def flush():
                nonlocal done
                for s, predicted in zip(group, module.decode_many([s["input"] if "input" in s else s for s in group], workers=decode_workers, records=records,
                                                                   batch=decode_batch, encode_batch=encode_batch)):
                    actual = module.text_transform.post_process(s["target"])
                    module.total_edit_distance += compute_word_level_distance(actual, predicted)
                    module.total_length += len(actual.split())
                    if log is not None:
                        log(done, module.total_edit_distance, module.total_length)
                    done += 1
                group.clear()

            for sample in loader:
                group.append({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in sample.items()})
                if len(group) == 4 * max(decode_batch, decode_workers, encode_batch):
                    flush()
            if group:
                flush()
    module.timestamp_records = None
    if timestamps:
        with open(timestamps, "w", encoding="utf8") as f:
            for i, rec in enumerate(records):
                f.write(json.dumps({"utt": i, **rec}, ensure_ascii=False) + "\n")
    return module.on_test_epoch_end()


def cli_main(argv=None):
    import torch

    from datamodule.data_module import DataModule
    from lightning import HAVE_LIGHTNING, ModelModule

    args = parse_args(argv)
    from auto_avsr_amd import functional as AF

    AF.set_mode(args.numerics)  # evaluation is forward-only: "precise" here is also what the hpf training mode's forward runs
    logging.basicConfig(format="%(asctime)s %(message)s" if args.debug else "%(message)s",
                        level=logging.DEBUG if args.debug else logging.INFO, datefmt="%Y-%m-%d %H:%M:%S")
    if not torch.cuda.is_available():
        raise SystemExit("eval.py needs an MI355X: the model runs on libavsr_hip.so only (no CPU path)")
    if args.root_dir is None and not args.synthetic_utterances:
        args.synthetic_utterances = 4
    module = ModelModule(args)
    datamodule = DataModule(args)
    if HAVE_LIGHTNING and not args.synthetic_utterances and not args.timestamps:
        from pytorch_lightning import Trainer

        Trainer(num_nodes=1, devices=1, accelerator="gpu").test(model=module, datamodule=datamodule)
        return
    module = module.cuda().eval()
    if args.synthetic_utterances:
        from auto_avsr_amd.synthetic import utterance_lengths
        from datamodule.av_dataset import SyntheticAVDataset

        lens = [min(int(t), args.max_test_frames) for t in utterance_lengths(args.synthetic_utterances, seed=7)]
        loader = torch.utils.data.DataLoader(
            SyntheticAVDataset(len(lens), args.modality, odim=module.model.odim, seed=2, lengths=lens), batch_size=None)
    else:
        loader = datamodule.test_dataloader()
    wer = run_test_loop(module, loader, torch.device("cuda"), decode_workers=args.decode_workers, timestamps=args.timestamps,
                        decode_batch=args.decode_batch, encode_batch=args.encode_batch,
                        log=lambda i, d, n: logging.info(f"utt {i}: running WER {d / max(n, 1):.4f} ({d}/{n} words)"))
    print(f"WER {wer:.4f} over {module.total_length} reference words")
    return wer


if __name__ == "__main__":
    cli_main()
