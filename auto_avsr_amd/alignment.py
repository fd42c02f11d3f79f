"""From a CTC forced alignment (nets.CTC.align / forced_align: one token id per encoder frame) to token segments and word
timestamps.  Host-side bookkeeping only; the trellis itself runs on the device (csrc/ctc_align.hip).

The encoder emits one frame per 40 ms for both modalities (25 fps video; 640 samples of 16 kHz audio)."""

FRAME_SECONDS = 0.04


def _frames(ali, ignore_id):
    if hasattr(ali, "tolist"):
        ali = ali.tolist()
    return [int(a) for a in ali if int(a) != ignore_id]


def segments(ali, blank=0, ignore_id=-1):
    """Frame alignment -> list of (token_id, first_frame, last_frame).  A run of equal non-blank frames is one token; a blank
    between two equal tokens separates them.  Frames that carry ignore_id (beyond the utterance) end the alignment."""
    out = []
    prev = blank
    for t, a in enumerate(_frames(ali, ignore_id)):
        if a != blank:
            if a == prev:
                out[-1] = (a, out[-1][1], t)
            else:
                out.append((a, t, t))
        prev = a
    return out


def word_timestamps(ali, token_list, frame_seconds=FRAME_SECONDS, blank=0, ignore_id=-1):
    """Frame alignment -> list of {"word", "start", "end"} in seconds.  SentencePiece pieces are merged into words by the rule
    TextTransform.post_process implies (pieces joined, "▁" becomes a space): a piece that starts with "▁" opens a word.
    start = first frame of the word's first piece * frame_seconds, end = (last frame of its last piece + 1) * frame_seconds."""
    words = []
    for tok, first, last in segments(ali, blank, ignore_id):
        piece = token_list[tok]
        if piece.startswith("▁") or not words:
            words.append({"word": "", "start": first * frame_seconds, "end": (last + 1) * frame_seconds})
        w = words[-1]
        w["word"] += piece
        w["end"] = (last + 1) * frame_seconds
    for w in words:
        w["word"] = w["word"].replace("▁", " ").strip()
    return [w for w in words if w["word"]]
