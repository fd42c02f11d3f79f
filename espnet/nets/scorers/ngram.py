"""espnet.nets.scorers.ngram (ESPnet's import path of its n-gram scorers) -> auto_avsr_amd.ngram."""
from auto_avsr_amd.ngram import NgramScorer  # noqa: F401
