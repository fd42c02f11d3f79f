"""espnet.nets.scorers.context_bias (import path next to the reference's scorers) -> auto_avsr_amd.bias."""
from auto_avsr_amd.bias import ContextBiasScorer  # noqa: F401
