"""Import path that ESPnet `rnnlm_conf` files name as `model_module` (espnet/nets/pytorch_backend/lm/transformer.py); implementation: auto_avsr_amd.lm (HIP kernels)."""
from auto_avsr_amd.lm import TransformerLM  # noqa: F401
