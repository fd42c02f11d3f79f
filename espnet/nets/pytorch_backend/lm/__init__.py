"""Import-path shim: the ESPnet layout re-exported from auto_avsr_amd (see auto_avsr_amd/lm.py)."""
