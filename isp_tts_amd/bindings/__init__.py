"""Tensor-level wrappers of libispk.so by kernel family; import them through `isp_tts_amd.runtime`."""
