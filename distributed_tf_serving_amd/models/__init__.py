"""CTR model families (random-init; see ctr.py)."""
from .ctr import DCN, DLRM, FAMILIES, AutoInt, CTRModel, DCNv2, DeepFM, WideDeep, XDeepFM, build_model  # noqa: F401
