"""reference `data/dataset.py` import path -> change3d_amd.data.dataset (see ../README.md)."""
from change3d_amd.data.dataset import *  # noqa: F401,F403
from change3d_amd.data import dataset as _impl

__all__ = [n for n in dir(_impl) if not n.startswith("_")]
globals().update({n: getattr(_impl, n) for n in __all__})
