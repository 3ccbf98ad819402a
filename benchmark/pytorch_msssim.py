"""``from pytorch_msssim import ssim_matlab`` of the reference's evaluation scripts (benchmark/test_vimeo90k.py, test_ucf101.py,
test_snufilm.py) resolves here: the reference's signature and return types, computed by the fused HIP metric kernel
(atm-vfi_amd/metrics.py).  CUDA tensors only; the 2-D ``ssim`` / ``msssim`` of the reference module are not provided."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module

_metrics = import_module("atm-vfi_amd.metrics")
ssim_matlab = _metrics.ssim_matlab

__all__ = ["ssim_matlab"]
