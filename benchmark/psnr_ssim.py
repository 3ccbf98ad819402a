"""``from psnr_ssim import calculate_psnr, calculate_ssim`` of the reference's Xiph script (benchmark/test_xiph.py) resolves here:
both return numpy fp32 scalars as the reference's do, computed by the fused HIP metric kernel (atm-vfi_amd/metrics.py).  CUDA
tensors only."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module

_metrics = import_module("atm-vfi_amd.metrics")
calculate_psnr = _metrics.calculate_psnr
calculate_ssim = _metrics.calculate_ssim

__all__ = ["calculate_psnr", "calculate_ssim"]
