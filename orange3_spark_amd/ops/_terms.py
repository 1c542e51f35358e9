"""Operand packing of the 32-row MFMA tile kernels (csrc/mfma_tile.h)."""
import torch


def pad_rows(W: torch.Tensor, rows: int, D: int) -> torch.Tensor:
    """W [k, d] -> fp32 [rows, D] on W's device, zero past k rows and d columns."""
    Wp = torch.zeros((rows, D), dtype=torch.float32, device=W.device)
    Wp[:W.shape[0], :W.shape[1]] = W
    return Wp


def split3(Wp: torch.Tensor) -> torch.Tensor:
    """fp32 Wp -> bf16 [3, *Wp.shape]: hi, mid, lo, each the rounding of the remainder so far."""
    hi = Wp.to(torch.bfloat16)
    r1 = Wp - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo])


def hi_lo(x64: torch.Tensor):
    """fp64 x -> fp32 (hi = fp32(x), lo = fp32(x - hi)); lo = 0 where hi is not finite."""
    hi = x64.float()
    lo = (x64 - hi.double()).float()
    return hi, torch.where(torch.isfinite(hi), lo, torch.zeros_like(lo))
