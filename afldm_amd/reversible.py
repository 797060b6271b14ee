"""ReversibleCode — what the bit-reversible sampler (engine.ReversibleEngine, MyLDMPipeline.sample_reversible / invert_reversible)
hands back and takes: two adjacent states of the trajectory as int64 fixed point on the grid 2^-32, and a record of everything the
bit-for-bit guarantee depends on."""
from dataclasses import dataclass, fields, replace

import torch

GRID_BITS = 32          # an int64 X stands for X 2^-32 (Q31.32)


def decode(X):
    """The fp32 view of int64 fixed-point latents: rn_f32(X) 2^-32 - one int64 -> fp32 rounding to nearest even and an exact
    power-of-two scale, on whatever device X lives; the operations the kernels use."""
    return X.to(torch.float32) * 2.0 ** -GRID_BITS


@dataclass(frozen=True, eq=False)
class ReversibleCode:
    """hi = X_k and lo = X_{k-1}, int64 [B, C, H, W]; k is N at the noise end (what inverting returns and sampling takes) and 1 at
    the image end (what sampling returns and inverting takes).  num_inference_steps and strength say which levels; batch, dtype,
    model_key (engine.model_state_key of the UNet: valid within the process that made it) and library (_lib.library_hash) say what
    made the bits: the UNet's plans differ per batch size, so another batch size, dtype, set of weights or build of the library
    gives other roundings, and inverting then no longer undoes sampling exactly."""
    hi: torch.Tensor
    lo: torch.Tensor
    k: int
    num_inference_steps: int
    strength: object
    batch: int
    dtype: torch.dtype
    model_key: int
    library: str

    def latents(self):
        """The lower state X_{k-1} as fp32 latents (for k = 1: the sample)."""
        return decode(self.lo)

    def to(self, device):
        return replace(self, hi=self.hi.to(device), lo=self.lo.to(device))

    def cpu(self):
        return self.to("cpu")

    def __getitem__(self, rows):
        """The code of some samples (a slice or an index list).  `batch` stays the batch size that made the bits."""
        rows = slice(rows, rows + 1) if isinstance(rows, int) else rows
        return replace(self, hi=self.hi[rows].contiguous(), lo=self.lo[rows].contiguous())

    def __reduce__(self):          # (torch.save / torch.load: the class called on its fields)
        return ReversibleCode, tuple(getattr(self, f.name) for f in fields(self))

    def mismatches(self, **want):
        """The recorded fields that differ from `want`, as [(name, recorded, wanted)]."""
        return [(k, getattr(self, k), v) for k, v in want.items() if getattr(self, k) != v]


if hasattr(torch.serialization, "add_safe_globals"):
    torch.serialization.add_safe_globals([ReversibleCode])
