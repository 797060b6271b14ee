"""A built-in optical-flow estimator on MI355X, so that the flow-guided interpolation modes (warp_method 0 / 1 / 2) can be
reached from two images alone.

The reference estimates flow with GMFlow (flow_utils.py:182-193, `predict_flow`), a trained network whose weights are not
available here.  PyramidLKFlow is NOT GMFlow and is not pinned to the reference: it is a classical, deterministic estimator
this project defines — dense pyramidal Lucas-Kanade with Tikhonov damping and iterative warping — and
its flows differ from a learned estimator's (no occlusion reasoning, displacements bounded by the pyramid).  Its oracle is the
float64 restatement of the same arithmetic in tests/flowest_oracle.py.  It is opt-in: nothing uses it unless a caller builds
one and hands it to predict_flow or to LDMInterpolationPipeline(flow_model=...).

  1. pyramid: level l + 1 = level l filtered with [1, 3, 3, 1] / 8 along each axis, decimated by 2    (afldm_flowest_pyr_down)
  2. u = 0 at the coarsest level; to a finer level u <- 2 * bilinear_up2(u)                            (afldm_flowest_up2)
  3. `iters` times per level: one damped LK step on I1 and I2 warped along u                         (afldm_flowest_lk_step)
  4.   followed by a [1, 4, 6, 4, 1] / 16 smoothing of u                                               (afldm_flowest_smooth)

predict_flow keeps the reference's signature and output convention.  get_warped_and_mask and alpha_warp stay absent: they
need flow_warp2, which this project does not have."""
import math

import torch

from .. import ops
from .flow_utils import forward_backward_consistency_check

MAX_CHANNELS, MAX_RADIUS = 4, 4          # the limits of afldm_flowest_lk_step


def default_levels(H, W):
    """log2(min(H, W)) - 2: the coarsest level's shorter side is 8 for a power-of-two image."""
    return max(int(math.log2(min(H, W))) - 2, 1)


class PyramidLKFlow:
    """flow = PyramidLKFlow(levels=None, iters=3, radius=3, lam=1e-3); fwd, bwd = flow(image1, image2).

    image1, image2: [N, C, H, W] device tensors (fp32 or bf16, C <= 4, values in [-1, 1]; H and W divisible by
    2^(levels - 1)).  fwd, bwd: fp32 [N, 2, H, W], channel 0 = ROW displacement, with image2(p + fwd(p)) ~ image1(p) and
    image1(p + bwd(p)) ~ image2(p); both come from one batched run over the pairs (image1 -> image2, image2 -> image1).
    levels=None takes default_levels(H, W).  The pyramids and two ping-pong flow buffers per level are cached per shape;
    the call issues kernel launches only (no host synchronisation), so it can be captured in a HIP graph and replayed on new
    image contents.  Two calls on the same input agree bit for bit."""

    def __init__(self, levels=None, iters=3, radius=3, lam=1e-3):
        if levels is not None and (not isinstance(levels, int) or levels < 1):
            raise ValueError(f"levels must be an integer >= 1 (or None), got {levels!r}")
        if not isinstance(iters, int) or iters < 1:
            raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
        if not isinstance(radius, int) or not 1 <= radius <= MAX_RADIUS:
            raise ValueError(f"radius must be an integer in [1, {MAX_RADIUS}] (the window is (2 radius + 1)^2), got {radius!r}")
        if not lam > 0:
            raise ValueError(f"lam must be positive (it keeps the 2 x 2 system regular), got {lam!r}")
        self.levels, self.iters, self.radius, self.lam = levels, iters, radius, float(lam)
        self._ws = {}

    def _check(self, image1, image2):
        for name, im in (("image1", image1), ("image2", image2)):
            if not torch.is_tensor(im) or im.dim() != 4:
                raise ValueError(f"{name} must be a tensor [N, C, H, W], got {tuple(im.shape) if torch.is_tensor(im) else type(im).__name__}")
        if image1.shape != image2.shape or image1.dtype != image2.dtype:
            raise ValueError(f"image1 and image2 must share shape and dtype, got {tuple(image1.shape)} {image1.dtype} and "
                             f"{tuple(image2.shape)} {image2.dtype}")
        N, C, H, W = image1.shape
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"C = {C}: 1 to {MAX_CHANNELS} channels are supported")
        levels = default_levels(H, W) if self.levels is None else self.levels
        if H % (1 << (levels - 1)) or W % (1 << (levels - 1)) or min(H, W) >> (levels - 1) < 1:
            raise ValueError(f"H = {H} and W = {W} must be divisible by 2^(levels - 1) = {1 << (levels - 1)}")
        for name, im in (("image1", image1), ("image2", image2)):
            if not im.is_cuda:
                raise RuntimeError(f"afldm_amd: {name} must live on an MI355X (cuda) device; there is no CPU path")
        return N, C, H, W, levels

    def _workspace(self, key):
        ws = self._ws.get(key)
        if ws is None:
            N, C, H, W, levels, device = key
            f32 = dict(dtype=torch.float32, device=device)
            # planes of a level: [image1; image2; image2; image1]: the first half is I1 of the batched pair, the second I2
            pyr = [torch.empty((4 * N, C, H >> l, W >> l), **f32) for l in range(levels)]
            flows = [(torch.empty((2 * N, 2, H >> l, W >> l), **f32), torch.empty((2 * N, 2, H >> l, W >> l), **f32))
                     for l in range(levels)]
            ws = self._ws[key] = (pyr, flows)
        return ws

    @torch.no_grad()
    def __call__(self, image1, image2):
        N, C, H, W, levels = self._check(image1, image2)
        image1, image2 = image1.contiguous(), image2.contiguous()
        pyr, flows = self._workspace((N, C, H, W, levels, image1.device))
        for slot, im in enumerate((image1, image2, image2, image1)):
            ops.flowest_pyr_down(im, factor=1, out=pyr[0][slot * N:(slot + 1) * N])
        for l in range(1, levels):
            ops.flowest_pyr_down(pyr[l - 1], out=pyr[l])
        out = torch.empty((2 * N, 2, H, W), dtype=torch.float32, device=image1.device)
        flows[levels - 1][0].zero_()
        for l in range(levels - 1, -1, -1):
            u, tmp = flows[l]
            if l < levels - 1:
                ops.flowest_up2(flows[l + 1][0], out=u)
            I1, I2 = pyr[l][:2 * N], pyr[l][2 * N:]
            for it in range(self.iters):
                ops.flowest_lk_step(I1, I2, u, self.radius, self.lam, out=tmp)
                ops.flowest_smooth(tmp, out=out if (l == 0 and it == self.iters - 1) else u)
        return out[:N], out[N:]


@torch.no_grad()
def predict_flow(flow_model, image1, image2):
    """The reference's predict_flow (flow_utils.py:182-193) for an estimator of this module: (fwd_flow, fwd_occ, bwd_flow,
    bwd_occ) with the flows [1, 2, H, W] fp32 in the reference's output convention (channel 0 = x displacement: what
    LDMInterpolationPipeline takes as flows=) and the occlusion masks [1, 1, H, W] from forward_backward_consistency_check,
    called on the returned flows as the reference calls it (:191).  flow_model(image1, image2) returns (fwd, bwd) with channel
    0 = row displacement (PyramidLKFlow); no padding is needed (the reference pads to a multiple of 8 for GMFlow)."""
    for name, im in (("image1", image1), ("image2", image2)):
        if not torch.is_tensor(im) or im.dim() != 4 or im.shape[0] != 1:
            raise ValueError(f"predict_flow takes two image tensors [1, C, H, W]: {name} is "
                             f"{tuple(im.shape) if torch.is_tensor(im) else type(im).__name__}")
    if image1.shape != image2.shape:
        raise ValueError(f"predict_flow: image1 {tuple(image1.shape)} and image2 {tuple(image2.shape)} must have one shape")
    fwd, bwd = flow_model(image1, image2)
    fwd_flow, bwd_flow = torch.flip(fwd, (1,)).contiguous(), torch.flip(bwd, (1,)).contiguous()
    fwd_occ, bwd_occ = forward_backward_consistency_check(fwd_flow, bwd_flow)
    return fwd_flow, fwd_occ, bwd_flow, bwd_occ
