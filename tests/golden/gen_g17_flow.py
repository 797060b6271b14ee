#!/usr/bin/env python
"""Records tests/golden/g17_flow.npz: inputs and outputs of the reference's flow utilities
(afldm/shift_utils/flow_utils.py, flow_utils_np.py) on a few 32^2 / 64^2 cases.

    python tests/golden/gen_g17_flow.py --reference /path/to/reference/checkout

Runs on the CPU only, never on a GPU machine.  numba is not needed: a stand-in module whose `njit` returns the function
unchanged is installed first, so the reference's loops run as plain Python (seconds at these sizes).  Only the recorded
arrays are kept; nothing of the reference's text is.  Draws the reference takes from the global RNG are recorded by
re-seeding: torch.manual_seed(k) in front of the call and in front of an identical draw that is saved."""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def smooth_flow(H, A, sign, seed_phase=0.0):
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(H, dtype=np.float64), indexing="ij")
    f0 = sign * A * np.sin(2 * np.pi * (i / H + 0.3 * j / H) + 0.4 + seed_phase)
    f1 = sign * A * np.cos(2 * np.pi * (j / H - 0.2 * i / H) + 1.1 + seed_phase)
    return np.stack([f0, f1]).astype(np.float32)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--out", default=os.path.join(HERE, "g17_flow.npz"))
    args = ap.parse_args()
    stand_in = types.ModuleType("numba")
    stand_in.njit = lambda f=None, *a, **k: f if callable(f) else (lambda g: g)
    sys.modules["numba"] = stand_in
    sys.path.insert(0, args.reference)
    from afldm.shift_utils import flow_utils as rf

    g = torch.Generator().manual_seed(17)
    out = {}

    # forward_flow_warp: a random flow (sources leave through every border), a smooth one that drives sources across the top / left border
    for name, H, C, flow in (("rand32", 32, 3, torch.randn(1, 2, 32, 32, generator=g) * 2.5),
                             ("neg64", 64, 2, torch.from_numpy(smooth_flow(64, 3.0, -1.0)))):
        x = torch.randn(1, C, H, H, generator=g)
        res, occ = rf.forward_flow_warp(x, flow)
        out.update({f"splat_{name}_x": x.numpy(), f"splat_{name}_flow": flow.numpy(), f"splat_{name}_res": res.numpy(),
                    f"splat_{name}_occ": occ.numpy()})

    # forward_upsample_flow_warp: 8^2 -> 64^2 by the ideal filter, warp, every 8th pixel
    x = torch.randn(1, 2, 8, 8, generator=g)
    flow = torch.from_numpy(smooth_flow(64, 5.0, -1.0, 0.7))
    res, occ = rf.forward_upsample_flow_warp(x, flow, scale=8)
    out.update(upwarp_x=x.numpy(), upwarp_flow=flow.numpy(), upwarp_res=res.numpy(), upwarp_occ=occ.numpy())

    # upsample_noise, collect_noise_pixel, continuous_noise_fwd_warp with their draws recorded (4^2 -> 32^2; the latter two on upnoise_y)
    x = torch.randn(1, 2, 4, 4, generator=g)
    torch.manual_seed(101)
    hi = rf.upsample_noise(x, 8)
    torch.manual_seed(101)
    out.update(upnoise_x=x.numpy(), upnoise_z=torch.randn(1, 2, 32, 32).numpy(), upnoise_y=hi.numpy())
    occ = (torch.rand(1, 1, 32, 32, generator=g) < 0.1).float()
    torch.manual_seed(102)
    y = rf.collect_noise_pixel(hi, occ, 8)
    torch.manual_seed(102)
    out.update(collect_occ=occ.numpy(), collect_z=torch.randn_like(hi).numpy(), collect_y=y.numpy())
    flow = torch.from_numpy(smooth_flow(32, 8.0, -1.0, 0.2))
    torch.manual_seed(103)
    y = rf.continuous_noise_fwd_warp(hi, flow, 0.375, 8)
    torch.manual_seed(103)
    out.update(cnfw_flow=flow.numpy(), cnfw_alpha=np.float32(0.375), cnfw_z=torch.randn_like(hi).numpy(),
               cnfw_y=y.numpy())

    # flow_warp (bilinear with mask, nearest) at 32^2: a fractional field that leaves the plane at the borders, and
    # integer + 0.25 for nearest
    x = torch.randn(2, 3, 32, 32, generator=g)
    flow = torch.randn(2, 2, 32, 32, generator=g) * 3
    y, m = rf.flow_warp(x, flow, mask=True)
    qflow = torch.randint(-4, 5, (2, 2, 32, 32), generator=g).float() + 0.25
    out.update(warp_x=x.numpy(), warp_flow=flow.numpy(), warp_y=y.numpy(), warp_mask=m.numpy(), warp_qflow=qflow.numpy(),
               warp_ynear=rf.flow_warp(x, qflow, mode="nearest").numpy())

    # get_patch_moving_flow and forward_backward_consistency_check on a consistent pair: a patch moved by (5, -7) and back
    tmpl = torch.zeros(1, 3, 64, 64)
    box, disp = (12, 36, 24, 50), (5, -7)
    bwd, bwd_occ = rf.get_patch_moving_flow(tmpl, box, disp)
    half, half_occ = rf.get_patch_moving_flow(tmpl, box, disp, alpha=0.5)
    fwd = torch.zeros(1, 2, 64, 64)
    fwd[:, 0, box[0]:box[1], box[2]:box[3]] = disp[0]
    fwd[:, 1, box[0]:box[1], box[2]:box[3]] = disp[1]
    f_occ, b_occ = rf.forward_backward_consistency_check(fwd, bwd)
    out.update(patch_box=np.array(box), patch_disp=np.array(disp), patch_bwd=bwd.numpy(), patch_bwd_occ=bwd_occ.numpy(),
               patch_half=half.numpy(), patch_half_occ=half_occ.numpy(), patch_fwd=fwd.numpy(), fb_fwd_occ=f_occ.numpy(),
               fb_bwd_occ=b_occ.numpy())
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {len(out)} arrays, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
