#!/usr/bin/env python
"""FFHQ frame-sequence editing on MI355X — the flow of the reference's scripts/video_editing.py on the unconditional FFHQ
model (afldm_amd LDMVideoPipeline: DDIM inversion of every frame with cross-frame attention to the keyframes - or, with
--sdedit, the noised frames - then one STORE pass over the keyframes and LOAD passes over all frames).

--input is a directory of images (sorted by name) or an animated GIF; frames are resized to the model's size.  No network on
the target machines: pass --ckpt /path/to/alias_free_ldm_ffhq (diffusers-format directory with unet/, scheduler/, vae/) or
--random-init for seeded random weights of the FFHQ architecture and seeded synthetic frames (demonstrates the full flow; the
pictures are noise).  Writes the edited frames as one GIF."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp", ".webp")


def _keyframes(text):
    try:
        return tuple(int(k) for k in text.split(","))
    except ValueError:
        raise argparse.ArgumentTypeError(f"--keyframes takes comma-separated frame indices, got {text!r}")


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--input", type=str, default=None, help="a directory of images (sorted by name) or an animated GIF")
    p.add_argument("--output_path", type=str, default="results/video_edit.gif")
    p.add_argument("--n-frames", type=int, default=16, help="use the first N frames of the input (or make N synthetic ones)")
    p.add_argument("--n_steps", type=int, default=50)
    p.add_argument("--strength", type=float, default=-1.0,
                   help="< 0: the whole schedule; in (0, 1]: the last int(n_steps * strength) steps (the reference's get_timesteps)")
    p.add_argument("--sdedit", action="store_true", help="start from the noised frames (needs --strength > 0) instead of their inversion")
    p.add_argument("--keyframes", type=_keyframes, default=(0,),
                   help="comma-separated, sorted frame indices beginning with 0 whose attention maps are stored; a frame between "
                        "two keyframes attends to both, blended by its position in time (default 0: the reference's anchor frame)")
    p.add_argument("--frame-batch", type=int, default=16, help="frames per LOAD graph replay")
    p.add_argument("--ckpt", type=str, default=os.environ.get("AFLDM_CKPT"))
    p.add_argument("--random-init", action="store_true",
                   help="seeded random weights of the FFHQ architecture; without --input also seeded synthetic frames")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--eager", action="store_true",
                   help="run the passes as the eager loop that follows the reference statement by statement instead of replayed "
                        "HIP graphs")
    p.add_argument("--timings", type=str, default=None, metavar="FILE.json",
                   help="run the call twice (the first captures the graphs) and write both wall times, synchronised, as JSON")
    args = p.parse_args(argv)
    if args.n_frames < 1:
        p.error("--n-frames must be >= 1")
    if args.frame_batch < 1:
        p.error("--frame-batch must be >= 1")
    if args.sdedit and not args.strength > 0:
        p.error("--sdedit needs --strength > 0")
    if not args.random_init and not args.ckpt:
        p.error("pass --ckpt (or --random-init for seeded random weights)")
    if not args.input and not args.random_init:
        p.error("pass --input (or --random-init for synthetic frames)")
    return args


def synthetic_frames(seed, n, size=256):
    """n smooth seeded frames [n, 3, size, size] in [-1, 1]: one random 8 x 8 colour field drifting towards another."""
    g = torch.Generator().manual_seed(seed)
    a, b = (torch.rand(1, 3, 8, 8, generator=g) * 2 - 1 for _ in range(2))
    fields = torch.cat([a + (b - a) * (f / max(n - 1, 1)) for f in range(n)])
    return torch.nn.functional.interpolate(fields, size=(size, size), mode="bicubic", align_corners=False).clamp(-1, 1)


def load_frames(path, n, size):
    """The first n frames of a directory of images or of a GIF, as PIL RGB images of size x size."""
    from PIL import Image, ImageSequence
    if os.path.isdir(path):
        names = sorted(f for f in os.listdir(path) if f.lower().endswith(IMAGE_SUFFIXES))
        frames = [Image.open(os.path.join(path, f)).convert("RGB") for f in names[:n]]
    else:
        with Image.open(path) as im:
            frames = [fr.convert("RGB") for _, fr in zip(range(n), ImageSequence.Iterator(im))]
    if not frames:
        raise SystemExit(f"{path}: no frames found")
    return [f if f.size == (size, size) else f.resize((size, size), Image.LANCZOS) for f in frames]


def build_pipeline(args):
    from afldm_amd.pipelines.video_editing_pipeline import LDMVideoPipeline
    if args.ckpt:
        return LDMVideoPipeline.from_pretrained(args.ckpt)
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import image_interpolation_ffhq as base          # the same seeded FFHQ-architecture UNet and AF-VAE
    return LDMVideoPipeline(**base.build_pipeline(args).components)


def main(argv=None):
    args = parse_args(argv)
    from afldm_amd.af_modules.af_api import make_af_unet, make_af_vae_from_config
    from afldm_amd.io_utils import save_gif_from_tensors
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    pipe = build_pipeline(args).to("cuda").to(dtype)
    pipe.set_progress_bar_config(disable=True)
    make_af_unet(pipe.unet)
    make_af_vae_from_config(pipe.vae)
    size = pipe.unet.config.sample_size * pipe._vae_ratio()
    frames = load_frames(args.input, args.n_frames, size) if args.input else synthetic_frames(args.seed, args.n_frames, size)

    def call():
        return pipe(frames, num_inference_steps=args.n_steps, strength=args.strength, use_sdedit=args.sdedit,
                    keyframes=args.keyframes, generator=torch.Generator().manual_seed(args.seed), frame_batch=args.frame_batch,
                    output_type="pt", use_graph=not args.eager)
    walls = []
    for _ in range(2 if args.timings else 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    if args.timings:
        os.makedirs(os.path.dirname(os.path.abspath(args.timings)), exist_ok=True)
        with open(args.timings, "w") as f:
            json.dump({"frames": int(out.shape[0]), "steps": args.n_steps, "strength": args.strength, "keyframes": list(args.keyframes),
                       "frame_batch": args.frame_batch, "dtype": args.dtype, "graph": not args.eager, "first_call_s": walls[0],
                       "second_call_s": walls[1]}, f)
    save_gif_from_tensors(list(out.float().cpu()), args.output_path, denorm=True)
    print(f"wrote {args.output_path}: {out.shape[0]} frames of {tuple(out.shape[1:])}" +
          (f"; calls took {walls[0]:.3f} s and {walls[1]:.3f} s" if args.timings else ""))
    return out


if __name__ == "__main__":
    main()
