"""CPU oracle of self-attention guidance (Hong et al., ICCV 2023; diffusers StableDiffusionSAGPipeline restricted to an unconditional
UNet, epsilon prediction, no clipping) on the oracle UNet (oracle/unet.py, which is not edited: its attention core is wrapped while
a context manager is open).  Written in diffusers' form:

    e        = UNet(x, t)                                  at ONE site the probabilities P [B, heads, T, T] are observed
    mass     = P.mean(1).sum(1)                            [B, T], per key
    M        = F.interpolate((mass > 1).view(B, 1, hm, hm) repeated over the channels, (H, W))      (nearest)
    x0       = p x + q e                                   p = 1 / sqrt(abar), q = -sqrt(1 - abar) / sqrt(abar)
    degraded = gaussian_blur_2d(x0, 9, 1.0) M + x0 (1 - M)
    x_d      = add_noise(degraded, noise = e, t) = sqrt(abar) degraded + sqrt(1 - abar) e
    e_d      = UNet(x_d, t)
    g        = e + s (e - e_d), then pag_oracle.pag_step's row

`degrade_product_form` is the product's algebraically equal x_d = x + M (G x0 - x0) / p, for the host test that compares the two
in float64."""
import contextlib

import torch
import torch.nn.functional as F

import pag_oracle as po
from oracle import unet as ou


def gaussian_window(kernel_size=9, sigma=1.0, dtype=torch.float64):
    """diffusers gaussian_blur_2d's 1-D window."""
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size, dtype=dtype)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur_2d(img, window, boundary="reflect"):
    """diffusers gaussian_blur_2d with the window given: the 2-D outer-product kernel, F.pad (mode 'reflect' as diffusers, or
    'circular'), a grouped F.conv2d."""
    n = window.numel()
    window = window.to(img.dtype)
    kernel = torch.mm(window[:, None], window[None, :]).expand(img.shape[-3], 1, n, n)
    img = F.pad(img, [n // 2] * 4, mode=boundary)
    return F.conv2d(img, kernel, groups=img.shape[-3])


def upsampled_mask(mask, H, W):
    """mask bool [B, T] -> float64 [B, 1, H, W] by nearest up-sampling of the [hm, hm] map, as diffusers' sag_masking."""
    B, T = mask.shape
    hm = int(round(T ** 0.5))
    assert hm * hm == T
    return F.interpolate(mask.view(B, 1, hm, hm).double(), (H, W))


def degrade(x, e, mask, p, q, window, boundary="reflect"):
    """diffusers' form, float64: x, e [B, C, H, W]; mask bool [B, T]."""
    x, e = x.double(), e.double()
    p, q = float(p), float(q)
    sqrt_ab, sqrt_1mab = 1.0 / p, -q / p
    M = upsampled_mask(mask, *x.shape[-2:])
    x0 = p * x + q * e
    degraded = gaussian_blur_2d(x0, window, boundary) * M + x0 * (1.0 - M)
    return sqrt_ab * degraded + sqrt_1mab * e


def degrade_product_form(x, e, mask, p, q, window, boundary="reflect"):
    """The product's form, float64: x_d = x + M (G x0 - x0) / p."""
    x, e = x.double(), e.double()
    p, q = float(p), float(q)
    M = upsampled_mask(mask, *x.shape[-2:])
    x0 = p * x + q * e
    return x + M * (gaussian_blur_2d(x0, window, boundary) - x0) / p


def key_mass(q, k, heads, scale=None):
    """mass [B, T] float64 from q, k [B, T, heads * d]: softmax(scale q k^T).mean(heads).sum(queries)."""
    B, T, C = q.shape
    d = C // heads
    scale = d ** -0.5 if scale is None else scale
    qh = q.double().view(B, T, heads, d).transpose(1, 2)
    kh = k.double().view(B, T, heads, d).transpose(1, 2)
    P = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return P.mean(1).sum(1)


@contextlib.contextmanager
def observed_attention(site):
    """While open, oracle.unet's attention core also records, at the module `site` (a full module path), the attention mass of
    every key - from the block's own q and k, the probabilities in float64 - in the yielded dict under "mass" (and how often the
    site ran under "calls"); the block's result is the original core's.  The original is put back on exit, also on an
    exception."""
    original = ou._attention_core
    seen = {"calls": 0}

    def core(c, prefix, x, kv_src):
        if prefix == site:
            assert kv_src is None, "SAG observes plain self-attention"
            sd, cfg = c.sd, c.cfg
            b, ch, hh, ww = x.shape
            heads = ch // cfg["attention_head_dim"]
            h = F.group_norm(x.view(b, ch, hh * ww), c.groups, sd[prefix + ".group_norm.weight"], sd[prefix + ".group_norm.bias"],
                             c.eps).transpose(1, 2)
            q = F.linear(h, sd[prefix + ".to_q.weight"], sd[prefix + ".to_q.bias"])
            k = F.linear(h, sd[prefix + ".to_k.weight"], sd[prefix + ".to_k.bias"])
            seen["mass"] = key_mass(q, k, heads)
            seen["calls"] += 1
        return original(c, prefix, x, kv_src)

    ou._attention_core = core
    try:
        yield seen
    finally:
        ou._attention_core = original


def sample(sd, cfg, x, schedule, site, window=None, boundary="reflect", draw=None):
    """The float64 loop over a "sag" (or "pag") Schedule: the oracle UNet (fp32, CPU) evaluated with the site observed, the
    degradation in diffusers' form, the oracle UNet again, then pag_oracle.pag_step.  draw(): the next noise tensor, called once
    per step that draws, in step order.  Returns (latents float64, [mass float64 [B, T] per step])."""
    window = gaussian_window() if window is None else window
    z = x.double() * schedule.init_noise_sigma
    masses = []
    for k, (t, row) in enumerate(zip(schedule.timesteps, schedule.rows)):
        noise = draw() if schedule.slots(k) else None
        with observed_attention(site) as seen:
            e = ou.unet_forward(sd, cfg, z.float(), int(t))
        assert seen["calls"] == 1
        masses.append(seen["mass"])
        z_d = degrade(z, e, seen["mass"] > 1.0, row[0], row[1], window, boundary)
        e_d = ou.unet_forward(sd, cfg, z_d.float(), int(t))
        z = po.pag_step(z, e, e_d, noise, row)
    return z, masses


def margin(masses):
    """min |mass - 1| over every step, sample and key."""
    return min(float((m - 1.0).abs().min()) for m in masses)


# The closed-loop fp32 configurations of tests/test_gpu_sag_pipeline.py: (site, seed of the start latents, steps, B, sag_scale, eta,
# seed of the noise generator).  tests/test_sag_host.py asserts the margin condition for every one of them on the CPU.
LATENT_SHAPE = (4, 16, 16)
CLOSED_LOOPS = {
    "up": ("up_blocks.1.attentions.0", 2, 4, 2, 0.75, 0.0, 13),
    "mid": ("mid_block.attentions.0", 4, 4, 2, 0.75, 0.0, 13),
    "mid_s3": ("mid_block.attentions.0", 4, 4, 2, 3.0, 0.0, 13),
}
MARGIN = 1e-4


def start_latents(seed, B):
    return torch.randn(B, *LATENT_SHAPE, generator=torch.Generator().manual_seed(seed))


_RUNS = {}


def closed_loop(name, sd, cfg):
    """(start latents, oracle latents, oracle masses, margin) of CLOSED_LOOPS[name], computed once per process."""
    if name not in _RUNS:
        from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
        site, seed, steps, B, scale, eta, gseed = CLOSED_LOOPS[name]
        x = start_latents(seed, B)
        sched = ffhq_ddim_scheduler().sag_schedule(steps, eta, scale, 0.0)
        g = torch.Generator().manual_seed(gseed)
        z, masses = sample(sd, cfg, x, sched, site, draw=sched.drawer(g, tuple(x.shape), torch.device("cpu"), torch.float32))
        _RUNS[name] = (x, z, masses, margin(masses))
    return _RUNS[name]


# The graph-against-eager-loop configurations: both sides are the product, but a mass on the threshold could still flip a mask
# between them, so the oracle loop's margin is asserted for these too (CPU and list generators: the draws are CPU draws).  A CUDA
# generator's draws exist on the device only: there the GPU test asserts the margin on the product's own recorded masses.
GRAPH_SITE, GRAPH_STEPS, GRAPH_XSEED, GRAPH_GSEED, GRAPH_SCALE = "mid_block.attentions.0", 6, 3, 1, 0.75


def graph_generator(kind, seed=GRAPH_GSEED):
    if kind == "list":
        return [torch.Generator().manual_seed(seed + i) for i in range(2)]
    return torch.Generator("cuda" if kind == "cuda" else "cpu").manual_seed(seed)


def graph_loop(sd, cfg, eta, kind):
    """(oracle latents, masses, margin) of the graph-against-eager configuration with a CPU or list generator."""
    key = ("graph", eta, kind)
    if key not in _RUNS:
        from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
        x = start_latents(GRAPH_XSEED, 2)
        sched = ffhq_ddim_scheduler().sag_schedule(GRAPH_STEPS, eta, GRAPH_SCALE, 0.0)
        draw = sched.drawer(graph_generator(kind), tuple(x.shape), torch.device("cpu"), torch.float32)
        z, masses = sample(sd, cfg, x, sched, GRAPH_SITE, draw=draw)
        _RUNS[key] = (z, masses, margin(masses))
    return _RUNS[key]
