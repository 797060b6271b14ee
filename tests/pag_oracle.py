"""CPU oracle of perturbed-attention guidance (Ahn et al. 2024; diffusers PAGMixin / PAGIdentitySelfAttnProcessor2_0) on the oracle
UNet (oracle/unet.py, which is not edited: its attention core is swapped while a context manager is open).

    e   = UNet(x, t)
    e_p = UNet_P(x, t)          every attention block in P computes x + to_out(to_v(GroupNorm(x))): the identity attention map
    g   = e + s (e - e_p);      phi > 0:  g <- g (phi std(e) / std(g) + 1 - phi) per sample, the ratio 1 where std(g) = 0
    x0  = clamp(p x + q g, lo, hi);   x_out = a x + b x0 + d g + c z

The identity block is written UNFOLDED here (two linear layers, as diffusers runs them); `identity_block_folded` is the product's
one-GEMM form for the host test that compares the two in float64."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import unet as ou


def _selected(prefix, sites):
    return any(prefix == s or prefix.startswith(s + ".") for s in sites)


def identity_block(sd, prefix, x, groups, eps):
    """x [B, C, H, W] -> x + to_out(to_v(GroupNorm(x))), in x's dtype."""
    b, ch, hh, ww = x.shape
    w = {k: sd[prefix + k].to(x.dtype) for k in (".group_norm.weight", ".group_norm.bias", ".to_v.weight", ".to_v.bias",
                                                 ".to_out.0.weight", ".to_out.0.bias")}
    h = F.group_norm(x.view(b, ch, hh * ww), groups, w[".group_norm.weight"], w[".group_norm.bias"], eps).transpose(1, 2)
    v = F.linear(h, w[".to_v.weight"], w[".to_v.bias"])
    o = F.linear(v, w[".to_out.0.weight"], w[".to_out.0.bias"])
    return o.transpose(-1, -2).reshape(b, ch, hh, ww) + x


def folded_weights(sd, prefix):
    """(W_vo, b_vo) in float64: W_vo = W_o W_v, b_vo = W_o b_v + b_o."""
    wo, wv = sd[prefix + ".to_out.0.weight"].double(), sd[prefix + ".to_v.weight"].double()
    return wo @ wv, wo @ sd[prefix + ".to_v.bias"].double() + sd[prefix + ".to_out.0.bias"].double()


def identity_block_folded(sd, prefix, x, groups, eps):
    """The same block as ONE GEMM on the folded weight, in float64."""
    b, ch, hh, ww = x.shape
    x = x.double()
    h = F.group_norm(x.view(b, ch, hh * ww), groups, sd[prefix + ".group_norm.weight"].double(),
                     sd[prefix + ".group_norm.bias"].double(), eps).transpose(1, 2)
    w, bias = folded_weights(sd, prefix)
    return F.linear(h, w, bias).transpose(-1, -2).reshape(b, ch, hh, ww) + x


@contextlib.contextmanager
def perturbed_attention(sites):
    """While open, oracle.unet's attention core computes the identity block at every site `sites` selects (a module path or a
    prefix of one on a '.' boundary) and the original everywhere else.  The original is put back on exit, also on an exception."""
    original = ou._attention_core
    sites = tuple(sites)

    def core(c, prefix, x, kv_src):
        if not _selected(prefix, sites):
            return original(c, prefix, x, kv_src)
        assert kv_src is None, "PAG perturbs plain self-attention"
        return identity_block(c.sd, prefix, x, c.groups, c.eps)

    ou._attention_core = core
    try:
        yield
    finally:
        ou._attention_core = original


def unet_forward_perturbed(sd, cfg, x, t, sites):
    with perturbed_attention(sites):
        return ou.unet_forward(sd, cfg, x, t)


def pag_step(x, e, e_p, z, row):
    """The guided update in float64; row = (p, q, lo, hi, a, b, d, c, s, phi, ...), z None where c = 0."""
    p, q, lo, hi, a, b, d, c, s, phi = [float(v) for v in row[:10]]
    x, e, e_p = x.double(), e.double(), e_p.double()
    g = e + s * (e - e_p)
    if phi > 0.0:
        dims = tuple(range(1, x.dim()))
        se, sg = e.std(dim=dims, keepdim=True), g.std(dim=dims, keepdim=True)
        ratio = torch.where(sg > 0, se / torch.where(sg > 0, sg, torch.ones_like(sg)), torch.ones_like(sg))
        g = g * (phi * ratio + 1.0 - phi)
    out = a * x + b * torch.clamp(p * x + q * g, lo, hi) + d * g
    if c != 0.0:
        out = out + c * z.double()
    return out


def sample(sd, cfg, x, schedule, sites, draw=None):
    """The float64 loop over a "pag" Schedule: the oracle UNet (fp32, CPU) evaluated plainly and perturbed at `sites`, then
    pag_step.  draw(): the next noise tensor, called once per step that draws, in step order."""
    z = x.double() * schedule.init_noise_sigma
    for k, (t, row) in enumerate(zip(schedule.timesteps, schedule.rows)):
        noise = draw() if schedule.slots(k) else None
        e = ou.unet_forward(sd, cfg, z.float(), int(t))
        e_p = unet_forward_perturbed(sd, cfg, z.float(), int(t), sites)
        z = pag_step(z, e, e_p, noise, row)
    return z
