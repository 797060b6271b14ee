"""CPU restatements for the frame-sequence editing tests: the keyframe source table, the reference's get_timesteps and
ddim_inversion coefficients (video_equiv_editing_pipeline.py:320-328, :186-195), and a float64 model of one banked LOAD of an
attention block: GroupNorm of the stored map -> K / V projection -> per-source softmax attention -> blend -> to_out + residual.
Nothing here imports the code under test."""
import math

import torch
import torch.nn.functional as F


def sources(num_frames, keyframes):
    """[(s0, s1)], [alpha]: frame f with k_i <= f < k_{i+1} attends to keyframes i and i + 1 blended by (f - k_i) / (k_{i+1} - k_i);
    a keyframe, and a frame past the last keyframe, attends to one source (i, i) with alpha 0."""
    keys = list(keyframes)
    src, alpha = [], []
    for f in range(num_frames):
        i = len([k for k in keys if k <= f]) - 1
        if keys[i] == f or i + 1 == len(keys):
            src.append((i, i))
            alpha.append(0.0)
        else:
            src.append((i, i + 1))
            alpha.append((f - keys[i]) / (keys[i + 1] - keys[i]))
    return src, alpha


def valid_keyframes(num_frames, keyframes):
    keys = list(keyframes)
    return (len(keys) > 0 and keys[0] == 0 and all(b > a for a, b in zip(keys, keys[1:])) and keys[-1] < num_frames)


def get_timesteps(all_timesteps, num_inference_steps, strength):
    """reference :320-328 on a list (scheduler.order = 1); strength < 0: the whole list (:558)."""
    if strength < 0:
        return list(all_timesteps)
    init_timestep = min(int(num_inference_steps * strength), num_inference_steps)
    t_start = max(num_inference_steps - init_timestep, 0)
    return list(all_timesteps)[t_start:]


def inversion_rows(alphas_cumprod, final_alpha_cumprod, timesteps):
    """reference :177-195 and :211-212: timesteps reversed; per step (t, mu_prev, sigma_prev, mu, sigma) in float64 from the
    scheduler's fp32 alphas_cumprod; latent <- mu (latent - sigma_prev eps) / mu_prev + sigma eps."""
    ts = list(reversed([int(t) for t in timesteps]))
    rows = []
    for i, t in enumerate(ts):
        alpha_prod_t = float(alphas_cumprod[t])
        alpha_prod_t_prev = float(alphas_cumprod[ts[i - 1]]) if i > 0 else float(final_alpha_cumprod)
        rows.append((t, math.sqrt(alpha_prod_t_prev), math.sqrt(1 - alpha_prod_t_prev), math.sqrt(alpha_prod_t),
                     math.sqrt(1 - alpha_prod_t)))
    return rows


def bank_load(x, bank, src, alpha, sd, heads, groups, eps):
    """float64.  x [B, H, W, C] the LOAD batch's attention input, bank [S, H, W, C] the stored maps, src [(s0, s1)] * B, alpha
    [B], sd the Attention module's state dict (group_norm, to_q, to_k, to_v, to_out.0).  Q comes from GroupNorm(x), K / V from
    GroupNorm(bank[s]) with the same layer (reference cross_frame_attn.py:88-125), out = to_out(blend) + x."""
    sd = {k: v.double().cpu() for k, v in sd.items()}
    x, bank = x.double().cpu(), bank.double().cpu()
    B, H, W, C = x.shape
    d = C // heads

    def tokens(m):                                                  # [n, H, W, C] -> group-normed [n, HW, C]
        y = F.group_norm(m.permute(0, 3, 1, 2), groups, sd["group_norm.weight"], sd["group_norm.bias"], eps)
        return y.permute(0, 2, 3, 1).reshape(m.shape[0], H * W, C)

    def lin(name, t):
        return F.linear(t, sd[f"{name}.weight"], sd[f"{name}.bias"])

    def split(t):
        return t.view(t.shape[0], -1, heads, d).transpose(1, 2)

    out = []
    for b in range(B):
        q = split(lin("to_q", tokens(x[b:b + 1])))
        acc = 0.0
        for s, w in ((src[b][0], 1.0 - float(alpha[b])), (src[b][1], float(alpha[b]))):
            if w == 0.0:
                continue
            kv = tokens(bank[s:s + 1])
            k, v = split(lin("to_k", kv)), split(lin("to_v", kv))
            p = torch.softmax(q @ k.transpose(2, 3) * d ** -0.5, dim=-1)
            acc = acc + w * (p @ v).transpose(1, 2).reshape(1, H * W, C)
        out.append(lin("to_out.0", acc).view(1, H, W, C) + x[b:b + 1])
    return torch.cat(out)
