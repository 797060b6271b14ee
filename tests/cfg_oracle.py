"""CPU oracle of class conditioning and classifier-free guidance on the oracle UNet (oracle/unet.py, which is not edited and knows
no class embedding).  diffusers adds the class row to the time embedding before the SiLU in front of the time_emb_proj layers:

    emb = time_embedding(t) + c = linear_2(h) + (b_2 + c)

so a sample with class row c is oracle.unet.unet_forward on a state dict whose time_embedding.linear_2.bias is b_2 + c, one sample
at a time (the bias is shared by a batch).  On top, the float64 guided loop in tests/pag_oracle.py's style:

    e_c = UNet(x, t, c);  e_u = UNet(x, t, c_null);  g = e_c + (w - 1) (e_c - e_u), rescaled towards std(e_c) by phi;
    the "sde" row applied to g (pag_oracle.pag_step with s = w - 1).

The tiny class-conditional model of the tests: test_gpu_dpm.build("tiny")'s weights plus a seeded class table of K = 5 rows, the
last one the null class."""
import torch

import pag_oracle as po
from oracle import unet as ou

K = 5                   # classes of the tiny model, the null class (K - 1) included
TABLE_SCALE = 1.0       # standard deviation of the seeded class table: test_cfg_host asserts that it separates the classes
B2 = "time_embedding.linear_2.bias"


def tiny():
    """(cfg, sd) of test_gpu_dpm.build("tiny")."""
    from oracle import configs as oc
    cfg = oc.tiny_unet()
    return cfg, ou.randomize_norm_affine(ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1))


def class_table(sd, k=K, scale=TABLE_SCALE, seed=17):
    """A seeded class table [k, temb_dim] (fp32)."""
    return torch.randn(k, sd[B2].shape[0], generator=torch.Generator().manual_seed(seed)) * scale


def unet_forward_cond(sd, cfg, x, t, rows):
    """The oracle UNet on x [B, C, H, W] at timestep t (a number or a [B] tensor) with class rows [B, temb_dim]: per sample,
    unet_forward on the state dict whose linear_2 bias is b_2 + row."""
    assert rows.shape[0] == x.shape[0]
    outs = []
    for i in range(x.shape[0]):
        sdi = dict(sd)
        sdi[B2] = sd[B2] + rows[i].to(sd[B2].dtype)
        ti = t[i] if torch.is_tensor(t) and t.numel() > 1 else t
        outs.append(ou.unet_forward(sdi, cfg, x[i:i + 1], ti))
    return torch.cat(outs)


def sample(sd, cfg, x, schedule, cond_rows, null_rows, draw=None):
    """The float64 loop over a "cfg" Schedule: the oracle UNet (fp32, CPU) on the conditional and on the unconditional rows, then
    pag_oracle.pag_step (s = guidance_scale - 1).  draw(): the next noise tensor, called once per step that draws, in step order."""
    assert schedule.kind == "cfg"
    z = x.double() * schedule.init_noise_sigma
    for k, (t, row) in enumerate(zip(schedule.timesteps, schedule.rows)):
        noise = draw() if schedule.slots(k) else None
        e_c = unet_forward_cond(sd, cfg, z.float(), int(t), cond_rows)
        e_u = e_c if row[8] == 0.0 else unet_forward_cond(sd, cfg, z.float(), int(t), null_rows)
        z = po.pag_step(z, e_c, e_u, noise, row)
    return z


def build_cond(dtype, table=None, class_embed_type=None, name="tiny"):
    """test_gpu_dpm.build(name)'s model with class conditioning on the GPU: (unet, cfg, sd, table).  class_embed_type None: an
    nn.Embedding of `table` (default class_table); 'identity': no table in the model (the rows are the caller's)."""
    from afldm_amd.af_modules.af_api import make_af_unet
    from afldm_amd.models.unet_2d import UNet2DModel
    from oracle import configs as oc
    if name == "tiny":
        cfg, sd = tiny()
    else:
        cfg = oc.FFHQ_UNET
        sd = ou.init_unet_params(cfg, seed=0, conv_out_scale=0.1)
    table = class_table(sd) if table is None else table
    if class_embed_type is None:
        unet = UNet2DModel.from_config(cfg, num_class_embeds=table.shape[0])
        unet.load_state_dict(dict(sd, **{"class_embedding.weight": table}))
    else:
        unet = UNet2DModel.from_config(cfg, class_embed_type=class_embed_type)
        unet.load_state_dict(sd)
    make_af_unet(unet)
    return unet.to("cuda").to(dtype), cfg, sd, table
