"""Class conditioning and classifier-free guidance, host side (no GPU): the oracle (tests/cfg_oracle.py) - a zero class row is the
plain oracle UNet bit for bit - the "cfg" schedule (rows, draws, key, refusals), that the guidance separates from the conditional
and from the unconditional sample on the tiny oracle UNet at the settings the GPU tests compare at, UNet2DModel's class surface
(module, state-dict key, ValueErrors, save / load), the bindings and the script."""
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

import cfg_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sched(**kw):
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.schedulers.ddim import DDIMScheduler
    return DDIMScheduler.from_config(FFHQ_DDIM_CONFIG, **kw)


def rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


def _x():
    return torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3))


# ------------------------------------------------------------------------------------------------ oracle
def test_a_zero_class_row_is_the_plain_oracle():
    """b_2 + 0 is b_2: per sample (the restatement evaluates one sample at a time, and a CPU convolution's bits may depend on the
    batch size), unet_forward's tensor exactly; and a non-zero row moves it."""
    from oracle import unet as ou
    cfg, sd = co.tiny()
    x = _x()
    zero = torch.zeros(2, sd[co.B2].shape[0])
    for t in (501, torch.tensor([501, 21])):
        plain = torch.cat([ou.unet_forward(sd, cfg, x[i:i + 1], t[i] if torch.is_tensor(t) else t) for i in range(2)])
        assert torch.equal(co.unet_forward_cond(sd, cfg, x, t, zero), plain)
    table = co.class_table(sd)
    assert table.shape == (co.K, sd[co.B2].shape[0])
    moved = co.unet_forward_cond(sd, cfg, x, 501, table[[0, 4]])
    assert rel_rms(moved, plain) > 1e-3
    # row 0 does not see row 1's class
    assert torch.equal(moved[:1], co.unet_forward_cond(sd, cfg, x, 501, table[[0, 2]])[:1])


# ------------------------------------------------------------------------------------------------ schedule
@pytest.mark.parametrize("n", [4, 50])
@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_cfg_schedule_rows_draws_and_key(n, eta):
    from afldm_amd.schedulers.schedule import KINDS, NOISE_SLOTS, ROW_WIDTH
    assert KINDS["cfg"] == (12, 1, True) and ROW_WIDTH["cfg"] == 12 and NOISE_SLOTS["cfg"] == 1
    cfg = sched().cfg_schedule(n, eta, 3.0, 0.7)
    sde = sched().stochastic_schedule(n, eta)
    pag = sched().pag_schedule(n, eta, 2.0, 0.7)
    assert cfg.kind == "cfg" and cfg.timesteps == sde.timesteps and len(cfg.rows) == n
    for r, w in zip(cfg.rows, sde.rows):
        assert r[:8] == w and r[8:] == (2.0, 0.7, 0.0, 0.0)                 # float for float; s = guidance_scale - 1
    assert cfg.rows == pag.rows and cfg.draws == pag.draws and cfg.key != pag.key
    assert torch.equal(cfg.table("cpu")[:, :8], sde.table("cpu"))
    if eta:
        assert cfg.draws == sde.draws and all(cfg.draws)
        assert [cfg.slots(k) for k in range(n)] == [sde.slots(k) for k in range(n)]
    else:
        assert not any(cfg.draws) and all(r[7] == 0.0 for r in cfg.rows)
    assert sched().cfg_schedule(n, eta, 2.0, 0.7).key != cfg.key and sched().cfg_schedule(n, eta, 3.0, 0.0).key != cfg.key
    assert sched().cfg_schedule(n, eta, 3.0, 0.7) is cfg and cfg.key != sde.key
    one = sched().cfg_schedule(n, eta, 1.0, 0.0)
    assert all(r[8] == 0.0 for r in one.rows)
    for bad in ((0.5, 0.0), (-1.0, 0.0), (0.0, 0.0), (float("nan"), 0.0), (3.0, 1.5), (3.0, -0.1)):
        with pytest.raises(ValueError):
            sched().cfg_schedule(n, eta, *bad)
    assert inspect.signature(sched().cfg_schedule).parameters["guidance_scale"].default == 3.0


def test_guidance_separates_on_the_tiny_oracle():
    """The class table's scale (cfg_oracle.TABLE_SCALE) is chosen here, on the CPU oracle: at w = 3 the guided sample must be
    more than 1e-2 rel-RMS away from the w = 1 (conditional) sample and from the sample of the null row alone, so that the GPU
    tests' 1e-3 bound cannot hide a guidance that does nothing; the GPU "away" checks rest on this."""
    cfg, sd = co.tiny()
    table = co.class_table(sd)
    x = _x()
    cond, null = table[[0, 3]], table[[co.K - 1, co.K - 1]]
    guided = co.sample(sd, cfg, x, sched().cfg_schedule(4, 0.0, 3.0, 0.0), cond, null)
    one = co.sample(sd, cfg, x, sched().cfg_schedule(4, 0.0, 1.0, 0.0), cond, null)
    uncond = co.sample(sd, cfg, x, sched().cfg_schedule(4, 0.0, 1.0, 0.0), null, null)
    # w = 1 is the conditional sampler: the plain loop over the "sde" rows
    import pag_oracle as po
    plain = x.double()
    for t, row in zip(sched().stochastic_schedule(4, 0.0).timesteps, sched().stochastic_schedule(4, 0.0).rows):
        e = co.unet_forward_cond(sd, cfg, plain.float(), int(t), cond)
        plain = po.pag_step(plain, e, e, None, row + (0.0, 0.0))
    assert torch.equal(one, plain)
    d1, dn = rel_rms(guided, one), rel_rms(guided, uncond)
    print(f"[tiny oracle, 4 steps, table scale {co.TABLE_SCALE}] w = 3 vs w = 1 {d1:.2e}; vs the null row alone {dn:.2e}")
    assert d1 > 1e-2 and dn > 1e-2


# ------------------------------------------------------------------------------------------------ model surface
def _unet(**kw):
    from afldm_amd.models.unet_2d import UNet2DModel
    cfg, sd = co.tiny()
    return UNet2DModel.from_config(cfg, **kw), cfg, sd


def test_class_embedding_module_and_key():
    unet, cfg, sd = _unet(num_class_embeds=co.K)
    D = sd[co.B2].shape[0]
    assert isinstance(unet.class_embedding, torch.nn.Embedding) and tuple(unet.class_embedding.weight.shape) == (co.K, D)
    assert "class_embedding.weight" in unet.state_dict() and unet.config.num_class_embeds == co.K
    assert not unet.class_embedding.weight.requires_grad
    table = co.class_table(sd)
    unet.load_state_dict(dict(sd, **{"class_embedding.weight": table}))          # a diffusers checkpoint trained with labels loads
    rows = unet.class_embed([0, 4])
    assert rows.dtype == unet.dtype and torch.equal(rows, table[[0, 4]])
    assert torch.equal(unet.class_embed(torch.tensor([3])), table[[3]])
    # no conditioning: no module, no key, and the old state dict still loads strictly
    plain, _, _ = _unet()
    assert plain.class_embedding is None and not any("class_embedding" in k for k in plain.state_dict())
    assert "class_embedding" not in dict(plain.named_modules())
    plain.load_state_dict(sd)
    with pytest.raises(RuntimeError):
        plain.load_state_dict(dict(sd, **{"class_embedding.weight": table}))
    ident, _, _ = _unet(class_embed_type="identity")
    assert isinstance(ident.class_embedding, torch.nn.Identity) and not any("class_embedding" in k for k in ident.state_dict())
    assert torch.equal(ident.class_embed(table[[0, 4]]), table[[0, 4]])
    with pytest.raises(NotImplementedError):
        _unet(class_embed_type="timestep")
    with pytest.raises(NotImplementedError):
        _unet(class_embed_type="timestep", num_class_embeds=co.K)


def test_label_errors_are_raised_on_the_host():
    unet, _, _ = _unet(num_class_embeds=co.K)
    plain, _, _ = _unet()
    ident, _, _ = _unet(class_embed_type="identity")
    x = torch.zeros(2, 4, 16, 16)
    with pytest.raises(ValueError, match="class_labels should be provided when doing class conditioning"):
        unet(x, 5)
    with pytest.raises(ValueError, match="class_embedding needs to be initialized in order to use class conditioning"):
        plain(x, 5, class_labels=[0, 1])
    for bad in ([0, co.K], [-1, 0], torch.tensor([co.K + 3, 0])):
        with pytest.raises(ValueError, match="outside"):
            unet(x, 5, class_labels=bad)
        with pytest.raises(ValueError, match="outside"):
            unet.class_embed(bad)
    with pytest.raises(ValueError):
        unet(x, 5, class_labels=[0.5, 1.0])                                       # float labels for a table
    with pytest.raises(ValueError):
        unet(x, 5, class_labels=[0, 1, 2])                                        # three labels for a batch of two
    with pytest.raises(ValueError):
        ident(x, 5, class_labels=[0, 1])                                          # integer labels for 'identity'
    with pytest.raises(ValueError):
        ident(x, 5, class_labels=torch.zeros(2, 7))                               # rows of the wrong width
    with pytest.raises(ValueError):
        ident(x, 5)
    # no CPU path: valid labels reach the device check
    with pytest.raises(RuntimeError, match="MI355X"):
        unet(x, 5, class_labels=[0, 1])
    with pytest.raises(RuntimeError):
        plain(x, 5)


def test_save_and_load_round_trip(tmp_path):
    from afldm_amd.models.unet_2d import UNet2DModel
    unet, _, sd = _unet(num_class_embeds=co.K)
    unet.load_state_dict(dict(sd, **{"class_embedding.weight": co.class_table(sd)}))
    unet.save_pretrained(str(tmp_path))
    back = UNet2DModel.from_pretrained(str(tmp_path))
    assert back.config.num_class_embeds == co.K and back.config.class_embed_type is None
    a, b = unet.state_dict(), back.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(back.class_embed([1, 4]), unet.class_embed([1, 4]))
    ident, _, _ = _unet(class_embed_type="identity")
    ident.save_pretrained(str(tmp_path / "ident"))
    assert isinstance(UNet2DModel.from_pretrained(str(tmp_path / "ident")).class_embedding, torch.nn.Identity)


def test_pipeline_refusals_on_the_host():
    from afldm_amd.configs import FFHQ_DDIM_CONFIG
    from afldm_amd.pipelines.i2sb_pipeline import I2SBLDMPipeline
    from afldm_amd.pipelines.ldm_pipeline import MyLDMPipeline
    from afldm_amd.schedulers.ddim import ffhq_ddim_scheduler
    from afldm_amd.schedulers.dpmsolver import DPMSolverMultistepScheduler
    unet, _, _ = _unet(num_class_embeds=co.K)
    pipe = MyLDMPipeline(None, unet, ffhq_ddim_scheduler())
    pipe.set_progress_bar_config(disable=True)
    sig = inspect.signature(pipe.cfg_latents).parameters
    assert list(sig) == ["class_labels", "guidance_scale", "guidance_rescale", "null_label", "null_embedding", "eta",
                         "num_inference_steps", "generator", "latents", "use_graph"]
    assert sig["guidance_scale"].default == 3.0 and sig["null_label"].default is None and sig["num_inference_steps"].default == 50
    assert list(inspect.signature(pipe.cfg).parameters)[-2:] == ["output_type", "return_dict"]
    for kw in (dict(guidance_scale=0.5), dict(guidance_rescale=1.5), dict(null_embedding=torch.zeros(256))):
        with pytest.raises(ValueError):
            pipe.cfg_latents([0, 1], num_inference_steps=2, **kw)
    with pytest.raises(ValueError, match="outside"):
        pipe.cfg_latents([0, co.K], num_inference_steps=2)
    with pytest.raises(ValueError, match="outside"):
        pipe.cfg_latents([0, 1], null_label=co.K, num_inference_steps=2)
    with pytest.raises(ValueError):
        pipe.cfg_latents([0, 1], latents=torch.zeros(3, 4, 16, 16), num_inference_steps=2)
    with pytest.raises(RuntimeError):                                              # no CPU path
        pipe.cfg_latents([0, 1], num_inference_steps=2)
    plain = MyLDMPipeline(None, _unet()[0], ffhq_ddim_scheduler())
    with pytest.raises(ValueError):
        plain.cfg_latents([0, 1], num_inference_steps=2)
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(FFHQ_DDIM_CONFIG)
    for call in (pipe.cfg_latents, pipe.cfg):
        with pytest.raises(NotImplementedError, match="classifier-free guidance"):
            call([0, 1], num_inference_steps=2)
    for name in ("cfg_latents", "cfg"):
        with pytest.raises(NotImplementedError):
            getattr(I2SBLDMPipeline, name)(None, [0, 1])


# ------------------------------------------------------------------------------------------------ bindings and tooling
def test_cond_embed_entry_points_are_bound_and_documented():
    from afldm_amd import _lib, build, ops
    hdr = open(os.path.join(ROOT, "include", "afldm_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    want = {"afldm_cond_embed": ["emb_table", "n", "step_idx", "class_rows", "act", "rows", "D", "dtype", "stream"],
            "afldm_cond_embed_flat": ["emb", "emb_rows", "class_rows", "act", "rows", "D", "dtype", "stream"]}
    for name, params in want.items():
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name) and name in doc
        m = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m, name
        got = [p.split()[-1].lstrip("*") for p in m.group(1).replace("\n", " ").split(",")]
        assert got == params and len(getattr(_lib.lib, name).argtypes) == len(params)
    assert "const int* step_idx" in hdr                                           # the kernel only reads the counter
    assert "cond.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "cond.hip"))
    assert callable(ops.cond_embed) and callable(ops.cond_embed_flat)
    assert len(_lib.EXPORTS) == 112
    # refusals before any launch: a width that is no multiple of 8, NULL pointers
    lib = _lib.lib
    assert lib.afldm_cond_embed(16, 3, 16, 16, 16, 2, 12, 0, None) == -1
    assert lib.afldm_cond_embed_flat(16, 1, 16, 16, 2, 12, 1, None) == -1
    assert lib.afldm_cond_embed_flat(16, 3, 16, 16, 2, 16, 1, None) == -1          # emb_rows neither 1 nor rows
    assert lib.afldm_cond_embed(None, 3, None, None, None, 2, 16, 0, None) == -5
    assert lib.afldm_cond_embed_flat(None, 1, None, None, 2, 16, 0, None) == -5
    # no CPU path
    x = torch.zeros(2, 16)
    with pytest.raises(RuntimeError):
        ops.cond_embed_flat(x[:1], x)
    with pytest.raises(RuntimeError):
        ops.cond_embed(x, torch.zeros(1, dtype=torch.int32), x)


def test_engine_surface():
    from afldm_amd import engine, ops
    assert engine.CFGEngine.ONE_BRANCH and set(engine.CFGEngine.UPDATES) == {"cfg", "ddim", "sde"}
    assert engine.CFGEngine.UPDATES["cfg"][0] is ops.pag_step                     # no new update kernel
    assert engine.CFGEngine.UPDATES["ddim"] == engine.DenoiseEngine.UPDATES["ddim"]
    assert engine.CFGEngine.UPDATES["sde"] == engine.DenoiseEngine.UPDATES["sde"]
    assert "cfg" not in engine.DenoiseEngine.UPDATES and "cfg" not in engine.PAGEngine.UPDATES
    unet, _, _ = _unet(num_class_embeds=co.K)
    with pytest.raises(ValueError, match="class-conditional"):
        engine.refuse_class_conditional(unet, "DenoiseEngine")
    engine.refuse_class_conditional(_unet()[0], "DenoiseEngine")


def test_script_help():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cfg_ffhq.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for flag in ("--labels", "--guidance-scale", "--guidance-rescale", "--null-label", "--random-init", "--num-classes", "--eager",
                 "--timings"):
        assert flag in r.stdout, flag
