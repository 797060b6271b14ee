"""The class-conditional UNet2DModel.forward on MI355X: the tiny UNet with a table of 5 classes, fp32, batch 2, against the CPU
oracle restatement (tests/cfg_oracle.py: the class row folded into time_embedding.linear_2.bias, 1e-3, the project's bound for the
UNet against the oracle); a zeroed class table against the unconditional model of the same weights (1e-5, the bound of
test_gpu_pag_pipeline.test_scale_zero_is_the_plain_sampler); a neighbour's label changes nothing (bit for bit); the 'identity'
class embedding fed the table's rows is the Embedding model (bit for bit); bf16 against fp32 by the `det` rule of
test_gpu_pag_pipeline.py: no number fixed in advance - the conditional bf16 forward may differ from its fp32 run by 1.5x what the
unconditional bf16 forward differs from its fp32 run on the same input."""
import pytest
import torch

import cfg_oracle as co
from test_gpu_dpm import build, rel_rms

pytestmark = pytest.mark.gpu

LABELS = [0, 4]


def _x(seed=3):
    return torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def cond32():
    return co.build_cond(torch.float32)


@pytest.mark.parametrize("t", [501, torch.tensor([501, 21])], ids=["scalar", "per_sample"])
def test_forward_against_the_oracle(cond32, t):
    unet, cfg, sd, table = cond32
    x = _x()
    want = co.unet_forward_cond(sd, cfg, x, t, table[LABELS])
    got = unet(x.cuda(), t, class_labels=LABELS).sample
    err = rel_rms(got, want)
    from oracle import unet as ou
    away = rel_rms(torch.cat([ou.unet_forward(sd, cfg, x[i:i + 1], t[i] if torch.is_tensor(t) else t) for i in range(2)]), want)
    print(f"[tiny class-conditional forward, labels {LABELS}] fp32 rel-RMS vs the oracle {err:.3e}; the unconditional output is {away:.3e} away")
    assert err <= 1e-3, err
    assert away > 1e-2, away
    got_t = unet(x.cuda(), t, class_labels=torch.tensor(LABELS, device="cuda"), return_dict=False)[0]
    assert torch.equal(got_t, got)                                              # labels as a device tensor: the same rows


def test_a_zero_table_is_the_unconditional_model(cond32):
    _, cfg, sd, table = cond32
    zeroed, _, _, _ = co.build_cond(torch.float32, table=torch.zeros_like(table))
    plain, _, _ = build("tiny", torch.float32)
    x = _x().cuda()
    for t in (501, torch.tensor([501, 21])):
        err = rel_rms(zeroed(x, t, class_labels=LABELS).sample, plain(x, t).sample)
        print(f"[tiny, zeroed class table, t = {t if not torch.is_tensor(t) else t.tolist()}] vs the unconditional model rel-RMS {err:.2e}")
        assert err <= 1e-5, err


def test_a_neighbours_label_changes_nothing(cond32):
    unet = cond32[0]
    x = _x().cuda()
    a = unet(x, 501, class_labels=[0, 4]).sample
    b = unet(x, 501, class_labels=[0, 2]).sample
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])


def test_identity_embedding_fed_the_tables_rows(cond32):
    unet, _, _, table = cond32
    ident, _, _, _ = co.build_cond(torch.float32, class_embed_type="identity")
    x = _x().cuda()
    for t in (501, torch.tensor([501, 21])):
        a = unet(x, t, class_labels=LABELS).sample
        rows = unet.class_embedding.weight[torch.tensor(LABELS, device="cuda")]
        assert torch.equal(ident(x, t, class_labels=rows).sample, a)
        assert torch.equal(ident(x, t, class_labels=table[LABELS]).sample, a)      # host rows too


def test_missing_and_stray_labels_on_the_device(cond32):
    unet = cond32[0]
    plain, _, _ = build("tiny", torch.float32)
    x = _x().cuda()
    with pytest.raises(ValueError, match="class_labels should be provided"):
        unet(x, 501)
    with pytest.raises(ValueError, match="class_embedding needs to be initialized"):
        plain(x, 501, class_labels=LABELS)
    with pytest.raises(ValueError, match="outside"):
        unet(x, 501, class_labels=[0, co.K])
    with pytest.raises(ValueError):
        unet.forward_nhwc(torch.zeros(2, 16, 16, 4, device="cuda"), 501)           # no rows, no slices: nothing ignores the labels


def test_bf16_against_fp32(cond32):
    u32 = cond32[0]
    u16, _, _, _ = co.build_cond(torch.bfloat16)
    p32, _, _ = build("tiny", torch.float32)
    p16, _, _ = build("tiny", torch.bfloat16)
    x = _x(seed=21).cuda()
    for t in (501, torch.tensor([501, 21])):
        det = rel_rms(p16(x, t).sample.float(), p32(x, t).sample)
        got = u16(x, t, class_labels=LABELS).sample
        assert got.dtype == torch.float32 or got.dtype == x.dtype
        err = rel_rms(got.float(), u32(x, t, class_labels=LABELS).sample)
        print(f"[tiny class-conditional forward bf16] det {det:.3e}; conditional vs fp32 {err:.3e} (<= {1.5 * det:.3e})")
        assert err <= 1.5 * det, (det, err)
