"""CPU checks of tests/batch_oracle.py: a clean per-sample function passes every relation, each planted batch-position fault is
caught by at least one of them (tests/test_gpu_batch_positions.py runs them on the kernels)."""
import math

import pytest
import torch

import batch_oracle as bo

ROTATIONS = (1, 3, 8, 16, 17)
G = 16                  # samples of one workgroup in the planted faults (dense2.hip's)


def layer(x, temb, fault=None):
    """A stand-in for a resnet layer on [B, H, W, C] with a time-embedding row per sample: a vertical 3-tap filter over a zero
    halo, + temb, per-sample normalisation, one bf16 rounding - with one fault planted:
      neighbour_stats: sample b is normalised with the statistics of sample b ^ 1;
      swap_at_16:      samples 3 and 4 change places, only when B >= 16 (a policy switch on the batch);
      halo_row:        the last sample of every group of 16 reads the first row of the next sample as its bottom halo;
      odd_rounding:    odd positions are rounded to bf16 by truncation instead of to nearest."""
    B, H = x.shape[:2]
    x = x.double()
    pad = torch.zeros_like(x[:, :1])
    below = pad.clone()
    if fault == "halo_row":
        for b in range(G - 1, B - 1, G):
            below[b] = x[b + 1, :1]
    xp = torch.cat([pad, x, below], 1)
    y = 0.25 * xp[:, :H] + 0.5 * xp[:, 1:H + 1] + 0.25 * xp[:, 2:H + 2] + temb.double()[:, None, None, :]
    mean, std = y.mean((1, 2, 3), keepdim=True), y.std((1, 2, 3), keepdim=True)
    if fault == "neighbour_stats":
        nb = (torch.arange(B) ^ 1).clamp_max(B - 1)
        mean, std = mean[nb], std[nb]
    y = ((y - mean) / std).float()
    out = y.to(torch.bfloat16)
    if fault == "odd_rounding":
        trunc = (y.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
        out[1::2] = trunc[1::2]
    if fault == "swap_at_16" and B >= 16:
        out[[3, 4]] = out[[4, 3]]
    st = torch.stack([out.float().sum((1, 2)), out.float().pow(2).sum((1, 2))], -1)[:, None]       # [B, 1, C, 2]
    out.gn_partial = st
    return out


FAULTS = ["neighbour_stats", "swap_at_16", "halo_row", "odd_rounding"]


def inputs(B, seed=0):
    return bo.distinct_batch(B, (4, 4, 8), seed), bo.distinct_batch(B, (8,), seed + 1)


def failed_relations(f, x):
    """Names of the relations that f breaks on x."""
    B = x[0].shape[0]
    base = bo.run(f, x)
    bad = []
    for r in sorted({r for r in ROTATIONS + (B - 1,) if 0 < r < B}):
        try:
            bo.check_rotation(f, x, r, base=base, what="host")
        except AssertionError:
            bad.append(f"rot{r}")
    for value, name in ((math.nan, "nan"), (bo.BIG, "big")):
        for p in sorted({0, G - 1, G, B - 1} & set(range(B))):
            try:
                bo.check_poison(f, x, p, value, base=base, what="host")
            except AssertionError:
                bad.append(f"{name}{p}")
    return bad


@pytest.mark.parametrize("B", [8, 17, 33])
def test_clean_function_passes_every_relation(B):
    assert failed_relations(layer, inputs(B)) == []


@pytest.mark.parametrize("fault", FAULTS)
def test_each_planted_fault_is_caught(fault):
    f = lambda x, t: layer(x, t, fault)
    bad = failed_relations(f, inputs(33))
    print(f"[{fault}] caught by: {' '.join(bad)}")
    assert bad, f"{fault}: no relation noticed"
    # which relations can see which fault
    if fault == "odd_rounding":
        assert all(b.startswith("rot") for b in bad), bad                                # no poison sees a rounding
        even = failed_relations(f, inputs(32))
        assert even and all(int(b[3:]) % 2 == 1 for b in even), even                     # nor a rotation that keeps the parity
    if fault == "halo_row":
        assert "nan16" in bad and "nan0" not in bad and "rot1" in bad, bad
    if fault == "neighbour_stats":
        assert {"rot1", "nan0", "big0"} <= set(bad), bad
    if fault == "swap_at_16":
        assert "rot1" in bad and failed_relations(f, inputs(8)) == [], "the fault only exists from batch 16"


def test_failure_messages_name_positions_and_size():
    x = inputs(33)
    with pytest.raises(AssertionError, match=r"rotation by 1 of batch 33, output 0: .*positions differ.*largest difference"):
        bo.check_rotation(lambda a, t: layer(a, t, "halo_row"), x, 1, what="msg")
    with pytest.raises(AssertionError, match=r"sample\(s\) \[16\] of batch 33 poisoned with nan, output 0: samples \[15\] changed"):
        bo.check_poison(lambda a, t: layer(a, t, "halo_row"), x, 16, what="msg")
    with pytest.raises(AssertionError, match="it was not read"):
        bo.check_poison(lambda a, t: layer(a * 0, t * 0 + 1, None).nan_to_num(), x, 2, what="msg")
    # two samples poisoned together; a tensor on its own instead of a tuple; a tuple of outputs
    bo.check_poison(layer, x, (15, 16))
    one = lambda a: (a * 2, a.flatten(1).sum(1, keepdim=True))
    bo.check_rotation(one, x[0], 5)
    bo.check_poison(one, x[0], 32, bo.BIG)


def test_helpers():
    x = bo.distinct_batch(64, (4, 32, 32), 3)
    m, s = x.mean((1, 2, 3)), x.std((1, 2, 3))
    assert bool((m[0::2] > 0).all()) and bool((m[1::2] < 0).all())
    assert bool((s[1:] > s[:-1] * 0.95).all()) and 0.45 < float(s[0]) < 0.55 and 1.9 < float(s[63]) < 2.1
    assert float((m.abs()[8:] - m.abs()[:-8]).min()) > 0                       # the offset grows with b
    assert bo.distinct_batch(3, (5,), 1, torch.bfloat16).dtype == torch.bfloat16
    assert torch.equal(bo.distinct_batch(5, (7,), 9), bo.distinct_batch(5, (7,), 9))
    t = torch.arange(12.0).view(4, 3)
    ints = torch.arange(4)
    pt, pi = bo.poisoned((t, ints), (1, 3), math.nan)
    assert torch.isnan(pt[[1, 3]]).all() and torch.equal(pt[[0, 2]], t[[0, 2]]) and torch.equal(pi, ints)
    assert torch.equal(bo.poisoned(t, 2, bo.BIG)[0][2], t[2] * 1e4) and float(t[2, 0]) == 6.0      # the input is not written
    y = torch.zeros(2, 3)
    y.gn_partial = torch.ones(2, 1, 3, 2)
    assert len(bo.outputs((y, torch.zeros(2)))) == 3
