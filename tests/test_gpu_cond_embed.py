"""afldm_cond_embed / afldm_cond_embed_flat on MI355X, bit for bit: act[r] = silu(rnd(emb_table[s] + class_rows[r])) against torch's
add in the same dtype (one rounding) followed by ops.silu (k_silu, the same SiLU device code).  No tolerance anywhere.  Shapes: one
row, two, an odd count, more rows than one workgroup's items at D = 8 (128 rows: one 256-thread workgroup holds 256 items) and
several workgroups at the wider rows; D = 8 (one item per row), 256 (the tiny UNet) and 896 (UNet2DModel's default
config, 4 x 224; no multiple of 256).  A counter outside the table is checked over the same matrix."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 3
SENTINEL = 7.5          # exact in bf16
DTYPES = [torch.float32, torch.bfloat16]


def _case(rows, D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * rows + D)
    table = (torch.randn(N, D, generator=g) * 2).to(dtype).cuda()
    cls = (torch.randn(rows, D, generator=g) * 2).to(dtype).cuda()
    return table, cls


def _act(rows, D, dtype):
    """(act [rows, D], the whole buffer [rows + 1, D]): a sentinel row lies directly behind act."""
    buf = torch.full((rows + 1, D), SENTINEL, dtype=dtype, device="cuda")
    return buf[:rows], buf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [8, 256, 896])
@pytest.mark.parametrize("rows", [1, 2, 3, 128])
@pytest.mark.parametrize("s", [0, 2])
def test_cond_embed_bits(rows, D, dtype, s):
    from afldm_amd import ops
    table, cls = _case(rows, D, dtype)
    idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
    act, buf = _act(rows, D, dtype)
    out = ops.cond_embed(table, idx, cls, out=act)
    assert out.data_ptr() == act.data_ptr()
    want = ops.silu((table[s] + cls).to(dtype).contiguous())          # torch's add rounds once; ops.silu is k_silu
    assert torch.equal(act, want)
    assert torch.equal(buf[rows], torch.full_like(buf[rows], SENTINEL))          # nothing behind the last row
    assert int(idx.item()) == s                                                   # the counter is read, never advanced
    # zero class rows: silu(emb_table[s]) in every row
    act0, buf0 = _act(rows, D, dtype)
    ops.cond_embed(table, idx, torch.zeros_like(cls), out=act0)
    assert torch.equal(act0, ops.silu(table[s].contiguous()).unsqueeze(0).expand(rows, D))
    assert torch.equal(buf0[rows], torch.full_like(buf0[rows], SENTINEL))
    # the flat form: one broadcast row, and a row per sample
    act1, buf1 = _act(rows, D, dtype)
    ops.cond_embed_flat(table[s:s + 1].contiguous(), cls, out=act1)
    assert torch.equal(act1, act) and torch.equal(buf1[rows], torch.full_like(buf1[rows], SENTINEL))
    act2, buf2 = _act(rows, D, dtype)
    ops.cond_embed_flat(table[s:s + 1].expand(rows, D).contiguous(), cls, out=act2)
    assert torch.equal(act2, act) and torch.equal(buf2[rows], torch.full_like(buf2[rows], SENTINEL))


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_see_their_own_embedding_in_the_flat_form(dtype):
    """emb_rows = rows with DIFFERENT rows (a [B] timestep): row r adds emb[r], not emb[0]."""
    from afldm_amd import ops
    table, cls = _case(3, 256, dtype)
    act, buf = _act(3, 256, dtype)
    ops.cond_embed_flat(table, cls, out=act)
    assert torch.equal(act, ops.silu((table + cls).to(dtype).contiguous()))
    assert torch.equal(buf[3], torch.full_like(buf[3], SENTINEL))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [8, 256, 896])
@pytest.mark.parametrize("rows", [1, 2, 3, 128])
@pytest.mark.parametrize("s", [-1, N])
def test_a_counter_outside_the_table_writes_nothing(rows, D, dtype, s):
    from afldm_amd import ops
    table, cls = _case(rows, D, dtype)
    idx = torch.full((1,), s, dtype=torch.int32, device="cuda")
    act, buf = _act(rows, D, dtype)
    ops.cond_embed(table, idx, cls, out=act)
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.full_like(buf, SENTINEL)) and int(idx.item()) == s


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_width_that_is_no_multiple_of_8_is_refused(dtype):
    from afldm_amd import _lib, ops
    table = torch.zeros(N, 12, dtype=dtype, device="cuda")
    cls = torch.zeros(2, 12, dtype=dtype, device="cuda")
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    act, buf = _act(2, 12, dtype)
    code = _lib.DTYPE_CODE[dtype]
    assert _lib.lib.afldm_cond_embed(table.data_ptr(), N, idx.data_ptr(), cls.data_ptr(), act.data_ptr(), 2, 12, code,
                                     _lib.stream_ptr()) == -1                    # AFLDM_ESHAPE
    assert _lib.lib.afldm_cond_embed_flat(table.data_ptr(), 1, cls.data_ptr(), act.data_ptr(), 2, 12, code, _lib.stream_ptr()) == -1
    with pytest.raises(_lib.AfldmError):
        ops.cond_embed(table, idx, cls, out=act)
    with pytest.raises(_lib.AfldmError):
        ops.cond_embed_flat(table[:1].contiguous(), cls, out=act)
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.full_like(buf, SENTINEL))
