"""Host checks of the convolution planner (no GPU: afldm_conv2d_tune and the plan queries only read their arguments).

  * afldm_conv2d_tune accepts exactly the live variant ids; every other id in 0 ... 68, and 69 and 255, is refused and leaves
    the forcing as it was.
  * The plan of the benchmark UNet's convolution sites and of the AF-VAE's 3x3 sites is pinned: afldm_conv2d_variant,
    afldm_conv2d_stats_splits and afldm_conv2d_workspace must equal conv_plan_table.json, which was recorded from the library
    of the commit BEFORE the variant table was rewritten (69 dense ids, three descriptions per variant), so the rewrite and
    whatever follows it is held to that plan.  A deliberate change of plan regenerates the table, from the library that holds the
    new plan, with the path of that library in AFLDM_LIB and

        AFLDM_LIB=.../libafldm_hip.so PYTHONPATH=tests python -c "import json, test_conv_plan_host as t; \\
            json.dump(t.record(), open(t.TABLE, 'w'), separators=(',', ':'))"          (from the repository root)
"""
import ctypes
import json
import os


LIVE_CONV_VARIANTS = [0, 1, 3, 29, 30, 31, 32, 33, 41, 43, 46, 51, 52, 54, 55, 58, 63, 65, 66, 67, 68]
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_plan_table.json")
BATCHES = (1, 8, 64)


def unet_sites():
    """(H, C1, C2, Cout, KS) of the FFHQ UNet (configs.py: block_out_channels [192, 384, 384, 768, 768], two layers per block,
    32^2 latents, attention at every level): conv1 / conv2 of every ResnetBlock2D (conv1 of the up path over the virtual concat
    hidden | skip), the 1x1 conv_shortcut, the fused q | k | v projection and to_out of every attention block, conv_in / conv_out."""
    chans = [192, 384, 384, 768, 768]
    sites = {(32, 4, 0, 192, 3), (32, 192, 0, 4, 3)}
    skips, prev = [(32, 192)], 192
    for lvl, c in enumerate(chans):                     # down path
        H = 32 >> lvl
        for _ in range(2):
            sites |= {(H, prev, 0, c, 3), (H, c, 0, c, 3), (H, c, 0, 3 * c, 1), (H, c, 0, c, 1)}
            if prev != c:
                sites.add((H, prev, 0, c, 1))
            prev = c
            skips.append((H, c))
        if lvl < 4:
            skips.append((H >> 1, c))                   # (the downsampler keeps the channel count)
    sites |= {(2, 768, 0, 768, 3), (2, 768, 0, 2304, 1), (2, 768, 0, 768, 1)}      # mid block
    for lvl in range(4, -1, -1):                        # up path: three resnets per block, each over hidden | skip
        H, c = 32 >> lvl, chans[lvl]
        for _ in range(3):
            _, s = skips.pop()
            sites |= {(H, prev, s, c, 3), (H, c, 0, c, 3), (H, prev, s, c, 1), (H, c, 0, 3 * c, 1), (H, c, 0, c, 1)}
            prev = c
    # the 3x3 convolutions of the 2^2 level in their dense form: one row per sample over the flattened plane
    for (H, c1, c2, co, ks) in sorted(sites):
        if H == 2 and ks == 3:
            sites.add((1, 4 * c1, 4 * c2, 4 * co, 1))
    return sorted(sites)


def vae_sites():
    """(H, C1, C2, Cout, KS = 3) of the AF-VAE (bench.py build_vae: [128, 256, 512, 512], two layers per block, 256^2 images):
    encoder, decoder (three resnets per up block, an upsampling convolution at the doubled size) and both mid blocks."""
    sites = set()
    enc = [(256, 128, 128), (128, 128, 256), (64, 256, 512), (32, 512, 512)]
    for H, cin, c in enc:
        sites |= {(H, cin, 0, c, 3), (H, c, 0, c, 3)}
    dec = [(32, 512, 512), (64, 512, 512), (128, 512, 256), (256, 256, 128)]
    for H, cin, c in dec:
        sites |= {(H, cin, 0, c, 3), (H, c, 0, c, 3)}
        if H < 256:
            sites.add((2 * H, c, 0, c, 3))
    return sorted(sites)


def cases():
    """[dtype, B, H, W, C1, C2, Cout, KS]: every UNet site at B = 1, 8, 64 and every AF-VAE site at B = 1, 8 (64^2 - 256^2 planes at
    64 samples are the same plan: the plan depends on the rows only through thresholds they are far beyond), both dtypes."""
    out = []
    for dt in (0, 1):
        for B in BATCHES:
            out += [[dt, B, H, H, c1, c2, co, ks] for (H, c1, c2, co, ks) in unet_sites()]
        for B in (1, 8):
            out += [[dt, B, H, H, c1, c2, co, ks] for (H, c1, c2, co, ks) in vae_sites()]
        out += [[dt, 64, H, H, 128, 0, 128, 3] for H in (64, 128, 256)]
    return out


def query(lib, ConvArgs, case):
    """(variant code, statistics splits, workspace bytes) with a workspace as large as any plan asks for."""
    dt, B, H, W, C1, C2, Cout, KS = case
    a = ConvArgs()
    base = 0x10000000                                    # dummy 16-byte aligned addresses: the queries never dereference them
    a.x1, a.w, a.y, a.bias = base, base + 16, base + 32, base + 48
    a.x2 = base + 64 if C2 else None
    a.workspace, a.workspace_bytes = base + 80, 1 << 40
    a.C1, a.C2, a.B, a.H, a.W, a.Cout, a.KS = C1, C2, B, H, W, Cout, KS
    a.y_ld, a.res_ld, a.dtype = Cout, Cout, dt
    r = ctypes.byref(a)
    return [lib.afldm_conv2d_variant(r), lib.afldm_conv2d_stats_splits(r), lib.afldm_conv2d_workspace(r)]


def record():
    from afldm_amd import _lib
    return [c + query(_lib.lib, _lib.ConvArgs, c) for c in cases()]


def test_tune_accepts_exactly_the_live_variants():
    from afldm_amd import _lib
    lib = _lib.lib
    try:
        for v in list(range(69)) + [69, 255]:
            rc = lib.afldm_conv2d_tune(v, -1)
            if v in LIVE_CONV_VARIANTS:
                assert rc == 0, f"live variant {v} refused: {lib.afldm_last_error()}"
            else:
                assert rc != 0, f"variant {v} accepted"
                assert str(v).encode() in lib.afldm_last_error(), lib.afldm_last_error()
    finally:
        assert lib.afldm_conv2d_tune(-1, -1) == 0


def test_a_refused_variant_leaves_the_forcing_alone_and_minus_one_resets_it():
    from afldm_amd import _lib
    lib = _lib.lib
    case = [1, 64, 32, 32, 192, 0, 192, 3]              # automatic plan: the halo-patch tile 41
    auto = query(lib, _lib.ConvArgs, case)
    assert auto[0] & 255 == 41
    try:
        assert lib.afldm_conv2d_tune(29, 1) == 0
        assert query(lib, _lib.ConvArgs, case)[0] & 255 == 29
        assert lib.afldm_conv2d_tune(40, 1) != 0         # retired: the forcing of 29 stays
        assert query(lib, _lib.ConvArgs, case)[0] & 255 == 29
    finally:
        assert lib.afldm_conv2d_tune(-1, -1) == 0
    assert query(lib, _lib.ConvArgs, case) == auto


def test_site_tables_cover_what_they_claim():
    u, v = unet_sites(), vae_sites()
    for H in (32, 16, 8, 4, 2):
        assert any(s[0] == H and s[4] == 3 and s[2] == 0 for s in u) and any(s[0] == H and s[4] == 3 and s[2] > 0 for s in u)
        assert any(s[0] == H and s[4] == 1 and s[2] == 0 for s in u) and any(s[0] == H and s[4] == 1 and s[2] > 0 for s in u)
    assert (1, 3072, 0, 3072, 1) in u and (1, 3072, 3072, 3072, 1) in u
    assert {s[0] for s in v} == {32, 64, 128, 256} and all(s[4] == 3 for s in v)


def test_plan_of_the_model_sites_is_the_recorded_one():
    from afldm_amd import _lib
    with open(TABLE) as f:
        table = json.load(f)
    assert [row[:8] for row in table] == cases(), "conv_plan_table.json does not list the cases of this file"
    wrong = []
    for row in table:
        got = query(_lib.lib, _lib.ConvArgs, row[:8])
        if got != row[8:]:
            wrong.append((row[:8], row[8:], got))
    assert not wrong, f"{len(wrong)} of {len(table)} plans changed; first: {wrong[:5]}"
    assert {row[8] & 255 for row in table if row[8] >= 0} <= set(LIVE_CONV_VARIANTS)
