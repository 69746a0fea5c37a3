"""The default aspect buckets (config.ImageConfig.supported_dims) against the shapes the GPU tests hard-code: no GPU.

tests/_buckets.py derives latent shapes, level shapes and token counts from the config; tests/_bucket_cases.py holds the
numbers the GPU parametrizations use.  Every one of those numbers must be a member of the derived table, so a change to the
bucket list fails here instead of silently leaving the GPU tests at shapes the trainer no longer meets."""
import _bucket_cases as BK
import _buckets as T

# the issue's table: per-sample pixels at level 0 / 1 / 2, one row per bucket pair, plus the square bucket
TOKEN_TRIPLES = {(15360, 3840, 960), (15808, 3952, 988), (16128, 4032, 1008), (16384, 4096, 1024)}
BATCHES = (1, 2, 3, 4)          # the batch sizes the op-level cases use


def test_there_are_nine_buckets_with_latent_sides_divisible_by_8():
    lat = T.latent_shapes()
    assert len(lat) == 9 and len(set(lat)) == 9
    for H, W in lat:
        assert H % 8 == 0 and W % 8 == 0, (H, W)
    assert {(W, H) for H, W in lat} == set(lat)                 # both orientations of every bucket
    assert (128, 128) in lat and (96, 168) in lat and (168, 96) in lat


def test_token_count_triples_are_the_four_families_and_the_square():
    triples = {T.level_tokens(H, W) for H, W in T.latent_shapes()}
    # 896 x 1152 and 1344 x 768 share their token counts (16128 / 4032 / 1008) with other row widths: four distinct triples
    assert triples == TOKEN_TRIPLES
    assert T.tokens_at_level(0) == [15360, 15808, 16128, 16384]
    assert T.tokens_at_level(1) == [3840, 3952, 4032, 4096]
    assert T.tokens_at_level(2) == [960, 988, 1008, 1024]


def test_level_shapes_halve_twice():
    assert T.level_shapes(104, 152) == [(104, 152), (52, 76), (26, 38)]
    assert T.level_shapes(192, 80) == [(192, 80), (96, 40), (48, 20)]
    assert T.level_of(52, 76) == [1] and T.level_of(42, 24) == [2] and T.level_of(50, 50) == []
    assert T.non_transposed() == [(80, 192), (96, 168), (104, 152), (112, 144)]


def _assert_image(h, w, levels=(0, 1, 2), what=""):
    lv = T.level_of(h, w)
    assert lv and set(lv) <= set(levels), f"{what}: {h} x {w} is at levels {lv} of the default buckets, wanted one of {levels}"


def test_conv_cases_are_bucket_level_images():
    for B, H, W, Cin, Cout, stride in BK.CONV_S1:
        assert stride == 1 and B in BATCHES
        _assert_image(H, W, what="conv stride 1")
    # one level-2, one level-1 and one level-0 image for each of the seven (H, W) orientations that had none
    for level, n in ((2, 7), (1, 7), (0, 7)):
        at = {(H, W) for _, H, W, *_ in BK.CONV_S1 if T.level_of(H, W) == [level]}
        assert len(at) == n, (level, sorted(at))
    new = set(T.latent_shapes()) - {(128, 128), (96, 168)}
    assert {(H, W) for _, H, W, *_ in BK.CONV_S1 if T.level_of(H, W) == [0]} == new
    for B, H, W, Cin, Cout in BK.CONV_S2_DGRAD:                 # the image a down-sampler reads: level 0 or 1
        _assert_image(H, W, (0, 1), "conv stride 2")
    for B, H, W, Cin, Cout in BK.UPCONV:                        # the image an up-sampler reads: level 2 or 1
        _assert_image(H, W, (1, 2), "upsampling conv")
    assert [(B * H * W) % 64 == 0 for B, H, W, _, _ in BK.UPCONV] == [False, False, True, False, True]
    # the 832 x 1216 bucket has no whole 64-pixel reduction steps at its level-2 up-sampler's input at any batch size up to 4, and at
    # its level-1 up-sampler's input only at B = 4 (15 808 = 247 * 64): the weight gradient on the upsampled image is what it runs
    assert all((b * 26 * 38) % 64 for b in BATCHES)
    assert [b for b in BATCHES if (b * 52 * 76) % 64 == 0] == [4]
    for B, H, W, Cin, Cout in BK.CONV_WGRAD3:
        _assert_image(H, W, (0,), "three-tap weight gradient")
        assert W % 64 == 0 and W // 64 == 3
    assert [B * H * W >= 16384 for B, H, W, _, _ in BK.CONV_WGRAD3] == [True, True, False]


def test_token_cases_are_bucket_token_counts():
    l1, l2 = set(T.tokens_at_level(1)), set(T.tokens_at_level(2))
    for B, heads, Nq, Nk, self_attn in BK.ATTENTION:
        assert Nq in (l1 if heads == 10 else l2), (heads, Nq)               # 10 heads of 64 = the 640-wide level, 20 = the 1280-wide one
        assert Nk == (Nq if self_attn else 77)
    assert any(B > 1 and Nq % 64 for B, _, Nq, _, _ in BK.ATTENTION)        # a (batch, head) seam at a ragged row count
    for B, heads, Nq, Nk in BK.ATTENTION_BWD_PL:
        assert Nq == Nk and Nq in l1 | l2
    for B, Nq, N, K, addend in BK.LINEAR_DGRAD_DELTA:
        assert Nq in l2 and N == K == 1280 and B in BATCHES
    rows = {640: set(T.rows_multiples(l1, BATCHES)), 1280: set(T.rows_multiples(l2, BATCHES))}
    for M, Cc in BK.LAYERNORM:
        assert M in rows[Cc], (M, Cc)
    for M, K, C4, G in BK.FF_GEGLU:
        assert M in rows[K] and C4 == 4 * K, (M, K, C4)
    by_level = {0: (320, 640, 960), 1: (320, 640, 960, 1280, 1920), 2: (640, 1280, 1920, 2560)}      # channel counts of the GroupNorms at each level
    for B, HW, Cc, silu in BK.GROUPNORM:
        assert any(HW in T.tokens_at_level(l) and Cc in cs for l, cs in by_level.items()), (HW, Cc)


def test_gemm_cases_pair_row_counts_with_widths_of_their_level():
    l1, l2 = T.tokens_at_level(1), T.tokens_at_level(2)
    rows = {640: set(T.rows_multiples(l1, (1, 4))), 1280: set(T.rows_multiples(l2, (1, 4)))}
    widths = {(1920, 640), (640, 640), (3840, 1280), (1280, 1280), (1280, 5120)}          # (N, K): qkv, out, qkv, out, ff.net.2
    level_width = lambda N, K: 640 if (N, K) in ((1920, 640), (640, 640)) else 1280
    cases = [(M, N, K) for M, N, K in BK.GEMM_NT + BK.GEMM_NN] + [(R, Mo, No) for Mo, No, R, _ in BK.GEMM_TN] + \
            [(R, Mo, No) for Mo, No, R in BK.GEMM_TN_LONG]
    assert 12 <= len(cases) <= 16
    for M, N, K in cases:
        assert (N, K) in widths, (N, K)
        assert M in rows[level_width(N, K)], (M, N, K)
        assert M in (988, 3952, 15808, 960, 3840, 15360)
    assert {R for _, _, R, _ in BK.GEMM_TN} | {R for _, _, R in BK.GEMM_TN_LONG} >= {988, 3952, 15808}      # the ragged reductions
    assert 15808 == 247 * 64 and 988 % 64 == 28 and 3952 % 64 == 48
    assert any(s == 0 for *_, s in BK.GEMM_TN)                                               # the policy's own split-K


def test_model_cases_are_bucket_latents():
    lat = set(T.latent_shapes())
    assert {(H, W) for _, H, W in BK.TINY_LATENTS} == lat and all(B == 1 for B, _, _ in BK.TINY_LATENTS)
    assert len(BK.TINY_LATENTS) == 9
    for B, H, W in BK.TINY_LATENTS_B2:
        assert B == 2 and (H, W) in lat
    assert len(BK.TINY_DDPM) == 4 and set(BK.TINY_DDPM) <= set(BK.TINY_LATENTS)
    assert not any((1, W, H) in BK.TINY_DDPM for _, H, W in BK.TINY_DDPM)                    # one orientation of each
    assert BK.TINY_REPEAT in BK.TINY_LATENTS_B2 and BK.TINY_REPEAT[2] % 64 == 0
    for B, H, W in BK.SHALLOW_ORACLE + BK.SHALLOW_DECOMPOSE + BK.SHALLOW_MIXED:
        assert (H, W) in lat, (H, W)
    assert all(B == 1 for B, _, _ in BK.SHALLOW_ORACLE) and all(B == 4 for B, _, _ in BK.SHALLOW_DECOMPOSE + BK.SHALLOW_MIXED)
    # the two new row-count families
    assert {T.level_tokens(H, W) for _, H, W in BK.SHALLOW_ORACLE} == {(15808, 3952, 988), (15360, 3840, 960)}
