"""The shapes the GPU tests hard-code for the default aspect buckets (config.ImageConfig.supported_dims), in one place.

Not a test module.  tests/test_gpu_ops.py, test_gpu_model.py and test_gpu_buckets.py parametrize over these lists;
tests/test_host_buckets.py checks every one of them against the table tests/_buckets.py derives from the config, without a
GPU.  The 1024 x 1024 bucket and one orientation of 1344 x 768 have their cases in the test modules themselves (they came first);
here are the other seven: latent 80 x 192, 104 x 152, 112 x 144, their transposes, and 168 x 96.

Channel counts are small unless the channel count is part of the edge: the geometry (row widths, pixel and token counts, and
their remainders modulo the tile sizes) is what changes from bucket to bucket."""

# ---- 3x3 convolution, stride 1 (B, H, W, Cin, Cout, stride): one level-2, one level-1 and one level-0 image per width family
CONV_S1 = [
    # level 2 (B = 2, 3)
    (2, 26, 38, 128, 64, 1), (3, 38, 26, 64, 64, 1), (2, 20, 48, 64, 64, 1), (2, 48, 20, 128, 64, 1),
    (2, 28, 36, 64, 64, 1), (2, 36, 28, 128, 64, 1), (2, 42, 24, 64, 64, 1),
    # level 1 (B = 1)
    (1, 52, 76, 64, 64, 1), (1, 76, 52, 128, 64, 1), (1, 40, 96, 128, 64, 1), (1, 96, 40, 64, 64, 1),
    (1, 56, 72, 128, 64, 1), (1, 72, 56, 64, 64, 1), (1, 84, 48, 64, 64, 1),
    # level 0 (B = 1, 64 -> 64)
    (1, 104, 152, 64, 64, 1), (1, 152, 104, 64, 64, 1), (1, 80, 192, 64, 64, 1), (1, 192, 80, 64, 64, 1),
    (1, 112, 144, 64, 64, 1), (1, 144, 112, 64, 64, 1), (1, 168, 96, 64, 64, 1),
]

# ---- stride-2 convolution's input gradient by output phase (B, H, W, Cin, Cout): H x W is the image that is down-sampled
CONV_S2_DGRAD = [(2, 104, 152, 64, 128), (2, 52, 76, 64, 64), (1, 192, 80, 64, 64), (2, 40, 96, 64, 128), (1, 144, 112, 64, 64)]

# ---- conv3x3(nearest-2x(x)) (B, H, W, Cin, Cout): H x W is the LOW-resolution image.  B * H * W % 64 != 0 in the first two (and in
# (1, 52, 76)): forward and input gradient only, the plan takes the weight gradient on the upsampled image there
UPCONV = [(1, 26, 38, 128, 64), (4, 26, 38, 128, 64), (2, 20, 48, 128, 64), (1, 52, 76, 64, 64), (1, 40, 96, 64, 64)]

# ---- three-tap weight gradient (B, H, W, Cin, Cout): W = 192 is three K-steps per image row.  The last has 15 360 pixels, below
# the policy's 16 384: the same problem through the one-tap route (parity only)
CONV_WGRAD3 = [(2, 80, 192, 64, 64), (4, 80, 192, 320, 320), (1, 80, 192, 64, 64)]

# ---- attention (B, heads, Nq, Nk, self)
ATTENTION = [(1, 10, 3952, 3952, True), (1, 10, 3840, 3840, True), (1, 20, 988, 988, True), (1, 20, 960, 960, True),
             (2, 4, 988, 988, True),                   # a (batch, head) seam at a ragged row count
             (1, 10, 3952, 77, False), (1, 20, 988, 77, False)]
ATTENTION_BWD_PL = [(1, 2, 3952, 3952), (1, 4, 988, 988)]        # (B, heads, Nq, Nk), diagnostics build

# ---- out-projection dgrad with the Delta epilogue (B, Nq, N, K, addend)
LINEAR_DGRAD_DELTA = [(1, 988, 1280, 1280, True), (4, 988, 1280, 1280, False), (1, 960, 1280, 1280, True)]

LAYERNORM = [(988, 1280), (3952, 640), (15808, 640)]                                        # (rows, C)
FF_GEGLU = [(988, 1280, 5120, 80), (3952, 640, 2560, 80), (3952, 1280, 5120, 64)]           # (rows, K, C4, group)
GROUPNORM = [(1, 15808, 320, 1), (1, 3952, 960, 1), (2, 988, 1920, 0), (1, 960, 2560, 1)]   # (B, HW, C, silu)

# ---- policy-routed GEMMs at bucket row counts with the model's real widths.  640-wide layers live at level 1 (3952 / 3840 tokens;
# 15 808 / 15 360 rows at B = 4), 1280-wide at level 2 (988 / 960 tokens; 3952 / 3840 rows at B = 4).
GEMM_NT = [(3952, 1920, 640), (15808, 640, 640), (988, 3840, 1280), (988, 1280, 5120), (3840, 1280, 1280)]      # (rows, N, K)
GEMM_NN = [(15360, 640, 640), (960, 3840, 1280), (3952, 1280, 5120), (3840, 1920, 640)]                        # (rows, N, K)
GEMM_TN = [(1920, 640, 3952, 0), (3840, 1280, 988, 0), (1280, 5120, 988, 2), (1280, 1280, 3840, 1)]            # (M_out, N_out, rows, splitk)
GEMM_TN_LONG = [(640, 640, 15808), (1920, 640, 15808), (1280, 1280, 3952)]                                     # (M_out, N_out, rows) x splitk 0, 1, 3

# ---- the tiny UNet at every bucket's latent shape (B, H, W)
TINY_LATENTS = [(1, 80, 192), (1, 96, 168), (1, 104, 152), (1, 112, 144), (1, 128, 128), (1, 144, 112), (1, 152, 104), (1, 168, 96),
                (1, 192, 80)]
TINY_LATENTS_B2 = [(2, 80, 192), (2, 104, 152)]
TINY_DDPM = [(1, 80, 192), (1, 104, 152), (1, 112, 144), (1, 168, 96)]      # ddpm: one orientation of each new family (96 x 168 has its full-size tests)
TINY_REPEAT = (2, 80, 192)                     # the step that is also repeated bit for bit (three-tap path at W = 192)

# ---- the real-width shallow UNet (B, H, W)
SHALLOW_ORACLE = [(1, 104, 152), (1, 80, 192)]
SHALLOW_DECOMPOSE = [(4, 104, 152), (4, 80, 192), (4, 192, 80), (4, 112, 144)]
SHALLOW_MIXED = [(4, 104, 152), (4, 128, 128)]
