"""The problems tests/test_linear_bf16_input_{cpu,gpu}.py run qe_quantlinear_bf16_input on.

Each ROWS entry is (B, K, O, w_bits, x_offset_bytes, path, note).  path 1 = linear_bf16in_kernel (tile 128 x 128, 32-deep
stages, two stage buffers), path 0 = the widening pass + the float-input plan.  The weight regime of row i is REGIMES[i % 4].
"""
ROWS = [
    (197, 768, 768, 8, 0, 1, "one ViT-B image: two row tiles, the second ragged"),
    (12608, 768, 768, 8, 0, 1, "64 ViT-B images: 99 row tiles"),
    (257, 1280, 1280, 8, 0, 1, "ViT-H width: 40 stages, one row past two tiles"),
    (333, 3072, 96, 8, 0, 1, "deep K, ragged both ways"),
    (1, 32, 1, 8, 0, 1, "one stage, B = O = 1: element stores"),
    (130, 64, 40, 8, 0, 1, "two stages: the double buffer's first wrap, O < one tile"),
    (129, 96, 200, 8, 0, 1, "odd stage count, ragged second column tile"),
    (64, 100, 40, 8, 0, 0, "K % 32 != 0"),
    (70, 64, 48, 4, 0, 0, "4-bit weights"),
    (66, 64, 40, 8, 2, 0, "x two bytes off a 16-byte boundary"),
]

# (signed codes, per-tensor parameters, zero point kind, bias, activations)
REGIMES = [
    (True, False, "none", True, "normal"),          # signed per-channel symmetric weights
    (False, True, "mid", True, "abs"),              # unsigned per-tensor, zero point ~ the middle code, positive-mean |N(0,1)|
    (True, False, "fractional", True, "normal"),    # fractional per-channel zero points, with bias
    (True, False, "fractional", False, "normal"),   # ... without
]


def row_id(r):
    return "%dx%dx%d-w%d%s-path%d" % (r[0], r[1], r[2], r[3], "-off%d" % r[4] if r[4] else "", r[5])
