"""One problem per instance of the linear kernels (qe_linear.hip), shared by the CPU coverage test and the GPU tests of every
epilogue.

ROWS: int8 x int8 problems, (B, K, O, env, form, note).  `form` is what qe_quantlinear_form must name with `env` applied:
0 = linear_generic_kernel<false> (the order-preserving fp32 kernel), 1 = linear_mfma_kernel<2> (64-deep, 128 x 128 tiles),
2 = linear_mfma_kernel<4> (64-deep, 128 x 256), 3 = linear_mfma8_kernel<2> (8 waves, 320 x 256), 4 = linear_mfma8_kernel<1>
(4 waves, 160 x 256).  The MFMA forms run every epilogue on the same kernel -- F32 (qe_quantlinear), CODES / CODES_GELU
(qe_quantlinear_requant) and RES (qe_quantlinear_residual) -- so a row reaches four template instances; form 0 has only
the F32 one (the fused entries run it in two passes).

F_ROWS: fp32-activation problems (qe_quantlinear_float_input), same layout; form 1 = linear_f32_mfma_kernel (F32 and, through
qe_quantlinear_float_input_residual, RES), 0 = linear_generic_kernel<true>.

The first rows are real ViT layer shapes (S/16, B/16, L/16, H/14 at 1, 16, 64 and 256 images: 197 or 257 tokens per image,
196 or 256 patches) that the planner places without knobs; the forced rows after them take each kernel to its edges.
XQ[i % 3] is the activation quantiser of row i (the GPU tests draw the operands with it)."""

F32, CODES, CODES_GELU, RES = "F32", "CODES", "CODES_GELU", "RES"
EPIS = (F32, CODES, CODES_GELU, RES)
KERNEL = {0: "linear_generic_kernel<false>", 1: "linear_mfma_kernel<2>", 2: "linear_mfma_kernel<4>",
          3: "linear_mfma8_kernel<2>", 4: "linear_mfma8_kernel<1>"}
F_KERNEL = {0: "linear_generic_kernel<true>", 1: "linear_f32_mfma_kernel"}

N4 = {"QE_LIN_NJ": "4"}
W8, W4 = {"QE_LIN8": "1"}, {"QE_LIN8": "2"}

ROWS = [
    # ---- placed by the planner ----
    (12608, 768, 3072, None, 4, "ViT-B/16 fc1 at 64 images"),
    (12608, 3072, 768, None, 3, "ViT-B/16 fc2 at 64 images"),
    (12608, 768, 768, None, 4, "ViT-B/16 q / k / v at 64 images"),
    (12544, 768, 768, None, 4, "ViT-B/16 patch GEMM at 64 images"),
    (64, 768, 1000, None, 1, "ViT-B/16 head at 64 images: one ragged row tile, O % 16 = 8"),
    (197, 768, 768, None, 1, "ViT-B/16 q / k / v at 1 image"),
    (3152, 768, 3072, None, 4, "ViT-B/16 fc1 at 16 images"),
    (3152, 3072, 768, None, 1, "ViT-B/16 fc2 at 16 images: 48 stages on the three-slot ring"),
    (50432, 768, 768, None, 4, "ViT-B/16 q / k / v at 256 images"),
    (50432, 3072, 768, None, 3, "ViT-B/16 fc2 at 256 images"),
    (50432, 384, 384, None, 2, "ViT-S/16 q / k / v at 256 images"),
    (50432, 1536, 384, None, 2, "ViT-S/16 fc2 at 256 images"),
    (12608, 384, 1536, None, 4, "ViT-S/16 fc1 at 64 images"),
    (12608, 1536, 384, None, 1, "ViT-S/16 fc2 at 64 images"),
    (12608, 4096, 1024, None, 3, "ViT-L/16 fc2 at 64 images: 32 stages, the two-slot ring wraps"),
    (3152, 4096, 1024, None, 1, "ViT-L/16 fc2 at 16 images"),
    (16448, 5120, 1280, None, 3, "ViT-H/14 fc2 at 64 images: 40 stages"),
    (257, 1280, 1280, None, 1, "ViT-H/14 q / k / v at 1 image"),
    (256, 588, 1280, None, 0, "ViT-H/14 patch GEMM at 1 image: K = 588 is not a multiple of 64"),
    # ---- forced onto a kernel: the edges ----
    (1, 256, 512, W8, 3, "B = 1"),
    (1, 128, 256, W4, 4, "B = 1, a single stage"),
    (1, 64, 256, N4, 2, "B = 1, a single stage"),
    (1, 64, 16, None, 1, "B = 1, a single stage, O < 64"),
    (100, 256, 256, W8, 3, "fewer rows than one tile"),
    (70, 3072, 256, W4, 4, "fewer rows than one tile, 24 stages through the one stage buffer"),
    (33, 192, 512, N4, 2, "fewer rows than one tile"),
    (333, 1024, 512, W8, 3, "ragged last row tile"),
    (700, 128, 512, W8, 3, "a single stage, ragged last row tile"),
    (481, 384, 768, W4, 4, "ragged last row tile"),
    (370, 128, 512, W4, 4, "a single stage, ragged last row tile"),
    (300, 64, 512, N4, 2, "a single stage, ragged last row tile"),
    (130, 64, 96, None, 1, "a single stage, O % 64 = 32"),
    (129, 3072, 96, None, 1, "deep K: 48 stages"),
    (200, 4096, 512, N4, 2, "deep K: 64 stages"),
    (650, 5120, 256, W8, 3, "deep K: 40 stages, ragged"),
    (330, 4096, 256, W4, 4, "deep K: 32 stages, ragged"),
    (257, 192, 40, None, 1, "O < 64, O % 16 = 8"),
    (300, 128, 36, N4, 2, "O < 64, O % 16 = 4"),
    (333, 256, 200, N4, 2, "O % 16 = 8, ragged both ways"),
    (64, 100, 40, None, 0, "K % 64 != 0"),
]

F_ROWS = [
    (197, 768, 768, None, 1, "ViT-B/16 out_proj at 1 image"),
    (12608, 768, 768, None, 1, "ViT-B/16 out_proj at 64 images"),
    (257, 1280, 1280, None, 1, "ViT-H/14 out_proj at 1 image"),
    (333, 3072, 96, None, 1, "deep K, ragged rows and columns"),
    (1, 32, 1, None, 1, "B = O = 1, a single stage"),
    (64, 100, 40, None, 0, "K % 32 != 0"),
    (197, 768, 768, {"QE_LIN_F32_MFMA": "0"}, 0, "ViT-B/16 out_proj on the fp32 chain kernel"),
]

# activation quantiser of row i: (signed codes, per-row scales, asymmetric zero points)
XQ = [(True, False, False), (True, True, True), (False, True, True)]


def epilogues(form):
    """The epilogues whose template instance a row of this form runs."""
    return EPIS if form != 0 else (F32,)


def f_epilogues(form):
    return (F32, RES) if form == 1 else (F32,)


def instances(row):
    return {(KERNEL[row[4]], e) for e in epilogues(row[4])}


def f_instances(row):
    return {(F_KERNEL[row[4]], e) for e in f_epilogues(row[4])}


def covered():
    out = set()
    for r in ROWS:
        out |= instances(r)
    for r in F_ROWS:
        out |= f_instances(r)
    return out


def every_instance():
    """The 20 instances the linear launchers can select."""
    out = {(KERNEL[f], e) for f in (1, 2, 3, 4) for e in EPIS}
    out |= {(KERNEL[0], F32), (F_KERNEL[0], F32), (F_KERNEL[1], F32), (F_KERNEL[1], RES)}
    return out
