"""One problem per instance of the linear kernels (qe_linear.hip, qe_linear_bf16in.hip), shared by the CPU coverage test and
the GPU tests of every epilogue.

ROWS: int8 x int8 problems, (B, K, O, env, form, note).  `form` is what qe_quantlinear_form must name with `env` applied:
0 = linear_generic_kernel<false> (the order-preserving fp32 kernel, LIN_FORM_CHAIN), 1 = linear_mfma_kernel<2> (64-deep,
128 x 128 tiles, LIN_FORM_NJ2), 2 = linear_mfma_kernel<4> (64-deep, 128 x 256, LIN_FORM_NJ4), 3 = linear_mfma8_kernel<2>
(8 waves, 320 x 256, LIN_FORM_W8), 4 = linear_mfma8_kernel<1> (4 waves, 160 x 256, LIN_FORM_W4).  The MFMA forms run every
epilogue on the same kernel -- F32 (qe_quantlinear), CODES / CODES_GELU (qe_quantlinear_requant), RES
(qe_quantlinear_residual) and BF16 (qe_quantlinear_bf16) -- so a row reaches five template instances; tests/
test_linear_bf16_gpu.py runs the BF16 one on the rows with B <= 3152 (BF16_MAX_B).  Form 0 has only the F32 instance (the
fused entries run it in two passes).

F_ROWS: fp32-activation problems (qe_quantlinear_float_input), same layout; form 1 = linear_f32_mfma_kernel (the fp32 rows
split into three bf16 parts, LIN_FORM_F32_SPLIT: F32 and, through qe_quantlinear_float_input_residual, RES),
0 = linear_generic_kernel<true> (LIN_FORM_CHAIN_F32).

bf16-activation problems (qe_quantlinear_bf16_input) are the rows of tests/lin_bf16in_instances.py: path 1 =
linear_bf16in_kernel (bf16 rows as stored, LIN_FORM_BF16_ROWS: F32 and, with a residual, RES -- tests/
test_linear_bf16_input_gpu.py runs both on every row), path 0 = the widening pass and a float-input kernel.

The first rows are real ViT layer shapes (S/16, B/16, L/16, H/14 at 1, 16, 64 and 256 images: 197 or 257 tokens per image,
196 or 256 patches) that the planner places without knobs; the forced rows after them take each kernel to its edges.
XQ[i % 3] is the activation quantiser of row i (the GPU tests draw the operands with it)."""
import lin_bf16in_instances as bi

F32, CODES, CODES_GELU, RES, BF16 = "F32", "CODES", "CODES_GELU", "RES", "BF16"
EPIS = (F32, CODES, CODES_GELU, RES, BF16)
KERNEL = {0: "linear_generic_kernel<false>", 1: "linear_mfma_kernel<2>", 2: "linear_mfma_kernel<4>",
          3: "linear_mfma8_kernel<2>", 4: "linear_mfma8_kernel<1>"}
F_KERNEL = {0: "linear_generic_kernel<true>", 1: "linear_f32_mfma_kernel"}
B_KERNEL = "linear_bf16in_kernel"
BF16_MAX_B = 3152        # tests/test_linear_bf16_gpu.py runs the rows up to this many batch rows

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


def epilogues(row):
    """The epilogues whose template instance a row runs: all of an MFMA form (BF16 on the rows test_linear_bf16_gpu.py runs)."""
    if row[4] == 0:
        return (F32,)
    return tuple(e for e in EPIS if e != BF16 or row[0] <= BF16_MAX_B)


def f_epilogues(form):
    return (F32, RES) if form == 1 else (F32,)


def instances(row):
    return {(KERNEL[row[4]], e) for e in epilogues(row)}


def f_instances(row):
    return {(F_KERNEL[row[4]], e) for e in f_epilogues(row[4])}


def b_instances(row):
    """A bf16-input row: both instances of linear_bf16in_kernel on path 1; on path 0 the float-input kernels, which F_ROWS
    count."""
    return {(B_KERNEL, F32), (B_KERNEL, RES)} if row[5] == 1 else set()


def covered():
    out = set()
    for r in ROWS:
        out |= instances(r)
    for r in F_ROWS:
        out |= f_instances(r)
    for r in bi.ROWS:
        out |= b_instances(r)
    return out


def every_instance():
    """The 26 instances the linear launchers can select (the non-null launchers of kLinForms in qe_linear.hip)."""
    out = {(KERNEL[f], e) for f in (1, 2, 3, 4) for e in EPIS}
    out |= {(KERNEL[0], F32), (F_KERNEL[0], F32), (F_KERNEL[1], F32), (F_KERNEL[1], RES), (B_KERNEL, F32), (B_KERNEL, RES)}
    return out
