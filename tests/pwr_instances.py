"""One shape per instance of the resident-tile 1x1 kernels (qe_conv_pwr.hip), shared by the fp32, re-quantising (RQ) and
residual block-end (RES) tests.

Each ROWS entry is (shape, base instance, note, env).  The base instance is what the launcher must select for the plain
fp32 call; the re-quantising call selects the same one with RQ, the residual call the same one with RES (stride 1 only;
7x7 planes: the 512-channel form only).  The rows also vary what these kernels branch on: strips per wave (two, many,
uneven), tiles per plane, more tiles than XCDs, batch sizes 1 and odd, non-square planes, and one QE_PWR_GROUPS split.

instance() restates only the launcher's dispatch (launch_pwr / launch_pwr7): which template instance a shape lands on
once the planner has put it on the resident-tile route.  Whether the planner does is checked on the GPU (the tests assert
the fused paths; a kernel trace names the instances)."""

PWR, PWR7 = "conv_pwr_kernel", "conv_pwr7_kernel"

# (N, IC, H, W, OC, K, stride, pad)
ROWS = [
    # tiles of 224 pixels, IC = 64: conv_pwr_kernel<7, 4, 2, 224>
    ((1, 64, 56, 56, 256, 1, 1, 0), (PWR, 4, 2, 224, False), "ResNet-50 layer1 expansion, N = 1: 14 tiles, two strips per wave", None),
    ((3, 64, 28, 16, 288, 1, 1, 0), (PWR, 4, 2, 224, False), "448-pixel planes, odd N, 9 strips on 4 waves", None),
    ((2, 64, 14, 16, 1024, 1, 1, 0), (PWR, 4, 2, 224, False), "one tile per plane, 8 strips per wave", None),
    ((1, 64, 56, 80, 256, 1, 1, 0), (PWR, 4, 2, 224, False), "4480-pixel planes (56 x 80): 20 tiles", None),
    # IC = 128: conv_pwr_kernel<7, 4, 4, 224>
    ((2, 128, 28, 40, 512, 1, 1, 0), (PWR, 4, 4, 224, False), "1120-pixel planes (28 x 40): 5 tiles", None),
    ((1, 128, 28, 16, 320, 1, 1, 0), (PWR, 4, 4, 224, False), "448-pixel planes, 10 strips on 4 waves", None),
    # IC = 256: conv_pwr_kernel<7, 8, 8, 224>
    ((2, 256, 28, 32, 512, 1, 1, 0), (PWR, 8, 8, 224, False), "896-pixel planes, two strips per wave", None),
    ((1, 256, 28, 16, 544, 1, 1, 0), (PWR, 8, 8, 224, False), "17 strips on 8 waves", None),
    # tiles of 196 pixels
    ((2, 64, 28, 28, 256, 1, 1, 0), (PWR, 4, 2, 196, False), "4 tiles per plane, two strips per wave", None),
    ((40, 64, 14, 14, 256, 1, 1, 0), (PWR, 4, 2, 196, False), "whole-plane tiles, more tiles than XCDs", None),
    ((2, 128, 28, 28, 512, 1, 1, 0), (PWR, 4, 4, 196, False), "ResNet-50 layer2 expansion", None),
    ((3, 128, 14, 14, 288, 1, 1, 0), (PWR, 4, 4, 196, False), "9 strips on 4 waves", None),
    ((2, 128, 28, 28, 512, 1, 1, 0), (PWR, 4, 4, 196, False), "two channel groups per tile", {"QE_PWR_GROUPS": "2"}),
    ((2, 256, 14, 14, 1024, 1, 1, 0), (PWR, 8, 8, 196, False), "ResNet-50 layer3 expansion", None),
    ((3, 256, 14, 14, 544, 1, 1, 0), (PWR, 8, 8, 196, False), "17 strips on 8 waves, odd N", None),
    # the stride-2 form
    ((2, 64, 28, 64, 256, 1, 2, 0), (PWR, 4, 2, 224, True), "14 x 32 output planes: 2 tiles of 7 rows", None),
    ((2, 128, 28, 64, 256, 1, 2, 0), (PWR, 4, 4, 224, True), "14 x 32 output planes", None),
    ((2, 256, 28, 64, 512, 1, 2, 0), (PWR, 8, 8, 224, True), "14 x 32 output planes", None),
    ((2, 64, 56, 56, 256, 1, 2, 0), (PWR, 4, 2, 196, True), "28 x 28 output planes: 4 tiles of 7 rows", None),
    ((1, 128, 56, 56, 512, 1, 2, 0), (PWR, 4, 4, 196, True), "ResNet-50 layer3.0 downsample shape at IC = 128", None),
    ((3, 256, 56, 56, 512, 1, 2, 0), (PWR, 8, 8, 196, True), "ResNet-50 layer2.0 downsample", None),
    # 7x7 planes
    ((2, 512, 7, 7, 2048, 1, 1, 0), (PWR7, 16, 2), "ResNet-50 layer4 expansion: 2 images per tile", None),
    ((8, 512, 7, 7, 512, 1, 1, 0), (PWR7, 16, 2), "two strips per wave", None),
    ((4, 256, 7, 7, 768, 1, 1, 0), (PWR7, 8, 4), "4 images per tile, 3 strips per wave", None),
    ((8, 128, 7, 7, 1024, 1, 1, 0), (PWR7, 4, 4), "IC = 128", None),
]


def instance(shape):
    """The base instance launch_pwr / launch_pwr7 dispatch a resident-tile shape to: (conv_pwr_kernel, WV, KS, TW, S2)
    with KS = IC / 32, 8 waves at KS = 8, TW = 224 when it divides the output plane, else 196; (conv_pwr7_kernel, KS, GI)
    on 7x7 planes by IC."""
    N, IC, H, W, OC, K, stride, pad = shape
    if stride == 1 and H * W == 49:
        return (PWR7,) + {512: (16, 2), 256: (8, 4), 128: (4, 4)}[IC]
    OH, OW = (H // 2, W // 2) if stride == 2 else (H, W)
    ks = IC // 32
    return (PWR, 8 if ks == 8 else 4, ks, 224 if (OH * OW) % 224 == 0 else 196, stride == 2)


def has_res(base):
    """The residual block end exists for stride-1 conv_pwr_kernel instances and conv_pwr7_kernel<16, 2> only."""
    return not base[-1] if base[0] == PWR else base[1:] == (16, 2)


def full(base, rq, res):
    """The template instance of an epilogue: conv_pwr_kernel<7, WV, KS, TW, S2, RQ, RES>, conv_pwr7_kernel<KS, GI, RQ, RES>."""
    return base + (rq, res)


def kernel_name(inst):
    """As a kernel trace shows it (template arguments spelled out, defaults included)."""
    b = lambda v: "true" if v else "false"
    if inst[0] == PWR:
        _, wv, ks, tw, s2, rq, res = inst
        return "%s<7, %d, %d, %d, %s, %s, %s>" % (PWR, wv, ks, tw, b(s2), b(rq), b(res))
    _, ks, gi, rq, res = inst
    return "%s<%d, %d, %s, %s>" % (PWR7, ks, gi, b(rq), b(res))


def dispatchable():
    """Every instance the launchers can select: 24 plain / RQ conv_pwr_kernel, 12 RES conv_pwr_kernel, 6 plain / RQ and
    2 RES conv_pwr7_kernel."""
    out = set()
    for wv, ks in ((4, 2), (4, 4), (8, 8)):
        for tw in (224, 196):
            for rq in (False, True):
                for s2 in (False, True):
                    out.add((PWR, wv, ks, tw, s2, rq, False))
                out.add((PWR, wv, ks, tw, False, rq, True))
    for ks, gi in ((16, 2), (8, 4), (4, 4)):
        for rq in (False, True):
            out.add((PWR7, ks, gi, rq, False))
    for rq in (False, True):
        out.add((PWR7, 16, 2, rq, True))
    return out


def covered():
    """The instances the fp32, RQ and RES tests reach through ROWS."""
    out = set()
    for _, base, _, _ in ROWS:
        for rq in (False, True):
            out.add(full(base, rq, False))
            if has_res(base):
                out.add(full(base, rq, True))
    return out


def res_rows():
    return [r for r in ROWS if has_res(r[1])]
