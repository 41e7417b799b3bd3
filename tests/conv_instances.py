"""One small problem per kernel instance the int8 conv planner can select outside the resident-tile route: the MFMA families
(halo, warp-specialised, two-strip, stem, flat, flat stride 2, flat 4-bit activations, flatg), the LDS-DMA ring kernel flatd
and the pre-passes (strided gathers, 8-bit expansion).  Shared by the CPU coverage test and the GPU tests of every epilogue.

An instance is named as the host-side plan names it (capi.conv_plan_info, qe_conv_plan_info in include/quant_engine.h):

    ("halo", cfg, niw, kkt, ns, rq, patch)   conv_mfma_kernel<WM, WN, NIW, KKT, NS, RQ, PATCH>, cfg 0 / 1 / 2 = 4x1 / 2x2 / 1x4 waves
    ("ws", niw, split, rq)                   conv_mfma_ws_kernel
    ("sm2", cfg, split, rq, patch)           conv_mfma_sm2_kernel, two strips per wave at cfg 0, one at cfg 1
    ("stem", cfg, niw, rq, patch)            conv_mfma_smallic_kernel
    ("flat", cfg, niw, ns, wraw)             conv_mfma_flat_kernel: one instance stores fp32 or codes (a runtime branch)
    ("flat_s2", cfg, niw, ns, wraw)          ... its stride-2 form
    ("flat_x4", niw, ns)                     ... its 4-bit-activation form
    ("flatg", niw, ns, wraw)                 conv_mfma_flatg_kernel
    ("flatd", w8, rq)                        conv_flatd_kernel<3, 8 | 4 waves, RQ>
    ("pre", kind, log_up)                    subsample2_kernel<LOG_UP>, subsample_kernel<wide | narrow>, subsample_x4_kernel,
                                             expand (expand_codes_s8); log_up 0 except for sub2

ROWS: (shape, x_bits, w_bits, env, expected, note) with shape = (N, IC, H, W, OC, K, stride, pad).  `expected` is the instance
conv_plan_info must name for the plain fp32 call with `env` applied: the conv kernel's fp32 instance, or for a pre-pass row
the pre-pass.  The re-quantising call of a row reaches the RQ instance (lane = pixel families), its PATCH form where the plan
picks one, and the non-PATCH form again under QE_RQ_PATCH=0: modes() lists the calls the GPU tests make of a row, launched()
the instances one call runs, covered() their union over the table.

every_instance() asks the library what it compiles (qe_conv_mfma_has_instance: the selectors stay the whole rule),
reachable() sweeps conv_plan_info over grid(), UNREACHABLE lists the compiled instances no request selects, each with the
planner condition that excludes it."""
import ctypes
import functools
import itertools

from quantize_amd import capi, resnet50

ALIGNED = 1 << 20        # a 16-byte aligned stand-in address: the queries look at alignment only

FAMILY = capi.CONV_FAMILIES
PRE = capi.CONV_PREPASSES
LANE_PIXEL = ("halo", "ws", "sm2", "stem")     # families with separate RQ (and PATCH) instances
FLAT = ("flat", "flat_s2", "flat_x4", "flatg")


def mfma_instance(family, cfg, niw, kkt, ns, split, wraw, rq, patch):
    """The name of an MFMA-family instance: the parameters its selector switches on (mfma_instance, qe_conv_mfma.hip)."""
    f = FAMILY[family] if isinstance(family, int) else family
    if f == "halo":
        return (f, cfg, niw, kkt, ns, bool(rq), bool(patch))
    if f == "ws":
        return (f, niw, split, bool(rq))
    if f == "sm2":
        return (f, cfg, split, bool(rq), bool(patch))
    if f == "stem":
        return (f, cfg, niw, bool(rq), bool(patch))
    if f in ("flat", "flat_s2"):
        return (f, cfg, niw, ns, bool(wraw))
    if f == "flat_x4":
        return (f, niw, ns)
    if f == "flatg":
        return (f, niw, ns, bool(wraw))
    raise ValueError(family)


def family_of(inst):
    return inst[1] if inst[0] == "pre" else inst[0]


PRE_INSTANCES = [("pre", "sub2", k) for k in range(3, 9)] + [("pre", k, 0) for k in ("sub_wide", "sub_narrow", "sub_x4", "expand")]
FLATD_INSTANCES = [("flatd", w8, rq) for w8 in (False, True) for rq in (False, True)]


@functools.lru_cache(maxsize=None)
def every_instance():
    """Every instance the libraries compile for these routes: what qe_conv_mfma_has_instance answers over a parameter box
    wider than any selector, plus conv_flatd_kernel's four and the ten pre-pass kernels."""
    out = set()
    for fam, cfg, niw, kkt, ns, split, wraw, rq, patch in itertools.product(
            range(1, 9), range(0, 4), range(1, 9), (0, 1, 9), (1, 2, 3, 4, 8), (1, 2, 3, 4, 8), (0, 1), (0, 1), (0, 1)):
        if capi.conv_mfma_has_instance(fam, cfg, niw, kkt, ns, split, wraw, rq, patch):
            out.add(mfma_instance(fam, cfg, niw, kkt, ns, split, wraw, rq, patch))
    return frozenset(out | set(PRE_INSTANCES) | set(FLATD_INSTANCES))


def launched(info):
    """The instances of this table one call with plan `info` runs: its conv kernel (MFMA family or flatd; none for the
    resident-tile and generic routes) and its pre-passes."""
    out = set()
    route = capi.CONV_ROUTES[info.route]
    if route == "generic":
        return out
    if route == "mfma":
        out.add(mfma_instance(info.family, info.cfg, info.niw, info.kkt, info.ns, info.split, info.wraw, info.rq, info.patch))
    elif route == "flatd":
        out.add(("flatd", bool(info.fd_w8), bool(info.fused)))
    if info.pre:
        out.add(("pre", PRE[info.pre], info.sub2_log_up if PRE[info.pre] == "sub2" else 0))
    if info.expand and not info.sub_x4:
        out.add(("pre", "expand", 0))
    return out


# ---- operands of a host-only query ------------------------------------------------------------------------------------
def qparam(bits):
    return capi.QeQParam(ALIGNED, bits, 1, ALIGNED, ALIGNED, 1)


def requant8():
    """The consumer's quantiser the fused epilogues take: 8-bit codes, one scale."""
    return capi.QeRequant(ALIGNED, ALIGNED, 1, -128.0, 127.0, 8, 1)


def plan(shape, x_bits=8, w_bits=8, rq=False, codes=ALIGNED, out=ALIGNED):
    N, IC, H, W, OC, K, stride, pad = shape
    return capi.conv_plan_info(capi.conv_shape(N, IC, H, W, OC, K, K, stride, pad), qparam(x_bits), qparam(w_bits),
                               requant8() if rq else None, out, codes)


# ---- the sweep grid ----------------------------------------------------------------------------------------------------
def _named_shapes():
    """The shapes the suite already runs: both networks' layers at N = 1, 5, 256 and the hand-picked lists."""
    from test_conv_gpu import RESNET18_CIFAR, SWEEP_SHAPES, VARIANT_SHAPES
    from test_requant_gpu import SHAPES as REQUANT_SHAPES
    out = []
    nets = [(l.IC, l.OC, l.K, l.stride, l.pad, l.H) for l in resnet50.conv_layers()] + list(RESNET18_CIFAR)
    for IC, OC, K, s, p, H in nets:
        for N in (1, 5, 256):
            out.append((N, IC, H, H, OC, K, s, p))
    return list(dict.fromkeys(out + list(SWEEP_SHAPES) + list(VARIANT_SHAPES) + list(REQUANT_SHAPES)))


ICS = (1, 3, 4, 8, 16, 24, 33, 64, 96, 160, 256, 512, 2048)
OCS = (8, 32, 33, 64, 65, 128, 130, 256, 1024)
# square and a few non-square planes; the last four are there for subsample2_kernel<4 | 6 | 8> and the widest one-row tile
PLANES = ((1, 1), (4, 4), (7, 7), (7, 8), (8, 8), (14, 14), (15, 13), (16, 16), (28, 28), (12, 40), (30, 26), (56, 56),
          (112, 112), (32, 16), (80, 12), (112, 56), (1, 190))
BITS = tuple((xb, wb) for xb in (8, 4, 3) for wb in (8, 4))


def _product_shapes(ics=ICS, ocs=OCS, n=2):
    out = []
    for K in (1, 3, 5, 7):
        for stride in (1, 2, 3):
            for pad in sorted({0, 1, K // 2}):
                for H, W in PLANES:
                    if H + 2 * pad < K or W + 2 * pad < K:
                        continue
                    for IC in ics:
                        for OC in ocs:
                            out.append((n, IC, H, W, OC, K, stride, pad))
    return out


from test_conv_gpu import VARIANT_ENVS  # noqa: E402

# the knob sets of test_kernel_variants_forced_by_env, then one set per knob the planner reads on these routes
KNOB_SETS = [{}] + [dict(e) for e in VARIANT_ENVS] + [
    {"QE_RQ_PATCH": "0"}, {"QE_X4": "0"}, {"QE_SUB_X4": "0"}, {"QE_SUB2": "0"}, {"QE_FLAT_NS": "1"}, {"QE_FLAT_NS": "2"},
    {"QE_FLATD8": "0"}, {"QE_FLATD8": "1"}, {"QE_PWR": "0"}, {"QE_FLATD": "0"}]
# the calls of one problem: plain fp32; re-quantising with aligned codes; with codes one byte past a 16-byte boundary
F32, RQ, RQ_OFF1 = (False, ALIGNED), (True, ALIGNED), (True, ALIGNED + 1)
W8A8, W8A4 = (8, 8), (4, 8)      # (x_bits, w_bits)


def grid():
    """(env, shapes, bit pairs, requests) blocks of the sweep, about 1.3 million plans.  Under every knob set: the named
    shapes and the table's own rows, every bit pair, all three requests.  Default knobs: the whole product in every bit
    pair for the fp32 call, and for the re-quantising calls at W8A8 and W8A4.  Every other knob set: a thinned product."""
    named = _named_shapes() + [r[0] for r in ROWS]
    thin = _product_shapes((3, 16, 33, 64, 160, 512), (32, 65, 130, 1024))
    envs = KNOB_SETS + [r[3] for r in ROWS if r[3] and r[3] not in KNOB_SETS]
    for env in [e for k, e in enumerate(envs) if e not in envs[:k]]:
        yield env, named, BITS, (F32, RQ, RQ_OFF1)
        if not env:
            yield env, _product_shapes(), BITS, (F32,)
            yield env, _product_shapes(), (W8A8, W8A4), (RQ, RQ_OFF1)
        else:
            four_bit = any(k in env for k in ("QE_X4", "QE_SUB_X4", "QE_SUBSAMPLE", "QE_SUB2"))
            yield env, thin, (W8A8, W8A4) if four_bit else (W8A8,), (F32, RQ)


def plan_problems(shape, codes, info):
    """What must hold of every plan: an MFMA-route plan names a compiled instance (launch_conv_mfma never answers
    QE_ERR_UNSUPPORTED), its dynamic LDS fits the launch's limit, its grid is not empty, and a PATCH plan has one image per
    tile, dword-aligned planes, row tiles and codes (plan_rq_patch)."""
    out = []
    if capi.CONV_ROUTES[info.route] == "generic":
        return out
    if info.blocks <= 0:
        out.append("blocks = %d" % info.blocks)
    if capi.CONV_ROUTES[info.route] != "mfma":
        return out
    if not info.has_instance:
        out.append("no compiled instance")
    if info.lds > (80 if FAMILY[info.family] == "sm2" else 64) * 1024:
        out.append("lds = %d" % info.lds)
    if info.patch and not (info.rq and info.gi == 1 and (info.oh * info.ow) % 4 == 0 and (info.th * info.ow) % 4 == 0
                           and codes % 4 == 0):
        out.append("PATCH without its conditions")
    return out


@functools.lru_cache(maxsize=None)
def scan():
    """One pass over the grid: (instances some request launches, number of plans, [(request, problem)] of plan_problems)."""
    L = capi.lib()
    info = capi.QeConvPlanInfo()
    rq = requant8()
    q = {b: qparam(b) for b in (8, 4, 3)}
    pinfo, prq = ctypes.byref(info), ctypes.byref(rq)
    reached, n, problems = set(), 0, []
    for env, shapes, bits, requests in grid():
        with capi.knobs(**env):
            for shape in shapes:
                N, IC, H, W, OC, K, stride, pad = shape
                sh = ctypes.byref(capi.QeConvShape(N, IC, H, W, OC, K, K, stride, pad))
                for xb, wb in bits:
                    x, w = ctypes.byref(q[xb]), ctypes.byref(q[wb])
                    for want_rq, codes in requests:
                        rc = L.qe_quantconv2d_plan_info(sh, x, w, prq if want_rq else None, ALIGNED, codes, pinfo)
                        assert rc == 0, (shape, rc)
                        n += 1
                        reached |= launched(info)
                        for what in plan_problems(shape, codes, info):
                            problems.append(((env, shape, xb, wb, want_rq, codes), what))
    return frozenset(reached), n, problems


def reachable():
    """The instances some request of the grid launches."""
    return scan()[0]


# ---- the table ---------------------------------------------------------------------------------------------------------
ROWS = [
    # ---- halo ----
    ((3, 33, 2, 94, 130, 5, 3, 2), 8, 8, None,
     ('halo', 0, 2, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, no class table: bands overlap, partial image group, ragged OC tile, several OC tiles, several image groups, several images per tile, several stages, stride 3"),
    ((1, 8, 4, 4, 130, 1, 2, 0), 8, 8, None,
     ('halo', 0, 2, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, ROWMUL / COLMUL, class table, ragged OC tile, several OC tiles, stride 2"),
    ((1, 70, 5, 5, 130, 1, 3, 1), 8, 8, None,
     ('halo', 0, 2, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several OC tiles, several stages, stride 3"),
    ((1, 160, 4, 4, 130, 1, 2, 0), 8, 8, None,
     ('halo', 0, 2, 1, 4, False, False), "NCH padded to NS, ROWMUL / COLMUL, class table, ragged OC tile, several OC tiles, several stages, stride 2"),
    ((1, 33, 4, 4, 130, 3, 2, 0), 8, 8, {'QE_SM2': '0', 'QE_WS': '0'},
     ('halo', 0, 2, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several stages, stride 2"),
    ((1, 33, 14, 30, 130, 5, 2, 0), 8, 8, None,
     ('halo', 0, 4, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several stages, stride 2"),
    ((1, 8, 14, 30, 130, 1, 3, 1), 8, 8, None,
     ('halo', 0, 4, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several OC tiles, stride 3"),
    ((1, 70, 14, 30, 130, 1, 3, 1), 8, 8, None,
     ('halo', 0, 4, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several OC tiles, several stages, stride 3"),
    ((1, 160, 14, 30, 130, 1, 3, 1), 8, 8, None,
     ('halo', 0, 4, 1, 4, False, False), "NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several OC tiles, several stages, stride 3"),
    ((1, 33, 32, 16, 130, 3, 3, 1), 8, 8, None,
     ('halo', 0, 4, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several stages, stride 3"),
    ((2, 33, 14, 30, 130, 5, 2, 0), 8, 8, None,
     ('halo', 0, 7, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several images per tile, several stages, stride 2"),
    ((2, 70, 9, 9, 136, 5, 1, 2), 8, 8, None,
     ('halo', 0, 7, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several images per tile, several stages"),
    ((3, 33, 1, 190, 130, 1, 3, 1), 8, 8, None,
     ('halo', 0, 7, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, ROWMUL / COLMUL, no class table: bands overlap, ragged OC tile, several OC tiles, several images per tile, several stages, stride 3"),
    ((2, 70, 14, 30, 130, 1, 3, 1), 8, 8, None,
     ('halo', 0, 7, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several OC tiles, several images per tile, several stages, stride 3"),
    ((1, 160, 9, 11, 130, 1, 1, 1), 8, 8, None,
     ('halo', 0, 7, 1, 4, False, False), "NCH padded to NS, no class table: too many classes, ragged OC tile, several OC tiles, several stages"),
    ((2, 33, 32, 32, 130, 3, 2, 1), 8, 4, None,
     ('halo', 0, 7, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, partial row tile, ragged OC tile, several OC tiles, several image groups, several row tiles, several stages, stride 2, sub-8-bit weights"),
    ((1, 33, 5, 5, 33, 5, 1, 0), 8, 8, None,
     ('halo', 1, 1, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages"),
    ((1, 8, 4, 4, 33, 1, 2, 0), 8, 8, None,
     ('halo', 1, 1, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, ROWMUL / COLMUL, class table, ragged OC tile, stride 2"),
    ((1, 70, 4, 4, 33, 1, 2, 0), 8, 8, None,
     ('halo', 1, 1, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ROWMUL / COLMUL, class table, ragged OC tile, several stages, stride 2"),
    ((1, 160, 4, 4, 33, 1, 2, 0), 8, 8, None,
     ('halo', 1, 1, 1, 4, False, False), "NCH padded to NS, ROWMUL / COLMUL, class table, ragged OC tile, several stages, stride 2"),
    ((1, 33, 4, 4, 33, 3, 2, 0), 8, 8, None,
     ('halo', 1, 1, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages, stride 2"),
    ((1, 33, 14, 30, 33, 5, 2, 0), 8, 8, None,
     ('halo', 1, 2, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages, stride 2"),
    ((1, 8, 14, 30, 33, 1, 3, 1), 8, 8, None,
     ('halo', 1, 2, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, stride 3"),
    ((1, 70, 14, 30, 33, 1, 3, 1), 8, 8, None,
     ('halo', 1, 2, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several stages, stride 3"),
    ((1, 160, 14, 30, 33, 1, 3, 1), 8, 8, None,
     ('halo', 1, 2, 1, 4, False, False), "NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several stages, stride 3"),
    ((1, 33, 32, 16, 33, 3, 3, 1), 8, 8, None,
     ('halo', 1, 2, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages, stride 3"),
    ((2, 33, 14, 30, 33, 5, 2, 0), 8, 8, None,
     ('halo', 1, 4, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several images per tile, several stages, stride 2"),
    ((1, 40, 12, 12, 40, 7, 1, 3), 8, 8, None,
     ('halo', 1, 4, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages"),
    ((3, 33, 1, 190, 33, 1, 3, 1), 8, 8, None,
     ('halo', 1, 4, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, ROWMUL / COLMUL, no class table: bands overlap, ragged OC tile, several images per tile, several stages, stride 3"),
    ((2, 70, 14, 30, 33, 1, 3, 1), 8, 8, None,
     ('halo', 1, 4, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several images per tile, several stages, stride 3"),
    ((1, 160, 9, 11, 33, 1, 1, 1), 8, 8, None,
     ('halo', 1, 4, 1, 4, False, False), "NCH padded to NS, no class table: too many classes, ragged OC tile, several stages"),
    ((3, 33, 10, 18, 33, 3, 2, 1), 8, 8, None,
     ('halo', 1, 4, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several images per tile, several stages, stride 2"),
    ((1, 33, 5, 5, 8, 5, 1, 0), 8, 8, None,
     ('halo', 2, 1, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, class table, ragged OC tile, several stages"),
    ((1, 8, 4, 4, 8, 1, 2, 0), 8, 8, None,
     ('halo', 2, 1, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, ROWMUL / COLMUL, class table, ragged OC tile, stride 2"),
    ((1, 70, 4, 4, 8, 1, 2, 0), 8, 8, None,
     ('halo', 2, 1, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, OC below one strip, ROWMUL / COLMUL, class table, ragged OC tile, several stages, stride 2"),
    ((1, 160, 4, 4, 8, 1, 2, 0), 8, 8, None,
     ('halo', 2, 1, 1, 4, False, False), "NCH padded to NS, OC below one strip, ROWMUL / COLMUL, class table, ragged OC tile, several stages, stride 2"),
    ((1, 33, 4, 4, 8, 3, 2, 0), 8, 8, None,
     ('halo', 2, 1, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, class table, ragged OC tile, several stages, stride 2"),
    ((2, 33, 14, 30, 8, 5, 2, 0), 8, 8, None,
     ('halo', 2, 2, 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, class table, ragged OC tile, several images per tile, several stages, stride 2"),
    ((3, 33, 1, 190, 8, 1, 3, 1), 8, 8, None,
     ('halo', 2, 2, 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, ROWMUL / COLMUL, no class table: bands overlap, ragged OC tile, several images per tile, several stages, stride 3"),
    ((2, 70, 14, 30, 8, 1, 3, 1), 8, 8, None,
     ('halo', 2, 2, 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, OC below one strip, ROWMUL / COLMUL, no class table: too many classes, ragged OC tile, several images per tile, several stages, stride 3"),
    ((1, 160, 9, 11, 8, 1, 1, 1), 8, 8, None,
     ('halo', 2, 2, 1, 4, False, False), "NCH padded to NS, OC below one strip, no class table: too many classes, ragged OC tile, several stages"),
    ((3, 33, 10, 18, 8, 3, 2, 1), 8, 8, None,
     ('halo', 2, 2, 9, 1, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, class table, ragged OC tile, several images per tile, several stages, stride 2"),
    # ---- ws ----
    ((1, 33, 1, 190, 130, 3, 3, 1), 8, 8, None,
     ('ws', 2, 1, False), "IC % 16 != 0, IC % 32 != 0, no class table: bands overlap, ragged OC tile, several OC tiles, several stages, stride 3"),
    ((1, 33, 2, 94, 130, 3, 2, 1), 8, 8, None,
     ('ws', 2, 2, False), "IC % 16 != 0, IC % 32 != 0, no class table: bands overlap, ragged OC tile, several OC tiles, several stages, stride 2"),
    ((1, 33, 4, 4, 130, 3, 2, 0), 8, 8, None,
     ('ws', 2, 4, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several stages, stride 2"),
    ((2, 33, 37, 41, 130, 3, 3, 0), 8, 4, {'QE_SM2': '0', 'QE_WS': '1'},
     ('ws', 4, 1, False), "IC % 16 != 0, IC % 32 != 0, class table, partial row tile, ragged OC tile, several OC tiles, several image groups, several row tiles, several stages, stride 3, sub-8-bit weights"),
    ((5, 33, 15, 13, 130, 3, 3, 0), 8, 8, None,
     ('ws', 4, 1, False), "IC % 16 != 0, IC % 32 != 0, class table, partial image group, ragged OC tile, several OC tiles, several image groups, several images per tile, several stages, stride 3"),
    ((2, 33, 14, 14, 130, 3, 2, 0), 8, 8, None,
     ('ws', 4, 2, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several images per tile, several stages, stride 2"),
    ((2, 33, 8, 8, 130, 3, 1, 0), 8, 8, None,
     ('ws', 4, 4, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several images per tile, several stages"),
    ((3, 33, 10, 18, 130, 3, 2, 1), 8, 8, None,
     ('ws', 7, 1, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several images per tile, several stages, stride 2"),
    ((1, 33, 2, 94, 130, 3, 1, 1), 8, 8, {'QE_SM2': '0', 'QE_WS': '1'},
     ('ws', 7, 2, False), "IC % 16 != 0, IC % 32 != 0, no class table: bands overlap, ragged OC tile, several OC tiles, several stages"),
    ((2, 33, 12, 6, 130, 3, 1, 1), 8, 8, None,
     ('ws', 7, 4, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several images per tile, several stages"),
    # ---- sm2 ----
    ((2, 33, 32, 32, 130, 3, 2, 1), 8, 4, {'QE_SM2': '1'},
     ('sm2', 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, partial row tile, ragged OC tile, several OC tiles, several image groups, several row tiles, several stages, stride 2, sub-8-bit weights"),
    ((3, 33, 12, 40, 130, 3, 3, 1), 8, 8, {'QE_SM2': '1'},
     ('sm2', 0, 1, False, False), "IC % 16 != 0, IC % 32 != 0, partial image group, ragged OC tile, several OC tiles, several image groups, several images per tile, several stages, stride 3"),
    ((1, 33, 2, 94, 130, 3, 1, 1), 8, 8, None,
     ('sm2', 0, 2, False, False), "IC % 16 != 0, IC % 32 != 0, no class table: bands overlap, ragged OC tile, several OC tiles, several stages"),
    ((1, 33, 6, 6, 130, 3, 3, 0), 8, 8, {'QE_SM2': '1'},
     ('sm2', 0, 4, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, several stages, stride 3"),
    ((1, 33, 12, 40, 33, 3, 1, 1), 8, 8, None,
     ('sm2', 1, 1, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages"),
    ((1, 33, 2, 94, 33, 3, 1, 1), 8, 8, None,
     ('sm2', 1, 2, False, False), "IC % 16 != 0, IC % 32 != 0, no class table: bands overlap, ragged OC tile, several stages"),
    ((1, 33, 4, 4, 33, 3, 1, 0), 8, 8, None,
     ('sm2', 1, 4, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several stages"),
    # ---- stem ----
    ((2, 1, 32, 32, 130, 1, 2, 0), 8, 4, {'QE_SUBSAMPLE': '0'},
     ('stem', 0, 7, False, False), "IC % 16 != 0, IC % 32 != 0, class table, partial row tile, ragged OC tile, several OC tiles, several image groups, several row tiles, stride 2, sub-8-bit weights"),
    ((1, 3, 20, 20, 130, 7, 2, 3), 8, 4, None,
     ('stem', 0, 7, False, False), "IC % 16 != 0, IC % 32 != 0, class table, ragged OC tile, several OC tiles, stride 2, sub-8-bit weights"),
    ((1, 1, 8, 8, 33, 1, 3, 1), 8, 8, None,
     ('stem', 1, 7, False, False), "IC % 16 != 0, IC % 32 != 0, no class table: too many classes, ragged OC tile, stride 3"),
    ((2, 3, 40, 40, 64, 7, 2, 3), 8, 8, None,
     ('stem', 1, 7, False, False), "IC % 16 != 0, IC % 32 != 0, class table, several image groups, stride 2"),
    ((1, 4, 20, 24, 48, 5, 1, 2), 8, 8, None,
     ('stem', 1, 7, False, False), "IC % 16 != 0, IC % 32 != 0, class table, partial row tile, ragged OC tile, several row tiles"),
    ((1, 1, 1, 190, 8, 1, 3, 1), 8, 8, None,
     ('stem', 2, 2, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, no class table: bands overlap, ragged OC tile, stride 3"),
    ((2, 4, 12, 12, 8, 3, 1, 1), 8, 8, None,
     ('stem', 2, 2, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, class table, ragged OC tile, several image groups"),
    ((1, 3, 37, 41, 24, 7, 2, 3), 8, 8, None,
     ('stem', 2, 2, False, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, class table, partial row tile, ragged OC tile, several row tiles, stride 2"),
    # ---- flat ----
    ((1, 33, 56, 56, 136, 1, 1, 0), 8, 8, None,
     ('flat', 0, 4, 1, False), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles, several pixel tiles, several stages"),
    ((1, 48, 56, 56, 200, 1, 1, 0), 8, 8, None,
     ('flat', 0, 4, 1, True), "IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles, several pixel tiles, several stages"),
    ((1, 70, 8, 8, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 4, 2, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 96, 8, 8, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 4, 2, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 160, 8, 8, 130, 1, 1, 0), 8, 4, None,
     ('flat', 0, 4, 4, False), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit weights"),
    ((1, 160, 8, 8, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 4, 4, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 24, 12, 12, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 5, 1, False), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles"),
    ((1, 16, 12, 12, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 5, 1, True), "IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles"),
    ((1, 70, 12, 12, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 5, 2, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 96, 12, 12, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 5, 2, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 160, 12, 12, 130, 1, 1, 0), 8, 4, None,
     ('flat', 0, 5, 4, False), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit weights"),
    ((1, 160, 12, 12, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 5, 4, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 24, 10, 18, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 7, 1, False), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles"),
    ((1, 16, 10, 18, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 7, 1, True), "IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles"),
    ((2, 70, 20, 20, 130, 1, 1, 0), 8, 4, None,
     ('flat', 0, 7, 2, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several image groups, several pixel tiles, several stages, sub-8-bit weights"),
    ((1, 96, 10, 18, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 7, 2, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 160, 10, 18, 130, 1, 1, 0), 8, 4, None,
     ('flat', 0, 7, 4, False), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit weights"),
    ((1, 160, 10, 18, 130, 1, 1, 0), 8, 8, None,
     ('flat', 0, 7, 4, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    ((1, 24, 8, 8, 33, 1, 1, 0), 8, 8, None,
     ('flat', 1, 4, 1, False), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile"),
    ((1, 16, 8, 8, 33, 1, 1, 0), 8, 8, None,
     ('flat', 1, 4, 1, True), "IC % 32 != 0, partial pixel tile, ragged OC tile"),
    ((1, 70, 8, 8, 33, 1, 1, 0), 8, 8, None,
     ('flat', 1, 4, 2, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several stages"),
    ((1, 96, 8, 8, 33, 1, 1, 0), 8, 8, None,
     ('flat', 1, 4, 2, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several stages"),
    ((1, 160, 8, 8, 33, 1, 1, 0), 8, 4, None,
     ('flat', 1, 4, 4, False), "NCH padded to NS, partial pixel tile, ragged OC tile, several stages, sub-8-bit weights"),
    ((1, 160, 8, 8, 33, 1, 1, 0), 8, 8, None,
     ('flat', 1, 4, 4, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several stages"),
    ((1, 24, 8, 8, 8, 1, 1, 0), 8, 8, None,
     ('flat', 2, 2, 1, False), "IC % 16 != 0, IC % 32 != 0, OC below one strip, partial pixel tile, ragged OC tile"),
    ((1, 16, 8, 8, 8, 1, 1, 0), 8, 8, None,
     ('flat', 2, 2, 1, True), "IC % 32 != 0, OC below one strip, partial pixel tile, ragged OC tile"),
    ((1, 70, 8, 8, 8, 1, 1, 0), 8, 8, None,
     ('flat', 2, 2, 2, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, OC below one strip, partial pixel tile, ragged OC tile, several stages"),
    ((1, 96, 8, 8, 8, 1, 1, 0), 8, 8, None,
     ('flat', 2, 2, 2, True), "NCH padded to NS, OC below one strip, partial pixel tile, ragged OC tile, several stages"),
    ((1, 160, 8, 8, 8, 1, 1, 0), 8, 4, None,
     ('flat', 2, 2, 4, False), "NCH padded to NS, OC below one strip, partial pixel tile, ragged OC tile, several stages, sub-8-bit weights"),
    ((1, 160, 8, 8, 8, 1, 1, 0), 8, 8, None,
     ('flat', 2, 2, 4, True), "NCH padded to NS, OC below one strip, partial pixel tile, ragged OC tile, several stages"),
    # ---- flat_s2 ----
    ((2, 70, 32, 32, 130, 1, 2, 0), 8, 4, {'QE_SUBSAMPLE': '0'},
     ('flat_s2', 0, 7, 2, False), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several image groups, several pixel tiles, several stages, sub-8-bit weights"),
    ((1, 96, 16, 16, 130, 1, 2, 0), 8, 8, {'QE_SUBSAMPLE': '0'},
     ('flat_s2', 0, 7, 2, True), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages"),
    # ---- flat_x4 ----
    ((1, 33, 56, 56, 136, 1, 1, 0), 4, 8, None,
     ('flat_x4', 4, 1), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles, several pixel tiles, several stages, sub-8-bit activations"),
    ((1, 70, 8, 8, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 4, 2), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit activations"),
    ((1, 160, 8, 8, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 4, 4), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit activations"),
    ((1, 24, 12, 12, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 5, 1), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles, sub-8-bit activations"),
    ((1, 70, 12, 12, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 5, 2), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit activations"),
    ((1, 160, 12, 12, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 5, 4), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit activations"),
    ((1, 24, 10, 18, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 7, 1), "IC % 16 != 0, IC % 32 != 0, partial pixel tile, ragged OC tile, several OC tiles, sub-8-bit activations"),
    ((2, 70, 20, 20, 130, 1, 1, 0), 4, 4, None,
     ('flat_x4', 7, 2), "IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several image groups, several pixel tiles, several stages, sub-8-bit activations, sub-8-bit weights"),
    ((1, 160, 10, 18, 130, 1, 1, 0), 4, 8, None,
     ('flat_x4', 7, 4), "NCH padded to NS, partial pixel tile, ragged OC tile, several OC tiles, several stages, sub-8-bit activations"),
    # ---- flatg ----
    ((1, 70, 7, 7, 130, 1, 1, 0), 8, 4, None,
     ('flatg', 7, 2, False), "49-pixel planes, IC % 16 != 0, IC % 32 != 0, NCH padded to NS, ragged OC tile, several OC tiles, several stages, sub-8-bit weights"),
    ((5, 70, 7, 7, 130, 1, 1, 0), 8, 8, None,
     ('flatg', 7, 2, False), "49-pixel planes, IC % 16 != 0, IC % 32 != 0, NCH padded to NS, partial image group, ragged OC tile, several OC tiles, several image groups, several images per tile, several stages"),
    ((1, 96, 7, 8, 130, 1, 1, 0), 8, 8, None,
     ('flatg', 7, 2, True), "56-pixel planes, NCH padded to NS, ragged OC tile, several OC tiles, several stages"),
    ((1, 160, 7, 7, 130, 1, 1, 0), 8, 4, None,
     ('flatg', 7, 4, False), "49-pixel planes, NCH padded to NS, ragged OC tile, several OC tiles, several stages, sub-8-bit weights"),
    # ---- flatd ----
    ((1, 128, 7, 7, 64, 1, 1, 0), 8, 8, None,
     ('flatd', False, False), "whole tiles"),
    ((3, 192, 7, 7, 96, 1, 1, 0), 8, 8, None,
     ('flatd', False, False), "whole tiles"),
    ((1, 128, 7, 7, 136, 1, 1, 0), 8, 8, {'QE_FLATD8': '1'},
     ('flatd', True, False), "whole tiles"),
    ((1, 128, 7, 7, 256, 1, 1, 0), 8, 8, {'QE_FLATD8': '1'},
     ('flatd', True, False), "whole tiles"),
    ((5, 192, 7, 7, 1024, 1, 1, 0), 8, 8, None,
     ('flatd', True, False), "whole tiles"),
    # ---- pre ----
    ((2, 40, 9, 11, 40, 3, 1, 1), 3, 8, None,
     ('pre', 'expand', 0), "OW = 11, then halo"),
    ((1, 70, 12, 12, 130, 3, 2, 1), 4, 4, None,
     ('pre', 'expand', 0), "OW = 6, then ws"),
    ((2, 3, 20, 20, 24, 5, 2, 2), 4, 8, None,
     ('pre', 'expand', 0), "OW = 10, then stem"),
    ((1, 70, 14, 14, 130, 1, 2, 0), 8, 8, None,
     ('pre', 'sub2', 3), "OW = 7, then flatg"),
    ((1, 70, 32, 16, 130, 1, 2, 0), 8, 8, None,
     ('pre', 'sub2', 4), "OW = 8, then flat"),
    ((1, 70, 20, 20, 130, 1, 2, 0), 8, 8, None,
     ('pre', 'sub2', 5), "OW = 10, then flat"),
    ((2, 64, 80, 12, 40, 1, 2, 0), 8, 8, None,
     ('pre', 'sub2', 6), "OW = 6, then flat"),
    ((1, 70, 56, 56, 130, 1, 2, 0), 8, 8, {'QE_SUBSAMPLE': '1'},
     ('pre', 'sub2', 7), "OW = 28, then flat"),
    ((1, 70, 112, 56, 130, 1, 2, 0), 8, 8, {'QE_SUBSAMPLE': '1'},
     ('pre', 'sub2', 8), "OW = 28, then flat"),
    ((1, 70, 9, 11, 130, 1, 3, 0), 4, 8, None,
     ('pre', 'sub_narrow', 0), "OW = 4, then halo"),
    ((1, 70, 10, 18, 130, 1, 3, 0), 8, 8, None,
     ('pre', 'sub_narrow', 0), "OW = 6, then halo"),
    ((1, 70, 14, 14, 130, 1, 3, 0), 8, 8, None,
     ('pre', 'sub_narrow', 0), "OW = 5, then halo"),
    ((1, 70, 2, 94, 130, 1, 2, 0), 8, 8, None,
     ('pre', 'sub_narrow', 0), "OW = 47, then halo"),
    ((1, 70, 12, 40, 130, 1, 2, 0), 8, 8, None,
     ('pre', 'sub_wide', 0), "OW = 20, then flat"),
    ((1, 70, 2, 94, 130, 1, 2, 0), 4, 8, None,
     ('pre', 'sub_x4', 0), "OW = 47, then halo"),
    ((1, 70, 16, 16, 130, 1, 2, 0), 4, 8, None,
     ('pre', 'sub_x4', 0), "OW = 8, then flat"),
    ((2, 64, 30, 22, 40, 1, 2, 0), 4, 8, None,
     ('pre', 'sub_x4', 0), "OW = 11, then halo"),
]

# compiled instances that no request selects: {instance: the planner condition that excludes it}.  Empty today: the two
# that look unreachable from the networks' shapes are not -- conv_mfma_ws_kernel<2, 1> takes a one-row, 64-pixel-wide tile
# of a stride-3 3x3 layer (more than 128 staging units for two column tiles), subsample2_kernel<6> 33 to 64 output rows of
# at most 8 pixels -- and both have a row.
UNREACHABLE = {}


def modes(row):
    """The calls the GPU tests make of a row, as (env, rq, codes offset): fp32, re-quantising, and -- where that took the
    PATCH form -- re-quantising with QE_RQ_PATCH=0."""
    shape, xb, wb, env, expected, note = row
    env = dict(env or {})
    out = [(env, False, 0), (env, True, 0)]
    with capi.knobs(**env):
        if plan(shape, xb, wb, rq=True).patch:
            out.append((dict(env, QE_RQ_PATCH="0"), True, 0))
    return out


def row_instances(row, rq=None):
    """The instances the GPU tests run through a row (rq None: every call; False / True: its fp32 / re-quantising calls)."""
    out = set()
    for env, want_rq, off in modes(row):
        if rq is None or rq == want_rq:
            with capi.knobs(**env):
                out |= launched(plan(row[0], row[1], row[2], rq=want_rq, codes=ALIGNED + off))
    return out


@functools.lru_cache(maxsize=None)
def covered():
    """The instances the GPU tests reach through ROWS."""
    out = set()
    for row in ROWS:
        out |= row_instances(row)
    return frozenset(out)


def _clipped(I, K, stride, pad, O):
    """Output rows (columns) whose first / last taps fall outside the image: plan_mfma_launch's border bands."""
    lo = min(O, (pad + stride - 1) // stride)
    full_last = (I + pad - K) // stride if I + pad - K >= 0 else -1
    return lo, max(0, min(O, O - 1 - full_last))


def edges(shape, x_bits, w_bits, info):
    """What a problem exercises of the kernel its plan names: the branches listed in the note of its row."""
    N, IC, H, W, OC, K, stride, pad = shape
    fam = FAMILY[info.family]
    out = set()
    if capi.CONV_ROUTES[info.route] != "mfma":
        return out
    if OC % info.mt:
        out.add("ragged OC tile")
    if OC > info.mt:
        out.add("several OC tiles")
    if fam != "stem" and (IC + 31) // 32 > info.ns:
        out.add("several stages")
    if -(-N // info.gi) > 1:
        out.add("several image groups")
    if OC < 32:
        out.add("OC below one strip")
    if IC % 32:
        out.add("IC % 32 != 0")
    if IC % 16:
        out.add("IC % 16 != 0")
    if w_bits < 8:
        out.add("sub-8-bit weights")
    if x_bits < 8:
        out.add("sub-8-bit activations")
    if info.gi > 1:
        out.add("several images per tile")
        if N % info.gi:
            out.add("partial image group")
    P = info.oh * info.ow
    if fam in LANE_PIXEL:
        if info.oh % info.th:
            out.add("partial row tile")
        if info.oh > info.th:
            out.add("several row tiles")
        if stride > 1:
            out.add("stride %d" % stride)
        if info.rowmul > 1 or info.colmul > 1:
            out.add("ROWMUL / COLMUL")
        if fam == "halo" and info.nch > (IC + 31) // 32:
            out.add("NCH padded to NS")
        top, bot = _clipped(H, K, stride, pad, info.oh)
        lft, rgt = _clipped(W, K, stride, pad, info.ow)
        if info.ctab:
            out.add("class table")
        elif top + bot >= info.oh or lft + rgt >= info.ow:
            out.add("no class table: bands overlap")
        elif (1 + top + bot) * (1 + lft + rgt) > (K + 1) * (K + 1):
            out.add("no class table: too many classes")
    else:
        if ((IC + 31) // 32) % info.ns:
            out.add("NCH padded to NS")
        if fam == "flatg":
            out.add("%d-pixel planes" % P)
        elif P % (32 * info.ni):
            out.add("partial pixel tile")
        if fam != "flatg" and P > 32 * info.ni:
            out.add("several pixel tiles")
    return out


def rows_of(*families):
    return [r for r in ROWS if family_of(r[4]) in families]
