"""Operand types, per decode site: one table of (bit width, sign) settings for every place where packed codes become numbers,
shared by tests/test_quant_instances_cpu.py and the GPU tests (tests/test_quant_instances_gpu.py).

A packed operand has 1 to 8 bits, signed or unsigned: 16 settings (SETTINGS, "s1" .. "u8").  A decode site is one piece of
device code that turns a stream into numbers (SITES below, each confirmed from the launch code: launch_conv_mfma /
plan_conv, launch_conv_f32, launch_conv_generic, plan_linear).  Sites the list in the issue did not have: none; two of its
entries are one site here -- the QE_X4=0 rows are 4-bit rows of "expand_1x1" and the QE_SUB_X4=0 rows 4-bit rows of
"expand_gather", since with the knob off those streams go through expand_codes_s8 like every other width.

ROWS: (site, entry, shape, (x_bits, x_sign), (w_bits, w_sign), env, note).
  site    key of SITES.  A run passes an activation site and a weight site; the row names the one it is there for and
          planned_sites(row) derives both from the host-side plan queries.
  entry   "capi" (the C ABI's plain fp32 call) | "torch" (the torch operator of the same call) | "requant" | "residual" |
          "bf16" (the fused entries: qe_quantconv2d_requant_prepared, qe_quantconv2d_residual_prepared,
          qe_quantlinear_requant / _residual / _bf16).  Rows with knobs stay on the C ABI.
  shape   conv: (N, IC, H, W, OC, K, stride, pad); linear: (B, K, O).  The smallest that lands on the site, with odd element
          counts so the last code of a stream ends inside a byte and the straddling widths 3, 5, 6, 7 end on a straddle.
          EVEN_X lists the shapes whose planner conditions rule that out for the activations (tests check the rest).
  x       (0, 0): fp32 activations, (16, 0): bf16 activations.

Where a site decodes both operands (the two order-preserving kernels) the 16 settings of one operand are walked and setting
i paired with setting (5 i + 3) % 16 of the other, then the roles swapped: every setting twice, with different partners.

operands(k, regime) draws the tensors of ROWS[k].  Both regimes: each packed operand's first element is its minimum code and
its last element its maximum code (a strided 1x1 layer never reads the last pixels of its input: the last element it does
read holds the maximum as well, and is the one the sensitivity test perturbs).

"exact": sx = 2^-6, sw a power of two in [2^-7, 2^-3] per channel (per tensor on every third row), non-zero integer zero
points with |z| <= min(3, 2^bits / 4 + 1), bias an integer multiple of sx sw[oc]; fp32 / bf16 activations integer multiples
of 2^-4 with at most 8 significant bits (they play sx = 2^-4, codes |m| <= 255, z = 0).  Every product and partial sum is
then an integer multiple of lsb[oc] = sx sw[oc] below 2^24 lsb, in the direct form sum (q - z)(q - z) and in the matrix-core
form (codes re-centred, then S_aw - zw' S_x - zx' S_w + K zx' zw'), in any order: fp32 holds them exactly and the kernel must
return the float64 value bit for bit.  bound(k) is the issue's figure K (A_x + Z_x)(A_w + Z_w) + max |bias| / lsb, A = 2^bits,
Z = max |z| (+ 128 for unsigned 8-bit); it stays below 2^24 on every row but the four of TIGHT, where it cannot: pwr7, flatd
and linear forms 3 and 4 take no reduction shorter than K = 128, and 128 x 385 x 385 > 2^24 for a pair of unsigned 8-bit
operands whatever the zero points.  Those four rows are held to tight_bound(k) instead, which is what the arithmetic needs:
a re-centred 8-bit code is at most 128 in magnitude, not 256, and q - z = a - z', so both forms sum at most
K (128 + |z'_x|)(128 + |z'_w|) = 128 x 259 x 259 < 2^23.

"parity": headline scales (sx 2e-3, sw about 5e-4), fractional zero points including unsigned mid-range ones, random bias,
as test_conv_gpu._random_case and test_linear_gpu._random_case draw them -- for the project's own tolerance rule."""
import functools

import numpy as np

import quant_ref as qr
from quantize_amd import capi

ALIGNED = 1 << 20
SETTINGS = tuple((b, s) for b in range(1, 9) for s in (1, 0))        # s1, u1, s2, u2, ..., s8, u8
F32X, BF16X = (0, 0), (16, 0)
S8, U8 = (8, 1), (8, 0)


def tag(q):
    return "f32" if q == F32X else "bf16" if q == BF16X else ("s" if q[1] else "u") + str(q[0])


def partner(i):
    return SETTINGS[(5 * i + 3) % 16]


ALL16 = frozenset(tag(q) for q in SETTINGS)
SUB8 = frozenset(tag(q) for q in SETTINGS if q[0] < 8)
SIGN_PAIRS = frozenset((a, b) for a in ("s8", "u8") for b in ("s8", "u8"))

# site -> (operation, the device code that decodes)
SITES = {
    # packed-input conv, weights
    "prep": ("conv", "conv_mfma_prep_kernel: unpack_code - code_bias into the MFMA fragments of every non-stem family"),
    "prep_smallic": ("conv", "conv_mfma_prep_smallic_kernel: the same for the stem (IC <= 4)"),
    "wraw_flat": ("conv", "conv_mfma_flat_kernel, raw 8-bit weights re-centred in the kernel (w_bits == 8, IC % 16 == 0)"),
    "wraw_flat_s2": ("conv", "conv_mfma_flat_kernel's stride-2 form, raw 8-bit weights"),
    "wraw_flatg": ("conv", "conv_mfma_flatg_kernel, raw 8-bit weights"),
    "pwr": ("conv", "resident-tile kernel (qe_conv_pwr.hip): 8-bit codes of both operands re-centred in the kernel"),
    "pwr7": ("conv", "resident-tile kernel on 7x7 planes"),
    "flatd": ("conv", "LDS-DMA ring kernel (qe_conv_flatd.hip)"),
    "generic": ("conv", "conv_generic_kernel<true>: unpack_elem on x and on w"),
    # packed-input conv, activations
    "expand_3x3": ("conv", "expand_codes_s8 (tunpack_kernel<b>, shifted offset) in front of a 3x3 family"),
    "expand_1x1": ("conv", "expand_codes_s8 in front of a 1x1 family (4-bit streams too where FlatX4 does not apply or is off)"),
    "expand_gather": ("conv", "expand_codes_s8, then the strided-1x1 gather pre-pass (4-bit streams under QE_SUB_X4=0)"),
    "sub_x4": ("conv", "subsample_x4_kernel: nibbles of a stride-2 1x1 layer"),
    "flat_x4": ("conv", "conv_mfma_flat_kernel's 4-bit form: nibbles decoded in its staging"),
    # float-input conv
    "f32_prep": ("conv_f32", "conv_f32_prep_kernel: f32_unpack_code"),
    "f32_prep_stem": ("conv_f32", "conv_f32_prep_stem_kernel: f32_unpack_code"),
    "generic_f32": ("conv_f32", "conv_generic_kernel<false>: unpack_elem on w"),
    # linear
    "lin_generic": ("lin", "linear_generic_kernel<false>: lin_unpack on x and on w"),
    "lin_generic_f32": ("lin_f32", "linear_generic_kernel<true>: lin_unpack on w"),
    "lin_f32_mfma": ("lin_f32", "linear_f32_mfma_kernel: 8-bit weight codes centred in its staging"),
    "lin_bf16in": ("lin_bf16", "linear_bf16in_kernel: 8-bit weight codes centred in its staging"),
    "lin_mfma1": ("lin", "linear_mfma_kernel<2>: u ^ 0x80 on the fragments"),
    "lin_mfma2": ("lin", "linear_mfma_kernel<4>"),
    "lin_mfma3": ("lin", "linear_mfma8_kernel<2>"),
    "lin_mfma4": ("lin", "linear_mfma8_kernel<1>"),
}
# Sites held to |got - exact64| <= lsb / 4 instead of equality, with the operation that rounds: none.  Every site
# reproduces the float64 value bit for bit on an MI355X.
QUARTER_STEP = {}

C3 = (1, 5, 5, 7, 9, 3, 1, 1)          # 3x3, IC % 16 != 0: prepared fragments; x 175, w 405 elements
STEM = (1, 3, 5, 7, 9, 3, 1, 1)        # IC <= 4; x 105, w 243
FLAT = (1, 33, 8, 8, 33, 1, 1, 0)      # 1x1 stride 1, 64-channel workgroups: no FlatX4; w 1089
FLAT128 = (1, 33, 8, 8, 65, 1, 1, 0)   # 128-channel workgroups: FlatX4 for 4-bit x; w 2145
GATHER = (1, 33, 13, 13, 33, 1, 2, 0)  # stride-2 1x1, odd plane: the last pixel is read; x 5577, w 1089
GATHER4 = (1, 33, 6, 8, 33, 1, 2, 0)   # ... W even for subsample_x4_kernel
WIDE3 = (1, 5, 5, 3, 7, 3, 1, 1)       # W < 4: the order-preserving kernel; x 75, w 315
F_MAIN = (1, 9, 5, 5, 9, 3, 1, 1)      # float input, IC >= 8; w 729
F_STEM = (1, 3, 5, 5, 9, 3, 1, 1)      # float input, IC <= 4; w 243
F_GEN = (1, 5, 5, 5, 7, 3, 1, 1)       # float input, 4 < IC < 8: the order-preserving kernel; w 315
LIN0 = (33, 37, 35)                    # K % 64 != 0, K % 32 != 0, two row and two column tiles; x 1221, w 1295
LIN64 = (33, 64, 35)
LIN128 = (33, 128, 256)

PWR, PWR7, FLATD = (1, 64, 14, 14, 256, 1, 1, 0), (4, 128, 7, 7, 512, 1, 1, 0), (1, 128, 7, 7, 64, 1, 1, 0)
W_FLAT, W_FLAT_S2, W_FLATG = (1, 16, 8, 8, 33, 1, 1, 0), (1, 64, 16, 16, 65, 1, 2, 0), (1, 64, 7, 7, 65, 1, 1, 0)
# shapes whose activation count cannot be odd: the planner condition that forces it (the weights' always can be)
EVEN_X = {FLAT: "plan_flat: H W % 4 == 0", FLAT128: "plan_flat: H W % 4 == 0", GATHER4: "make_plan (sub_x4): W % 2 == 0"}

ROWS = []


def _add(site, shape, x, w, env=None, note="", entry=None):
    if entry is None:
        entry = "capi" if env or x == BF16X or len(ROWS) % 2 == 0 else "torch"
    ROWS.append((site, entry, shape, x, w, env, note))


def _build():
    eight = lambda i: (S8, U8)[i % 2]
    # ---- packed-input conv: weights ----
    for i, w in enumerate(SETTINGS):
        _add("prep", C3, eight(i), w, note="ws / sm2 / halo fragments")
    for i, w in enumerate(SETTINGS):
        _add("prep_smallic", STEM, eight(i + 1), w, note="stem fragments")
    for site, shape, env in (("wraw_flat", W_FLAT, None), ("wraw_flat_s2", W_FLAT_S2, {"QE_SUBSAMPLE": "0"}),
                             ("wraw_flatg", W_FLATG, None), ("pwr", PWR, None), ("pwr7", PWR7, None), ("flatd", FLATD, None)):
        for x in (S8, U8):
            for w in (S8, U8):
                _add(site, shape, x, w, env, "sign pair")
    for i, x in enumerate(SETTINGS):
        _add("generic", WIDE3, x, partner(i), note="x walks, w = partner")
    for i, w in enumerate(SETTINGS):
        _add("generic", WIDE3, partner(i), w, note="w walks, x = partner")
    # ---- packed-input conv: activations ----
    sub8 = [q for q in SETTINGS if q[0] < 8]
    for i, x in enumerate(sub8):
        _add("expand_3x3", C3, x, partner(i), note="then a 3x3 family")
    for i, x in enumerate(sub8):
        _add("expand_1x1", FLAT, x, partner(i + 7), note="then flat")
    for x, w in (((3, 1), S8), ((3, 0), (4, 0)), ((5, 1), U8), ((5, 0), (6, 1))):
        _add("expand_gather", GATHER, x, w, note="then the gather")
    for x, w in (((4, 1), S8), ((4, 0), U8)):
        _add("sub_x4", GATHER4, x, w, note="nibble gather")
    for x, w in (((4, 1), S8), ((4, 0), U8)):
        _add("expand_gather", GATHER4, x, w, {"QE_SUB_X4": "0"}, "QE_SUB_X4=0")
    for x in ((4, 1), (4, 0)):
        for w in (S8, U8, (4, 1), (3, 0), (7, 1)):
            _add("flat_x4", FLAT128, x, w, note="nibbles in the staging")
    for x in ((4, 1), (4, 0)):
        for w in (S8, U8, (4, 1), (3, 0), (7, 1)):
            _add("expand_1x1", FLAT128, x, w, {"QE_X4": "0"}, "QE_X4=0")
    # the fused entries behind every activation-decode site, and the in-kernel re-centring of 8-bit codes
    _add("expand_3x3", C3, (5, 0), S8, entry="requant")
    _add("expand_1x1", FLAT, (3, 1), U8, entry="requant")
    _add("expand_gather", GATHER, (7, 0), S8, entry="requant")
    _add("sub_x4", GATHER4, (4, 0), S8, entry="requant")
    _add("flat_x4", FLAT128, (4, 1), (4, 0), entry="requant")
    _add("pwr", PWR, U8, S8, entry="requant")
    # the block end runs on the resident-tile kernels only, which take 8-bit operands: no plan accepts it behind an
    # expansion, a nibble gather or FlatX4 (plan_conv: m.sub || m.expand -> two passes)
    _add("pwr", PWR, U8, U8, entry="residual")
    # ---- float-input conv ----
    mid = [q for q in SETTINGS if q[0] in (5, 6, 7)]
    for w in mid:
        _add("f32_prep", F_MAIN, F32X, w)
    for w in mid:
        _add("f32_prep_stem", F_STEM, F32X, w)
    for w in SETTINGS:
        _add("generic_f32", F_GEN, F32X, w)
    # ---- linear ----
    for i, x in enumerate(SETTINGS):
        _add("lin_generic", LIN0, x, partner(i), note="x walks, w = partner")
    for i, w in enumerate(SETTINGS):
        _add("lin_generic", LIN0, partner(i), w, note="w walks, x = partner")
    for w in SETTINGS:
        _add("lin_generic_f32", LIN0, F32X, w)
    for w in (S8, U8):
        _add("lin_f32_mfma", LIN64, F32X, w)
    for w in (S8, U8):
        _add("lin_bf16in", LIN64, BF16X, w)
    for site, shape, env in (("lin_mfma1", LIN64, None), ("lin_mfma2", LIN64, {"QE_LIN_NJ": "4"}),
                             ("lin_mfma3", LIN128, {"QE_LIN8": "1"}), ("lin_mfma4", LIN128, {"QE_LIN8": "2"})):
        for x in (S8, U8):
            for w in (S8, U8):
                _add(site, shape, x, w, env, "sign pair")
    _add("lin_generic", LIN0, (3, 1), (5, 0), entry="requant", note="form 0: two passes")
    _add("lin_generic", LIN0, (6, 0), (2, 1), entry="residual", note="form 0: two passes")
    _add("lin_generic", LIN0, (7, 1), (4, 0), entry="bf16", note="form 0: two passes")


_build()
# unsigned 8-bit x unsigned 8-bit on the kernels whose shortest reduction is K = 128 (module docstring)
TIGHT = tuple(k for k, r in enumerate(ROWS) if r[0] in ("pwr7", "flatd", "lin_mfma3", "lin_mfma4") and r[3] == U8 and r[4] == U8)


def op_of(row):
    return SITES[row[0]][0]


def row_id(k):
    site, entry, shape, x, w, env, note = ROWS[k]
    return "%d-%s-%s-x%s-w%s%s" % (k, site, entry, tag(x), tag(w), "-" + "-".join("%s=%s" % kv for kv in env.items()) if env else "")


def rows_of(site):
    return [k for k, r in enumerate(ROWS) if r[0] == site]


def macs(row):
    s = row[2]
    if len(s) == 3:
        return s[0] * s[1] * s[2]
    N, IC, H, W, OC, K, st, p = s
    return N * OC * ((H + 2 * p - K) // st + 1) * ((W + 2 * p - K) // st + 1) * IC * K * K


def reduction(row):
    s = row[2]
    return s[1] if len(s) == 3 else s[1] * s[5] * s[5]


# ---- host-side plan queries ---------------------------------------------------------------------------------------------
def _q(setting_, n_param=1):
    return capi.QeQParam(ALIGNED, setting_[0], setting_[1], ALIGNED, ALIGNED, n_param)


def _rq8():
    return capi.QeRequant(ALIGNED, ALIGNED, 1, -128.0, 127.0, 8, 1)


def planned_sites(row):
    """The decode sites a call of the row passes, read from the plan queries with the row's knobs: its activation site
    (None: no pass or kernel of its own) and its weight site."""
    site, entry, shape, x, w, env, note = row
    op = op_of(row)
    L = capi.lib()
    import ctypes
    with capi.knobs(**(env or {})):
        if op == "conv":
            N, IC, H, W, OC, K, st, p = shape
            sh = capi.conv_shape(N, IC, H, W, OC, K, K, st, p)
            xq, wq = _q(x), _q(w)
            info = capi.conv_plan_info(sh, xq, wq, _rq8() if entry == "requant" else None, ALIGNED, ALIGNED)
            route = capi.CONV_ROUTES[info.route]
            assert capi.conv_path(sh, xq, wq) == (route != "generic")
            if entry == "residual":
                assert capi.residual_path(sh, xq, wq, None) == 1 and route in ("pwr", "pwr7"), "the block end runs in two passes"
            if route != "mfma":
                return {route}
            fam = capi.CONV_FAMILIES[info.family]
            if capi.CONV_PREPASSES[info.pre] == "sub_x4":
                act = "sub_x4" if info.sub_x4 else "?"    # (launch_conv_mfma: no expansion runs in front of this pass)
            elif fam == "flat_x4":
                act = "flat_x4" if not info.expand and not info.pre else "?"
            elif info.expand:
                act = "expand_gather" if info.pre else ("expand_1x1" if K == 1 else "expand_3x3")
            else:
                act = None
            wsite = "wraw_" + fam if info.wraw else ("prep_smallic" if fam == "stem" else "prep")
            return {act, wsite}
        if op == "conv_f32":
            N, IC, H, W, OC, K, st, p = shape
            sh = capi.conv_shape(N, IC, H, W, OC, K, K, st, p)
            info = capi.conv_f32_plan_info(sh)
            assert bool(capi.float_input_path(sh, _q(w))) == bool(info.ok)
            return {"generic_f32" if not info.ok else ("f32_prep_stem" if info.stem else "f32_prep")}
        B, K, O = shape
        wq = _q(w, O)
        if op == "lin":
            xq = _q(x)
            form = capi.linear_form(xq, wq, B, K, O)
            assert capi.linear_path(xq, wq, B, K, O) == (form != 0)
            if entry == "requant":
                assert L.qe_quantlinear_requant_path(ctypes.byref(xq), ctypes.byref(wq), B, K, O, ctypes.byref(_rq8()), ALIGNED) == 0
            if entry == "residual":
                assert capi.linear_residual_path(xq, wq, B, K, O) == 0
            if entry == "bf16":
                assert L.qe_quantlinear_bf16_path(ctypes.byref(xq), ctypes.byref(wq), B, K, O, ALIGNED) == 0
            return {"lin_generic" if form == 0 else "lin_mfma%d" % form}
        if op == "lin_f32":
            return {"lin_f32_mfma" if L.qe_quantlinear_float_input_path(ALIGNED, ctypes.byref(wq), B, K, O) else "lin_generic_f32"}
        return {"lin_bf16in" if L.qe_quantlinear_bf16_input_path(ALIGNED, ctypes.byref(wq), B, K, O) == 1 else "widened"}


# ---- operands -------------------------------------------------------------------------------------------------------------
def _last_read(shape):
    """Index of the last input element a conv reads."""
    N, IC, H, W, OC, K, st, p = shape
    OH, OW = (H + 2 * p - K) // st + 1, (W + 2 * p - K) // st + 1
    return (N - 1, IC - 1, min(H - 1, (OH - 1) * st - p + K - 1), min(W - 1, (OW - 1) * st - p + K - 1))


def _codes(rng, shape, q, last=None):
    lo, hi = qr.code_range(*q)
    c = rng.randint(lo, hi + 1, size=shape).astype(np.int64)
    c.flat[0], c.flat[-1] = lo, hi
    if last is not None:
        c[last] = hi
    return c


def _zmax(bits):
    return min(3, (1 << bits) // 4 + 1)


def _exact_zero(rng, q, n, k):
    """Non-zero integer zero points (as subtracted), |z| <= min(3, 2^bits / 4 + 1).  The narrowest formats keep q - z off
    zero on every code (a partner that is zero at an operand's edge would hide that edge): unsigned 1- and 2-bit codes get
    z < 0, signed 1-bit codes z = +1; the sign alternates over the rows elsewhere."""
    bits, sign = q
    mag = rng.randint(1, _zmax(bits) + 1, size=n)
    if not sign and bits <= 2:
        sgn = -1
    elif sign and bits == 1:
        sgn = 1
    else:
        sgn = 1 if k % 2 == 0 else -1
    return (sgn * mag).astype(np.float32)


def _packed(c, q, s, z):
    return dict(q=c, bits=q[0], sign=q[1], packed=qr.pack(c, *q), s=np.asarray(s, np.float32).reshape(-1),
                z=np.asarray(z, np.float32).reshape(-1), shape=c.shape)


@functools.lru_cache(maxsize=None)
def operands(k, regime):
    """The tensors of ROWS[k]: x (a packed operand dict, or a float32 array under "xf"), w, bias, and in the exact regime
    lsb[oc] = sx sw[oc].  Zero points are stored as the engine takes them: subtracted by the convs and by the float-input
    linears, added by the packed linear."""
    site, entry, shape, x, w, env, note = ROWS[k]
    op = op_of(ROWS[k])
    exact = regime == "exact"
    rng = np.random.RandomState(9000 + 2 * k + (0 if exact else 1))
    conv = op in ("conv", "conv_f32")
    packed_x = x not in (F32X, BF16X)
    if conv:
        N, IC, H, W, OC, K, st, p = shape
        x_shape, w_shape, n_out, last = (N, IC, H, W), (OC, IC, K, K), OC, _last_read(shape)
    else:
        B, Kd, O = shape
        x_shape, w_shape, n_out, last = (B, Kd), (O, Kd), O, None
    add = op == "lin"                                   # the packed linear adds its zero points
    per_tensor_w = k % 3 == 0
    nw = 1 if per_tensor_w else n_out
    out = dict(stride=shape[6] if conv else None, pad=shape[7] if conv else None, x_last=last)
    qw = _codes(rng, w_shape, w)
    if exact:
        sw = 2.0 ** -rng.randint(3, 8, size=nw)
        zw = _exact_zero(rng, w, nw, k)
        sx = np.array([2.0 ** -6 if packed_x else 2.0 ** -4])
        lsb = (sx * sw * np.ones(n_out)).astype(np.float64)
        bias = None if k % 4 == 3 else (rng.randint(-1000, 1001, size=n_out) * lsb).astype(np.float32)
        out["lsb"] = lsb
    else:
        sw = rng.uniform(2.5e-4, 7.5e-4, size=nw)
        zw = rng.uniform(-3, 3, size=nw)
        bias = None if k % 4 == 3 else rng.normal(0, 0.1, size=n_out).astype(np.float32)
    out["w"] = _packed(qw, w, sw, -zw if add and exact else zw)
    out["bias"] = bias
    if packed_x:
        qx = _codes(rng, x_shape, x, last)
        lo, hi = qr.code_range(*x)
        if exact:
            zx = _exact_zero(rng, x, 1, k + 1)
            zx = -zx if add else zx
        elif conv:
            zx = rng.uniform(0.3, 0.7, size=1) * (hi + 1) if not x[1] else rng.uniform(-5, 5, size=1)
        else:
            # per batch row on every third row; unsigned codes about their mid-range (added: negative) on odd rows
            n = x_shape[0] if k % 3 == 0 else 1
            sx = rng.uniform(1e-3, 3e-3, size=n)
            zx = -rng.uniform(0.3, 0.7, size=n) * (hi + 1) if (not x[1] and k % 2) else rng.uniform(-5, 5, size=n)
        if not exact and conv:
            sx = np.array([2e-3])
        out["x"] = _packed(qx, x, sx, zx)
    else:
        if exact:
            m = rng.randint(-255, 256, size=x_shape)
            m.flat[0], m.flat[-1] = -255, 255
            if last is not None:
                m[last] = 255
            xf = (m / 16.0).astype(np.float32)
        else:
            xf = rng.normal(0, 1, size=x_shape).astype(np.float32)
            if x == BF16X:
                xf = qr.bf16_round(xf).astype(np.float32)
        out["xf"] = xf
    return out


def reference(k, regime, ops=None):
    """The numpy float64 value of ROWS[k] on operands(k, regime) (or on `ops`)."""
    site, entry, shape, x, w, env, note = ROWS[k]
    o = operands(k, regime) if ops is None else ops
    op = op_of(ROWS[k])
    W = o["w"]
    wargs = (W["packed"], W["shape"], W["bits"], W["sign"], W["s"], W["z"], o["bias"])
    if op == "conv":
        X = o["x"]
        return qr.quantconv2d(X["packed"], X["shape"], X["bits"], X["sign"], X["s"], X["z"], *wargs, o["stride"], o["pad"])
    if op == "conv_f32":
        return qr.quantconv2d_float_input(o["xf"], *wargs, o["stride"], o["pad"])
    if op == "lin":
        X = o["x"]
        return qr.quantlinear(X["packed"], X["shape"], X["bits"], X["sign"], X["s"], X["z"], *wargs)
    return qr.quantlinear_float_input(o["xf"], *wargs)


def lsb_of(k, out_shape):
    """lsb[oc] of the exact regime broadcast over an output of `out_shape` (channel axis 1)."""
    lsb = operands(k, "exact")["lsb"]
    return lsb.reshape([1, -1] + [1] * (len(out_shape) - 2))


@functools.lru_cache(maxsize=None)
def fused_extras(k):
    """Exact regime, fused entries: the consumer's quantiser (a power-of-two scale that spreads the outputs over the 8-bit
    range, an integer zero point), the identity / residual (integer multiples of lsb) and the bf16 post scale."""
    ref = reference(k, "exact")
    rng = np.random.RandomState(500 + k)
    amax = max(float(np.abs(ref).max()), 2.0 ** -20)
    e = int(np.ceil(np.log2(amax / 100.0)))
    ident = (rng.randint(-4096, 4097, size=ref.shape) * lsb_of(k, ref.shape)).astype(np.float32)
    return dict(rq_scale=np.float32(2.0 ** e), rq_zero=np.float32(3.0), qmin=-128, qmax=127, identity=ident, post_scale=0.5)


def _terms(k):
    """(K, A_x, A_w, |z_x| max, |z_w| max, x unsigned 8-bit, w unsigned 8-bit, extra = (max |bias| + max |identity|) / lsb)."""
    row = ROWS[k]
    o = operands(k, "exact")
    lsb = o["lsb"]
    extra = 0.0 if o["bias"] is None else float(np.abs(o["bias"].astype(np.float64) / lsb).max())
    if row[1] == "residual":
        ident = fused_extras(k)["identity"].astype(np.float64)
        extra += float(np.abs(ident / lsb_of(k, ident.shape)).max())
    if "x" in o:
        ax, zx, ux = 1 << row[3][0], float(np.abs(o["x"]["z"]).max()), row[3] == U8
    else:
        ax, zx, ux = 256, 0.0, False                     # |x| 16 <= 255
    return reduction(row), ax, 1 << row[4][0], zx, float(np.abs(o["w"]["z"]).max()), ux, row[4] == U8, extra


def bound(k):
    """G + max |bias| / lsb of the issue: K (A_x + Z_x)(A_w + Z_w), A = 2^bits, Z = max |z| + 128 for unsigned 8-bit."""
    K, ax, aw, zx, zw, ux, uw, extra = _terms(k)
    return K * (ax + zx + 128 * ux) * (aw + zw + 128 * uw) + extra


def tight_bound(k):
    """The same with what a re-centred 8-bit operand really holds: |a| <= 128 and z' = z -+ 128 (module docstring)."""
    K, ax, aw, zx, zw, ux, uw, extra = _terms(k)
    a = lambda A: 128 if A == 256 else A
    return K * (a(ax) + zx + 128 * ux) * (a(aw) + zw + 128 * uw) + extra
